/* kp_spec.h -- constants of the kaptive_amd nucleotide aligner ("kp-align v5") and of the packed data layout.
 *
 * The reference delegates gene-vs-contig alignment to the third-party rammappy 0.1.3 wheel
 * (src/kaptive/serotyping/core.py:147-155), whose source is not in the reference tree; parity at that stage is
 * UNPINNED. This header is therefore the specification of the replacement: the HIP kernels
 * (kaptive_amd/csrc) and the CPU restatement (oracle/kp_oracle.c) both include it and must agree bit for bit.
 * Parameters follow minimap2's documented defaults where the design has an equivalent (k, scoring, -s 80 peak score,
 * >=3 seeds and >=40 seeded bases per chain, chaining of anchors across diagonal jumps of up to 500); DESIGN.md lists every deviation.
 */
#ifndef KP_SPEC_H
#define KP_SPEC_H

#include <stdint.h>

/* ---- base codes -------------------------------------------------------------------------------------------------
 * A C G T(U) = 0 1 2 3, case-insensitive; every other byte is "N" (code 4).  Packed streams hold 2 bits per base,
 * 16 bases per little-endian uint32 (base i of a word at bits 2i..2i+1); N positions are stored as code 0 and listed
 * separately as sorted, disjoint [start,end) runs in the same coordinate space. */
#define KP_CODE_N 4

/* ---- assembly layout --------------------------------------------------------------------------------------------
 * An assembly is one padded coordinate space: contig c occupies [ctg_start[c], ctg_start[c]+ctg_len[c]) and every
 * ctg_start is a multiple of KP_CONTIG_ALIGN; the gap up to the next contig is code 0.  Assemblies of a batch are
 * laid back to back, each starting on a KP_ASM_ALIGN boundary. */
#define KP_CONTIG_ALIGN 32u
#define KP_ASM_ALIGN 64u

/* ---- seeding (kp-align v3): minimap2's (w = 10, k = 15) minimizers on BOTH sides ----------------------------------------
 * The reference indexes the assembly and queries it with the genes (src/kaptive/core/genome.py:177-191,
 * src/kaptive/serotyping/core.py:147-155: Aligner(index, preset=None)); with no preset minimap2 samples both with
 * mm_sketch(w = 10, k = 15).  This section restates that sampling; it is the one place where v2 (a context-free rule at
 * density 1/4) measurably left the published algorithm (profiles/concordance_r3.md).
 *
 * Value of the 15-mer that STARTS at base p of a sequence (codes c[p..p+14], all in 0..3):
 *     fwd = sum c[p+j] << 2(14-j)   (first base in the high bits)      rev = sum (3 - c[p+j]) << 2j   (its reverse complement)
 *     z = fwd < rev ? 0 : 1  (k is odd: fwd != rev)                    x(p) = kp_hash30(z ? rev : fwd)
 * A 15-mer with an ambiguous base has no value (x = +inf).  kp_hash30 is minimap2's hash64 under the 30-bit mask; it is a
 * bijection of 30-bit values, so equal x means equal canonical 15-mers.
 *
 * Which positions are SEEDS is defined by the state machine of mm_sketch, restated here (KP_W = 10, steps over the bases
 * i = 0..len-1 of one contig or gene; the 15-mer ending at base i starts at i - 14):
 *     l(i)   = number of consecutive unambiguous bases ending at i (0 at an ambiguous base)
 *     info(i) = x(i - 14) if l(i) >= KP_K else +inf;   buf = info of the last KP_W steps;   min = (+inf) initially
 *     step i:  (1) if l(i) == KP_W + KP_K - 1 and min != +inf: every buffered entry other than this step's and other than
 *                  `min` itself whose value equals min's is a seed                      [ties of the first full window]
 *              (2) if info(i) <= min:  `min` is a seed if l(i) >= KP_W + KP_K and min != +inf;  min = info(i)
 *                  else if `min` is the entry that leaves the buffer at this step:
 *                       `min` is a seed if l(i) >= KP_W + KP_K - 1;  min = the LAST smallest buffered entry;
 *                       if l(i) >= KP_W + KP_K - 1 and min != +inf: every other buffered entry equal to it is a seed
 *     after the last base: `min` is a seed if it is not +inf.
 * Away from sequence ends and ambiguous bases this is: p is a seed iff x(p) is a smallest value (ties included) of at
 * least one of the KP_W windows of KP_W consecutive 15-mers that contain it -- the form the scan kernel evaluates for
 * every position whose 15-mer starts at least KP_W bases after the start of its clean stretch and ends at least KP_W bases
 * before the end of it; the remaining positions (contig ends, the flanks of N runs) are decided by running the state
 * machine itself (kp_scan.hip: kp_edge_kernel).  Expected density 2 / (KP_W + 1).
 *
 * A gene seed (start qs on the gene's forward strand, strand bit zq) and a contig seed (start ts, strand bit zt) with the
 * same x make one ANCHOR: same strand if zq == zt, query position qs; otherwise the gene's reverse complement, query
 * position gene_len - KP_K - qs.
 *
 * OCCURRENCE CUT (v4; round 6: the quantile).  minimap2 drops a query seed that occurs more than mid_occ times in the index --
 * here: among the assembly's minimizers, both strands -- with mid_occ = max(min_mid_occ = 10, 1 + the count at position
 * (int)((1 - 2e-4f) n) of the sorted occurrence counts of the index's n distinct minimizers) (mm_idx_cal_max_occ).  A gene
 * seed with more than mid_occ anchors in an assembly (one anchor per occurrence, whichever strand) loses all of them.  The
 * quantile can matter only where some gene seed has more than KP_MID_OCC anchors (mid_occ >= 10 whatever the assembly holds),
 * and it is WORKED OUT only for an assembly in which some gene has at least KP_MIN_ANCHORS such seeds (kp_chain.hip: the block
 * that meets them sketches its assembly once more and counts every minimizer); in every other assembly the cut is the floor,
 * KP_MID_OCC.  (One or two seeds of a gene beyond the floor -- in practice a 15-mer it shares by chance with a repeat of the
 * genome: on a background with IS-like repeats 7 in 10 assemblies have one -- cannot make a chain on their own, minimap2's
 * -n 3; cutting them at the floor where minimap2 would keep some of them takes at most two anchors off a chain of the gene's
 * own copy.  Counting 0.9 M minimizers per assembly for them costs more than the rest of the pass.)  Counts are capped at KP_MID_OCC_HIST - 1 (minimap2's own cap,
 * max_mid_occ, is 10^6; an assembly whose 2e-4 quantile is a minimizer in 2 000 copies is not a bacterial genome).
 * minimap2's rescue of high-occurrence seeds in seed-poor stretches (mm_seed_select) is not restated. */
#define KP_MID_OCC 10
#define KP_MID_OCC_FRAC 2e-4f
#define KP_MID_OCC_HIST 2048
#define KP_K 15
#define KP_W 10
#define KP_KMER_MASK 0x3FFFFFFFu
#ifndef KP_SPEC_FN
#ifdef __HIPCC__ /* the HIP sources use the same statement on the device */
#define KP_SPEC_FN __host__ __device__ inline
#else
#define KP_SPEC_FN static inline
#endif
#endif
KP_SPEC_FN uint32_t kp_hash30(uint32_t key) { /* minimap2 sketch.c: hash64(key, (1 << 30) - 1), all in 32 bits */
    key = (~key + (key << 21)) & KP_KMER_MASK;
    key = key ^ key >> 24;
    key = ((key + (key << 3)) + (key << 8)) & KP_KMER_MASK;
    key = key ^ key >> 14;
    key = ((key + (key << 2)) + (key << 4)) & KP_KMER_MASK;
    key = key ^ key >> 28;
    return key; /* the last step, key + (key << 31), adds nothing below bit 30 */
}
#define KP_MAX_GENE_LEN 65535       /* query positions are 16-bit fields of the anchor key and of the hit order's keys */
#define KP_FILL16_MAX_GENE_LEN 15800 /* longest gene the packed 16-bit fill kernel takes: biased scores (<= 2 * length + 14) stay below
                                        0x7C00 (kp_sw.hip); tasks of longer genes are filled with 32-bit scores (kp_sw_long_kernel) */
#define KP_MAX_GENES 131071   /* (gene*2+strand) is stored in 18 bits */
#define KP_MAX_ASM_LEN ((1u << 30) - 65536u)

/* anchor key (sortable): [gs:18][diag:30][qpos:16], diag = tpos - qpos + 65536, gs = gene*2 + (strand<0) */
#define KP_DIAG_BIAS 65536
#define KP_ANCHOR_KEY(gs, diag, qpos) (((uint64_t)(gs) << 46) | ((uint64_t)(diag) << 16) | (uint64_t)(qpos))
#define KP_KEY_GS(k) ((uint32_t)((k) >> 46))
#define KP_KEY_DIAG(k) ((uint32_t)(((k) >> 16) & 0x3FFFFFFFu))
#define KP_KEY_QPOS(k) ((uint32_t)((k) & 0xFFFFu))

/* ---- anchors -> DP tasks ----------------------------------------------------------------------------------------
 * Anchors of one assembly are sorted by key and cut into clusters: a new cluster starts when gs changes, the contig
 * changes, the diagonal jumps by more than KP_DIAG_GAP, or the cluster would span more than KP_MAX_SPREAD diagonals.
 *
 * Which clusters become tasks follows minimap2's chaining thresholds -n 3 -m 40 (mm_chain_dp + mg_chain_backtrack):
 *   a cluster of n <= KP_CHAIN_DP_MAX anchors is chained exactly as minimap2 chains that anchor set (with so few anchors
 *   its max_skip / max_iter heuristics cannot act): anchors in (target, query) order, f[i] = max(KP_K, max over earlier j
 *   of f[j] + sc(i, j)) with the FIRST maximum met going backwards from i - 1, where for dq = q_i - q_j, dr = t_i - t_j:
 *       sc = invalid if dq <= 0, dr == 0 (dr > 0 then holds: target order) or dq > KP_CHAIN_MAX_DIST;
 *       dd = |dr - dq|, dg = min(dr, dq), sc = min(KP_K, dg), minus kp_chain_pen[dd] if dd != 0 or dg > KP_K
 *   (kp_chain_pen[dd] = int(0.12 dd + 0.5 mg_log2(dd + 1)), minimap2's gap cost for k = 15, tabulated below; dd <= the
 *   cluster's spread).  The chain is the one ending at the largest f (the later anchor on ties), walked back along the
 *   chosen predecessors and cut where the score counted from its end peaks (mg_chain_backtrack's max_i); its score is that
 *   peak.  The cluster becomes a task iff the score is >= KP_MIN_CHAIN_SCORE (which needs >= KP_MIN_ANCHORS anchors); the
 *   task's n_anchors is the chain's anchor count and chain_score its score.
 *   A cluster of more anchors becomes a task iff its anchors cover >= KP_MIN_SEED_SPAN query bases (qmax - qmin + K);
 *   n_anchors = n, chain_score = min(KP_K * n, qmax - qmin + K) (what a co-linear chain of them scores).
 * The band is the cluster's diagonal range (all its anchors) widened on both sides and centred: by
 * KP_BAND_MARGIN_NARROW when that fits 16 diagonals (anchors on one or two adjacent diagonals: no indel seen), otherwise by
 * KP_BAND_MARGIN, rounded up to 32, 64 or 128 diagonals. */
#define KP_DIAG_GAP 32
#define KP_BAND_MARGIN 15
#define KP_BAND_MARGIN_NARROW 7 /* clusters whose anchors span at most 2 diagonals get a 16-diagonal band */
#define KP_MAX_BAND 128
#define KP_MAX_SPREAD (KP_MAX_BAND - 2 * KP_BAND_MARGIN - 1)
#define KP_MIN_ANCHORS 3
#define KP_MIN_SEED_SPAN 40
#define KP_CHAIN_DP_MAX 24
#define KP_CHAIN_MAX_DIST 5000 /* minimap2's max_gap */
#define KP_CHAIN_PEN_SIZE 512 /* dd 0..500 (minimap2's bw), padded */
#define KP_CHAIN_PEN_TABLE                                                                                            \
    {0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 6, 6, \
     6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, \
     10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 13, 13, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, \
     14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 16, 16, 16, 16, 16, 16, 16, 16, 17, 17, 17, 17, 17, 17, 17, 17, 18, 18, 18, 18, 18, 18, \
     18, 18, 19, 19, 19, 19, 19, 19, 19, 19, 20, 20, 20, 20, 20, 20, 20, 20, 21, 21, 21, 21, 21, 21, 21, 21, 22, 22, 22, 22, 22, 22, \
     22, 22, 23, 23, 23, 23, 23, 23, 23, 23, 24, 24, 24, 24, 24, 24, 24, 24, 25, 25, 25, 25, 25, 25, 25, 25, 26, 26, 26, 26, 26, 26, \
     26, 26, 27, 27, 27, 27, 27, 27, 27, 27, 28, 28, 28, 28, 28, 28, 28, 28, 29, 29, 29, 29, 29, 29, 29, 29, 30, 30, 30, 30, 30, 30, \
     30, 30, 31, 31, 31, 31, 31, 31, 31, 31, 32, 32, 32, 32, 32, 32, 32, 32, 33, 33, 33, 33, 33, 33, 33, 33, 33, 34, 34, 34, 34, 34, \
     34, 34, 34, 35, 35, 35, 35, 35, 35, 35, 35, 36, 36, 36, 36, 36, 36, 36, 36, 37, 37, 37, 37, 37, 37, 37, 37, 38, 38, 38, 38, 38, \
     38, 38, 38, 39, 39, 39, 39, 39, 39, 39, 39, 39, 40, 40, 40, 40, 40, 40, 40, 40, 41, 41, 41, 41, 41, 41, 41, 41, 42, 42, 42, 42, \
     42, 42, 42, 42, 43, 43, 43, 43, 43, 43, 43, 43, 44, 44, 44, 44, 44, 44, 44, 44, 45, 45, 45, 45, 45, 45, 45, 45, 45, 46, 46, 46, \
     46, 46, 46, 46, 46, 47, 47, 47, 47, 47, 47, 47, 47, 48, 48, 48, 48, 48, 48, 48, 48, 49, 49, 49, 49, 49, 49, 49, 49, 50, 50, 50, \
     50, 50, 50, 50, 50, 50, 51, 51, 51, 51, 51, 51, 51, 51, 52, 52, 52, 52, 52, 52, 52, 52, 53, 53, 53, 53, 53, 53, 53, 53, 54, 54, \
     54, 54, 54, 54, 54, 54, 55, 55, 55, 55, 55, 55, 55, 55, 55, 56, 56, 56, 56, 56, 56, 56, 56, 57, 57, 57, 57, 57, 57, 57, 57, 58, \
     58, 58, 58, 58, 58, 58, 58, 59, 59, 59, 59, 59, 59, 59, 59, 59, 60, 60, 60, 60, 60, 60, 60, 60, 61, 61, 61, 61, 61, 61, 61, 61, \
     62, 62, 62, 62, 62, 62, 62, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64}

/* ---- banded local alignment (Smith-Waterman-Gotoh; scores <= 2 * KP_MAX_GENE_LEN) ----------------------------------------------------------
 * H = max(0, Hdiag + s, E, F);  E (gap in query, moves along the target) = max(Hleft - (O+X), Eleft - X);
 * F (gap in target, moves along the query) = max(Hup - (O+X), Fup - X).  Opening wins ties against extending; the
 * diagonal wins ties against E, E against F; a cell whose best is <= 0 is a restart cell.  The reported cell is the
 * first maximum in (query row, target column) order.  Cells outside the band or the contig read as H=0, E=F=-inf.
 * Hits whose cell score is below KP_MIN_DP_SCORE are dropped.
 *
 * The recurrence charges a gap of length n with KP_GAP_OPEN + n * KP_GAP_EXT (minimap2's first affine piece).  The score a
 * hit REPORTS is that of its path under minimap2's two-piece cost min(4 + 2n, 24 + n): every gap longer than
 * KP_GAP_LONG = 20 columns is credited n - 20 during the traceback (minimap2 itself re-scores the finished path with the
 * two-piece cost for its reported DP score).  Gaps that long need a 32-diagonal band or wider and are rare; the path is
 * still the one-piece optimum. */
#define KP_SC_MATCH 2
#define KP_SC_MISMATCH (-4)
#define KP_SC_N (-1) /* either base is N */
#define KP_GAP_OPEN 4
#define KP_GAP_EXT 2
#define KP_GAP_OPEN2 24
#define KP_GAP_EXT2 1
#define KP_GAP_LONG ((KP_GAP_OPEN2 - KP_GAP_OPEN) / (KP_GAP_EXT - KP_GAP_EXT2)) /* from here on the second piece is cheaper */
#define KP_MIN_DP_SCORE 80
#define KP_MIN_CHAIN_SCORE 40 /* minimap2 -m: floor of the secondary score in the mapping quality (kp_mapq.h) */
#define KP_MASK_LEVEL_NUM 1   /* a hit is secondary to a better hit of its gene that covers more than */
#define KP_MASK_LEVEL_DEN 2   /* KP_MASK_LEVEL_NUM / KP_MASK_LEVEL_DEN of the shorter one's query span (minimap2 -M 0.5) */
#define KP_NEG_INF (-(1 << 29))

/* ---- kp-align v5: chains of ANCHORS across diagonal jumps of up to KP_JOIN_BW (minimap2's bw = 500) --------------------------
 * minimap2 chains anchors whose diagonals differ by up to bw = 500 and aligns through the gap; a gene with an insertion or
 * deletion of 33-500 bases is ONE hit there -- also when the stretch beyond the event is too short to be a chain of its own
 * (an event next to a gene's end), and when two events nearly cancel so that the stretches before and after them share a
 * diagonal.  The clusters above stop at KP_DIAG_GAP; the JOIN sits on top of them and leaves everything else as it was: every
 * accepted cluster is still a band task with a hit of its own unless a chain CONSUMES it (below).
 *
 * GROUPS.  Every cluster counts, weak ones (fewer than KP_MIN_ANCHORS anchors or than KP_MIN_SEED_SPAN query bases: no band
 * task) included; a cluster is PROVISIONAL when it has >= KP_MIN_ANCHORS anchors covering >= KP_MIN_SEED_SPAN query bases (it
 * may still be rejected by its chain score).  Per gene/strand AND contig, take the clusters in the order of the sorted
 * anchors (diagonals are in the assembly's padded coordinates: near a contig boundary the clusters of two contigs interleave
 * in that order, which is why the contig is part of the key): a cluster continues the open sequence of its contig iff its
 * lowest diagonal is at most KP_JOIN_BW above the highest diagonal of the sequence's last cluster and the sequence holds
 * fewer than KP_JOIN_GROUP_MAX clusters; otherwise it closes that sequence and opens a new one.  At most KP_JOIN_OPEN
 * sequences of a gene/strand are open at a time: the cluster of a further contig closes the one whose last cluster ends on
 * the lowest diagonal (the lowest contig on ties).  A closed sequence of two or more clusters, at least one of them
 * provisional, whose clusters hold KP_MIN_ANCHORS..KP_JOIN_ANCHOR_MAX anchors in all, is a GROUP.
 *
 * CHAINS OF ANCHORS.  All anchors of the group's clusters, (t, q) = (target, query) position, t = q + diagonal, in (t, q)
 * order, are chained as mm_chain_dp chains them -- exactly, i.e. without its max_skip / max_iter shortcuts:
 *     f[i] = max(KP_K, max over earlier j of f[j] + sc(i, j)),  the FIRST maximum met going backwards from i - 1,
 * sc as for a cluster's chain (above: dq = q_i - q_j, dr = t_i - t_j; invalid if dq <= 0, dr == 0, dq or dr > KP_CHAIN_MAX_DIST;
 * dd = |dr - dq|, dg = min(dr, dq); sc = min(KP_K, dg) minus kp_chain_pen[dd] if dd != 0 or dg > KP_K) and also invalid if
 * dd > KP_JOIN_BW.  Backtracking as mg_chain_backtrack: repeatedly take the unused anchor with the largest f >=
 * KP_MIN_CHAIN_SCORE (the later one on ties) and walk its predecessors until a used anchor or the start, stopping early once
 * the score counted from the end has fallen KP_JOIN_BW below its peak; the chain is cut at that peak, its score is the peak
 * and its anchors become used -- also when it is then discarded for scoring below KP_MIN_CHAIN_SCORE or holding fewer than
 * KP_MIN_ANCHORS anchors.
 *
 * PIECES.  A chain's anchors in query order fall into pieces: a new piece starts where the diagonal differs from the anchor
 * before by more than KP_DIAG_GAP, or where the piece would come to span more than KP_MAX_SPREAD diagonals.  A chain of one
 * piece is what its cluster's band task already aligns; a chain of 2..KP_JOIN_MAX_PIECES pieces is a JOIN (more pieces: none).
 * Every piece gets a band of the same width W and margin M -- those of a cluster's band task for the widest piece's diagonal
 * range: 16 diagonals and KP_BAND_MARGIN_NARROW when that holds it, otherwise the smallest of 32, 64, 128 with KP_BAND_MARGIN
 * (kp_piece_margin / kp_piece_width below) --, centred on its own range:  lo[k] = dmin[k] - M - (W - need[k]) / 2,
 * need[k] = dmax[k] - dmin[k] + 1 + 2 M.  n_anchors and chain score of the join are the chain's.
 *
 * JOINED FILL.  Every piece is filled as a band task (the recurrence above: local, H >= 0, restarts) over the ROWS between its
 * neighbours' anchors: piece k covers rows [R0, R1), R0 = 0 for the first piece, otherwise the query position of the LAST anchor
 * of piece k - 1 rounded down to a multiple of 8; R1 = the gene's length for the last piece, otherwise the query position of
 * the FIRST anchor of piece k + 1 plus KP_K (a chain's alignment runs through its anchors: a piece is left after its last
 * anchor and entered before its first); rows outside read as outside the contig (H = 0, E = F = -inf).  In a
 * piece k > 0, H has two more candidates, the CROSS gaps from piece k - 1.  When piece k lies on higher diagonals
 * (lo[k] > lo[k-1]: an insertion in the contig) a gap along row r from a live cell (r, t') of piece k - 1 left of piece k's
 * band in that row (t' < lo[k] + r):
 *     X1 = max (H(r, t') + 2 t') - 4 - 2 t        X2 = max (H(r, t') + t') - 24 - t      (first / second piece of the gap cost)
 * otherwise (a deletion) a gap down column t from a live cell (r', t) of piece k - 1 on a diagonal above piece k's band
 * (t - r' > lo[k] + W - 1):   X1 = max (H(r', t) + 2 r') - 4 - 2 r,   X2 = max (H(r', t) + r') - 24 - r.
 * (Live: H > 0.)  A cross gap starts and ends in rows of the JUNCTION ZONE, the rows the two pieces share: r (and r') in
 * [R0 of piece k, R1 of piece k - 1) -- the stretch of the query between the last anchor of the piece before and the first
 * anchor of this one.  The source cell of a maximum is the first one in increasing t' (r').  H = max(diagonal, E, F, X1, X2) with
 * ties in that order (a candidate must beat everything before it); H <= 0 is a restart cell.  A path therefore crosses a gap
 * only where that pays -- which is what minimap2 comes to: it cuts a chain's end off when it is shorter than twice the gap
 * behind it (mm_fix_bad_ends) and lets the extension, a free local decision, reach across or not; an end long enough to be
 * kept always pays for its gap at the identities Kaptive works with.
 *
 * THE JOINED PATH.  The best cell of a piece is its first maximum of H in (row, column) order.  The pieces are tried in the
 * order of their best cells' scores (the earlier piece on ties): nothing is reported from a best cell below KP_MIN_DP_SCORE;
 * otherwise walk back from it (through cross gaps into earlier pieces, to where the path starts).  On the way: suf = score of
 * the part of the path behind the current cell with the costs of the cross gaps left out, sufmax = its largest value at a cell
 * in state H so far; at a cell that takes a cross gap, and at every cell in state H once a gap has been crossed, if
 * sufmax - suf > KP_JOIN_DROP the path is REJECTED (minimap2's z-drop of 400 against the open cost of the second gap piece,
 * which forgives a gap its length: mm_test_zdrop would have split the chain there), the piece is set aside and the next one
 * tried.  The first path that is not
 * rejected settles the chain: if it crosses at least one gap it is the JOINED HIT -- score = H(best cell) + the long-gap
 * credit of its in-band gaps, coordinates from its first and last cell, columns = cells + gap columns, matches counted base
 * by base, n_seeds and chain score those of the chain, plus the BONUS of its order score (below) --; if it crosses none, the
 * band task of that piece's cluster already reports it.
 *
 * CONSUMED PIECES.  minimap2 reports one alignment per chain (two where it splits one), and it cuts a chain's end off before
 * aligning when that end is shorter than twice the gap behind it (mm_fix_bad_ends): such an end is reported only if the
 * extension reaches across the gap.  So: the band tasks of the clusters that hold an anchor of a piece the joined hit runs
 * through report no hit of their own; and, unless a path of the chain was rejected, neither do those of the pieces of the
 * chain's WEAK ENDS (kp_weak_ends below) that the settled path does not run through.
 *
 * Not restated: minimap2's max_skip heuristic in the chaining DP, its mm_filter_bad_seeds (anchors between gaps that nearly
 * cancel are skipped as fill boundaries: the joined fill has no fill boundaries inside a piece), an extension that reaches
 * across a gap to a stretch WITHOUT any anchor (its band of 751 diagonals finds it, a piece needs an anchor to exist), the
 * re-chaining with bw_long = 20 000. */
#define KP_JOIN_BW 500
/* WEAK ENDS of a chain of n pieces (kp_spec.h, CONSUMED PIECES; minimap2's mm_fix_bad_ends restated on pieces).  qlo / qhi:
 * query position of every piece's first / last anchor; jump_before[k]: the diagonal jump between piece k - 1 and k.  Going in
 * from the first piece, L = query bases from the chain's first anchor to the end of piece k: pieces 0..k are a weak end if the
 * jump behind piece k exceeds L / 2; the walk ends once L >= KP_JOIN_BW or 2 L >= the chain's query extent.  Likewise from
 * the last piece.  Returns the mask of weak-end pieces. */
KP_SPEC_FN int kp_weak_ends(int n, const int *qlo, const int *qhi, const int *jump_before) {
    const int extent = qhi[n - 1] + KP_K - qlo[0];
    int mask = 0;
    for (int k = 0; k + 1 < n; ++k) {
        const int L = qhi[k] + KP_K - qlo[0];
        if (2 * jump_before[k + 1] > L) mask |= (1 << (k + 1)) - 1;
        if (L >= KP_JOIN_BW || 2 * L >= extent) break;
    }
    for (int k = n - 1; k >= 1; --k) {
        const int L = qhi[n - 1] + KP_K - qlo[k];
        if (2 * jump_before[k] > L) mask |= ((1 << n) - 1) & ~((1 << k) - 1);
        if (L >= KP_JOIN_BW || 2 * L >= extent) break;
    }
    return mask;
}
/* ORDER SCORE.  minimap2 orders a query's hits, filters them (-s) and computes mapping qualities with dp_max -- the best
 * running score of the path when a gap of n columns is charged KP_GAP_OPEN + 2 log2(1 + n) -- not with the alignment score.
 * For band tasks the two are as good as equal; a joined path's cross gaps make them differ by hundreds.  A joined hit
 * therefore carries a BONUS = sum over its cross gaps of (cost charged - (KP_GAP_OPEN + kp_log2x2(n))), floored at 0 per
 * gap and capped at KP_HIT_BONUS_MAX; order score = score + bonus takes the place of the score in the emission order
 * and in the mapping quality.  Until a hit's mapping quality is set the bonus rides in the bits of `score` from
 * KP_HIT_BONUS_SHIFT up; finished hit records hold the plain score. */
#define KP_HIT_BONUS_SHIFT 20
#define KP_HIT_BONUS_MAX 2047
#define KP_HIT_SCORE(field) ((int32_t)((uint32_t)(field) & ((1u << KP_HIT_BONUS_SHIFT) - 1u)))
#define KP_HIT_OSCORE(field) (KP_HIT_SCORE(field) + (int32_t)((uint32_t)(field) >> KP_HIT_BONUS_SHIFT))
KP_SPEC_FN int kp_log2x2(uint32_t n) { /* 2 log2(1 + n) to the nearest integer or so: exponent + the top mantissa bits, integers only */
    const uint32_t m = n + 1u;
    int e = 0;
    while ((m >> e) > 1u) ++e;
    const uint32_t mant = e >= 4 ? (m >> (e - 4)) & 15u : (m << (4 - e)) & 15u;
    return 2 * e + (mant >= 3u) + (mant >= 11u);
}
/* band of a join's pieces from the widest piece's diagonal range `spread` (largest minus smallest diagonal of its anchors): the
 * rule of a cluster's band task -- KP_BAND_MARGIN_NARROW either side when that fits 16 diagonals, KP_BAND_MARGIN otherwise */
KP_SPEC_FN int kp_piece_margin(int spread) { return spread + 1 + 2 * KP_BAND_MARGIN_NARROW <= 16 ? KP_BAND_MARGIN_NARROW : KP_BAND_MARGIN; }
KP_SPEC_FN int kp_piece_width(int spread) {
    const int need = spread + 1 + 2 * kp_piece_margin(spread);
    return need <= 16 ? 16 : (need <= 32 ? 32 : (need <= 64 ? 64 : 128));
}
#define KP_JOIN_GROUP_MAX 16
#define KP_JOIN_ANCHOR_MAX 4096 /* groups with more anchors than this are not chained (a gene beyond ~22 kb whose group holds them all) */
#define KP_JOIN_OPEN 4
#define KP_JOIN_MAX_PIECES 8
#define KP_JOIN_DROP (400 - KP_GAP_OPEN2)

/* ---- protein alignment (restates src/kaptive/core/pairwise.py:395-584) ------------------------------------------------ */
#define KP_PROT_GAP_OPEN 11
#define KP_PROT_GAP_EXT 1
#define KP_PROT_K 20
#define KP_PROT_NEG_INF (-1000000000)
#define KP_PROT_FILL (-128) /* BLOSUM62 lookup value for bytes outside ARNDCQEGHILKMFPSTWYVBJZX* */

/* ---- hit record (one per reported alignment; emission order: gene asc, score desc, contig asc, t_start asc,
 * forward strand first, q_start asc, q_end asc, t_end asc, matches desc, block_len asc, seeds desc; hits with the same
 * span -- gene, contig, strand and both intervals -- are emitted once, the first of them in that order).
 * Mapping quality: walking a gene's hits in emission order, a hit is SECONDARY (mapq 0) when its query span overlaps
 * that of an earlier primary hit of the gene by more than KP_MASK_LEVEL of the shorter span; it then counts towards that
 * primary's n_sub and best secondary score.  Every other hit is PRIMARY, mapq = kp_mapq_value (kp_mapq.h). ------------ */
typedef struct kp_hit {
    int32_t gene;    /* database gene index */
    int32_t contig;  /* contig index within the assembly */
    int32_t q_start; /* on the gene's forward strand, 0-based half-open */
    int32_t q_end;
    int32_t t_start; /* on the contig's forward strand, 0-based half-open */
    int32_t t_end;
    int32_t score;
    int32_t matches;   /* identical aligned bases */
    int32_t block_len; /* alignment columns */
    int8_t strand;     /* +1 / -1 */
    uint8_t mapq;      /* kp_mapq.h; 0 for secondary hits */
    uint8_t n_seeds;   /* anchors of the band task behind the hit, capped at 255 */
    uint8_t pad_;
} kp_hit;

/* ---- CIGAR (optional: computed only where the caller asks for it; no hit and no field of a hit depends on it) ----------------
 * The CIGAR of a hit is the path its fields were computed from, as run-length ops in BAM encoding -- what the reference's
 * parse_cigar_string produces (src/kaptive/core/alignment.py:872): uint32 len << KP_CIGAR_SHIFT | op, op M = 0, I = 1, D = 2.
 * The query is the gene and the target the contig, as in minimap2 and PAF: a diagonal step of the path is an M column, a
 * step in state E (gap in the query, moves along the target) a D column, a step in state F (gap in the target, moves along
 * the query) an I column; the columns of a joined path's cross gap are D when the gap runs along a row (the later piece
 * lies on higher diagonals) and I when it runs down a column.  Ops are listed in the order of increasing target position;
 * for strand -1 that is the order of the reverse-complemented gene, as minimap2 writes them.
 *
 * CANONICAL FORM.  No op has length 0; no two neighbouring ops have the same kind -- a cross gap that touches an in-band gap
 * of its kind is one op with it --; the first and the last op are M (a local path starts and ends on a diagonal step: a gap
 * state lies strictly below the H it derives from).
 *
 * CONSISTENCY WITH THE HIT.  sum M + sum I = q_end - q_start; sum M + sum D = t_end - t_start; sum M + sum I + sum D =
 * block_len; the M columns hold exactly `matches` pairs of equal unambiguous bases.  Scoring the ops again -- KP_SC_MATCH /
 * KP_SC_MISMATCH / KP_SC_N per M column, min(4 + 2 n, 24 + n) per gap op of n columns -- gives exactly `score` for the hit of
 * a band task, and at least `score` for a joined hit (a merged op is cheaper than the gaps it was made of).
 *
 * SAME-SPAN HITS.  Of hits with the same span one record is emitted (above); its CIGAR is the path of the source -- band task
 * or joined path -- whose record that is, i.e. that agrees with it in every field.  Where several sources do, the CIGAR is that
 * of the first of them in this order: band tasks before joins; then the lower band origin `lo` (of a joined path: of the
 * piece it ends in); then the narrower band.  Sources that agree in these too fill the same band of the same contig with the
 * same gene; for band tasks that is the same fill and the same path.  The rule reads nothing but the data: it never depends
 * on the order in which the device appended records. */
#define KP_CIGAR_M 0
#define KP_CIGAR_I 1
#define KP_CIGAR_D 2
#define KP_CIGAR_SHIFT 4

/* ---- CS (optional, like the CIGAR: no hit, no op and no report byte depends on it) -------------------------------------------------
 * The cs string of a hit is a pure function of its CIGAR ops and its two sequences; the direction bits of the fill are not read.
 * The query is the gene AS ALIGNED -- its reverse complement for strand -1, starting at row len - q_end; at q_start for strand
 * +1 -- and the target the contig, forward, from t_start.  Tokens are listed in the order of increasing target position, in the
 * grammar of minimap2's short form:
 *     :<n>        a maximal run of n identical columns
 *     *<t><q>     one substituted column: target base, then gene base
 *     +<bases>    the gene bases of an I op
 *     -<bases>    the contig bases of a D op
 * Letters are the lower-case acgtn of the packed alphabet: a contig position inside an N run is n, a gene code above 3 is n.
 * A column is IDENTICAL iff both codes are <= 3 and equal -- the rule `matches` is counted by (KP_SC_MATCH pairs).  A column with
 * an ambiguous base on either side is therefore a * token (*na, *nn, ...).  This is the one deviation from minimap2, which
 * counts N against N as identical.
 * CANONICAL FORM.  No :0; two : tokens never touch; neighbouring substituted columns give neighbouring * tokens, never merged.
 * The first and last token of a hit are : tokens, since the first and last op are M and a local path begins and ends on a match.
 * CONSISTENCY.  The : lengths sum to `matches`; the number of * tokens plus the : lengths is the sum of the M lengths; the
 * letters behind + and - number the sums of the I and of the D lengths.
 * =/X CIGAR.  Derived from the cs string: :n gives n=, a run of k * tokens kX, + and - give I and D (BAM codes 7 and 8). */
#define KP_CIGAR_EQ 7
#define KP_CIGAR_X 8

/* ---- records of the batched reduction (one assembly = one summary, its kept hits and its locus pieces) ------------------
 * They carry what SerotypingResult needs (src/kaptive/serotyping/models.py:513-536) minus strings and sequences. */
#define KP_F_EXPECTED 1u /* gene belongs to the best locus and is not an extra gene (core.py:226-228) */
#define KP_F_INSIDE 2u   /* overlaps a locus piece (core.py:273-278) */
#define KP_F_EXTRA 4u    /* gene of an "Extra genes" record */
#define KP_F_PARTIAL 8u  /* clipped by a contig edge (alignment.py:774-809) */
#define KP_F_SPURIOUS 16u /* outside the locus and below the identity threshold: dropped from the result (core.py:383) */
#define KP_F_PRIMARY 32u /* top-scoring kept hit of an expected gene (core.py:236-245) */

#define KP_STATE_NORMAL 0
#define KP_STATE_PARTIAL 1
#define KP_STATE_TRUNCATED 2
#define KP_STATE_NOVEL 3

#define KP_MAX_LOCUS_GENES 256 /* width of the missing-gene mask */

typedef struct kp_kept { /* one hit that survived the overlap cull, emission order */
    int32_t gene, contig, q_start, q_end, t_start, t_end, score;
    int32_t prot_off, prot_len; /* translated protein inside the assembly's protein buffer */
    int32_t cluster;            /* spatial cluster id */
    int32_t dp[8];              /* protein DP: score, matches, mismatches, gaps, q_start, q_end, t_start, t_end */
    float pident, coverage;     /* float32, as the reference stores them */
    int8_t strand, state;
    uint8_t flags, pad_;
} kp_kept;

typedef struct kp_piece {
    int32_t contig, start, end, strand;
    double mean_pos; /* mean expected position of the piece's primary hits; the host orders pieces by it */
} kp_piece;

typedef struct kp_asm_summary {
    int32_t n_hits, n_kept, n_final, n_pieces;
    int32_t best_locus, n_expected, n_missing;
    int32_t overflow; /* bit0 kept list, bit1 pieces, bit2 locus wider than the mask, bit3 protein buffer */
    uint64_t missing_mask[KP_MAX_LOCUS_GENES / 64]; /* bit j: gene locus_gene_off + j not found inside the locus */
    float ident_sum;   /* float32 sum of the identities of NORMAL genes, associated exactly as np.add.reduce does */
    int32_t n_normal;  /* how many; mean identity = float32(float64(ident_sum) / n_normal) (core.py:395-396) */
} kp_asm_summary;

typedef struct kp_typing_params {
    double min_gene_coverage; /* Serotyper.min_gene_coverage */
    float id_threshold;       /* np.float32(metadata.id_threshold): identities are compared as float32 */
    int32_t max_locus_length; /* Database.max_locus_length, the clustering tolerance */
    int32_t edge_tolerance;   /* Serotyper.partial_edge_tolerance */
} kp_typing_params;

/* ---- VARIANTS (optional, like the CIGAR and the cs string: no hit, no op, no kept record and no report byte depends on them) ------
 * The variant records of a KEPT hit say, in the gene's own coordinates, where the contig differs from the database's gene and
 * what a substituted base does to the codon it lies in.  They are listed for the records of the kept list only (kp_kept), never
 * for hits the overlap cull dropped.
 *
 * ONE RECORD PER cs TOKEN.  Every * token of the hit's cs string (kp_spec.h, CS) is one SNV -- a column with an n on either side
 * included: the rule `matches` and the cs string use --, every + token one DEL (the gene has bases the contig lacks, a CIGAR I
 * op), every - token one INS (the contig has bases the gene lacks, a CIGAR D op); : runs give nothing.  Bases of inserted or
 * deleted runs are not listed: the cs string has them.
 * PURE FUNCTION.  The record list of a hit is a function of its CIGAR ops and its two sequences, nothing else.
 * CODON CONSEQUENCES ARE PER VARIANT, IN ISOLATION.  ref_aa is the amino acid of codon q_pos / 3 of the gene's own forward
 * sequence (the database's gene, frame 0), alt_aa that of the same codon with this ONE base replaced: two SNVs in one codon are
 * each annotated against the unmodified reference codon.  The table is the product's (kp_fill_codon_table: NCBI 11, a codon with
 * an ambiguous base is X); a last codon cut short by a gene length that is not a multiple of 3 is X on both sides.
 * ORDER.  Within a hit the records ascend in q_pos (for strand -1 that is the reverse of the ops' order); hits come in the order
 * of the kept list, assemblies in batch order; var_off[n_asm + 1] delimits the assemblies. */
#define KP_VAR_SNV 0
#define KP_VAR_INS 1
#define KP_VAR_DEL 2
typedef struct kp_variant {
    int32_t kept;  /* index of the record in the assembly's kept list, as kp_batch_typing returns that list */
    int32_t q_pos; /* 0-based, on the gene's FORWARD strand.  SNV: the base; DEL: the first gene base that is absent; INS: the gene
                      base before which the extra bases lie on the gene's forward strand */
    int32_t t_pos; /* 0-based, on the contig's forward strand.  SNV: the base; INS: the lowest coordinate of the extra bases; DEL: the
                      first contig base above the gap in contig-forward order */
    int32_t len;   /* 1 for an SNV, the op's length for INS and DEL */
    uint8_t kind;  /* KP_VAR_SNV: one differing M column; KP_VAR_INS: a CIGAR D op; KP_VAR_DEL: a CIGAR I op */
    uint8_t ref, alt;       /* SNV only: gene-strand codes 0..3, 4 = ambiguous; ref the gene's base, alt the contig's (complemented for
                               strand -1).  0 for INS and DEL */
    uint8_t ref_aa, alt_aa; /* SNV only, ASCII (above).  0 for INS and DEL */
    uint8_t pad_[3];        /* zero */
} kp_variant;

/* ---- BREAKPOINTS (optional, like the variant records: no hit, no kept record and no report byte depends on them) ------------------
 * kp-align joins pieces across diagonal jumps of at most KP_JOIN_BW only, so a gene cut by a larger event -- an insertion
 * sequence, a long deletion, an inversion, a contig end -- is reported as two clean hits, both of which survive the overlap cull
 * (it is by target) and sit in the kept list as two records of one gene.  A breakpoint record links two such records.
 *
 * ELIGIBLE RECORDS.  The records of an assembly's kept list (kp_kept) without KP_F_SPURIOUS.
 * FRAGMENT PAIR (a, b).  a != b, same gene, q_start_a < q_start_b and q_end_a < q_end_b (a precedes b along the gene; two full
 * copies are no pair) and q_end_a - q_start_b <= KP_BP_MAX_OVERLAP.
 * DERIVED VALUES.  q_gap = q_start_b - q_end_a (negative: the fragments overlap on the gene -- a target-site duplication).  pos_a
 * is a's junction-side base, 0-based on its contig: t_end_a - 1 for strand +1, t_start_a for strand -1; pos_b is b's: t_start_b for
 * strand +1, t_end_b - 1 for strand -1.  edge_a is the number of bases from pos_a to the contig end it faces: ctg_len - t_end_a for
 * strand +1, t_start_a for strand -1; edge_b likewise: t_start_b for strand +1, ctg_len - t_end_b for strand -1.
 * KIND.  COLLINEAR: same contig, same strand and t_gap >= -KP_BP_MAX_OVERLAP, where t_gap = t_start_b - t_end_a for strand +1 and
 * t_start_a - t_end_b for strand -1.  INVERTED: same contig, strands differ.  DISORDERED: same contig, same strand, not collinear.
 * CONTIGS: different contigs.
 * ONE RECORD PER b.  Every eligible b has at most one record; its a is the candidate with the smallest key (rank, dist, kept index
 * of a): rank 0 for COLLINEAR with dist = t_gap + KP_BP_MAX_OVERLAP, rank 1 for INVERTED and DISORDERED with dist =
 * |pos_a - pos_b|, rank 2 for CONTIGS with dist = edge_a + edge_b (64 bits).  A b without a candidate has no record; one a may
 * serve several b.
 * INVERTED REPEAT.  For COLLINEAR records with t_gap >= 2 only (else both fields are 0): S is the t_gap contig bases between the
 * fragments on the contig's forward strand, ir_cols = min(KP_BP_IR_COLS, t_gap / 2), ir_matches the number of i < ir_cols for which
 * S[i] and S[t_gap - 1 - i] are both unambiguous (a base inside an N run is ambiguous) and complementary.  Chance gives about a
 * quarter of the columns, the terminal repeats of an insertion sequence most of them.
 * ORDER.  Records ascend in kept_b within an assembly; assemblies come in batch order; bp_off[n_asm + 1] delimits them.
 * PURE FUNCTION of the kept list, the contig lengths and the contig bases: no CIGAR, no option and no trace is read. */
#define KP_BP_MAX_OVERLAP 64
#define KP_BP_IR_COLS 32
#define KP_BP_COLLINEAR 0
#define KP_BP_INVERTED 1
#define KP_BP_DISORDERED 2
#define KP_BP_CONTIGS 3
typedef struct kp_breakpoint {
    int32_t kept_a, kept_b; /* indices in the assembly's kept list, as kp_batch_typing returns it */
    int32_t q_gap;
    int32_t t_gap;          /* COLLINEAR only, else 0 */
    int32_t t_lo;           /* COLLINEAR with t_gap > 0: lowest contig coordinate of S, else 0 */
    int32_t edge_a, edge_b; /* always filled */
    uint8_t kind, ir_cols, ir_matches, pad_; /* pad_ zero */
} kp_breakpoint;

/* ---- ALLELES (optional, like the variant and breakpoint records: no hit, no kept record and no report byte depends on them) -------
 * A stable 64-bit digest of every kept record's bases, of its protein and of the assembly's locus: two isolates carry the same
 * allele of a gene exactly when the digests agree (up to the collision odds below), across runs and machines.
 *
 * SEQUENCE OF AN INTERVAL.  An interval (contig, start, end, strand) has L = end - start codes x_0 .. x_{L-1}.  For strand >= 0,
 * x_p = kp_code_at(start + p); for strand < 0, x_p is the complement of kp_code_at(end - 1 - p): 3 - v for v <= 3, 4 stays 4.
 * Codes are 0..3, or 4 inside an N run.  This is the strand-corrected sequence the extraction of kp_reduce_core.h translates and
 * the one gene_seqs / locus_seqs hold on the host.
 * MIXER.  MIX(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31 (64-bit wrap-around).
 * DIGEST of a block list v_0 .. v_{B-1}, a length L and a tag: S = sum over i of MIX(MIX(i + 1) ^ v_i) mod 2^64;
 * DIGEST = MIX(S ^ MIX((tag << 56) | L)).  S is a plain sum: the blocks are independent, any lane may take any block.
 * NUCLEOTIDE DIGEST (tag 1).  Block i covers columns 16i .. 16i + 15: w_i = sum of (x < 4 ? x : 0) << 2j, m_i = sum of (x == 4) << j
 * over its columns j (columns >= L contribute nothing), v_i = w_i | (uint64)m_i << 32.
 * PROTEIN DIGEST (tag 2).  Over the record's prot_len protein bytes -- the bytes kp_batch_proteins returns for it, so a protein cut
 * at a stop is digested as cut --, eight bytes per block, little-endian, zero-padded.  A record with prot_len == 0 has protein
 * digest 0 and prints ".".
 * LOCUS DIGEST (tag 3).  Its blocks are the nucleotide digests of the assembly's locus pieces in the order the product lists them
 * (numpy's argsort of mean_pos, as kp_format_json is given it); L is the number of pieces.  An assembly without a piece has locus
 * digest 0 and prints ".".
 * PURE FUNCTION of the kept list, the pieces, the protein buffer and the contig bases: no CIGAR, no option and no trace is read.
 * Every kept record has digests, KP_F_SPURIOUS ones included; the table lists the others, as the report does.
 * NOT CRYPTOGRAPHIC.  64 bits: among n distinct alleles of a gene two collide with odds of about n^2 / 2^65, and anyone can
 * construct a collision.  The digests tell alleles apart; they authenticate nothing.
 * KNOWN ANSWERS.  Bases "" 332e6d2b1a14193e, "a" c8754b03323395a8, "acgt" 5eeccfc7d63eed1e, "acgtnacgt" 90dd01a6934ea7e4; protein
 * "M" 137859f1719b82ad, "MKLVAAAAW" 973b1ff3dad4bcac; the pieces "acgt", "tgca" eef6d079d9303a4a (more in tests/test_alleles_cpu.py).
 * OUT OF SCOPE.  Digests of the database's own genes (a "matches the reference allele" column), allele numbering within a run and
 * any change to the TSV / JSON / PHA4GE bytes. */
typedef struct kp_allele {
    uint64_t nt; /* nucleotide digest of (contig, t_start, t_end, strand) */
    uint64_t aa; /* protein digest; 0 when prot_len == 0 */
} kp_allele;

/* ---- ALIGNED ROWS (optional, like the variant records: no hit, no op, no kept record and no report byte depends on them) ----------
 * The reference-anchored alignment row of a KEPT hit: the contig's bases projected through the hit's CIGAR onto the coordinates of
 * the database's gene.  Rows of one gene from any run on any machine have the same columns and stack into a multiple alignment
 * with no further work.  Rows are made for the records of the kept list only (kp_kept), never for hits the overlap cull dropped.
 *
 * COLUMNS.  The row of a record whose gene has Lq bases has Lq columns; column j is position j of the gene's FORWARD strand.
 * VALUE OF COLUMN j.  A code 0..3: the contig base that an M column of the hit's CIGAR aligns to gene base j, on the gene's strand
 * -- complemented, 3 - v, for strand -1 --; 4: that contig position lies inside an N run; GAP: j lies outside [q_start, q_end), or
 * inside an I op (the gene has bases the contig lacks).  The contig bases of D ops (bases the gene lacks) have no column: they are
 * dropped and only counted -- `inserted` is the sum of the D lengths, `n_ins` the number of D ops.  `covered` is the number of
 * columns that are not GAP; it equals the sum of the M lengths.
 * ORIENTATION is the CIGAR's and the cs string's: for strand +1 the ops run along the gene from row q_start; for strand -1 along
 * the reverse-complemented gene from row Lq - q_end, and row r of that walk is column Lq - 1 - r of the gene's forward strand.  The
 * contig is walked forward from t_start either way.  An op of a kind other than M, I and D moves nothing.
 * PACKED FORM.  Sixteen columns make a block; block b holds columns 16 b .. 16 b + 15.  It is the ALLELES block plus a gap mask:
 * v = w | (uint64)m << 32 | (uint64)g << 48, where w holds the 2-bit codes (column c in bits 2c, 2c + 1; 0 where m or g is set),
 * m has bit c set for code 4 and g has bit c set for GAP.  Columns at or beyond Lq contribute nothing to any of the three.  A row
 * has (Lq + 15) / 16 blocks.
 * PURE FUNCTION of the record's span and strand, the ops of the hit behind it and the contig's bases.  The gene's own bases are
 * not read: a column says what the contig holds, not whether it agrees with the gene.
 * INVALID WALK.  A record whose hit is not found in the finished hit table, or whose ops would leave the gene or the contig -- with
 * R the sum of the M and I lengths and C that of the M and D lengths: q0 < 0, q0 + R > Lq, t_start < 0 or t_start + C beyond the
 * contig's end, q0 being the walk's first row; the check the variant records make -- has a row of all GAP, and covered = inserted
 * = n_ins = 0.
 * WHICH RECORDS.  Every kept record has a row, KP_F_SPURIOUS ones included; the table lists the others, as the report does.
 * ORDER.  Rows follow the kept list, assemblies the batch; `off` is the row's first block in the batch's block array, and the
 * rows lie in it back to back in that order.
 * KNOWN ANSWERS.  Contig "ttacgtnacgga", gene of 20 bases, record q_start 2, q_end 12, t_start 2, ops 4M 2I 3M 1D 1M.  Strand +1:
 * "--acgt--nacg--------", blocks f0c3010000900e40 000f000000000000, covered 8, inserted 1, n_ins 1.  Strand -1 (the same ops, now
 * along the reverse complement from row 8): "--cgtn--acgt--------", blocks f0c3002000e40390 000f000000000000, the same counts.
 * OUT OF SCOPE.  Merging two fragments of one gene into one row; the dropped insertion bases (the cs string has them); codon or
 * protein alignments; per-gene output files; any change to the TSV / JSON / PHA4GE bytes. */
typedef struct kp_aligned_row {
    int64_t off;      /* first block of the row in the batch's block array */
    int32_t gene_len; /* Lq */
    int32_t covered, inserted, n_ins;
} kp_aligned_row;

/* ---- RESCUE (optional, like the reports above: no hit, no kept record and no report byte depends on it) ---------------------------
 * A gene of the best-match locus is listed as missing when no nucleotide seed landed in it -- because it is absent, or because it
 * has drifted below the 75-80 % nucleotide identity a (10, 15) minimizer needs.  The rescue records tell the two apart: every
 * missing gene's database protein is aligned against the six-frame translation of the contig windows around the locus pieces.
 *
 * SUBJECTS.  The genes of an assembly whose bit is set in kp_asm_summary.missing_mask after a finished reduction (bit j: gene
 * locus_gene_off[best_locus] + j), in ascending gene order: one record each.  An assembly whose summary has overflow bit 2 (locus
 * wider than the mask) has none.  rescue_off[n_asm + 1] delimits the assemblies.
 * WINDOWS.  Every piece p of the assembly (kp_piece, in the order kp_batch_typing returns them) gives one window on the piece's
 * contig: ws = max(0, start - F), we = min(ctg_len, end + F), F the option rescue_flank (default KP_RESCUE_FLANK: a design constant,
 * longer than nearly every gene, so that a gene just outside the bounding box of the primary hits still lies in the window).  An
 * assembly without a piece has no window.
 * FRAME TEXT.  For strand s in (+, -) and frame f in (0, 1, 2) the frame text has A = max(0, (we - ws - f) / 3) residues.  Forward,
 * residue a is the codon of contig bases ws + f + 3a .. + 2; reverse, the codon of the complements of bases we - 1 - f - 3a,
 * we - 2 - f - 3a, we - 3 - f - 3a.  The table is the product's (kp_fill_codon_table: NCBI 11); a codon with a base inside an N run
 * is X, stops are *, nothing is cut at a stop.  Byte for byte the reference's translate(extract(window, strand), frame f,
 * to_stop = False) (src/kaptive/core/seq.py:612-741).
 * ALIGNMENT.  Rows i run over the frame text (the reference's query: the assembly side), columns j over the database protein as
 * stored, its trailing * included.  The arithmetic is the reference's _batched_banded_gotoh (src/kaptive/core/pairwise.py:395-584)
 * with a band that covers the whole rectangle -- seeded mode, offset 0, k >= A + protein length --: BLOSUM62 through the 256 x 256
 * lookup, gap open KP_PROT_GAP_OPEN, extend KP_PROT_GAP_EXT, opening a gap beats extending one, the diagonal beats D beats I, a cell
 * with best <= 0 restarts the path, the reported cell is the first maximum in row-major order and the path counts are those of the
 * reference's traceback.  Scores are int32.  The eight values: score, matches, mismatches, gaps, a0, a1 (frame text, half-open),
 * p0, p1 (protein, half-open).
 * BEST OF A SUBJECT.  The maximum score over its tasks; task index = (piece * 2 + (strand < 0)) * 3 + f; ties go to the lowest
 * task index.  Score 0 means nothing: the record then has piece = -1 and every other field 0 except gene.
 * DERIVED FIELDS.  Forward: t_start = ws + f + 3 a0, t_end = ws + f + 3 a1; reverse: t_start = we - f - 3 a1, t_end = we - f - 3 a0;
 * both 0-based and half-open on the contig's forward strand.  stops = number of * in the frame text at [a0, a1) -- the gene's own
 * stop included where the alignment reaches the protein's trailing * (its last column is then * against *: nothing else scores
 * positive against *); the table does not count that one as an interruption.  edge bit 0:
 * t_start <= tol; bit 1: t_end >= ctg_len - tol; tol = kp_typing_params.edge_tolerance of the reduction.
 * PURE FUNCTION of the summaries, the pieces, the contig lengths, the packed contigs, the database proteins and the two options
 * (rescue_flank, edge_tolerance): no hit, no CIGAR and no trace is read.
 * NOT DONE.  A gene on a contig that holds no piece of the locus is not looked for.  A frameshifted gene is two alignments in two
 * frames: the better one is reported, as a fragment.  Completeness, confidence and every other column of the reports stay as they are.
 *
 * KP_RESCUE_MIN_SCORE, the table's default threshold between `absent` and a call, is a default, not a measurement: with BLAST's
 * published gapped parameters for BLOSUM62 11/1 (lambda 0.267, K 0.041), a 330-residue protein against six frames of a 43 kb window
 * is m n = 330 x 6 x 14 300 = 2.8e7 cell pairs, and E = K m n exp(-lambda S) = 0.041 x 2.8e7 x exp(-0.267 x 80) = 6e-4 at S = 80.  The
 * raw score is always in the table. */
#define KP_RESCUE_FLANK 4096
#define KP_RESCUE_FLANK_MAX 65535
#define KP_RESCUE_MIN_SCORE 80
typedef struct kp_rescue {
    int32_t gene;             /* index of the subject, as kp_kept.gene counts genes */
    int32_t piece;            /* index of the winning window's piece, as kp_batch_typing returns the pieces; -1: nothing found */
    int32_t contig;           /* contig index within the assembly */
    int32_t t_start, t_end;   /* on the contig's forward strand, 0-based half-open */
    int32_t score, matches, mismatches, gaps;
    int32_t p_start, p_end;   /* on the database protein, 0-based half-open */
    int32_t stops;            /* stop codons inside the aligned stretch of the frame text */
    int32_t a_len;            /* A: residues of the winning frame text */
    int8_t strand;            /* +1 / -1; 0 when nothing was found */
    uint8_t frame;            /* 0..2 */
    uint8_t edge;             /* bit 0: the alignment starts at the contig's start, bit 1: it ends at the contig's end */
    uint8_t pad_;             /* zero */
} kp_rescue;

/* ---- DISTANCES (optional; the first report about PAIRS of assemblies: no hit, no kept record and no report byte depends on it) -----
 * How many bases apart are the loci of two isolates that carry the same locus?  The aligned rows already put every isolate's genes
 * on the database's coordinates; a LOCUS ROW strings the rows of one locus's genes together, and a pair of locus rows reduces to
 * three counts.
 *
 * LOCUS ROW.  One per assembly and database.  It covers the genes of the assembly's best locus, locus_gene_off[best] .. +
 * locus_gene_len[best], in database order; gene g contributes (Lq + 15) / 16 blocks in the ALIGNED ROWS packed form, back to back.
 * Its blocks are those of the aligned row of the gene's kept record that carries KP_F_PRIMARY -- there is at most one per expected
 * gene --; without such a record the gene's blocks are all GAP.  Other kept records of the gene (fragments, copies outside the
 * locus) contribute nothing.
 * PADDING.  The columns at or beyond Lq in a gene's last block have their GAP bit set in a locus row.  This is the one difference
 * from the ALIGNED ROWS block format, where those columns carry no bit at all -- left that way they would read as base a on both
 * sides of a pair.  All locus rows of one locus have the same number of blocks, NB.
 * COUNTS of a pair (a, b), a < b, rows of the same locus, over all 16 NB columns.  compared: columns where both rows hold a code
 * 0..3 (neither GAP nor N).  differences: compared columns whose codes differ.  unshared: columns where exactly one row is GAP --
 * gene content present in one isolate and absent, or not aligned, in the other.  N against anything is neither compared nor
 * unshared; GAP against GAP (padding against padding included) is neither.  All three are int32: a locus of 16 NB >= 2^31 columns
 * is refused.
 * LISTED PAIRS.  A pair is listed iff differences <= max_diff and compared >= min_compared; max_diff = INT32_MAX with
 * min_compared = 0 lists every pair.  Listed pairs ascend in (a, b); the order depends on nothing else -- not on the tile shape,
 * not on scheduling.
 * KNOWN ANSWERS, on the two known-answer rows of ALIGNED ROWS (a gene of 20 bases).  "--acgt--nacg--------" against
 * "--cgtn--acgt--------": compared 6, differences 6, unshared 0.  Either against the all-GAP row: compared 0, differences 0,
 * unshared 8.  With the padding flagged the second block's gap mask is ffff, not 000f.
 * KP_DIST_MAX_DIFF and KP_DIST_MIN_COMPARED, the command line's defaults, are design constants like KP_RESCUE_FLANK, not
 * measurements: ten differences in a 25 kb locus is 0.04 %, well inside one outbreak and well below two variants of a locus; one
 * compared column keeps pairs of empty rows out of the table.
 * OUT OF SCOPE.  Merging fragments of one gene; distances between isolates of different loci or different databases; indel events
 * as events (an inserted run counts through `unshared` only); any change to an existing report byte.  (Clusters: CLUSTERS, a
 * minimum spanning tree: TREE, a neighbour-joining tree with inferred inner nodes: NJ, all below.) */
#define KP_DIST_MAX_DIFF 10
#define KP_DIST_MIN_COMPARED 1
typedef struct kp_dist_pair {
    int32_t a, b; /* rows of the matrix, a < b */
    int32_t compared, differences, unshared;
    int32_t pad_; /* zero */
} kp_dist_pair;

/* ---- CLUSTERS (optional; two reductions over the pairs of DISTANCES: no pair record, no report byte depends on them) --------------
 * Which isolates belong together at a threshold, and which isolate is closest to each?  Both are reductions over all pairs of one
 * matrix of locus rows; no pair is ever listed for them, so they work where the listing cannot be held.
 *
 * LEVELS.  K thresholds T_0 < T_1 < ... < T_{K-1}, all >= 0, 0 <= K <= KP_CLUST_MAX_LEVELS.  The command line's default is
 * 0, 1, 2, 5, 10: design constants, as KP_DIST_MAX_DIFF is.
 * EDGE.  A pair (a, b) of rows of one matrix is an edge at level k iff compared >= min_compared and differences <= T_k -- the
 * DISTANCES counts, and the DISTANCES listing predicate with max_diff = T_k.
 * CLUSTER.  The clusters at level k are the connected components of the rows under the level's edges (single linkage).  The LABEL
 * of a row at level k is the smallest row index of its component.  Levels nest: rows with equal labels at level k have equal
 * labels at every level above it.
 * NEAREST.  For row r, among all rows s != r with compared(r, s) >= min_compared the one with the smallest key (differences, s).
 * The record holds s and the three counts of the pair; a row without such an s has s = -1 and counts 0.  Nearest does not depend
 * on the levels: it also sees pairs far beyond every threshold.
 * PURE FUNCTION of the matrix, the levels and min_compared.  Neither labels nor nearest depend on the tile shape, on scheduling or
 * on the order in which edges are met.
 * CLUSTER NUMBER, in the table: the 1-based rank of a row's label among the labels of its level, ascending.  Numbers are ranks
 * within the run.
 * KNOWN ANSWERS, on the three rows of the DISTANCES known answers: A "--acgt--nacg--------" is row 0, B "--cgtn--acgt--------"
 * row 1, C, all GAP, row 2; levels (0, 6).  min_compared = 1: labels 0, 1, 2 at level 0 and 0, 0, 2 at level 6; nearest A -> (1;
 * compared 6, differences 6, unshared 0), B -> (0; 6, 6, 0), C -> none.  min_compared = 0: labels 0, 0, 0 at both levels; nearest
 * A -> 2, B -> 2, C -> 0, each with counts (0, 0, 8) -- the empty row is 0 differences from everything and links A to B, which is
 * the reason for the default of 1.
 * OUT OF SCOPE.  Any linkage other than single (the minimum spanning tree of the same edges: TREE, a neighbour-joining tree with
 * inferred inner nodes: NJ, both below); cluster names that are stable across runs; a threshold on `unshared`; merging fragments of
 * a split gene; any change to an existing report byte. */
#define KP_CLUST_MAX_LEVELS 8
typedef struct kp_dist_nearest { int32_t row, compared, differences, unshared; } kp_dist_nearest;  /* 16 bytes */

/* ---- TREE (optional; a third reduction over the pairs of DISTANCES: no pair record, no report byte depends on it) ------------------
 * Who links to whom inside a cluster, and in what order do the links form?  The minimum spanning forest of one matrix of locus rows
 * answers both, and it is the single-linkage dendrogram at every threshold at once.
 *
 * GRAPH.  The vertices are the rows of one matrix of locus rows.  A pair (a, b), a < b, is an edge iff compared >= min_compared --
 * the CLUSTERS edge rule without a threshold.
 * KEY.  An edge's key is (differences, a, b), compared lexicographically.  The key is a strict total order, so the minimum spanning
 * forest under it is unique: a PURE FUNCTION of the matrix and min_compared, which depends neither on the tile shape, nor on
 * scheduling, nor on the order in which edges are met.
 * FOREST.  Its edges are n_rows - n_components records of kp_dist_pair -- a, b and the pair's three counts --, ascending by key.
 * component[r] is the smallest row of r's tree.
 * PROPERTIES.  (1) For every T, the connected components of the forest's edges with differences <= T are the CLUSTERS labels at
 * level T with the same min_compared.  (2) Every row's NEAREST pair is an edge of the forest: among partners at equal differences
 * the smaller row wins under both keys.
 * PACKED KEY.  differences << 36 | a << 18 | b in 64 bits, ordered as the tuple: rows are below KP_DIST_MAX_ROWS = 2^18, and the
 * differences fit 28 bits when 16 * n_blocks < 2^28 (KP_TREE_MAX_COLUMNS, kp_caps.h).  A matrix beyond that is refused by the tree
 * alone.  All ones is "no edge": a < b keeps every key below it.
 * ROUNDS.  The forest is built by Boruvka's rounds: every component takes its lightest outgoing edge.  The components that still
 * have one at least halve each round, so ceil(log2(max(n_rows, 2))) + 1 rounds, the last of them empty, always suffice.
 * KNOWN ANSWERS, on the three rows of the DISTANCES known answers (A is row 0, B row 1, C, all GAP, row 2).  min_compared = 1: one
 * edge (0, 1; compared 6, differences 6, unshared 0), components 0, 0, 2.  min_compared = 0: edges (0, 2; 0, 0, 8) and (1, 2; 0, 0,
 * 8) in that order, components 0, 0, 0.
 * NEWICK (host only).  One tree per component, rooted at the component's smallest row.  Every node, inner ones included, is
 * labelled with its assembly's name; a node's children are its tree neighbours away from the root, ascending by (differences,
 * row); the branch length is the integer `differences`.  A node with children is written (child:len,child:len)name, a leaf name,
 * and the tree ends in ;.  A name is written bare when every byte is in A-Za-z0-9_.- and otherwise in single quotes with every '
 * doubled.  The known answers: (B:6)A; and C; with min_compared = 1, ((B:0)C:0)A; with 0.
 * OUT OF SCOPE.  Any linkage other than single; inferred inner nodes (the neighbour-joining tree of the same rows: NJ, below);
 * names that are stable across runs; any change to an existing report byte. */

/* ---- SITES (optional; a reduction over the COLUMNS of a DISTANCES matrix: no pair, no pair record, no report byte depends on it) ------
 * Where do the isolates of one locus differ, how many of them carry each base there, and what is the alignment of those columns
 * alone?  The pair reports answer "how far apart"; this one answers "where".  It reads the same matrix of locus rows, column by
 * column over all rows.
 *
 * PROFILE.  For a matrix of R locus rows of NB blocks (DISTANCES, LOCUS ROW, padding flagged) and a column c in [0, 16 NB): n[k] is
 * the number of rows whose code at c is k, k = 0..3; n_n the number of rows that hold an N there; gap = R - n[0] - n[1] - n[2] -
 * n[3] - n_n.
 * SITE.  Column c is a site iff at least two of n[0..3] are non-zero.  With the flag KP_SITES_CORE it must also have n_n == 0 and
 * gap == 0: every row holds a base.  A padding column is GAP in every row and is therefore never a site.  Sites ascend in column;
 * the order depends on nothing else -- not on the slab shape, not on scheduling.
 * RECORD.  kp_site: column, n[4], n_n -- 24 bytes, three 8-byte words, stored as a kp_dist_pair is.
 * DERIVED.  ALLELES: the number of non-zero n[k].  MAJOR: the smallest k among those with the largest n[k].  INFORMATIVE: at least
 * two k have n[k] >= 2.
 * SITE ROWS.  Row r's site row holds its codes at the S listed sites, in order, in the ALIGNED ROWS packed form: (S + 15) / 16
 * blocks, the columns at or beyond S GAP-flagged as LOCUS ROW padding is; S = 0 gives rows of 0 blocks.  A site matrix is therefore
 * itself a valid DISTANCES matrix.
 * PROPERTY.  Without KP_SITES_CORE every pair (a, b) has the same `differences` over the site matrix as over the full matrix: a
 * column in which a and b hold different bases is a site.
 * PURE FUNCTION of the matrix and the flag: the counts are integer sums, which no order of addition changes.
 * KNOWN ANSWERS, on the three rows of the DISTANCES known answers: A "--acgt--nacg--------", B "--cgtn--acgt--------", C all GAP.
 * The sites are the 0-based columns 2, 3, 4, 9, 10, 11; columns 5 and 8 hold one base and an N and are not sites.  Column 2 has n =
 * (1, 1, 0, 0), n_n = 0, gap 1, ALLELES 2, MAJOR a (the tie goes to the first) and is not informative.  The site rows are "acgacg",
 * "cgtcgt" and "------": blocks ffc0000000000924, ffc0000000000e79 and ffff000000000000.  With KP_SITES_CORE there are no sites;
 * for rows A and B alone it gives the same six.
 * OUT OF SCOPE.  Indel events as characters; sites between isolates of different loci; merging fragments of a split gene;
 * ambiguity codes; any change to an existing report byte. */
#define KP_SITES_CORE 1 /* flag: a site must hold a base in every row */
typedef struct kp_site {
    int32_t column; /* of the matrix, 0-based, padding columns counted */
    int32_t n[4];   /* rows that hold a, c, g, t there */
    int32_t n_n;    /* rows that hold an N there */
} kp_site;

/* ---- NJ (optional; a fourth reduction over the pairs of DISTANCES, and the first in floating point: no report byte depends on it) ----
 * How are the isolates of one locus related when they are not one outbreak?  The minimum spanning tree puts assemblies on inner
 * nodes; between lineages the neighbour-joining tree, whose inner nodes are inferred, is the usual picture.  Its update halves
 * distances at every join, so it cannot stay in integers: this section fixes every operation and its order instead, and the tree is
 * still a PURE FUNCTION of the matrix and min_compared -- the same bytes from the device, from kp_nj.h under g++ and from NumPy.
 *
 * TAXA.  For a matrix of R locus rows of NB blocks: W = 16 NB (padding columns counted); bases(r) the number of columns in which row
 * r holds a code 0..3 (the popcount of its `valid` plane); m0 = max(min_compared, 1).  Row r is a taxon iff 2 bases(r) >= W + m0.
 * Taxa are numbered 0 .. n - 1 in ascending row order.  The reason for the rule: two taxa a, b hold bases in bases(a) + bases(b)
 * columns of W, so by pigeonhole compared(a, b) >= bases(a) + bases(b) - W >= m0 -- every pair of taxa has a distance, and no pair
 * needs a check.  Rows that are not taxa are left out of the tree: an isolate with under half of the locus has no place in it.
 * DISTANCE.  d(a, b) = (double)differences / (double)compared, the p-distance, in IEEE binary64 with one correctly rounded division;
 * d(a, a) = +0.0.
 * SUM64(v[0 .. m)).  64 partial sums S_l, each the left fold from +0.0 of v[k] over k = l (mod 64), ascending; then for o = 32, 16,
 * 8, 4, 2, 1: S_l = S_l + S_{l+o} for l < o.  The result is S_0.  (One wavefront's strided adds and xor shuffles.)
 * STATE.  Slots 0 .. m - 1, always dense.  node[slot] is a node id: taxa are 0 .. n - 1, inner nodes n, n + 1, ... in the order they
 * are made.  Initially m = n, slot k holds taxon k and R_k = SUM64(d(k, .)).
 * JOIN, while m > 3.  With f = (double)(m - 2); every operation below is rounded to binary64 and none is fused into a multiply-add.
 *   Q(a, b) = ((f * d(a, b)) - R_a) - R_b for slots a < b; the pair (i, j) is the minimum of (Q, a, b), compared lexicographically.
 *   delta = (R_i - R_j) / f;  L_i = 0.5 * (d(i, j) + delta);  L_j = d(i, j) - L_i.  Emit (node[i], node[j], -1; L_i, L_j, 0).
 *   For every slot k other than i, j:  u_k = 0.5 * ((d(i, k) + d(j, k)) - d(i, j));  R_k = ((R_k - d(i, k)) - d(j, k)) + u_k.
 *   Slot i becomes the new node: d(i, k) = u_k, d(i, i) = 0.  If j != m - 1 the node in slot m - 1 moves to slot j with its row,
 *   its column and its R.  m becomes m - 1.  R_i = SUM64 over the slots 0 .. m - 1 of row i.
 * END.  With m = 3 and the slots as x, y, z = 0, 1, 2, emit (node[0], node[1], node[2]; l_x, l_y, l_z) with l_x = 0.5 * ((d_xy +
 * d_xz) - d_yz), l_y = 0.5 * ((d_xy + d_yz) - d_xz), l_z = 0.5 * ((d_xz + d_yz) - d_xy).  n = 3 gives this record only; n = 2 the
 * one record (0, 1, -1; 0.5 d, 0.5 d, 0); n <= 1 none; otherwise there are n - 2 records.  Negative lengths are left as they come.
 * RECORD.  kp_nj_node: a, b, c, pad_; la, lb, lc -- 40 bytes; c = -1 and lc = +0.0 for a binary join, pad_ zero.
 * KNOWN ANSWERS, on the level of a distance matrix (kp_nj_host).  The rows (0 5 9 9 8), (5 0 10 10 9), (9 10 0 8 7), (9 10 8 0 3),
 * (8 9 7 3 0) give (0, 1, -1; 2, 3, 0), (5, 2, -1; 3, 4, 0), (6, 4, 3; 2, 1, 2): the second join is a tie of Q = -28 between slots
 * (0, 2) and (1, 3), and the slot order decides it.  Six taxa with all distances 0 give (0, 1, -1), (6, 5, -1), (7, 4, -1), (8, 3, 2)
 * with every length 0: every choice is a tie, and every move of the last slot shows.
 * NEWICK (host only).  The tree is unrooted and written from the last record: (X:lx,Y:ly,Z:lz); -- a binary last record, which only
 * n = 2 gives, (A:l,B:l);.  An inner node is written (A:la,B:lb), unnamed, its children in record order; a leaf is its assembly's
 * name under the quoting rule of TREE's NEWICK.  Lengths are printed with %.9g.  The first known answer with the names a .. e:
 * (((a:2,b:3):3,c:4):2,e:1,d:2);
 * LIMIT.  KP_NJ_MAX_TAXA = 16384 (kp_caps.h): the dense matrix is n * n doubles, 2 GiB at the limit.  A matrix with more taxa is
 * refused by this call alone, after the taxa are counted and before anything large is allocated.
 * OUT OF SCOPE.  Any distance correction (JC69 and the like); rooting; clamping of negative lengths; BIONJ or FastME;
 * merging fragments of a split gene; trees across loci; any change to an existing report byte.  (Support values: BOOTSTRAP, below.) */
typedef struct kp_nj_node {
    int32_t a, b, c;   /* node ids: taxa 0 .. n - 1, inner nodes from n on; c = -1 for a binary join */
    int32_t pad_;      /* zero */
    double la, lb, lc; /* their branch lengths; lc = +0.0 for a binary join */
} kp_nj_node;

/* ---- BOOTSTRAP (optional; support values for the tree of NJ: no byte of NJ or of any other report depends on it) ----
 * Which inner branches of the neighbour-joining tree mean anything?  A replicate resamples the columns of the matrix with
 * replacement, its tree is NJ's tree of the resampled matrix, and the support of a branch is the number of replicates whose tree has
 * it.  Everything below is fixed, so the same rows, min_compared, seed and number of replicates give the same bytes on any run, on
 * any device and under any batching: the tree of a replicate is a PURE FUNCTION of the matrix, min_compared, the seed and the
 * replicate's number (kp_boot.h holds the arithmetic once, for the kernels and for g++).
 *
 * MIX(x), all of it mod 2^64:  z = x + 0x9e3779b97f4a7c15;  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) *
 * 0x94d049bb133111eb;  MIX = z ^ (z >> 31).
 * DRAWS.  A matrix of NB blocks has W = 16 NB block columns, padding columns included: no row holds a base in a padding column, so
 * a draw that lands on one adds nothing to any count.  Replicate r (0-based) makes W draws; draw t, 0 <= t < W, is column
 * MULHI64(MIX(MIX(MIX(seed) + r) + t), W), MULHI64 the high 64 bits of the 128-bit product -- below W always.  weight[c] =
 * min(number of draws of c, 255): the clamp does not depend on the order of the draws, and is never reached in practice (a column
 * drawn 256 times out of W >= 16 draws of W columns).
 * WEIGHTED COUNTS.  compared_w(a, b) = sum over c of weight[c] * [both rows hold a base at c]; differences_w(a, b) = sum over c of
 * weight[c] * [both hold a base and the bases differ].  Integers; both are at most the sum of the weights, W, and fit an int32: a
 * matrix of KP_TREE_MAX_COLUMNS = 2^28 columns or more is refused.  The distance is NJ's DISTANCE of (differences_w, compared_w),
 * unchanged, with its rule that a pair without a compared column is 0 apart: a replicate can draw such a pair -- the taxon rule
 * speaks of the unweighted rows and does not exclude it.
 * TAXA.  Those of NJ, from the unweighted rows.  Weights do not move them: every replicate tree has the taxa of the tree it supports.
 * TREE.  The tree of a replicate is NJ's tree of its weighted matrix, every rule unchanged: Q, the order of the pick, the lengths, the
 * update, SUM64 and the slot moves.
 * SPLITS.  For n >= 4 taxa, record t < n - 3 of a tree made node n + t; its split is the set of taxa below that node, taken on the
 * side without taxon 0.  These are the tree's n - 3 inner edges; the last record has none, and trees of 2 or 3 taxa have none.  Two
 * splits are equal when the sets are equal.  The device compares the pair (size, key) instead of the sets: key is the sum mod 2^64
 * of MIX(k + 1) over the taxa k of the set; the other side of a split has size n - size and key total - key, total the key of all
 * taxa.  Different sets of one size with one key would be counted as equal, which can only over-count: for keys that behave as
 * random words that happens with probability at most pairs-compared * 2^-64, pairs-compared <= replicates * (n - 3)^2 < 2^42.
 * SUPPORT.  support[t] of record t of the supported tree is the number of replicates, 0 .. N, whose tree holds record t's split; -1
 * for a record without an inner edge.  A count, not a percentage: nothing is rounded.
 * NEWICK (host only).  NJ's text byte for byte, but the closing parenthesis of the node of record t < n - 3 is followed by support[t]
 * as a decimal integer -- (A:0.1,B:0.2)87:0.05 --; the outermost node has no label.  The line has the column Replicates before the
 * Newick text.
 * LIMITS.  KP_BOOT_MAX_REPLICATES = 10000 replicates a call; KP_NJ_MAX_TAXA taxa, as NJ.  Replicates are joined in batches of the
 * largest b with b * n * n * 8 <= KP_BOOT_MATRIX_BYTES = 2 GiB (kp_caps.h), and no result depends on b.
 * OUT OF SCOPE.  Percentages; a consensus tree; resampling of real columns only, of sites only, or by gene; support for the minimum
 * spanning tree; anything NJ leaves out.  (Support that does not collapse on deep branches: TRANSFER, below.) */

/* ---- TRANSFER (optional; transfer support for the tree of NJ from BOOTSTRAP's replicates: no byte of NJ, of BOOTSTRAP or of any other
 * report depends on it) ----
 * BOOTSTRAP's support counts the replicates that hold EXACTLY a branch's split.  In a tree of a thousand taxa one isolate that hops
 * across a deep branch makes the replicate count as "branch absent", however well the rest agrees.  The transfer bootstrap
 * expectation (Lemoine et al., Nature 2018) asks instead how many taxa would have to move for the replicate to hold the branch, and
 * averages that.  The replicates are BOOTSTRAP's -- its draws, weights, counts, taxa and trees, unchanged --; this section fixes the
 * comparison.  Everything is integer arithmetic: no floating point appears before the label is printed.
 *
 * SETS.  For n >= 4 taxa, record t < n - 3 of a tree has the split A_t of BOOTSTRAP's SPLITS: the set of taxa below node n + t, on
 * the side without taxon 0.  s = |A_t|; its DEPTH is p_t = min(s, n - s), and p_t >= 2: a node has two taxa below it at least, and
 * the last record leaves two outside it.
 * DISTANCE OF TWO SPLITS.  For a split B of a replicate's tree: H = |A xor B| = |A| + |B| - 2 |A and B|, and delta(A, B) = min(H,
 * n - H) -- n - H is H taken from B's other side, so delta does not depend on the side either split is written on.
 * TRANSFER DISTANCE.  phi_r(t) = min(p_t - 1, min over the n - 3 splits B of replicate r's tree of delta(A_t, B)).  The bound
 * p_t - 1 is what the replicate's leaf branches contribute: a leaf's split is one taxon against the rest, and for a leaf k on the
 * light side of A_t, H = p_t - 1 from that side -- every other taxon of the light side moves.  No leaf does better, and every tree
 * has all the leaves, so the leaves need no pass of their own: the minimum starts at p_t - 1.
 * OUTPUT.  transfer[t] = sum over the replicates r of phi_r(t), in 64 bits; -1 for a record without an inner edge, exactly where
 * support[t] is -1.
 * SUPPORT RELATION.  support[t] as BOOTSTRAP defines it is the number of r with phi_r(t) = 0: delta is 0 for the same split only.
 * This section's call computes it so, on exact sets, where it cannot over-count as the comparison of keys can; BOOTSTRAP's own path
 * and its bytes are untouched.
 * LABEL (host only).  D = replicates * (p_t - 1) and K = floor((2000 * (D - transfer[t]) + D) / (2 * D)), in 64-bit integers: the
 * transfer support 1 - transfer[t] / D, rounded half up to thousandths.  The label is K / 1000 written with exactly three decimals,
 * 0.000 .. 1.000, behind the closing parenthesis where BOOTSTRAP's NEWICK puts its count -- (A:0.1,B:0.2)0.934:0.05 --, and the
 * line and its five columns are otherwise BOOTSTRAP's.  A label always contains a '.', and a count of BOOTSTRAP never does.
 * KNOWN ANSWER.  Six taxa.  The supported tree (0, 1, -1), (6, 2, -1), (7, 3, -1), (8, 4, 5) has the splits {2,3,4,5}, {3,4,5},
 * {4,5} with depths 2, 3, 2; one replicate's tree (0, 3, -1), (6, 1, -1), (7, 2, -1), (8, 4, 5) has {1,2,4,5}, {2,4,5}, {4,5}.
 * phi = (1, 1, 0): {2,3,4,5} is 2 from {1,2,4,5}, 1 from {2,4,5} and capped at 1; {3,4,5} is 3, 2 and 1 from the three.  support =
 * (0, 0, 1, -1), transfer = (1, 1, 0, -1), and with the one replicate the labels are 0.000, 0.500, 1.000: the middle branch is one
 * that BOOTSTRAP calls absent and this section calls half there.
 * LIMITS.  BOOTSTRAP's.  The taxa below a node are counted in 16 bits: KP_NJ_MAX_TAXA = 16384 (kp_caps.h asserts it).  D is below
 * 10000 * 8191 < 2^27 and the label's numerator below 2^39.
 * OUT OF SCOPE.  The transfer SET (which taxa move; lists of rogue taxa); percentages; a consensus tree; any change to a byte of
 * --nj or of --nj-bootstrap without the new flag. */

/* ---- PARSIMONY (optional; the columns of SITES' matrix put on the tree of NJ: no byte of NJ, of SITES or of any other report depends
 * on it) ----
 * SITES says at which columns the isolates of a locus differ, NJ how they are related.  This section says on which branch of the
 * tree a base changed, and which columns the tree cannot explain with one change for every further base: Fitch's small parsimony,
 * in Hartigan's form for the one node of three children, of every column of the matrix on the record list of NJ.  Everything is
 * set and integer arithmetic, 64 columns to a machine word on the planes of DISTANCES.
 *
 * TREE.  The records of NJ for the same matrix and min_compared: n taxa, node n + t made by record t.  The last record is the TOP
 * node: of three children for n >= 3, of two for n = 2.  It is where the joins ended, NOT A ROOT in the biological sense: nothing
 * below says which end of a branch is older.  Fewer than two taxa: no record, nothing to report.
 * LEAF SET of taxon k at column c of [0, 64 NW), NW = ceil(NB / 4) -- padding columns included, and the columns at or beyond 16 NB
 * of the last plane word, which no row holds: {code} where the row holds a base (its `valid` plane is set), {a, c, g, t} otherwise:
 * N and GAP are missing data.
 * UP-PASS, records ascending.  For a node with the children's sets X, Y [, Z]: K(s) is the number of children whose set holds s, M
 * the largest K; the node's set is {s : K(s) = M}, and the column's STEPS grow by (children - M).  For two children this is Fitch's
 * rule: the intersection if it is not empty, otherwise the union and one step.
 * DOWN-PASS, records descending.  The top node's STATE is the smallest code in its set.  A child's state is its parent's state if
 * the child's set holds it, otherwise the smallest code in the child's set.  A leaf without a base therefore takes its parent's
 * state and carries no change.
 * CHANGE.  Branch (parent, child) changes at column c iff the two states differ; `from` is the parent's state, `to` the child's:
 * read from the last join, not from a root.
 * ALLELES of a column: bit k is set iff some taxon holds base k there.
 * PROPERTIES.  The changes of a column number exactly its steps.  steps is the minimum over all assignments of states to the inner
 * nodes and does not depend on which record is last.  steps >= alleles - 1, counting the bits; steps = 0 iff at most one bit is
 * set.  A leaf's state is its base wherever it holds one.  EXCESS = steps - (alleles - 1) is the homoplasy of the column: changes
 * the tree needs beyond one for every further base.
 * RECORDS, two 8-byte words each.  kp_pars_site: column, steps, alleles, pad_ -- one per column with steps >= 1, ascending by
 * column.  kp_pars_change: column, node (the child end), parent, from, to, pad_ -- ascending by (node, column).
 * PURE FUNCTION of the matrix, min_compared and the records: not of a launch shape, not of scheduling.
 * KNOWN ANSWERS, on the tree of NJ's first known answer: five taxa, (0, 1, -1), (5, 2, -1), (6, 4, 3), node 7 the top.  A column
 * is written as the taxa's bases in order.
 *   "aaaaa": no step, no record.
 *   "ccaaa": node 5 {c}, node 6 {a, c} with a step, the top {a}.  steps 1, alleles a and c (3), excess 0; one change, node 5 under
 *            6, a to c.
 *   "gagaa": node 5 {a, g} with a step, node 6 {g}, the top {a} with a step (two of three).  steps 2, alleles 5, excess 1; the
 *            changes node 1 under 5, g to a, and node 6 under 7, a to g.
 *   "ccctg": the top's children hold {c}, {g}, {t}: a tie of three, the set {c, g, t}, two steps, and the smallest code, c, is the
 *            state.  steps 2, alleles 14, excess 0; the changes node 3 under 7, c to t, and node 4 under 7, c to g.
 *   "ccnaa": taxon 2 holds no base: node 6 is {c} and not {a, c}.  steps 1, alleles 3; one change, node 6 under 7, a to c -- taxon
 *            2 takes c from its parent and carries none.
 * LIMITS.  KP_NJ_MAX_TAXA taxa, as NJ: a column has at most n - 1 steps, 14 bits.  The node tables are of order n x NW words and
 * live for one call.
 * OUT OF SCOPE.  Gaps as a fifth state, indels as events; all most-parsimonious reconstructions, ACCTRAN / DELTRAN; weighted or
 * likelihood reconstruction; parsimony branch lengths in the Newick text; rooting; any change to an existing report byte. */
typedef struct kp_pars_site {
    int32_t column;  /* of the matrix, 0-based, padding columns counted: kp_site's */
    int32_t steps;   /* changes the tree needs there, >= 1 */
    int32_t alleles; /* bit k: some taxon holds base k */
    int32_t pad_;    /* zero */
} kp_pars_site;
typedef struct kp_pars_change {
    int32_t column;   /* as above */
    int32_t node;     /* the child end of the branch: a taxon below n, the node of record node - n otherwise */
    int32_t parent;   /* the other end */
    uint8_t from, to; /* the parent's state, the child's: 0..3 */
    uint16_t pad_;    /* zero */
} kp_pars_change;

#endif /* KP_SPEC_H */
