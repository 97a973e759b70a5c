// caps_harness.cpp -- TEST-ONLY: compiles kaptive_amd/csrc/kp_caps.h with g++ and exposes its buffer-size policy to ctypes
// (tests/test_caps_cpu.py), so that the arithmetic is checked without a GPU.  Never loaded by the product.
#include <cstring>

#include "../../kaptive_amd/csrc/kp_caps.h"

static int copy_message(const std::string &err, char *msg, int cap) {
    if (msg && cap > 0) { std::strncpy(msg, err.c_str(), (size_t)cap - 1); msg[cap - 1] = 0; }
    return (int)err.size();
}

extern "C" {

// sizes of the structs and the constants, so that the ctypes mirrors can be checked against the header
void kpc_layout(int32_t *out6) {
    out6[0] = (int32_t)sizeof(KpCapOptions); out6[1] = (int32_t)sizeof(KpLearnt); out6[2] = (int32_t)sizeof(KpPassCaps);
    out6[3] = (int32_t)sizeof(KpPassSeen); out6[4] = (int32_t)KP_CAPS_ANCHOR_SUBS; out6[5] = (int32_t)KP_OCC_SLOTS_MAX;
}
void kpc_default_options(KpCapOptions *o) { *o = KpCapOptions(); }
void kpc_size(const KpCapOptions *o, KpLearnt *L, int32_t n_asm, int64_t total_words, KpPassCaps *w) { kp_caps_size(*o, *L, n_asm, total_words, *w); }
int kpc_after_pass(KpLearnt *L, KpPassCaps *w, const KpPassSeen *s, char *msg, int msg_cap) {
    std::string err;
    const int verdict = (int)kp_caps_after_pass(*L, *w, *s, err);
    copy_message(err, msg, msg_cap);
    return verdict;
}
void kpc_grow_hits(KpLearnt *L, KpPassCaps *w, uint32_t max_hits, int headroom) { kp_caps_grow_hits(*L, *w, max_hits, headroom != 0); }
// caps3: kept_cap, piece_cap, prot_cap of one typing group; returns 1, or 0 with the message
int kpc_grow_run(int32_t *caps3, int flags, char *msg, int msg_cap) {
    KpRunCaps c;
    c.kept_cap = caps3[0]; c.piece_cap = caps3[1]; c.prot_cap = caps3[2];
    std::string err;
    const bool ok = kp_caps_grow_run(c, flags, err);
    caps3[0] = c.kept_cap; caps3[1] = c.piece_cap; caps3[2] = c.prot_cap;
    copy_message(err, msg, msg_cap);
    return ok ? 1 : 0;
}
// runs3: kept_cap, piece_cap, prot_cap of n_runs typing groups; returns whether `name` is a buffer-size option
int kpc_set_option(KpCapOptions *o, KpLearnt *L, int32_t *runs3, int n_runs, const char *name, int64_t value) {
    std::vector<KpRunCaps> runs((size_t)n_runs);
    for (int i = 0; i < n_runs; ++i) { runs[i].kept_cap = runs3[3 * i]; runs[i].piece_cap = runs3[3 * i + 1]; runs[i].prot_cap = runs3[3 * i + 2]; }
    const bool known = kp_caps_set_option(*o, *L, runs, name, value);
    for (int i = 0; i < n_runs; ++i) { runs3[3 * i] = runs[i].kept_cap; runs3[3 * i + 1] = runs[i].piece_cap; runs3[3 * i + 2] = runs[i].prot_cap; }
    return known ? 1 : 0;
}

}  // extern "C"
