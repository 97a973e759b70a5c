"""Typing engine, result containers and TSV rows (reference: src/kaptive/serotyping/)."""

from kaptive_amd.serotyping.io import KaptiveRow, Pha4geRow, ReportRow
from kaptive_amd.serotyping.models import GeneHits, GeneState, LocusPieces, SerotypingProblem, SerotypingResult

__all__ = ["GeneHits", "GeneState", "KaptiveRow", "LocusPieces", "MultiSerotyper", "Pha4geRow", "ReportRow",
           "SerotypingProblem", "SerotypingResult", "Serotyper"]  # fmt: skip


def __getattr__(name: str):
    if name in ("Serotyper", "MultiSerotyper"):  # imported lazily: they pull in the native engine glue
        from kaptive_amd.serotyping import core

        return getattr(core, name)
    raise AttributeError(name)
