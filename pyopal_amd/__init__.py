"""MI355X-native implementation of PyOpal's database-search hot path.

Drop-in for the names of ``pyopal`` (``src/pyopal/__init__.py:4-13``)::

    import pyopal_amd as pyopal
"""

from . import lib
from ._align import align
from .lib import (Aligner, Alphabet, BaseDatabase, Database, EndResult, FullResult, ProfileColumns, Pssm, ScoreFit,
                  ScoreResult, SignificantHits, __version__, matrix_lambda)
from .matrices import ScoringMatrix
from .occurrences import (find_occurrence_alignments_many, find_occurrence_alignments_many_arrays,
                          find_occurrence_alignments_pssm_many, find_occurrence_alignments_pssm_many_arrays,
                          find_occurrences, find_occurrences_arrays, find_occurrences_many, find_occurrences_many_arrays,
                          find_occurrences_pssm, find_occurrences_pssm_many, find_occurrences_pssm_many_arrays)

# (Pssm, the query type of Aligner.align_pssm, ScoreFit / SignificantHits of Aligner.significant_hits, and
# ProfileColumns / matrix_lambda of Aligner.profile_columns and Pssm.from_columns, and the occurrence searches
# find_occurrences / find_occurrences_pssm / find_occurrences_arrays and, for a panel of queries,
# find_occurrences_many / find_occurrences_many_arrays (ends) and find_occurrence_alignments_many /
# find_occurrence_alignments_many_arrays (starts and alignments), with their forms for a panel of PSSMs
# (find_occurrences_pssm_many, ..._arrays, find_occurrence_alignments_pssm_many, ..._arrays), are extensions: importable,
# not among the reference's names)
__all__ = [
    "Alphabet",
    "Aligner",
    "BaseDatabase",
    "Database",
    "ScoreResult",
    "EndResult",
    "FullResult",
    "align",
]
