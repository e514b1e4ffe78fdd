// The row-filled instantiations of the panel occurrence sweep (miopalSearchPssmBatchOccurrences: the LDS table of a
// group of position-specific scoring matrices filled from their own rows) and their launchers, a translation unit of
// their own: occurrences_batch.hip says what differs.
#define MIOPAL_OCCURRENCES_BATCH_PSSM 1
#include "occurrences_batch.hip"
