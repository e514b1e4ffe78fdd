// The alignment stage of the panel occurrence search (miopalSearchBatchOccurrencesAligned,
// host_batch_occurrence_align.inc): what the later passes of a `full` pair list need beside the occurrences' (score,
// row, column) - the origin of each occurrence's target and of its own query - gathered on the device
// (occurrence_align_batch.hip).
#pragma once
#include "common.h"

namespace miopal {

// For the n occurrences k0 .. k0 + n of a panel chunk (k: the occurrence's position in the chunk's output order, the
// order the write sweep left them in): `target` holds their target indices, target[x] = the target of occurrence
// k0 + x, in [0, nTargets). targetOff[x] = dbOffsets[target[x]], as launchOccurrencePairInputs gives it. head[0 ..
// nQueries] = the occurrences in front of each query of the chunk (ascending, head[0] = 0, head[nQueries] = the
// chunk's total, k0 + n at most that): the query of occurrence k is the last q < nQueries with head[q] <= k, and
// qBase[x] = queryOff[q], its origin in the chunk's concatenated query buffer. queryOff has nQueries entries at least.
hipError_t launchBatchOccurrenceOrigins(int n, int64_t k0, const int64_t* target, const int64_t* dbOffsets,
                                        int64_t nTargets, const int64_t* head, int nQueries, const int32_t* queryOff,
                                        int64_t* targetOff, int32_t* qBase, hipStream_t stream);

}  // namespace miopal
