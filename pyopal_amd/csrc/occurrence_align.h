// The alignment stage of the occurrence search (miopalSearchOccurrencesAligned, host_occurrence_align.inc): what the
// later passes of a `full` pair list need beside the occurrences' (score, row, column), gathered on the device from
// the handle's offsets (occurrence_align.hip).
#pragma once
#include "common.h"

namespace miopal {

// targetOff[k] = dbOffsets[target[k]] for the n occurrences target[0 .. n): where the target of occurrence k begins,
// what launchReverseJobs / launchTraceJobs take as `offsets`. target[k] in [0, nTargets).
hipError_t launchOccurrencePairInputs(int n, const int64_t* target, const int64_t* dbOffsets, int64_t nTargets,
                                      int64_t* targetOff, hipStream_t stream);

}  // namespace miopal
