// Batch form of the one-strip Smith-Waterman pair-table kernel (see interseq_batch_impl.h): many queries of
// one row class per launch, biased integer halves, scores only.
#include "interseq_batch_impl.h"

namespace miopal {

hipError_t launchInterseqBatchSw(const BatchArgs& a, int rows, int computeUnits, hipStream_t stream) {
    // (the row classes, kBatchRowClasses, are no arithmetic sequence: a list)
    return dispatchRowList<8, 16, 24, 32, 40, 48, 56, 60, 64>(rows, [&](auto r) { return launchBatchSwR<r, false>(a, computeUnits, stream); });
}

}  // namespace miopal
