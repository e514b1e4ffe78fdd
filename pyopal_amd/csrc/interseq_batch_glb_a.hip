// Batch form of the one-strip NW / HW / OV pair-table kernel (see interseq_batch_impl.h): many queries of
// one row class per launch, biased integer halves, scores and optional end locations; classes of 8 .. 32 rows.
#include "interseq_batch_impl.h"

namespace miopal {

hipError_t launchInterseqBatchGlobalA(const BatchArgs& a, int rows, int computeUnits, hipStream_t stream) {
    // (the row classes, kBatchRowClasses, are no arithmetic sequence: a list)
    return dispatchRowList<8, 16, 24, 32>(rows, [&](auto r) { return launchBatchGlobalR<r>(a, computeUnits, stream); });
}

}  // namespace miopal
