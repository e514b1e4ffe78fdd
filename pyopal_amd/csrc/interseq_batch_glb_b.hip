// Batch form of the one-strip NW / HW / OV pair-table kernel (see interseq_batch_impl.h): many queries of
// one row class per launch, biased integer halves, scores and optional end locations; classes of 40 .. 64 rows.
#include "interseq_batch_impl.h"

namespace miopal {

hipError_t launchInterseqBatchGlobalB(const BatchArgs& a, int rows, int computeUnits, hipStream_t stream) {
    switch (rows) {
        case 40: return launchBatchGlobalR<40>(a, computeUnits, stream);
        case 48: return launchBatchGlobalR<48>(a, computeUnits, stream);
        case 56: return launchBatchGlobalR<56>(a, computeUnits, stream);
        case 60: return launchBatchGlobalR<60>(a, computeUnits, stream);
        case 64: return launchBatchGlobalR<64>(a, computeUnits, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace miopal
