// Batch form of the one-strip NW / HW / OV pair-table kernel (see interseq_batch_impl.h): many queries of
// one row class per launch, biased integer halves, scores and optional end locations; classes of 8 .. 32 rows.
#include "interseq_batch_impl.h"

namespace miopal {

hipError_t launchInterseqBatchGlobalA(const BatchArgs& a, int rows, int computeUnits, hipStream_t stream) {
    switch (rows) {
        case 8: return launchBatchGlobalR<8>(a, computeUnits, stream);
        case 16: return launchBatchGlobalR<16>(a, computeUnits, stream);
        case 24: return launchBatchGlobalR<24>(a, computeUnits, stream);
        case 32: return launchBatchGlobalR<32>(a, computeUnits, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace miopal
