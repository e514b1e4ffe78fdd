// Batch form of the one-strip Smith-Waterman pair-table kernel (see interseq_batch_impl.h): many queries of
// one row class per launch, biased integer halves, with end locations (row keys in the low bits).
#include "interseq_batch_impl.h"

namespace miopal {

hipError_t launchInterseqBatchSwLoc(const BatchArgs& a, int rows, int computeUnits, hipStream_t stream) {
    switch (rows) {
        case 8: return launchBatchSwR<8, true>(a, computeUnits, stream);
        case 16: return launchBatchSwR<16, true>(a, computeUnits, stream);
        case 24: return launchBatchSwR<24, true>(a, computeUnits, stream);
        case 32: return launchBatchSwR<32, true>(a, computeUnits, stream);
        case 40: return launchBatchSwR<40, true>(a, computeUnits, stream);
        case 48: return launchBatchSwR<48, true>(a, computeUnits, stream);
        case 56: return launchBatchSwR<56, true>(a, computeUnits, stream);
        case 60: return launchBatchSwR<60, true>(a, computeUnits, stream);
        case 64: return launchBatchSwR<64, true>(a, computeUnits, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace miopal
