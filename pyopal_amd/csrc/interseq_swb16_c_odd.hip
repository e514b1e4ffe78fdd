// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): Smith-Waterman on
// biased integer halves, column-shifted, pair-indexed LDS profile; strips of 33..47 rows (odd), scores only.
#include "interseq_impl.h"

namespace miopal {

hipError_t launchInterseqPairSwBiasedOddC(const InterseqArgs& a, int rows, int computeUnits, hipStream_t stream) {
    return launchPairBiased<33, false>(a, rows, computeUnits, stream);
}

}  // namespace miopal
