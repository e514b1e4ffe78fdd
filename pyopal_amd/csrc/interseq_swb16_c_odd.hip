// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): Smith-Waterman on
// biased integer halves, column-shifted, pair-indexed LDS profile; strips of 33..47 rows (odd), scores only.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchPairBiased<33, false>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
