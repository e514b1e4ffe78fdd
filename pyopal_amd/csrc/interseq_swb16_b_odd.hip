// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): Smith-Waterman on
// biased integer halves, column-shifted, pair-indexed LDS profile; strips of 17..31 rows (odd), scores only.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchPairBiased<17, false>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
