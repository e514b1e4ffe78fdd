// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): Smith-Waterman on
// biased integer halves, column-shifted, pair-indexed LDS profile; strips of 2..16 rows, scores only.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchPairBiased<2, false>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
