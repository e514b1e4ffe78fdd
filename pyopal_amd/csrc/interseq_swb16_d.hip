// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): Smith-Waterman on
// biased integer halves, column-shifted, pair-indexed LDS profile; strips of 50..64 rows, scores only.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchPairBiased<50, false>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
