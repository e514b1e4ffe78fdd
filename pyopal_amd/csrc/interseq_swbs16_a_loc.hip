// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): Smith-Waterman scores
// with end locations of several strips on biased integer halves with the pair-indexed LDS profile;
// strips of 32..46 rows.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchPairStrips<32, true>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
