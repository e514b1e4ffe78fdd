// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): NW / HW / OV of several
// strips on biased integer halves with the pair-indexed LDS profile, with end locations; strips of 48 rows.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchPairGlobalStrips<48, true>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
