// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): NW / HW / OV on biased
// integer halves, column-shifted, pair-indexed LDS profile; strips of 18..32 rows.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchPairGlobal<18>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
