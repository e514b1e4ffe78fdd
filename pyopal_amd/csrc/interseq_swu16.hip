// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): Smith-Waterman scores on
// column-shifted unsigned patterns compared as half floats (ArithSwU16), any number of strips.
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchFlavour<ArithSwU16, true, false>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
