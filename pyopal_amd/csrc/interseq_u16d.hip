// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h): NW / HW / OV on unsigned
// anti-diagonally shifted patterns compared as half floats (ArithU16Diag).
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchFlavour<ArithU16Diag, false, false>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
