// One arithmetic flavour of the inter-sequence kernel, with end locations (interseq_impl.h).
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchFlavour<ArithI16, true, true>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
