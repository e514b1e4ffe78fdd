// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h).
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchFlavour<ArithI16, false, false>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
