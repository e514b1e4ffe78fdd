// One arithmetic flavour of the inter-sequence kernel (see interseq_impl.h).
#include "interseq_impl.h"

namespace miopal {

template hipError_t launchFlavour<ArithSwI16, true, false>(const InterseqArgs&, int, int, hipStream_t);

template hipError_t launchPairFlavour<ArithSwI16>(const InterseqArgs&, int, int, hipStream_t);

}  // namespace miopal
