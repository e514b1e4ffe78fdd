// The row-indexed instantiations of pairlist_forward_kernel (miopalAlignPairsPssm: a list of position-specific scoring
// matrices, their rows in one LDS table) and their launcher, a translation unit of their own: pairlist.hip says why.
#define MIOPAL_PAIRLIST_PSSM 1
#include "pairlist.hip"
