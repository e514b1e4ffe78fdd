// The alignment stage of the occurrence search, for gfx950 (occurrence_align.h; miopalSearchOccurrencesAligned,
// host_occurrence_align.inc).
//
// The stage has no DP kernel of its own: the occurrences the write sweep left in HBM - (target, score, row, column) -
// are end cells, and the later passes of a `full` pair list (reverse_jobs_kernel, perpair_kernel / intraseq_kernel,
// start_cells_kernel, the direction pass, the walk and the gather) take exactly such arrays. What those passes need
// beside them is where each occurrence's target begins; the query is the call's one query, at origin 0.
// occurrence_pair_inputs_kernel gathers that from the handle's offsets, so that nothing of the occurrence list has
// to go up over PCIe.
#include "occurrence_align.h"

namespace miopal {

namespace {

__global__ void occurrence_pair_inputs_kernel(int n, const int64_t* target, const int64_t* dbOffsets, int64_t nTargets,
                                              int64_t* targetOff) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t t = target[k];
    // (the write sweep only names targets of the handle; an index outside it reads nothing)
    targetOff[k] = (t >= 0 && t < nTargets) ? dbOffsets[t] : 0;
}

}  // namespace

hipError_t launchOccurrencePairInputs(int n, const int64_t* target, const int64_t* dbOffsets, int64_t nTargets,
                                      int64_t* targetOff, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!target || !dbOffsets || !targetOff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(occurrence_pair_inputs_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, target, dbOffsets,
                       nTargets, targetOff);
    return hipGetLastError();
}

}  // namespace miopal
