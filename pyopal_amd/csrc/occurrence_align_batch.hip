// The alignment stage of the panel occurrence search, for gfx950 (occurrence_align_batch.h;
// miopalSearchBatchOccurrencesAligned, host_batch_occurrence_align.inc).
//
// As in the single-query stage (occurrence_align.hip) the occurrences the write sweep left in HBM are the end cells of
// the later passes of a `full` pair list. A panel's occurrence has one thing more to say: WHICH query it belongs to.
// That is stored nowhere - a chunk's occurrences lie query after query, and head[q] (occurrences in front of query q,
// behind launchBatchOccurrencesBounds) says where each query's stretch begins. One thread per occurrence looks its
// position up in head: a binary search over nQueries + 1 values, wave-coherent for nearly every wavefront since a
// query's occurrences are contiguous (the lanes of a wavefront that lies inside one stretch take the same branches and
// read the same words). Queries without occurrences give equal neighbours in head; "the LAST q with head[q] <= k" is
// the one that owns k, never an empty query in front of it.
#include "occurrence_align_batch.h"

namespace miopal {

namespace {

__global__ void batch_occurrence_origins_kernel(int n, int64_t k0, const int64_t* target, const int64_t* dbOffsets,
                                                int64_t nTargets, const int64_t* head, int nQueries,
                                                const int32_t* queryOff, int64_t* targetOff, int32_t* qBase) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const int64_t t = target[x];
    // (the write sweep only names targets of the handle; an index outside it reads nothing)
    targetOff[x] = (t >= 0 && t < nTargets) ? dbOffsets[t] : 0;
    // head[lo] <= k (head[0] = 0) and, where hi < nQueries, head[hi] > k: the owner lies in [lo, hi)
    const int64_t k = k0 + x;
    int lo = 0, hi = nQueries;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (head[mid] <= k) lo = mid;
        else hi = mid;
    }
    qBase[x] = queryOff[lo];
}

}  // namespace

hipError_t launchBatchOccurrenceOrigins(int n, int64_t k0, const int64_t* target, const int64_t* dbOffsets,
                                        int64_t nTargets, const int64_t* head, int nQueries, const int32_t* queryOff,
                                        int64_t* targetOff, int32_t* qBase, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!target || !dbOffsets || !head || !queryOff || !targetOff || !qBase || nQueries < 1 || k0 < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_occurrence_origins_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, k0, target,
                       dbOffsets, nTargets, head, nQueries, queryOff, targetOff, qBase);
    return hipGetLastError();
}

}  // namespace miopal
