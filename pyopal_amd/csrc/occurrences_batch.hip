// Every occurrence of every query of a panel in each target, for gfx950 (occurrences_batch.h;
// miopalSearchBatchOccurrences, host_batch_occurrences.inc).
//
// occurrences_batch_sweep_kernel is occurrences_sweep_kernel's lane-per-target sweep (occurrences.hip, the model to
// read first) restricted to one strip: H - c and E of up to 64 query rows in VGPRs, the columns scaled by j * ext, six
// operations a cell, the picker fed after every column. What differs:
//   * the rows of a GROUP of queries are one table in dynamic LDS, in the row-indexed layout the PSSM form walks
//     (prow += rowInts): row r holds matrix[residue of r][.] + open and the pad column, a query's rows are followed by
//     pad rows up to a multiple of eight. The workgroup builds the table once, from the chunk's row list and the matrix;
//   * WRITE = false (the count sweep; blockIdx.y = the group): a lane walks its target once per query of the group -
//     HM, E, the diagonal, the picker and the count start over before each query, the row loop ends at that query's
//     own rows (wave-uniform: the lanes of a wavefront are at the same query) - and stores count[q * n + job.out];
//   * WRITE = true: a workgroup is ONE wavefront that takes 64 consecutive entries of the scan's list, all of one
//     query (occurrences_batch.h: how it finds them), builds that query's rows alone and stores the occurrences at
//     the entries' offsets. (Query, target) pairs without occurrences are not in the list: no cell is computed for
//     them beyond the lanes of a wavefront's last, ragged piece.
// The arithmetic, cell by cell and column by column, is occurrences_sweep_kernel's first strip: the answers are the
// single-query search's byte for byte.
//
// PSSM form (miopalSearchPssmBatchOccurrences; occurrences_batch_pssm.hip defines MIOPAL_OCCURRENCES_BATCH_PSSM and
// includes this file, as occurrences_pssm.hip includes occurrences.hip): the same sweep under the name
// occurrences_batch_pssm_sweep_kernel, cell for cell. Only the table's source differs: table row r is row
// rowSource[r] of the chunk's PSSM rows (-1: a pad row) + open - no residue list, no matrix.
#include "occurrences_batch.h"
#include "occurrence_picker.h"
#include "launch_layer.h"

namespace miopal {

namespace {

constexpr int kNegInf = INT32_MIN / 4;
constexpr int kPadScore = -(1 << 28);
constexpr int kBlock = 256;
#ifdef MIOPAL_OCCURRENCES_BATCH_PSSM
constexpr bool kPssmUnit = true;
#define MIOPAL_BATCH_SWEEP_KERNEL occurrences_batch_pssm_sweep_kernel
#else
constexpr bool kPssmUnit = false;
#define MIOPAL_BATCH_SWEEP_KERNEL occurrences_batch_sweep_kernel
#endif

template <int REGION, bool WRITE>
__global__ __launch_bounds__(kBlock) void MIOPAL_BATCH_SWEEP_KERNEL(BatchOccurrenceArgs a) {
    static_assert(REGION == kLastRow || REGION == kAllCells, "HW or SW");
    constexpr bool SW = REGION == kAllCells;
    constexpr bool ROWS = SW && WRITE;   // the row of a column's maximum: only the write pass stores it
    extern __shared__ __attribute__((aligned(16))) int table[];
    const int A = a.alphabet;
    const int open = a.gapOpen, ext = a.gapExt;
    const int rowInts = A + 1;
    const int c = open - ext;
    const int lane = threadIdx.x & 63;

    // the queries this workgroup walks, their rows in the chunk's row list, and the lane's target
    int qFirst, qCount, rowBase, rowCount;
    bool active;
    int64_t tOff = 0, at = 0, target = 0;
    int L = 0, out = 0;
    if constexpr (WRITE) {
        // the query of this wavefront: the largest q with first[q] / 64 + q <= w (base(0) = 0, base(nQueries) = the grid)
        const int w = blockIdx.x;
        int lo = 0, hi = a.nQueries;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.first[mid] / kLanes + mid <= w) lo = mid;
            else hi = mid;
        }
        const int q = lo;
        const int begin = a.first[q], end = a.first[q + 1];
        const int64_t e0 = (int64_t)begin + (int64_t)(w - (begin / kLanes + q)) * kLanes;
        if (e0 >= end) return;   // a wavefront left over (the whole workgroup)
        active = e0 + lane < end;
        if (active) {
            const int64_t entry = a.list[e0 + lane];
            const int64_t pos = entry - (int64_t)q * a.n;
            const int64_t first = a.dbOffsets[a.start + pos];
            tOff = first;
            L = (int)(a.dbOffsets[a.start + pos + 1] - first);
            at = a.offsets[entry];
            target = a.start + pos;
        }
        const int4 m = a.query[q];
        qFirst = q;
        qCount = 1;
        rowBase = m.x;
        rowCount = batchOccurrenceRows(m.y);
    } else {
        const int4 g = a.group[blockIdx.y];
        qFirst = g.x;
        qCount = g.y;
        rowBase = g.z;
        rowCount = g.w;
        const int idx = blockIdx.x * kBlock + threadIdx.x;
        active = idx < a.nJobs;
        if (active) {
            const PairJob job = a.jobs[idx];
            tOff = job.tOff;
            L = job.tLen;
            out = job.out;
        }
    }
    for (int k = threadIdx.x; k < rowCount * rowInts; k += blockDim.x) {
        const int r = k / rowInts, t = k - r * rowInts;
        if constexpr (kPssmUnit) {
            const int source = a.rowSource[rowBase + r];
            table[k] = (source >= 0 && t < A) ? a.rows[(int64_t)source * A + t] + open : kPadScore;
        } else {
            const int residue = a.rowResidue[rowBase + r];
            table[k] = (residue != kBatchOccurrencePadRow && t < A) ? a.matrix[residue * A + t] + open : kPadScore;
        }
    }
    __syncthreads();

    int maxL = L;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxL = max(maxL, __shfl_xor(maxL, off));
    maxL = __builtin_amdgcn_readfirstlane(maxL);
    const uint8_t* tptr = a.residues + tOff;

    for (int qi = 0; qi < qCount; ++qi) {
        const int4 m = a.query[qFirst + qi];   // (wave-uniform)
        const int Q = m.y;
        const char* qtab = (const char*)table + (size_t)(m.x - rowBase) * rowInts * 4;
        const int lastSub = (Q - 1) & 7;   // HW: the row that is read, counted inside its group of eight
        OccurrencePicker pick(m.z, m.w);
        int found = 0;
        auto emit = [&](int j, int v, int r) {
            if constexpr (WRITE) {
                a.outTarget[at + found] = target;
                a.outScore[at + found] = v;
                a.outColumn[at + found] = j;
                a.outRow[at + found] = r;
            }
            ++found;
        };
        // The columns are kept SCALED, as occurrences_sweep_kernel keeps them: what is stored for column j is the
        // value + j * ext, HM holds H' - c, and the picker is handed the value less the scale.
        int HM[kLanes], E[kLanes];
#pragma unroll
        for (int i = 0; i < kLanes; ++i) {
            HM[i] = i < Q ? (SW ? 0 : borderGap(i, open, ext)) - open : kNegInf;   // column -1 (scaled by -ext, less c)
            E[i] = kNegInf;
        }
        int aboveHmPrev = -open;   // the row above at column j - 1: the free top row
        int tcolNext = (L > 0 ? (int)tptr[0] : A) * 4;
        int scale = 0;   // j * ext
        for (int j = 0; j < maxL; ++j, scale += ext) {
            const int tcol = tcolNext;
            {
                int t = A;
                if (j + 1 < L) t = tptr[j + 1];
                tcolNext = t * 4;
            }
            const char* prow = qtab + tcol;   // the column's scores, row by row
            int hmUp = scale - c;             // the top row is free under HW and SW
            int fUp = kNegInf;
            int cmax = scale, crow = -1;      // SW: the column's maximum so far and its row
            int hmDiag = aboveHmPrev;
            aboveHmPrev = hmUp;
            int v = kNegInf;                  // HW: H of the query's last row
            [[maybe_unused]] int hg[8];
#pragma unroll
            for (int i = 0; i < kLanes; ++i) {
                if ((i & 7) == 0 && i >= Q) break;   // wave-uniform
                const int sc = *(const int*)prow;
                prow += rowInts * 4;
                const int e = max(HM[i], E[i]);
                const int f = max(hmUp, fUp) - ext;
                const int d = hmDiag + sc;
                int h = max(d, max(e, f));
                if constexpr (SW) h = max(h, scale);
                if constexpr (ROWS) {
                    const bool take = h > cmax;
                    cmax = take ? h : cmax;
                    crow = take ? i : crow;
                } else if constexpr (SW) {
                    cmax = max(cmax, h);
                } else {
                    hg[i & 7] = h;   // (what is left behind the loop: the last group of eight that ran)
                }
                const int hm = h - c;
                hmDiag = HM[i];
                HM[i] = hm;
                E[i] = e;
                hmUp = hm;
                fUp = f;
            }
            if constexpr (!SW) {
#pragma unroll
                for (int k = 0; k < 8; ++k) v = k == lastSub ? hg[k] : v;
            }
            if (j < L) pick.feed(j, (SW ? cmax : v) - scale, SW ? crow : Q - 1, emit);
        }
        pick.finish(emit);
        if constexpr (!WRITE) {
            if (active) a.count[(int64_t)(qFirst + qi) * a.n + out] = found;
        }
    }
}

#ifndef MIOPAL_OCCURRENCES_BATCH_PSSM
// first[q] = the position in the scan's list of the first entry >= q * n, head[q] = the occurrences in front of it
__global__ __launch_bounds__(kBlock) void occurrences_batch_bounds_kernel(OccurrenceScratch sc, int64_t n, int nQueries,
                                                                          int32_t* first, int64_t* head) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q > nQueries) return;
    const int64_t listed = sc.totals[1];
    const int64_t key = (int64_t)q * n;
    int64_t lo = 0, hi = listed;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)sc.list[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    first[q] = (int32_t)lo;
    head[q] = sc.offsets[key];   // (q = nQueries: the scan's total, stored behind the last entry)
    if (q == 0) {
        head[nQueries + 1] = sc.totals[0];
        head[nQueries + 2] = listed;
    }
}

#endif

template <int REGION, bool WRITE>
hipError_t launchSweep(const BatchOccurrenceArgs& a, dim3 grid, dim3 block, size_t ldsBytes, hipStream_t stream) {
    if (const hipError_t e = allowFullLds<&MIOPAL_BATCH_SWEEP_KERNEL<REGION, WRITE>>(); e != hipSuccess) return e;
    hipLaunchKernelGGL((MIOPAL_BATCH_SWEEP_KERNEL<REGION, WRITE>), grid, block, ldsBytes, stream, a);
    return hipGetLastError();
}

bool sweepArgsOk(const BatchOccurrenceArgs& a, int region, size_t ldsBytes) {
    if (region != kLastRow && region != kAllCells) return false;
    // (the PSSM unit: rowSource and rows lie where rowResidue and matrix do)
    if (!a.residues || !a.rowResidue || !a.query || !a.matrix || a.nQueries < 1 || a.n < 1) return false;
    return a.alphabet >= 1 && a.alphabet <= kMaxAlphabet && ldsBytes >= 1 && ldsBytes <= kCuLdsBytes;
}

}  // namespace

// the sweeps of this unit: occurrences_batch.o the plain form, occurrences_batch_pssm.o the row-filled one
#ifdef MIOPAL_OCCURRENCES_BATCH_PSSM
#define MIOPAL_BATCH_COUNT launchBatchOccurrencesCountPssm
#define MIOPAL_BATCH_WRITE launchBatchOccurrencesWritePssm
#else
#define MIOPAL_BATCH_COUNT launchBatchOccurrencesCount
#define MIOPAL_BATCH_WRITE launchBatchOccurrencesWrite
#endif

hipError_t MIOPAL_BATCH_COUNT(const BatchOccurrenceArgs& a, int region, int groups, size_t ldsBytes, hipStream_t stream) {
    if (a.nJobs <= 0) return hipSuccess;
    if (!sweepArgsOk(a, region, ldsBytes) || !a.jobs || !a.group || !a.count || groups < 1 || groups > 65535) return hipErrorInvalidValue;
    const dim3 grid((a.nJobs + kBlock - 1) / kBlock, groups), block(kBlock);
    return region == kLastRow ? launchSweep<kLastRow, false>(a, grid, block, ldsBytes, stream)
                              : launchSweep<kAllCells, false>(a, grid, block, ldsBytes, stream);
}

hipError_t MIOPAL_BATCH_WRITE(const BatchOccurrenceArgs& a, int region, int64_t listed, size_t ldsBytes, hipStream_t stream) {
    if (listed <= 0) return hipSuccess;
    if (!sweepArgsOk(a, region, ldsBytes) || !a.offsets || !a.list || !a.first || !a.dbOffsets || !a.outTarget || !a.outScore ||
        !a.outColumn || !a.outRow || listed > a.n * a.nQueries)
        return hipErrorInvalidValue;
    // one wavefront per workgroup: listed / 64 + queries of them cover every query's pieces (occurrences_batch.h)
    const dim3 grid((unsigned)(listed / kLanes + a.nQueries)), block(kLanes);
    return region == kLastRow ? launchSweep<kLastRow, true>(a, grid, block, ldsBytes, stream)
                              : launchSweep<kAllCells, true>(a, grid, block, ldsBytes, stream);
}

#ifndef MIOPAL_OCCURRENCES_BATCH_PSSM
hipError_t launchBatchOccurrencesBounds(const OccurrenceScratch& sc, int64_t n, int nQueries, int32_t* first, int64_t* head,
                                        hipStream_t stream) {
    if (n < 1 || nQueries < 1 || !first || !head) return hipErrorInvalidValue;
    hipLaunchKernelGGL(occurrences_batch_bounds_kernel, dim3((nQueries + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, n,
                       nQueries, first, head);
    return hipGetLastError();
}
#endif

}  // namespace miopal
