// Lane-per-pair forward pass of a PAIR LIST for gfx950 (miopalAlignPairs, host_pairs.inc): every lane owns one
// (query, target) pair with a query of its own and the search mode's own border rules.
//
// The structure is perpair_kernel's (perpair.hip, the model to read first): one lane sweeps its pair column by
// column at 32 bit, H - open and E of up to 64 query rows in VGPRs, the substitution matrix in LDS with a pad row
// and column (33 x 33 ints, `open` folded in), the lane's query rows as pre-scaled LDS row offsets packed two per
// VGPR; taller queries strip by strip, the strip's last row handed down through HBM. What differs:
//   * the border rules (topGap / leftGap / floor0, job.rules) and the answer region (template parameter) are the
//     search's own - perpair_kernel only knows the anchored problem with both borders penalised;
//   * the lane's query rows come from the call's concatenated queries in GLOBAL memory, once per strip: no LDS copy
//     of the queries, so their total length is unbounded;
//   * score-only instantiations (LOC = false) carry no location bookkeeping.
// PSSM (miopalAlignPairsPssm, a list of position-specific scoring matrices): the score of a row is the row's own. The
// call's PSSMs, end to end, are ONE table in dynamic LDS - perpair_kernel's row-indexed layout: [a.queryLength + 1]
// [A + 1] ints of score + open, pad column and pad row last (perPairPssmBytes: within 64 KB, so that a row's byte
// offset fits the 16 bits the lanes keep two of per register) - filled once per workgroup from a.rows; job.qOff is
// the first row of the lane's PSSM in it and a.query is not read. The column loop is the plain one, instruction
// for instruction, and the plain instantiations are the code they were. Lists whose rows do not fit keep the
// wavefront-per-pair kernel (host_pairs.inc).
// Two translation units are made of this file, as of interseq_impl.h: pairlist.o holds the eight plain instantiations
// and the job builder (pairlist.rpt: the eight entries tests/test_pairs_cpu.py counts), pairlist_pssm.o
// (pairlist_pssm.hip defines MIOPAL_PAIRLIST_PSSM and includes this file) the eight row-indexed ones, with
// resource remarks of their own in pairlist_pssm.rpt.
// Candidates in column-major order, a candidate replaces the best only when strictly greater, Smith-Waterman
// starts from best = 0 with no location; across strips the higher score wins, then the smaller column, then the
// upper strip. intraseq_kernel (intraseq.hip) is the other in-tree statement of this pass and the one this kernel
// agrees with cell for cell; the model is oracle/opal_oracle.c.
//
// Rows beyond the lane's query and columns beyond its target read the pad row / column: with the floor (region
// "all cells") every value computed there is bounded by a valid cell that comes earlier in the column-major scan,
// the other regions test row and column explicitly.
#include "common.h"

namespace miopal {

namespace {

constexpr int kNegInf = INT32_MIN / 4;
constexpr int kPadScore = -(1 << 28);
constexpr int kStride = kMaxAlphabet + 1;  // matrix rows in LDS, in ints (pad column included)
constexpr int kBlock = 256;
#ifdef MIOPAL_PAIRLIST_PSSM
constexpr bool kPssmUnit = true;
#else
constexpr bool kPssmUnit = false;
#endif

template <int REGION, bool LOC, bool PSSM = false>
__global__ __launch_bounds__(kBlock) void pairlist_forward_kernel(PerPairArgs a) {
    __shared__ int smat[PSSM ? 1 : kStride * kStride];
    extern __shared__ __attribute__((aligned(16))) int pssmTable[];
    const int A = a.alphabet;
    // (PSSM: ints per row of the table, and its pad row)
    [[maybe_unused]] const int pssmRowInts = A + 1;
    [[maybe_unused]] const int pssmPadRow = a.queryLength;
    if constexpr (PSSM) {
        // (consecutive threads read consecutive ints of a.rows but for the pad column's gaps)
        for (int idx = threadIdx.x; idx < (a.queryLength + 1) * pssmRowInts; idx += kBlock) {
            const int q = idx / pssmRowInts, t = idx - q * pssmRowInts;
            pssmTable[idx] = (q < a.queryLength && t < A) ? a.rows[q * A + t] + a.gapOpen : kPadScore;
        }
    } else {
        for (int idx = threadIdx.x; idx < kStride * kStride; idx += kBlock) {
            const int q = idx / kStride, t = idx % kStride;
            // `open` is folded into the scores: the columns keep H - open (perpair_kernel)
            smat[idx] = (q < A && t < A) ? a.matrix[q * A + t] + a.gapOpen : kPadScore;
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    // (the leading wavefronts' jobs are outliers of the sorted list, done by intraseq_kernel)
    const bool active = idx < a.nJobs && !(a.skipWaves != nullptr && (idx >> 6) < *a.skipWaves);
    PairJob job{};
    if (active) job = a.jobs[idx];
    const int Q = job.qLen, L = job.tLen;
    const int open = a.gapOpen, ext = a.gapExt;
    const bool topGap = job.rules & 1, leftGap = job.rules & 2, floor0 = job.rules & 4;
    const int floorV = floor0 ? 0 : kNegInf;   // the floor as a maximum that is always there

    int maxQ = Q, maxL = L;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        maxQ = max(maxQ, __shfl_xor(maxQ, off));
        maxL = max(maxL, __shfl_xor(maxL, off));
    }
    maxQ = __builtin_amdgcn_readfirstlane(maxQ);
    maxL = __builtin_amdgcn_readfirstlane(maxL);
    const int nStrips = (maxQ + kLanes - 1) / kLanes;  // of the wavefront's tallest query

    // running answer over the strips
    int best = floor0 ? 0 : INT32_MIN, brow = -1, bcol = -1;
    const uint8_t* tptr = a.residues + job.tOff;
    [[maybe_unused]] const uint8_t* qptr = PSSM ? nullptr : a.query + job.qOff;
    // strip boundaries of the wavefront: (H - open, F) of the strip's last row, per column
    int2* bnd = a.boundary ? a.boundary + (int64_t)(idx >> 6) * a.boundaryStride * kLanes + lane : nullptr;

    for (int s = 0; s < nStrips; ++s) {
        const int row0 = s * kLanes;
        const int rowsHere = min(maxQ - row0, kLanes);  // wave-uniform
        const bool toNext = s + 1 < nStrips;
        // LDS byte offsets of the lane's query rows, two per register; pad row beyond the query
        uint32_t qo[kLanes / 2];
#pragma unroll
        for (int i = 0; i < kLanes; i += 2) {
            if constexpr (PSSM) {
                const int q0 = row0 + i < Q ? job.qOff + row0 + i : pssmPadRow;
                const int q1 = row0 + i + 1 < Q ? job.qOff + row0 + i + 1 : pssmPadRow;
                qo[i >> 1] = (uint32_t)(q0 * pssmRowInts * 4) | ((uint32_t)(q1 * pssmRowInts * 4) << 16);
            } else {
                const int q0 = row0 + i < Q ? qptr[row0 + i] : A;
                const int q1 = row0 + i + 1 < Q ? qptr[row0 + i + 1] : A;
                qo[i >> 1] = (uint32_t)(q0 * kStride * 4) | ((uint32_t)(q1 * kStride * 4) << 16);
            }
        }
        int HM[kLanes], E[kLanes];
#pragma unroll
        for (int i = 0; i < kLanes; ++i) {
            HM[i] = row0 + i < Q ? (leftGap ? borderGap(row0 + i, open, ext) : 0) - open : kNegInf;  // column -1
            E[i] = kNegInf;
        }
        // first maximum of this strip (column-major inside the strip)
        int sbest = floor0 ? 0 : INT32_MIN, srow = -1, scol = -1;
        // row above the strip at column j - 1 (diagonal of the strip's first row)
        int aboveHmPrev = (s == 0 ? 0 : (leftGap ? borderGap(row0 - 1, open, ext) : 0)) - open;

        int tcolNext = (L > 0 ? (int)tptr[0] : A) * 4;
        for (int j = 0; j < maxL; ++j) {
            const int tcol = tcolNext;
            {
                int t = A;
                if (j + 1 < L) t = tptr[j + 1];
                tcolNext = t * 4;
            }
            const char* mcol = (PSSM ? (const char*)pssmTable : (const char*)smat) + tcol;
            int hmUp, fUp;
            if (s == 0) {
                hmUp = (topGap ? borderGap(j, open, ext) : 0) - open;
                fUp = kNegInf;
            } else {
                const int2 above = bnd[(int64_t)j * kLanes];
                hmUp = above.x;
                fUp = above.y;
            }
            int hmDiag = aboveHmPrev;
            aboveHmPrev = hmUp;
            const bool colOk = j < L, lastCol = j == L - 1;
            const int bestBefore = sbest;
#pragma unroll
            for (int i = 0; i < kLanes; ++i) {
                if ((i & 7) == 0 && i >= rowsHere) break;  // wave-uniform
                const uint32_t off = (i & 1) ? (qo[i >> 1] >> 16) : (qo[i >> 1] & 0xffffu);
                const int sc = *(const int*)(mcol + off);
                const int e = max(HM[i], E[i] - ext);
                const int f = max(hmUp, fUp - ext);
                const int d = hmDiag + sc;
                const int h = max(max(d, floorV), max(e, f));
                bool cand = true;  // kAllCells (with the floor): pad rows / columns never beat a valid cell
                if (REGION == kLastCell) cand = lastCol && row0 + i == Q - 1;
                if (REGION == kLastRow) cand = colOk && row0 + i == Q - 1;
                if (REGION == kLastRowCol) cand = colOk && (row0 + i == Q - 1 || (lastCol && row0 + i < Q));
                const bool take = cand && h > sbest;
                sbest = take ? h : sbest;
                if (LOC) srow = take ? i : srow;
                const int hm = h - open;
                hmDiag = HM[i];
                HM[i] = hm;
                E[i] = e;
                hmUp = hm;
                fUp = f;
            }
            // (after a full strip hmUp / fUp are those of its last row)
            if (toNext) bnd[(int64_t)j * kLanes] = make_int2(hmUp, fUp);
            if (LOC) scol = sbest != bestBefore ? j : scol;  // candidates only ever raise `sbest`
        }
        // fold the strip in: higher score, then smaller column, then the upper strip
        if (Q > row0 && (sbest > best || (LOC && sbest == best && scol >= 0 && scol < bcol))) {
            best = sbest;
            brow = row0 + srow;
            bcol = scol;
        }
    }

    if (active) {
        a.score[job.out] = best;
        if (LOC) {
            a.endI[job.out] = bcol >= 0 ? brow : -1;
            a.endJ[job.out] = bcol;
        }
    }
}

#ifndef MIOPAL_PAIRLIST_PSSM
// Jobs of a chunk of the pair list, built where the kernels read them: pair p aligns the whole of query
// pairQuery[p] with the whole of target pairTarget[p]. targetOff / queryBase: the pair's target and query origin,
// what launchReverseJobs / launchTraceJobs take as `offsets` and `queryBase`.
__global__ void pairlist_jobs_kernel(int n, const int32_t* pairQuery, const int64_t* pairTarget,
                                     const int32_t* queryOff, const int64_t* dbOffsets, int rules, int64_t wsStride,
                                     PairJob* jobs, int64_t* targetOff, int32_t* queryBase) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int32_t q = pairQuery[k];
    const int64_t t = pairTarget[k];
    PairJob j{};
    j.tOff = dbOffsets[t];
    j.tLen = (int32_t)(dbOffsets[t + 1] - dbOffsets[t]);
    j.tStep = 1;
    j.qOff = queryOff[q];
    j.qLen = queryOff[q + 1] - queryOff[q];
    j.qStep = 1;
    j.rules = rules;
    j.wsOff = (int64_t)k * wsStride;
    j.out = k;
    jobs[k] = j;
    targetOff[k] = j.tOff;
    queryBase[k] = j.qOff;
}
#endif

}  // namespace

#ifndef MIOPAL_PAIRLIST_PSSM
hipError_t launchPairListJobs(int n, const int32_t* pairQuery, const int64_t* pairTarget, const int32_t* queryOff,
                              const int64_t* dbOffsets, int rules, int64_t wsStride, PairJob* jobs,
                              int64_t* targetOff, int32_t* queryBase, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pairlist_jobs_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, pairQuery, pairTarget,
                       queryOff, dbOffsets, rules, wsStride, jobs, targetOff, queryBase);
    return hipGetLastError();
}

#endif

// (pairlist.o: launchPairListForward, which hands a list with position-specific scores to launchPairListForwardPssm
// of pairlist_pssm.o: the row-indexed form, when the list's table fits - the host asks perPairPssmBytes first)
#ifdef MIOPAL_PAIRLIST_PSSM
hipError_t launchPairListForwardPssm(const PerPairArgs& a, int region, bool locate, hipStream_t stream) {
#else
hipError_t launchPairListForward(const PerPairArgs& a, int region, bool locate, hipStream_t stream) {
#endif
    if (a.nJobs <= 0) return hipSuccess;
    if (!a.score || (locate && (!a.endI || !a.endJ))) return hipErrorInvalidValue;
    const dim3 grid((a.nJobs + kBlock - 1) / kBlock), block(kBlock);
#ifdef MIOPAL_PAIRLIST_PSSM
    const size_t lds = a.rows ? perPairPssmBytes(a.queryLength, a.alphabet) : 0;
    if (lds == 0) return hipErrorInvalidValue;
#else
    if (a.rows) return launchPairListForwardPssm(a, region, locate, stream);
    const size_t lds = 0;
#endif
#define MIOPAL_PAIRLIST_GO(R)                                                                                        \
    do {                                                                                                             \
        if (locate) hipLaunchKernelGGL((pairlist_forward_kernel<R, true, kPssmUnit>), grid, block, lds, stream, a);  \
        else hipLaunchKernelGGL((pairlist_forward_kernel<R, false, kPssmUnit>), grid, block, lds, stream, a);        \
    } while (0)
    switch (region) {
        case kAllCells: MIOPAL_PAIRLIST_GO(kAllCells); break;
        case kLastRow: MIOPAL_PAIRLIST_GO(kLastRow); break;
        case kLastRowCol: MIOPAL_PAIRLIST_GO(kLastRowCol); break;
        case kLastCell: MIOPAL_PAIRLIST_GO(kLastCell); break;
        default: return hipErrorInvalidValue;
    }
#undef MIOPAL_PAIRLIST_GO
    return hipGetLastError();
}

}  // namespace miopal
