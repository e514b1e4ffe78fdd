// Every occurrence of one query in each target, for gfx950 (occurrences.h; miopalSearchOccurrences, host_occurrences.inc).
//
// occurrences_sweep_kernel is pairlist_forward_kernel's sweep (pairlist.hip, the model to read first): one lane owns
// one target and walks it column by column at 32 bit, H and E of up to 64 query rows in VGPRs (scaled by the column,
// as perpair_kernel keeps them: six operations a cell), taller queries strip by strip with the strip's last row handed
// down through HBM. What differs:
//   * every lane aligns the SAME query, so what a row looks up is wave-uniform. Plain form: the strip's query profile
//     prof[row of the strip][residue] (64 x 33 ints, `open` folded in, pad rows behind the query and a pad column) is
//     built in LDS once per strip and a cell's score sits at (target residue) + a compile-time row offset - no row
//     offsets in VGPRs, no address arithmetic per cell. PSSM form (occurrences_pssm.hip defines MIOPAL_OCCURRENCES_PSSM
//     and includes this file, as pairlist_pssm.hip does): the PSSM's rows are ONE table in dynamic LDS,
//     pairlist_forward_kernel<., ., true>'s layout with pad rows up to a multiple of eight in the pad row's place
//     (perPairPssmBytes: the host refuses taller PSSMs), and a lane walks down its residue's column row by row;
//   * no best cell is kept: after each column of the LAST strip the lane feeds (column, value, row) to
//     OccurrencePicker. HW (REGION kLastRow): the value is H of the query's last row. SW (kAllCells): the column's
//     maximum and the smallest row that reaches it, carried from strip to strip beside the boundary row in a second
//     array (the upper strip wins ties); the count pass has no use for the row and keeps the maximum alone;
//   * WRITE = false counts the picker's emissions per target, WRITE = true stores them at the target's offset.
// Rows behind the query and columns behind the target read pad scores: under SW a pad row never exceeds the query's
// last row in the same column (its E and F are bounded by that row's, by induction over the columns), so the column's
// maximum and its smallest row are those of the valid rows; under HW pad rows lie below the row that is read.
// Columns behind the target are never fed to the picker.
//
// occurrences_pick_kernel (the hook, miopalTestPickOccurrences) runs the same picker on rows of values the caller
// supplies, through the same launchers. The offsets are a three-kernel exclusive scan that also lists, in ascending
// order, the entries that have occurrences: the write sweep runs over those alone.
#include "occurrences.h"
#include "occurrence_picker.h"   // OccurrencePicker: the rule, shared with occurrences_batch.hip
#include "launch_layer.h"

namespace miopal {

namespace {

constexpr int kNegInf = INT32_MIN / 4;
constexpr int kPadScore = -(1 << 28);
constexpr int kStride = kMaxAlphabet + 1;  // profile rows in LDS, in ints (pad column included)
constexpr int kBlock = 256;
// rows of the PSSM form's LDS table: the query's, then pad rows up to a multiple of eight
__host__ __device__ constexpr int occurrencePssmRows(int queryLength) { return (queryLength + 7) / 8 * 8; }
#ifdef MIOPAL_OCCURRENCES_PSSM
constexpr bool kPssmUnit = true;
#else
constexpr bool kPssmUnit = false;
#endif

template <int REGION, bool WRITE, bool PSSM>
__global__ __launch_bounds__(kBlock) void occurrences_sweep_kernel(OccurrenceArgs a) {
    static_assert(REGION == kLastRow || REGION == kAllCells, "HW or SW");
    constexpr bool SW = REGION == kAllCells;
    constexpr bool ROWS = SW && WRITE;   // the row of a column's maximum: only the write pass stores it
    __shared__ int prof[PSSM ? 1 : kLanes * kStride];
    extern __shared__ __attribute__((aligned(16))) int pssmTable[];
    const int A = a.alphabet, Q = a.queryLength;
    const int open = a.gapOpen, ext = a.gapExt;
    [[maybe_unused]] const int pssmRowInts = A + 1;
    if constexpr (PSSM) {
        // (rows up to the next multiple of eight: what the last strip's row groups read)
        for (int idx = threadIdx.x; idx < occurrencePssmRows(Q) * pssmRowInts; idx += kBlock) {
            const int q = idx / pssmRowInts, t = idx - q * pssmRowInts;
            pssmTable[idx] = (q < Q && t < A) ? a.rows[q * A + t] + open : kPadScore;
        }
        __syncthreads();
    }

    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    const bool active = idx < a.nJobs;
    PairJob job{};
    if (active) job = a.jobs[idx];
    const int L = job.tLen;
    // The columns are kept SCALED, perpair_kernel's way: what is stored for column j is the value + j * ext, so that
    // extending a horizontal gap costs nothing (E'[j] = max(H'[j - 1] - c, E'[j - 1]), c = open - ext), and HM holds
    // H' - c. A column's own cells share one scale: F and the strip boundaries are unaffected, SW's floor is the scale
    // itself, and the picker is handed the value less the scale. (Q + longest target) * ext is within the range check.
    const int c = open - ext;

    int maxL = L;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxL = max(maxL, __shfl_xor(maxL, off));
    maxL = __builtin_amdgcn_readfirstlane(maxL);
    const int nStrips = (Q + kLanes - 1) / kLanes;   // the same for every wavefront: one query

    const uint8_t* tptr = a.residues + job.tOff;
    const int64_t waveBase = (int64_t)(idx >> 6) * a.boundaryStride * kLanes + lane;
    int2* bnd = a.boundary ? a.boundary + waveBase : nullptr;
    [[maybe_unused]] int2* car = a.carry ? a.carry + waveBase : nullptr;

    OccurrencePicker pick(a.minScore, a.window);
    int found = 0;
    const int64_t at = (WRITE && active) ? a.offsets[job.out] : 0;
    const int64_t target = a.start + job.out;
    auto emit = [&](int j, int v, int r) {
        if constexpr (WRITE) {
            a.outTarget[at + found] = target;
            a.outScore[at + found] = v;
            a.outColumn[at + found] = j;
            a.outRow[at + found] = r;
        }
        ++found;
    };

    for (int s = 0; s < nStrips; ++s) {
        const int row0 = s * kLanes;
        const int rowsHere = min(Q - row0, kLanes);
        const bool toNext = s + 1 < nStrips;
        // HW: the row that is read, counted inside its group of eight
        [[maybe_unused]] const int lastSub = (Q - 1 - row0) & 7;
        if constexpr (!PSSM) {
            // the strip's profile; every wavefront of the block is between two strips here (one query: one strip count)
            if (s > 0) __syncthreads();
            for (int k = threadIdx.x; k < kLanes * kStride; k += kBlock) {
                const int i = k / kStride, t = k - i * kStride;
                prof[k] = (row0 + i < Q && t < A) ? a.matrix[(int)a.query[row0 + i] * A + t] + open : kPadScore;
            }
            __syncthreads();
        }
        int HM[kLanes], E[kLanes];
#pragma unroll
        for (int i = 0; i < kLanes; ++i) {
            HM[i] = row0 + i < Q ? (SW ? 0 : borderGap(row0 + i, open, ext)) - open : kNegInf;  // column -1 (scaled by -ext, less c)
            E[i] = kNegInf;
        }
        // row above the strip at column j - 1 (diagonal of the strip's first row)
        int aboveHmPrev = (s == 0 || SW ? 0 : borderGap(row0 - 1, open, ext)) - open;

        int tcolNext = (L > 0 ? (int)tptr[0] : A) * 4;
        int scale = 0;   // j * ext
        for (int j = 0; j < maxL; ++j, scale += ext) {
            const int tcol = tcolNext;
            {
                int t = A;
                if (j + 1 < L) t = tptr[j + 1];
                tcolNext = t * 4;
            }
            const char* mcol = (PSSM ? (const char*)pssmTable : (const char*)prof) + tcol;
            int hmUp, fUp;
            int cmax = scale, crow = -1 - row0;   // SW: the column's maximum so far and its row, counted from the strip's first
            if (s == 0) {
                hmUp = scale - c;   // the top row is free under HW and SW
                fUp = kNegInf;
            } else {
                const int2 above = bnd[(int64_t)j * kLanes];
                hmUp = above.x;
                fUp = above.y;
                if constexpr (SW) {
                    const int2 carried = car[(int64_t)j * kLanes];
                    cmax = carried.x;
                    crow = carried.y - row0;
                }
            }
            int hmDiag = aboveHmPrev;
            aboveHmPrev = hmUp;
            int v = kNegInf;   // HW: H of the query's last row
            [[maybe_unused]] int hg[8];
            [[maybe_unused]] const char* prow = mcol + row0 * pssmRowInts * 4;   // PSSM: the row's scores, row by row
#pragma unroll
            for (int i = 0; i < kLanes; ++i) {
                if ((i & 7) == 0 && i >= rowsHere) break;  // wave-uniform
                int sc;
                if constexpr (PSSM) {
                    sc = *(const int*)prow;
                    prow += pssmRowInts * 4;
                } else {
                    sc = *(const int*)(mcol + i * kStride * 4);
                }
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
                // the query's last row lies in the last group of the last strip
                if (!toNext) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v = k == lastSub ? hg[k] : v;
                }
            }
            if (toNext) {
                bnd[(int64_t)j * kLanes] = make_int2(hmUp, fUp);
                if constexpr (SW) car[(int64_t)j * kLanes] = make_int2(cmax, crow + row0);
            } else if (j < L) {
                pick.feed(j, (SW ? cmax : v) - scale, SW ? crow + row0 : Q - 1, emit);
            }
        }
    }
    pick.finish(emit);
    if (!WRITE && active) a.count[job.out] = found;
}

#ifndef MIOPAL_OCCURRENCES_PSSM
// the hook: the picker on row r of the caller's values, one lane per row
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void occurrences_pick_kernel(OccurrenceArgs a) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= a.nJobs) return;
    const int64_t r = WRITE ? a.list[k] : k;
    const int L = a.length[r];
    const int32_t* value = a.value + r * a.stride;
    const int32_t* valueRow = a.valueRow ? a.valueRow + r * a.stride : nullptr;
    OccurrencePicker pick(a.minScore, a.window);
    int found = 0;
    const int64_t at = WRITE ? a.offsets[r] : 0;
    auto emit = [&](int j, int v, int row) {
        if constexpr (WRITE) {
            a.outScore[at + found] = v;
            a.outColumn[at + found] = j;
            a.outRow[at + found] = row;
        }
        ++found;
    };
    for (int j = 0; j < L; ++j) pick.feed(j, value[j], valueRow ? valueRow[j] : -1, emit);
    pick.finish(emit);
    if (!WRITE) a.count[r] = found;
}

__global__ void occurrences_jobs_kernel(const int32_t* list, int64_t first, int n, const int64_t* dbOffsets, int64_t start,
                                        int queryLength, PairJob* jobs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t pos = list ? (int64_t)list[first + k] : first + k;
    const int64_t t = start + pos;
    PairJob j{};
    j.tOff = dbOffsets[t];
    j.tLen = (int32_t)(dbOffsets[t + 1] - dbOffsets[t]);
    j.tStep = 1;
    j.qLen = queryLength;
    j.qStep = 1;
    j.out = (int32_t)pos;
    jobs[k] = j;
}

// ---- offsets: exclusive scan of count[n], and the list of the entries whose count is not 0 -------------------------
constexpr int kScanPerThread = kOccScanBlock / kBlock;

// sums of the block's values (x) and of its non-zero entries (y), exclusive per thread, totals in *tx / *ty
__device__ void blockScan(int64_t x, int y, int64_t* exclX, int* exclY, int64_t* tx, int* ty) {
    __shared__ int64_t waveX[kBlock / kLanes];
    __shared__ int waveY[kBlock / kLanes];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t ix = x;
    int iy = y;
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) {
        const int64_t ux = __shfl_up(ix, off);
        const int uy = __shfl_up(iy, off);
        if (lane >= off) {
            ix += ux;
            iy += uy;
        }
    }
    __syncthreads();   // (the arrays of an earlier call are read no more)
    if (lane == kLanes - 1) {
        waveX[wave] = ix;
        waveY[wave] = iy;
    }
    __syncthreads();
    int64_t bx = 0, sx = 0;
    int by = 0, sy = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kLanes; ++w) {
        if (w < wave) {
            bx += waveX[w];
            by += waveY[w];
        }
        sx += waveX[w];
        sy += waveY[w];
    }
    *exclX = bx + ix - x;
    *exclY = by + iy - y;
    *tx = sx;
    *ty = sy;
}

__global__ __launch_bounds__(kBlock) void occurrences_block_sums_kernel(OccurrenceScratch sc, int64_t n) {
    const int64_t base = (int64_t)blockIdx.x * kOccScanBlock + threadIdx.x * kScanPerThread;
    int64_t x = 0;
    int y = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k)
        if (base + k < n) {
            const int c = sc.count[base + k];
            x += c;
            y += c != 0;
        }
    int64_t ex, tx;
    int ey, ty;
    blockScan(x, y, &ex, &ey, &tx, &ty);
    if (threadIdx.x == 0) {
        sc.blockSum[blockIdx.x] = tx;
        sc.blockListed[blockIdx.x] = ty;
    }
}

// one workgroup: the block sums become the sums of the blocks in front, the totals are written
__global__ __launch_bounds__(kBlock) void occurrences_scan_blocks_kernel(OccurrenceScratch sc, int64_t n, int64_t blocks) {
    int64_t runX = 0;
    int runY = 0;
    for (int64_t b0 = 0; b0 < blocks; b0 += kBlock) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t x = b < blocks ? sc.blockSum[b] : 0;
        const int y = b < blocks ? sc.blockListed[b] : 0;
        int64_t ex, tx;
        int ey, ty;
        blockScan(x, y, &ex, &ey, &tx, &ty);
        if (b < blocks) {
            sc.blockSum[b] = runX + ex;
            sc.blockListed[b] = runY + ey;
        }
        runX += tx;
        runY += ty;
    }
    if (threadIdx.x == 0) {
        sc.offsets[n] = runX;
        sc.totals[0] = runX;
        sc.totals[1] = runY;
    }
}

__global__ __launch_bounds__(kBlock) void occurrences_offsets_kernel(OccurrenceScratch sc, int64_t n) {
    const int64_t base = (int64_t)blockIdx.x * kOccScanBlock + threadIdx.x * kScanPerThread;
    int c[kScanPerThread];
    int64_t x = 0;
    int y = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        c[k] = base + k < n ? sc.count[base + k] : 0;
        x += c[k];
        y += c[k] != 0;
    }
    int64_t ex, tx;
    int ey, ty;
    blockScan(x, y, &ex, &ey, &tx, &ty);
    int64_t atX = sc.blockSum[blockIdx.x] + ex;
    int atY = sc.blockListed[blockIdx.x] + ey;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k)
        if (base + k < n) {
            sc.offsets[base + k] = atX;
            if (c[k] != 0) sc.list[atY++] = (int32_t)(base + k);
            atX += c[k];
        }
}
#endif

}  // namespace

#ifndef MIOPAL_OCCURRENCES_PSSM
size_t occurrenceScratchBytes(int64_t n) {
    const size_t blocks = (size_t)((n + kOccScanBlock - 1) / kOccScanBlock);
    return sizeof(int64_t) * ((size_t)n + 1 + 2 + blocks) + sizeof(int32_t) * (blocks + 2 * (size_t)n);
}

OccurrenceScratch occurrenceScratchLayout(void* base, int64_t n) {
    const size_t blocks = (size_t)((n + kOccScanBlock - 1) / kOccScanBlock);
    OccurrenceScratch sc;
    sc.offsets = (int64_t*)base;
    sc.totals = sc.offsets + n + 1;
    sc.blockSum = sc.totals + 2;
    sc.blockListed = (int32_t*)(sc.blockSum + blocks);
    sc.count = sc.blockListed + blocks;
    sc.list = sc.count + n;
    return sc;
}

hipError_t launchOccurrenceJobs(const int32_t* list, int64_t first, int n, int64_t start, const int64_t* dbOffsets,
                                int queryLength, PairJob* jobs, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(occurrences_jobs_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, list, first, n, dbOffsets, start,
                       queryLength, jobs);
    return hipGetLastError();
}

hipError_t launchOccurrencesOffsets(const OccurrenceScratch& sc, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipErrorInvalidValue;
    const int64_t blocks = (n + kOccScanBlock - 1) / kOccScanBlock;
    hipLaunchKernelGGL(occurrences_block_sums_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, sc, n);
    hipLaunchKernelGGL(occurrences_scan_blocks_kernel, dim3(1), dim3(kBlock), 0, stream, sc, n, blocks);
    hipLaunchKernelGGL(occurrences_offsets_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, sc, n);
    return hipGetLastError();
}
#endif

// the sweep of this unit: occurrences.o the plain form, occurrences_pssm.o the row-indexed one
static hipError_t launchSweep(const OccurrenceArgs& a, int region, bool write, hipStream_t stream) {
    if (a.nJobs <= 0) return hipSuccess;
    if (region != kLastRow && region != kAllCells) return hipErrorInvalidValue;
    if (a.queryLength <= 0 || !a.jobs || (write ? !a.offsets || !a.outTarget || !a.outScore || !a.outColumn || !a.outRow : !a.count))
        return hipErrorInvalidValue;
    if (a.queryLength > kLanes && (!a.boundary || (region == kAllCells && !a.carry))) return hipErrorInvalidValue;
    const dim3 grid((a.nJobs + kBlock - 1) / kBlock), block(kBlock);
    // (the PSSM's table with its pad rows may pass the 64 KB of a plain launch by a few hundred bytes)
    const size_t lds = kPssmUnit ? (size_t)occurrencePssmRows(a.queryLength) * (a.alphabet + 1) * sizeof(int) : 0;
    if (kPssmUnit ? (!a.rows || perPairPssmBytes(a.queryLength, a.alphabet) == 0) : (!a.query || !a.matrix)) return hipErrorInvalidValue;
#define MIOPAL_OCCURRENCES_LAUNCH(R, W)                                                                                \
    do {                                                                                                               \
        if (kPssmUnit) {                                                                                               \
            const hipError_t e = allowFullLds<occurrences_sweep_kernel<R, W, kPssmUnit>>();                           \
            if (e != hipSuccess) return e;                                                                             \
        }                                                                                                              \
        hipLaunchKernelGGL((occurrences_sweep_kernel<R, W, kPssmUnit>), grid, block, lds, stream, a);                 \
    } while (0)
#define MIOPAL_OCCURRENCES_GO(R)                                                                                       \
    do {                                                                                                               \
        if (write) MIOPAL_OCCURRENCES_LAUNCH(R, true);                                                                \
        else MIOPAL_OCCURRENCES_LAUNCH(R, false);                                                                     \
    } while (0)
    if (region == kLastRow) MIOPAL_OCCURRENCES_GO(kLastRow);
    else MIOPAL_OCCURRENCES_GO(kAllCells);
#undef MIOPAL_OCCURRENCES_GO
#undef MIOPAL_OCCURRENCES_LAUNCH
    return hipGetLastError();
}

#ifdef MIOPAL_OCCURRENCES_PSSM
hipError_t launchOccurrencesSweepPssm(const OccurrenceArgs& a, int region, bool write, hipStream_t stream) {
    return launchSweep(a, region, write, stream);
}
#else
static hipError_t launchPick(const OccurrenceArgs& a, bool write, hipStream_t stream) {
    if (a.nJobs <= 0) return hipSuccess;
    if (!a.length || a.stride < 1 || (write ? !a.list || !a.offsets || !a.outScore || !a.outColumn || !a.outRow : !a.count))
        return hipErrorInvalidValue;
    const dim3 grid((a.nJobs + kBlock - 1) / kBlock), block(kBlock);
    if (write) hipLaunchKernelGGL(occurrences_pick_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(occurrences_pick_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launchOccurrencesCount(const OccurrenceArgs& a, int region, hipStream_t stream) {
    if (a.value) return launchPick(a, false, stream);
    if (a.rows) return launchOccurrencesSweepPssm(a, region, false, stream);
    return launchSweep(a, region, false, stream);
}

hipError_t launchOccurrencesWrite(const OccurrenceArgs& a, int region, hipStream_t stream) {
    if (a.value) return launchPick(a, true, stream);
    if (a.rows) return launchOccurrencesSweepPssm(a, region, true, stream);
    return launchSweep(a, region, true, stream);
}
#endif

}  // namespace miopal
