// Batch forms of the one-strip pair-table kernels: many queries of at most 64 rows against one packed view in
// ONE persistent launch (miopalSearchBatch, host_batch.inc).
//
// A search of one short query against a database of a few ten thousand targets cannot fill the chip: 20 000
// targets are 157 groups of 128 for 256 workgroups x 12 wavefronts. Here the work is handed out as units of
// (query, run of groups), query-major, from a global counter:
//  * a workgroup takes a unit and, when its query differs from the one whose pair table it holds, rebuilds the
//    table from that query's profile (the strips kernels' rebuild: 150 KB of LDS writes, a few microseconds);
//  * the wavefronts of the workgroup take the unit's groups from an LDS counter (view order: longest first)
//    and sweep each exactly as the single-query kernel does;
//  * a barrier ends the unit (the table and the counter are then free for the next one).
// The host sizes the runs so that every workgroup gets work with few queries (a query's groups cut into
// several units) and the rebuild stays small next to the sweep with many (one unit per query).
//
// Rows: one launch serves the queries of one row class R (multiples of 8, and 60); a query of Q < R rows is
// padded with the padding symbol's score, which the kernels already handle:
//  * Smith-Waterman: a padding row's cell is below the real cell above it or equal to it (open = 0), never
//    strictly above every real cell of its column and the columns before; the column maximum keeps the FIRST
//    row of a tie and the running best moves on strictly greater values only, so neither a score nor an end
//    cell changes (tests/test_gpu_batch.py checks it, the best-is-0 tie included);
//  * NW / HW / OV: nothing flows upwards, and the answers are read on row Q - 1 (a select tree over the last
//    eight rows) and, for OV's last column, on rows below Q only.
// Results go straight to [row][target] database order (directOut style); the Smith-Waterman lanes that reach
// the biased range's limit are flagged per (query, lane half) and counted per query, and the host recomputes
// them with the int32 kernel. NW / HW / OV flag nothing (the host checks the static bounds with R rows).
#pragma once
#include "interseq_impl.h"

namespace miopal {

// (the last row of a query of class R lies in [R - 8, R - 1])
__host__ __device__ constexpr int batchRowLo(int R) { return R > 8 ? R - 8 : 0; }

// the unit a workgroup works on: every thread calls this; returns the query index (>= nQueries: done)
static __device__ __forceinline__ int batchTakeUnit(const BatchArgs& a, int* ctl, int* part) {
    __syncthreads();   // (everybody is done with the unit before: table and group counter are free)
    if (threadIdx.x == 0) {
        ctl[0] = atomicAdd(a.unitCounter, 1);
        ctl[1] = 0;
    }
    __syncthreads();
    const int unit = __builtin_amdgcn_readfirstlane(ctl[0]);
    const int q = unit / a.unitsPerQuery;
    *part = unit - q * a.unitsPerQuery;
    return q;
}

// next group of the unit for this wavefront (wave-uniform; >= end: none left)
static __device__ __forceinline__ int batchTakeGroup(int* ctl, int first, int lane) {
    int g = 0;
    if (lane == 0) g = atomicAdd(&ctl[1], 1);
    return __builtin_amdgcn_readfirstlane(g) + first;
}

// ---- Smith-Waterman: interseq_pair_biased_kernel<R, LOC>'s sweep, per (query, group) ---------------------
// Twelve wavefronts per workgroup (168 VGPRs) up to 56 rows, eight (256 VGPRs) beyond: the unit bookkeeping
// beside H[R], E[R] does not leave a 60- or 64-row column room in 168 registers.
__host__ __device__ constexpr int batchSwWaves(int rows) { return rows <= 56 ? kPairWavesPerGroup : 8; }

template <int R, bool LOC>
__global__ __launch_bounds__(batchSwWaves(R) * kLanes) void interseq_batch_sw_kernel(BatchArgs a) {
    constexpr int SLOTS = PairLayout<R>::kRowSlots;
    constexpr int NB4 = (R + 3) / 4;
    constexpr int kBits = LOC ? locRowBits(R) : 0;
    constexpr int kRowMask = (1 << kBits) - 1;
    extern __shared__ uint4 pairs[];

    const int lane = threadIdx.x & 63;
    const int nSym = a.nSymbols;
    const int ext = a.gapExt << kBits;   // pattern units
    const uint32_t ext2 = both(ext), openMinusExt2 = both((a.gapOpen << kBits) - ext);
    const uint32_t zero2 = both(LOC ? kLocZeroPattern : kBiasedZero);
    int* ctl = reinterpret_cast<int*>(pairs + nSym * nSym * SLOTS);   // [0] unit, [1] next group of the unit
    int tableQuery = -1;

    for (;;) {
        int part = 0;
        const int q = batchTakeUnit(a, ctl, &part);
        if (q >= a.nQueries) break;
        if (q != tableQuery) {
            // the table of this query: one thread per (pair row, query row), as the single-query kernel
            const int16_t* gp = a.profiles + (size_t)q * nSym * R;
            uint32_t* pw = reinterpret_cast<uint32_t*>(pairs);
            const int total = nSym * nSym * R;
            for (int idx = threadIdx.x; idx < total; idx += batchSwWaves(R) * kLanes) {
                const int row = idx / R, r = idx - row * R;
                const int tA = row / nSym, tB = row - tA * nSym;
                constexpr int kPadPattern = LOC ? -kLocGuardBand : kBiasedPad;
                const int vA = gp[tA * R + r], vB = gp[tB * R + r];
                const int sA = (vA == kBiasedPad ? kPadPattern : vA << kBits) + ext;
                const int sB = (vB == kBiasedPad ? kPadPattern : vB << kBits) + ext;
                pw[row * (SLOTS * 4) + r] = (uint32_t)(sB * 65536 + sA);
            }
            tableQuery = q;
            __syncthreads();
        }
        const int first = a.unitFirst[part], last = a.unitFirst[part + 1];
        const int outRow = a.qRows[q];
        for (;;) {
            const int g = batchTakeGroup(ctl, first, lane);
            if (g >= last) break;
            const uint2* pack = a.pack + a.groupOff[g];
            const int nChunks = a.groupChunks[g];
            uint32_t best = 0u;
            int colA = -1, colB = -1;
            uint32_t fl = zero2 - ext2;
            int shift = -ext;
            uint32_t H[R], E[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                H[r] = fl;
                E[r] = zero2;
            }
            uint2 cur = pack[lane];
            auto rowOf = [&](uint32_t tA, uint32_t tB) -> const uint4* {
                const uint32_t rowIdx = __umul24(tA, (uint32_t)nSym) + tB;
                return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(pairs) +
                                                      __umul24(rowIdx, (uint32_t)(SLOTS * 16)));
            };
            // (prefetch depth: three blocks; at 56 rows the unit bookkeeping takes the registers of one or two)
            constexpr int kWant = R == 56 ? (LOC ? 1 : 2) : 3;
            constexpr int kAhead = NB4 > kWant ? kWant : 1;
            const uint4* prowNext = rowOf(cur.x & 0xffu, cur.y & 0xffu);
            uint4 vn[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
            for (int c = 0; c < nChunks; ++c) {
                uint2 nxt = {0, 0};
                if (c + 1 < nChunks) nxt = pack[(size_t)(c + 1) * kLanes + lane];
                uint32_t ra = cur.x, rb = cur.y;
#pragma unroll 1
                for (int cc = 0; cc < 4; ++cc) {
                    const uint4* prow = prowNext;
                    uint4 v[NB4];
#pragma unroll
                    for (int k = 0; k < kAhead; ++k) v[k] = vn[k];
                    ra = cc < 3 ? ra >> 8 : nxt.x;
                    rb = cc < 3 ? rb >> 8 : nxt.y;
                    prowNext = rowOf(ra & 0xffu, rb & 0xffu);
                    auto score = [&](int r) -> uint32_t {
                        const uint4 x = v[r >> 2];
                        const int k = r & 3;
                        return k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w;
                    };
                    uint32_t dsum = fl + score(0);
                    fl += ext2;
                    uint32_t fl1 = fl + ext2;
                    asm volatile("" : "+v"(fl1));
                    uint32_t f = fl, cm = fl, held = fl;
#pragma unroll
                    for (int r4 = 0; r4 < NB4; ++r4) {
                        if (r4 + kAhead < NB4) v[r4 + kAhead] = prow[r4 + kAhead];
                        if (r4 == (NB4 > 3 ? NB4 - 3 : 0)) {
#pragma unroll
                            for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int r = r4 * 4 + k;
                            if (r >= R) continue;
                            uint32_t dnext = 0;
                            if (r + 1 < R) dnext = H[r] + score(r + 1);
                            const uint32_t h = pk_max3_f16(dsum, E[r], f);
                            const uint32_t hk = LOC ? h + both(kRowMask - r) : h;
                            if (r & 1) cm = pk_max3_f16(cm, held, hk);
                            else held = hk;
                            const uint32_t hmo = h - openMinusExt2;
                            E[r] = pk_max3_f16(E[r], hmo, fl1);
                            if (r + 1 < R) f = pk_max3_f16(f, hmo, fl1) - ext2;
                            H[r] = h;
                            dsum = dnext;
                        }
                        asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
                    }
                    if (R & 1) cm = pk_max3_f16(cm, held, held);
                    if constexpr (LOC) {
                        const uint32_t cand = cm - fl, thr = best | both(kRowMask);
                        const uint32_t ch = pk_max_u16(thr, cand) ^ thr;
                        const int j = c * 4 + cc;
                        if (ch & 0xffffu) {
                            best = (best & 0xffff0000u) | (cand & 0xffffu);
                            colA = j;
                        }
                        if (ch >> 16) {
                            best = (best & 0xffffu) | (cand & 0xffff0000u);
                            colB = j;
                        }
                    } else {
                        best = pk_max_u16(best, cm - fl);
                    }
                }
                cur = nxt;
                shift += 4 * ext;
                if (shift + 4 * ext > kBiasedMaxShift) {
                    const uint32_t d = both(shift);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        H[r] -= d;
                        E[r] -= d;
                    }
                    fl -= d;
                    shift = 0;
                }
            }
            const int lo = (int)(best & 0xffffu) >> kBits, hi = (int)(best >> 16) >> kBits;
            const int posA = g * kGroupTargets + lane, posB = posA + kLanes;
            const size_t rowBase = (size_t)outRow * a.outStride;
            auto put = [&](int pos, int value, int col, uint32_t half) {
                if (pos >= a.nPacked) return;
                const size_t at = rowBase + (size_t)(a.ids[pos] - a.sliceStart);
                a.score[at] = value;
                if constexpr (LOC) {
                    a.endI[at] = col < 0 ? -1 : kRowMask - (int)(half & kRowMask);
                    a.endJ[at] = col;
                }
                const bool flag = value >= a.biasedLimit;
                a.overflow[(size_t)outRow * a.nPacked + pos] = flag;
                if (flag) atomicAdd(&a.overflowCount[outRow], 1);
            };
            put(posA, lo, colA, best & 0xffffu);
            put(posB, hi, colB, best >> 16);
        }
    }
}

template <int R, bool LOC>
static hipError_t launchBatchSwR(const BatchArgs& a, int computeUnits, hipStream_t stream) {
    const size_t lds = PairLayout<R>::bytes(a.nSymbols) + 16;   // table + unit / group counters
    if (const hipError_t e = allowFullLds<&interseq_batch_sw_kernel<R, LOC>>(); e != hipSuccess) return e;
    const int blocks = std::max(1, std::min(computeUnits, a.nQueries * a.unitsPerQuery));
    hipLaunchKernelGGL((interseq_batch_sw_kernel<R, LOC>), dim3(blocks), dim3(batchSwWaves(R) * kLanes), lds, stream, a);
    return hipGetLastError();
}

// ---- NW / HW / OV: interseq_pair_global_kernel<R>'s sweep, per (query, group) ----------------------------
template <int R>
__global__ __launch_bounds__(globalWaves(R) * kLanes) void interseq_batch_global_kernel(BatchArgs a) {
    constexpr int kGlobalWaves = globalWaves(R);
    constexpr int SLOTS = PairLayout<R>::kRowSlots;
    constexpr int NB4 = (R + 3) / 4;
    constexpr int kLo = batchRowLo(R);
    extern __shared__ uint4 pairs[];

    const int lane = threadIdx.x & 63;
    const int nSym = a.nSymbols;
    const int ext = a.gapExt, open = a.gapOpen;
    const int zero = a.biasedZero;
    const bool topGap = a.topGap, leftGap = a.leftGap;
    const int region = a.region;
    const bool locate = a.endI != nullptr;
    const uint32_t openMinusExt2 = both(open - ext);
    int* ctl = reinterpret_cast<int*>(pairs + nSym * nSym * SLOTS);
    int tableQuery = -1;

    for (;;) {
        int part = 0;
        const int q = batchTakeUnit(a, ctl, &part);
        if (q >= a.nQueries) break;
        if (q != tableQuery) {
            const int16_t* gp = a.profiles + (size_t)q * nSym * R;
            uint32_t* pw = reinterpret_cast<uint32_t*>(pairs);
            const int total = nSym * nSym * R;
            for (int idx = threadIdx.x; idx < total; idx += kGlobalWaves * kLanes) {
                const int row = idx / R, r = idx - row * R;
                const int tA = row / nSym, tB = row - tA * nSym;
                const int vA = gp[tA * R + r], vB = gp[tB * R + r];
                const int sA = vA == kBiasedPad ? open - ext : vA + ext + open;
                const int sB = vB == kBiasedPad ? open - ext : vB + ext + open;
                pw[row * (SLOTS * 4) + r] = (uint32_t)(sB * 65536 + sA);
            }
            tableQuery = q;
            __syncthreads();
        }
        const int first = a.unitFirst[part], last = a.unitFirst[part + 1];
        const int outRow = a.qRows[q];
        const int Q = a.qLens[q];   // (wave-uniform: R - 8 < Q <= R)
        for (;;) {
            const int g = batchTakeGroup(ctl, first, lane);
            if (g >= last) break;
            const uint2* pack = a.pack + a.groupOff[g];
            const int nChunks = a.groupChunks[g];
            const size_t base = (size_t)g * kGroupTargets;
            const int lenA = a.lens[base + lane], lenB = a.lens[base + kLanes + lane];
            int runA = INT32_MIN, runB = INT32_MIN, colA = -1, colB = -1, rowA = -1, rowB = -1;
            int cbA = INT32_MIN, cbB = INT32_MIN, crowA = -1, crowB = -1;
            int sigma = zero - ext;
            int shift = -ext;
            uint32_t H[R], E[R];
            {
                int zeroHere = zero, openHere = open, extHere = ext;
                asm volatile("" : "+s"(zeroHere), "+s"(openHere), "+s"(extHere));
                int one = openHere, many = openHere, rowShift = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int left = (leftGap ? -min(one, many) : 0) + rowShift;
                    H[r] = both(zeroHere - extHere + left - (openHere - extHere));
                    E[r] = both(zeroHere + left - openHere);
                    one += extHere;
                    many += openHere;
                    rowShift += extHere;
                }
            }
            uint2 cur = pack[lane];
            auto rowOf = [&](uint32_t tA, uint32_t tB) -> const uint4* {
                const uint32_t rowIdx = __umul24(tA, (uint32_t)nSym) + tB;
                return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(pairs) +
                                                      __umul24(rowIdx, (uint32_t)(SLOTS * 16)));
            };
            constexpr int kWant = 3;
            constexpr int kAhead = NB4 > kWant ? kWant : 1;
            const uint4* prowNext = rowOf(cur.x & 0xffu, cur.y & 0xffu);
            uint4 vn[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
            for (int c = 0; c < nChunks; ++c) {
                uint2 nxt = {0, 0};
                if (c + 1 < nChunks) nxt = pack[(size_t)(c + 1) * kLanes + lane];
                uint32_t ra = cur.x, rb = cur.y;
#pragma unroll 1
                for (int cc = 0; cc < 4; ++cc) {
                    const int j = c * 4 + cc;
                    const uint4* prow = prowNext;
                    uint4 v[NB4];
#pragma unroll
                    for (int k = 0; k < kAhead; ++k) v[k] = vn[k];
                    ra = cc < 3 ? ra >> 8 : nxt.x;
                    rb = cc < 3 ? rb >> 8 : nxt.y;
                    prowNext = rowOf(ra & 0xffu, rb & 0xffu);
                    auto score = [&](int r) -> uint32_t {
                        const uint4 x = v[r >> 2];
                        const int k = r & 3;
                        return k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w;
                    };
                    const int topPrev = (j == 0 || !topGap) ? 0 : borderGap(j - 1, open, ext);
                    const int topHere = topGap ? borderGap(j, open, ext) : 0;
                    uint32_t dsum = both(sigma + topPrev - open) + score(0);
                    sigma += ext;
                    uint32_t f = both(sigma + topHere - open);
                    asm volatile("" : "+v"(f));
#pragma unroll
                    for (int r4 = 0; r4 < NB4; ++r4) {
                        if (r4 + kAhead < NB4) v[r4 + kAhead] = prow[r4 + kAhead];
                        if (r4 == (NB4 > 3 ? NB4 - 3 : 0)) {
#pragma unroll
                            for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int r = r4 * 4 + k;
                            if (r >= R) continue;
                            uint32_t dnext = 0;
                            if (r + 1 < R) dnext = H[r] + score(r + 1);
                            const uint32_t h = pk_max3_f16(dsum, E[r], f);
                            const uint32_t hmo = h - openMinusExt2;
                            E[r] = pk_max2_f16(E[r], hmo);
                            asm volatile("" : "+v"(E[r]));
                            if (r + 1 < R) f = pk_max2_f16(f, hmo);
                            H[r] = hmo;
                            dsum = dnext;
                        }
                        asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
#pragma unroll
                        for (int k = 1; k <= 4; ++k)
                            if (r4 * 4 + 3 + k < R) asm volatile("" : "+v"(H[r4 * 4 + 3 + k]));
                    }
                    // ---- answers on the query's last row, Q - 1 (the rows below it are padding)
                    const uint32_t hq = pickRow<kLo, R - 1>(H, Q - 1);
                    const int back = sigma + (Q - 1) * ext - (open - ext);
                    const int qA = (int)(hq & 0xffffu) - back, qB = (int)(hq >> 16) - back;
                    if (region == kLastCell) {
                        if (j == lenA - 1) { runA = qA; colA = j; }
                        if (j == lenB - 1) { runB = qB; colB = j; }
                    } else {
                        const int cut = region == kLastRowCol ? 1 : 0;
                        if (j < lenA - cut && qA > runA) { runA = qA; colA = j; }
                        if (j < lenB - cut && qB > runB) { runB = qB; colB = j; }
                        const bool lastA = j == lenA - 1, lastB = j == lenB - 1;
                        if (region == kLastRowCol && __builtin_amdgcn_ballot_w64(lastA || lastB) != 0) {
                            int mA = INT32_MIN, mB = INT32_MIN, ia = 0, ib = 0;
                            int off = (R - 1) * ext;
                            asm volatile("" : "+v"(off));
#pragma unroll
                            for (int r = R - 1; r >= 0; --r) {
                                // (padding rows: only the last eight can be, one scalar test each)
                                if (r < kLo || r < Q) {
                                    const int hA = (int)(H[r] & 0xffffu) - off, hB = (int)(H[r] >> 16) - off;
                                    if (hA >= mA) { mA = hA; ia = r; }
                                    if (hB >= mB) { mB = hB; ib = r; }
                                }
                                off -= ext;
                                asm volatile("" : "+v"(mA), "+v"(mB), "+v"(off));
                            }
                            const int back2 = sigma - (open - ext);
                            if (lastA) { cbA = mA - back2; crowA = ia; }
                            if (lastB) { cbB = mB - back2; crowB = ib; }
                        }
                    }
                }
                cur = nxt;
                shift += 4 * ext;
                if (!topGap && shift + 4 * ext > kBiasedMaxShift) {
                    const uint32_t d = both(shift);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        H[r] -= d;
                        E[r] -= d;
                    }
                    sigma -= shift;
                    shift = 0;
                }
            }
            rowA = colA >= 0 ? Q - 1 : -1;
            rowB = colB >= 0 ? Q - 1 : -1;
            if (region == kLastRowCol) {
                if (crowA >= 0 && (colA < 0 || cbA > runA)) { runA = cbA; rowA = crowA; colA = lenA - 1; }
                if (crowB >= 0 && (colB < 0 || cbB > runB)) { runB = cbB; rowB = crowB; colB = lenB - 1; }
            }
            const size_t rowBase = (size_t)outRow * a.outStride;
            auto put = [&](int pos, int value, int row, int col) {
                if (pos >= a.nPacked) return;
                const size_t at = rowBase + (size_t)(a.ids[pos] - a.sliceStart);
                a.score[at] = value;
                if (locate) {
                    a.endI[at] = row;
                    a.endJ[at] = col;
                }
            };
            put((int)base + lane, runA, rowA, colA);
            put((int)base + kLanes + lane, runB, rowB, colB);
        }
    }
}

template <int R>
static hipError_t launchBatchGlobalR(const BatchArgs& a, int computeUnits, hipStream_t stream) {
    const size_t lds = PairLayout<R>::bytes(a.nSymbols) + 16;
    if (const hipError_t e = allowFullLds<&interseq_batch_global_kernel<R>>(); e != hipSuccess) return e;
    constexpr int kGlobalWaves = globalWaves(R);
    const int blocks = std::max(1, std::min(computeUnits, a.nQueries * a.unitsPerQuery));
    hipLaunchKernelGGL((interseq_batch_global_kernel<R>), dim3(blocks), dim3(kGlobalWaves * kLanes), lds, stream, a);
    return hipGetLastError();
}

}  // namespace miopal
