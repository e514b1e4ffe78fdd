// Score statistics by length bin and the compaction with a threshold per bin (select_stats.h).
//   length_bins    offsets (or lengths) -> one uint8 bin per target
//   length_sums    per bin: targets and the sum of their lengths, of a slice of the offsets
//   rows_stats     every (row, block of 4096 scores): n, sum and sum of squares per bin of its entries at or below
//                  the row's ceilings; reduced in the thread, the wavefront and the block, then one 64-bit integer
//                  atomicAdd per non-empty (block, bin) and figure - integer adds: the same sums in any order
//   hits_binned_count / hits_binned_write
//                  select_hits.hip's count and write with score >= threshold[row][bin of the column], the row's
//                  512-byte table staged in LDS; the offsets scan between them is select_hits.hip's own
#include "select_stats.h"
#include "select_rows.h"

namespace miopal {
namespace {

typedef unsigned long long u64;

// ---- the reduction of (bin, n, sum, sum of squares) ----------------------------------------------------------------
// A thread keeps the two bins it saw last as runs in registers - a database of one length, or of two lengths
// alternating, never touches LDS entry by entry; a third bin sends the older run to the block's LDS table.
struct Runs {
    int b0 = -1, b1 = -1;
    u64 n0 = 0, n1 = 0, s0 = 0, s1 = 0, q0 = 0, q1 = 0;
};
__device__ inline void addTo(u64* acc, int b, u64 n, u64 s, u64 q) {
    atomicAdd(&acc[b * 3 + 0], n);
    atomicAdd(&acc[b * 3 + 1], s);
    atomicAdd(&acc[b * 3 + 2], q);
}
__device__ inline void take(Runs& r, u64* acc, int b, u64 s, u64 q) {
    if (b == r.b1) {
        ++r.n1;
        r.s1 += s;
        r.q1 += q;
    } else if (b == r.b0) {
        ++r.n0;
        r.s0 += s;
        r.q0 += q;
    } else {
        if (r.n0) addTo(acc, r.b0, r.n0, r.s0, r.q0);
        r.b0 = r.b1;
        r.n0 = r.n1;
        r.s0 = r.s1;
        r.q0 = r.q1;
        r.b1 = b;
        r.n1 = 1;
        r.s1 = s;
        r.q1 = q;
    }
}
// One run of every lane into the LDS table; every lane of the wavefront calls it. The lanes that hold anything hold
// the same bin (the whole wavefront inside one bin): shuffles, and one lane adds. Otherwise every lane adds its own.
__device__ inline void flushWave(u64* acc, int b, u64 n, u64 s, u64 q) {
    const bool has = n != 0;
    const u64 holders = __ballot(has);
    if (holders == 0) return;
    const int b0 = __shfl(b, __ffsll((long long)holders) - 1);
    if (__all(!has || b == b0)) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            n += __shfl_xor(n, d);
            s += __shfl_xor(s, d);
            q += __shfl_xor(q, d);
        }
        if (threadIdx.x % 64 == 0) addTo(acc, b0, n, s, q);
    } else if (has) {
        addTo(acc, b, n, s, q);
    }
}
__device__ inline void flushRuns(const Runs& r, u64* acc) {
    flushWave(acc, r.b0, r.n0, r.s0, r.q0);
    flushWave(acc, r.b1, r.n1, r.s1, r.q1);
}

// ---- bins and per-bin lengths ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void length_bins_kernel(const int64_t* offsets, const int32_t* length, int64_t n,
                                                                  uint8_t* bin) {
    for (int64_t i = (int64_t)blockIdx.x * kTopThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTopThreads) {
        const int64_t L = offsets ? offsets[i + 1] - offsets[i] : (int64_t)length[i];
        bin[i] = (uint8_t)lengthBin(L);
    }
}

constexpr int kSumsPerThread = 16;
__global__ __launch_bounds__(kTopThreads) void length_sums_kernel(const int64_t* offsets, int64_t n, int64_t* out) {
    __shared__ u64 acc[kStatBins * 3];
    for (int i = threadIdx.x; i < kStatBins * 3; i += kTopThreads) acc[i] = 0;
    __syncthreads();
    Runs runs;
#pragma unroll 4
    for (int k = 0; k < kSumsPerThread; ++k) {
        const int64_t i = ((int64_t)blockIdx.x * kSumsPerThread + k) * kTopThreads + threadIdx.x;
        if (i < n) {
            const int64_t L = offsets[i + 1] - offsets[i];
            take(runs, acc, lengthBin(L), (u64)L, 0);
        }
    }
    flushRuns(runs, acc);
    __syncthreads();
    if (threadIdx.x < kStatBins && acc[threadIdx.x * 3] != 0) {
        atomicAdd((u64*)&out[threadIdx.x * 2 + 0], acc[threadIdx.x * 3 + 0]);
        atomicAdd((u64*)&out[threadIdx.x * 2 + 1], acc[threadIdx.x * 3 + 1]);
    }
}

// ---- statistics of the rows ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void rows_stats_kernel(StatsArgs a, int nb, int r0) {
    __shared__ u64 acc[kStatBins * 3];
    __shared__ int32_t ceiling[kStatBins];
    const int r = r0 + blockIdx.x / nb, b = blockIdx.x % nb;
    if (a.skip && a.skip[r]) return;   // (the whole block: nothing of the row is read)
    for (int i = threadIdx.x; i < kStatBins * 3; i += kTopThreads) acc[i] = 0;
    if (threadIdx.x < kStatBins)
        ceiling[threadIdx.x] = a.ceiling ? a.ceiling[(size_t)r * kStatBins + threadIdx.x] : INT32_MAX;
    __syncthreads();
    const RowSpan rs = rowSpan(a.stride, r);
    Runs runs;
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
        if (s < rs.slots) {
            unsigned mask;
            const int4 v = loadSlot(a.score, rs, s, mask);
            // entry 0 of the slot: its column (below 0 in a first slot shared with the row before - masked out)
            const int64_t e = rs.a0 + 4 * s - rs.first;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!(mask >> c & 1)) continue;
                const int bin = a.bin[e + c];
                const int x = lane(v, c);
                if (x > ceiling[bin]) continue;
                const u64 sx = (u64)(int64_t)x;
                take(runs, acc, bin, sx, sx * sx);
            }
        }
    }
    flushRuns(runs, acc);
    __syncthreads();
    if (threadIdx.x < kStatBins && acc[threadIdx.x * 3] != 0) {
        u64* out = (u64*)a.stats + ((size_t)r * kStatBins + threadIdx.x) * 3;
        atomicAdd(out + 0, acc[threadIdx.x * 3 + 0]);
        atomicAdd(out + 1, acc[threadIdx.x * 3 + 1]);
        atomicAdd(out + 2, acc[threadIdx.x * 3 + 2]);
    }
}

// ---- compaction with a threshold per bin -------------------------------------------------------------------------
// the hits of a slot as a bit per entry
__device__ inline unsigned binnedHits(const int4& v, unsigned mask, const uint8_t* bin, int64_t e, const int32_t* thr) {
    unsigned hit = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (mask >> c & 1) hit |= lane(v, c) >= thr[bin[e + c]] ? 1u << c : 0u;
    return hit;
}

__global__ __launch_bounds__(kTopThreads) void hits_binned_count_kernel(HitsArgs a, HitsScratch sc, BinnedArgs t, int nb,
                                                                        int r0) {
    __shared__ int32_t thr[kStatBins];
    __shared__ unsigned waveSum[kTopThreads / 64];
    const int r = r0 + blockIdx.x / nb, b = blockIdx.x % nb;
    unsigned n = 0;
    if (!sc.skip[r]) {   // (the whole block)
        if (threadIdx.x < kStatBins) thr[threadIdx.x] = t.threshold[(size_t)r * kStatBins + threadIdx.x];
        __syncthreads();
        const RowSpan rs = rowSpan(a.stride, r);
#pragma unroll
        for (int i = 0; i < kTopVecs; ++i) {
            const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
            if (s < rs.slots) {
                unsigned mask;
                const int4 v = loadSlot(a.score, rs, s, mask);
                n += __popc(binnedHits(v, mask, t.bin, rs.a0 + 4 * s - rs.first, thr));
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    if (threadIdx.x % 64 == 0) waveSum[threadIdx.x / 64] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int x = 1; x < kTopThreads / 64; ++x) n += waveSum[x];
        sc.blockCount[(size_t)r * nb + b] = (int32_t)n;
    }
}

__global__ __launch_bounds__(kTopThreads) void hits_binned_write_kernel(HitsArgs a, HitsScratch sc, BinnedArgs t, int nb,
                                                                        int r0) {
    __shared__ int32_t thr[kStatBins];
    __shared__ unsigned waveTot[kTopVecs][kTopThreads / 64];
    const int r = r0 + blockIdx.x / nb, b = blockIdx.x % nb;
    const size_t at = (size_t)r * nb + b;
    if (sc.blockCount[at] == 0) return;   // (the whole block; skipped rows among them: nothing is read again)
    if (threadIdx.x < kStatBins) thr[threadIdx.x] = t.threshold[(size_t)r * kStatBins + threadIdx.x];
    __syncthreads();
    const RowSpan rs = rowSpan(a.stride, r);
    const int w = threadIdx.x / 64;
    int4 v[kTopVecs];
    unsigned hit[kTopVecs], pre[kTopVecs];
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
        unsigned mask = 0;
        v[i] = make_int4(0, 0, 0, 0);
        hit[i] = 0;
        if (s < rs.slots) {
            v[i] = loadSlot(a.score, rs, s, mask);
            hit[i] = binnedHits(v[i], mask, t.bin, rs.a0 + 4 * s - rs.first, thr);
        }
        unsigned tot;
        wavePrefix((unsigned)__popc(hit[i]), pre[i], tot);
        if (threadIdx.x % 64 == 0) waveTot[i][w] = tot;
    }
    __syncthreads();
    unsigned running = 0, base[kTopVecs];
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        for (int x = 0; x < kTopThreads / 64; ++x) {
            if (x == w) base[i] = running;
            running += waveTot[i][x];
        }
    }
    const int64_t off = sc.blockOffset[at];
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t e = rs.a0 + 4 * ((int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x) - rs.first;
        int64_t p = off + base[i] + pre[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!(hit[i] >> c & 1)) continue;
            if (p < a.capacity) {
                a.target[p] = a.start + e + c;
                a.outScore[p] = lane(v[i], c);
                if (a.outEndQ) {
                    a.outEndQ[p] = a.endI[rs.first + e + c];
                    a.outEndT[p] = a.endJ[rs.first + e + c];
                }
            }
            ++p;
        }
    }
}

}  // namespace

hipError_t launchLengthBins(const int64_t* offsets, const int32_t* length, int64_t n, uint8_t* bin, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if ((offsets == nullptr) == (length == nullptr) || !bin) return hipErrorInvalidValue;
    const int64_t blocks = (n + kTopThreads - 1) / kTopThreads;
    length_bins_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), kTopThreads, 0, stream>>>(offsets, length, n, bin);
    return hipGetLastError();
}

hipError_t launchLengthSums(const int64_t* offsets, int64_t n, int64_t* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!offsets || !out) return hipErrorInvalidValue;
    const int64_t per = (int64_t)kSumsPerThread * kTopThreads;
    length_sums_kernel<<<(unsigned)((n + per - 1) / per), kTopThreads, 0, stream>>>(offsets, n, out);
    return hipGetLastError();
}

hipError_t launchRowsStats(const StatsArgs& a, hipStream_t stream) {
    if (a.rows <= 0 || a.stride <= 0 || !a.score || !a.bin || !a.stats) return hipErrorInvalidValue;
    const int nb = blocksPerRow(a.stride);
    for (int r0 = 0; r0 < a.rows; r0 += kTopRowsPerLaunch) {
        const int rows = a.rows - r0 < kTopRowsPerLaunch ? a.rows - r0 : kTopRowsPerLaunch;
        rows_stats_kernel<<<(unsigned)rows * (unsigned)nb, kTopThreads, 0, stream>>>(a, nb, r0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launchHitsBinnedCount(const HitsArgs& a, const BinnedArgs& t, hipStream_t stream) {
    if (a.rows <= 0 || a.stride <= 0 || !t.bin || !t.threshold) return hipErrorInvalidValue;
    const int nb = blocksPerRow(a.stride);
    const HitsScratch sc = hitsScratchLayout(a.scratch, a.rows, a.stride);
    for (int r0 = 0; r0 < a.rows; r0 += kTopRowsPerLaunch) {
        const int rows = a.rows - r0 < kTopRowsPerLaunch ? a.rows - r0 : kTopRowsPerLaunch;
        hits_binned_count_kernel<<<(unsigned)rows * (unsigned)nb, kTopThreads, 0, stream>>>(a, sc, t, nb, r0);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = launchHitsOffsets(sc, nb, r0, rows, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launchHitsBinnedWrite(const HitsArgs& a, const BinnedArgs& t, hipStream_t stream) {
    if (a.rows <= 0 || a.stride <= 0 || a.capacity < 0 || !t.bin || !t.threshold) return hipErrorInvalidValue;
    const int nb = blocksPerRow(a.stride);
    const HitsScratch sc = hitsScratchLayout(a.scratch, a.rows, a.stride);
    for (int r0 = 0; r0 < a.rows; r0 += kTopRowsPerLaunch) {
        const int rows = a.rows - r0 < kTopRowsPerLaunch ? a.rows - r0 : kTopRowsPerLaunch;
        hits_binned_write_kernel<<<(unsigned)rows * (unsigned)nb, kTopThreads, 0, stream>>>(a, sc, t, nb, r0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace miopal
