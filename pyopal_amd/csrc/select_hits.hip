// Stable stream compaction of score rows (select_hits.h): every entry >= its row's threshold, in (row, index) order.
// Three launches per group of rows, the kernel boundary the only dependency between blocks - no atomics, no waiting:
//   count    every (row, block of 4096 scores): its entries >= minScore[row] -> blockCount (0 for a skipped row)
//   offsets  ONE workgroup: exclusive scan of the group's blockCount in (row, block) order, continued from the
//            group before it -> blockOffset, and rowOffset where a row starts
//   write    every (row, block) that counted anything reads its scores again, ranks its hits in index order and
//            writes index, score and - read at the hit positions only - end locations at blockOffset + rank
// The host reads rowOffset between offsets and write and hands the write the capacity of its outputs.
#include "select_hits.h"
#include "select_rows.h"

namespace miopal {
namespace {

constexpr int kScanThreads = 1024;

// ---- count -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void hits_count_kernel(HitsArgs a, HitsScratch sc, int nb, int r0) {
    const int r = r0 + blockIdx.x / nb, b = blockIdx.x % nb;
    unsigned n = 0;
    if (!sc.skip[r]) {
        const RowSpan rs = rowSpan(a.stride, r);
        const int T = sc.minScore[r];
#pragma unroll
        for (int i = 0; i < kTopVecs; ++i) {
            const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
            if (s < rs.slots) {
                unsigned mask;
                const int4 v = loadSlot(a.score, rs, s, mask);
#pragma unroll
                for (int c = 0; c < 4; ++c) n += (mask >> c & 1) && lane(v, c) >= T;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    __shared__ unsigned waveSum[kTopThreads / 64];
    if (threadIdx.x % 64 == 0) waveSum[threadIdx.x / 64] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int x = 1; x < kTopThreads / 64; ++x) n += waveSum[x];
        sc.blockCount[(size_t)r * nb + b] = (int32_t)n;
    }
}

// ---- offsets (one workgroup per group of rows) ---------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void hits_offsets_kernel(HitsScratch sc, int nb, int r0, int rows) {
    __shared__ unsigned waveTot[kScanThreads / 64];
    const int w = threadIdx.x / 64;
    // (the group before this one has left the entries before row r0 there)
    int64_t base = r0 == 0 ? 0 : sc.rowOffset[r0];
    const size_t f0 = (size_t)r0 * nb;
    const int64_t m = (int64_t)rows * nb;
    for (int64_t t0 = 0; t0 < m; t0 += kScanThreads) {
        const int64_t i = t0 + threadIdx.x;
        // (a tile holds at most 1024 x 4096 entries: 32 bits inside it, 64 across tiles)
        const unsigned c = i < m ? (unsigned)sc.blockCount[f0 + i] : 0u;
        unsigned x = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            x += (int)(threadIdx.x % 64) >= d ? y : 0u;
        }
        if (threadIdx.x % 64 == 63) waveTot[w] = x;
        __syncthreads();
        unsigned before = 0, tile = 0;
        for (int k = 0; k < kScanThreads / 64; ++k) {
            before += k < w ? waveTot[k] : 0u;
            tile += waveTot[k];
        }
        const int64_t excl = base + before + (x - c);
        if (i < m) {
            sc.blockOffset[f0 + i] = excl;
            if (i % nb == 0 && (i > 0 || r0 == 0)) sc.rowOffset[r0 + i / nb] = excl;
        }
        base += tile;
        __syncthreads();
    }
    if (threadIdx.x == 0) sc.rowOffset[r0 + rows] = base;
}

// ---- write -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void hits_write_kernel(HitsArgs a, HitsScratch sc, int nb, int r0) {
    __shared__ unsigned waveTot[kTopVecs][kTopThreads / 64];
    const int r = r0 + blockIdx.x / nb, b = blockIdx.x % nb;
    const size_t at = (size_t)r * nb + b;
    if (sc.blockCount[at] == 0) return;   // (skipped rows among them: nothing is read again)
    const RowSpan rs = rowSpan(a.stride, r);
    const int T = sc.minScore[r];
    const int w = threadIdx.x / 64;
    int4 v[kTopVecs];
    unsigned hit[kTopVecs], pre[kTopVecs];
    // one round per slot column: the threads' slots of a round are consecutive, so (round, wavefront, lane, entry)
    // is index order
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
        unsigned mask = 0;
        v[i] = make_int4(0, 0, 0, 0);
        if (s < rs.slots) v[i] = loadSlot(a.score, rs, s, mask);
        hit[i] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) hit[i] |= ((mask >> c & 1) && lane(v[i], c) >= T) ? 1u << c : 0u;
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
        // entry 0 of the slot: its index inside the row (below 0 in a first slot shared with the row before)
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

size_t hitsScratchBytes(int rows, int64_t stride) {
    const size_t cells = (size_t)rows * blocksPerRow(stride);
    return align256(sizeof(int64_t) * ((size_t)rows + 1)) + 2 * align256(sizeof(int32_t) * (size_t)rows) +
           align256(sizeof(int64_t) * cells) + align256(sizeof(int32_t) * cells);
}

HitsScratch hitsScratchLayout(void* base, int rows, int64_t stride) {
    const size_t cells = (size_t)rows * blocksPerRow(stride);
    char* p = (char*)base;
    HitsScratch s;
    s.rowOffset = (int64_t*)p;
    p += align256(sizeof(int64_t) * ((size_t)rows + 1));
    s.minScore = (int32_t*)p;
    p += align256(sizeof(int32_t) * (size_t)rows);
    s.skip = (int32_t*)p;
    p += align256(sizeof(int32_t) * (size_t)rows);
    s.blockOffset = (int64_t*)p;
    p += align256(sizeof(int64_t) * cells);
    s.blockCount = (int32_t*)p;
    return s;
}

hipError_t launchHitsCount(const HitsArgs& a, hipStream_t stream) {
    if (a.rows <= 0 || a.stride <= 0) return hipErrorInvalidValue;
    const int nb = blocksPerRow(a.stride);
    const HitsScratch sc = hitsScratchLayout(a.scratch, a.rows, a.stride);
    for (int r0 = 0; r0 < a.rows; r0 += kTopRowsPerLaunch) {
        const int rows = a.rows - r0 < kTopRowsPerLaunch ? a.rows - r0 : kTopRowsPerLaunch;
        hits_count_kernel<<<(unsigned)rows * (unsigned)nb, kTopThreads, 0, stream>>>(a, sc, nb, r0);
        hits_offsets_kernel<<<1, kScanThreads, 0, stream>>>(sc, nb, r0, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launchHitsOffsets(const HitsScratch& sc, int nb, int r0, int rows, hipStream_t stream) {
    hits_offsets_kernel<<<1, kScanThreads, 0, stream>>>(sc, nb, r0, rows);
    return hipGetLastError();
}

hipError_t launchHitsWrite(const HitsArgs& a, hipStream_t stream) {
    if (a.rows <= 0 || a.stride <= 0 || a.capacity < 0) return hipErrorInvalidValue;
    const int nb = blocksPerRow(a.stride);
    const HitsScratch sc = hitsScratchLayout(a.scratch, a.rows, a.stride);
    for (int r0 = 0; r0 < a.rows; r0 += kTopRowsPerLaunch) {
        const int rows = a.rows - r0 < kTopRowsPerLaunch ? a.rows - r0 : kTopRowsPerLaunch;
        hits_write_kernel<<<(unsigned)rows * (unsigned)nb, kTopThreads, 0, stream>>>(a, sc, nb, r0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace miopal
