// How the passes over rows of int32 scores read them (select_top.hip, select_hits.hip): a row of a [rows][stride]
// buffer in 16-byte slots, a block of kTopBlockSlots slots per workgroup, and the wavefront scan that ranks a
// block's chosen entries.
#pragma once
#include "select_top.h"

namespace miopal {

__host__ __device__ inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
__host__ __device__ inline int blocksPerRow(int64_t stride) {
    const int64_t slots = (stride + 3) / 4 + 1;   // (a row that starts mid-slot touches one slot more)
    return (int)((slots + kTopBlockSlots - 1) / kTopBlockSlots);
}

// The 16-byte slots of a row: slot s holds buffer entries [a0 + 4 s, a0 + 4 s + 4); entries outside
// [first, last) belong to other rows (or lie past the buffer) and are neither read nor counted.
struct RowSpan {
    int64_t first, last, a0, slots;
};
__device__ inline RowSpan rowSpan(int64_t stride, int r) {
    RowSpan rs;
    rs.first = (int64_t)r * stride;
    rs.last = rs.first + stride;
    rs.a0 = rs.first & ~(int64_t)3;
    rs.slots = (rs.last - rs.a0 + 3) >> 2;
    return rs;
}
// slot s of the row (s < rs.slots); `mask` bit c: entry c belongs to the row
__device__ inline int4 loadSlot(const int32_t* buf, const RowSpan& rs, int64_t s, unsigned& mask) {
    const int64_t e = rs.a0 + 4 * s;
    if (e >= rs.first && e + 4 <= rs.last) {
        mask = 0xF;
        return *(const int4*)(buf + e);
    }
    int v[4];
    mask = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool in = e + c >= rs.first && e + c < rs.last;
        v[c] = in ? buf[e + c] : 0;
        mask |= in ? 1u << c : 0u;
    }
    return make_int4(v[0], v[1], v[2], v[3]);
}
__device__ inline int lane(const int4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// exclusive prefix and total over the wavefront of per-lane counts (two 16-bit halves at once)
__device__ inline void wavePrefix(unsigned c, unsigned& prefix, unsigned& total) {
    const int lane = threadIdx.x % 64;
    unsigned x = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d);
        x += lane >= d ? y : 0u;
    }
    prefix = x - c;
    total = __shfl(x, 63);
}

}  // namespace miopal
