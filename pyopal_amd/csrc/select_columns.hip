// The m best rows of every column, folded piece by piece (select_columns.h). Two kernels, one thread per column:
//   fold    loads the column's M state entries into registers, walks the piece's rows - consecutive threads read
//           consecutive dwords of a row, kColUnroll rows in flight - inserts what beats the worst kept entry (its end
//           locations are read then, at the inserted cell only) and writes the state back if it changed
//   finish  state -> count[n] and the [n][m] arrays, -1 past the count
// No block talks to another: the only ordering is that of the launches (one fold complete before the next starts).
#include "select_columns.h"
#include "select_rows.h"

namespace miopal {
namespace {

constexpr int kColThreads = 64;   // (one wavefront: few columns still spread over the compute units)
constexpr int kColUnroll = 8;     // rows of a column loaded before the first is looked at

__device__ inline uint64_t columnKey(int score, int32_t row) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint32_t)(0x7fffffff - row);
}

template <int M, bool ENDS>
__global__ __launch_bounds__(kColThreads) void columns_fold_kernel(ColumnsState st, ColumnsPiece p, int64_t n, int minScore) {
    const int64_t t = (int64_t)blockIdx.x * kColThreads + threadIdx.x;
    if (t >= n) return;
    uint64_t key[M];
    int ei[M], ej[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        key[j] = st.key[(int64_t)j * n + t];
        ei[j] = ENDS ? st.endI[(int64_t)j * n + t] : 0;
        ej[j] = ENDS ? st.endJ[(int64_t)j * n + t] : 0;
    }
    bool changed = false;
    for (int r0 = 0; r0 < p.rows; r0 += kColUnroll) {
        int s[kColUnroll];
        bool ok[kColUnroll];
#pragma unroll
        for (int u = 0; u < kColUnroll; ++u) {
            const int r = r0 + u;
            ok[u] = r < p.rows && !(p.skip && p.skip[r]);   // (the same in every lane)
            s[u] = ok[u] ? p.score[(int64_t)r * n + t] : 0;
        }
#pragma unroll
        for (int u = 0; u < kColUnroll; ++u) {
            if (!ok[u] || s[u] < minScore) continue;
            const uint64_t k = columnKey(s[u], p.firstRow + r0 + u);
            if (k <= key[M - 1]) continue;
            const int64_t cell = (int64_t)(r0 + u) * n + t;
            key[M - 1] = k;
            if (ENDS) {
                ei[M - 1] = p.endI[cell];
                ej[M - 1] = p.endJ[cell];
            }
            changed = true;
            // (the new entry sinks to its place: the slots stay sorted, best first)
#pragma unroll
            for (int j = M - 1; j > 0; --j) {
                const bool up = key[j] > key[j - 1];
                const uint64_t a = key[j], b = key[j - 1];
                key[j - 1] = up ? a : b;
                key[j] = up ? b : a;
                if (ENDS) {
                    const int ia = ei[j], ib = ei[j - 1], ja = ej[j], jb = ej[j - 1];
                    ei[j - 1] = up ? ia : ib;
                    ei[j] = up ? ib : ia;
                    ej[j - 1] = up ? ja : jb;
                    ej[j] = up ? jb : ja;
                }
            }
        }
    }
    if (!changed) return;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        st.key[(int64_t)j * n + t] = key[j];
        if (ENDS) {
            st.endI[(int64_t)j * n + t] = ei[j];
            st.endJ[(int64_t)j * n + t] = ej[j];
        }
    }
}

template <int M, bool ENDS>
__global__ __launch_bounds__(kColThreads) void columns_finish_kernel(ColumnsState st, ColumnsOut out, int64_t n, int m) {
    const int64_t t = (int64_t)blockIdx.x * kColThreads + threadIdx.x;
    if (t >= n) return;
    int count = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        if (j >= m) break;
        const uint64_t k = st.key[(int64_t)j * n + t];
        const bool has = k != 0;
        count += has;
        const int64_t at = t * m + j;
        out.row[at] = has ? (int32_t)(0x7fffffffu - (uint32_t)k) : -1;
        out.score[at] = has ? (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u) : -1;
        if (ENDS) {
            out.endI[at] = has ? st.endI[(int64_t)j * n + t] : -1;
            out.endJ[at] = has ? st.endJ[(int64_t)j * n + t] : -1;
        }
    }
    out.count[t] = count;
}

template <int M>
hipError_t foldWith(const ColumnsState& st, const ColumnsPiece& p, int64_t n, int minScore, hipStream_t stream) {
    const unsigned blocks = (unsigned)((n + kColThreads - 1) / kColThreads);
    if (p.endI) columns_fold_kernel<M, true><<<blocks, kColThreads, 0, stream>>>(st, p, n, minScore);
    else columns_fold_kernel<M, false><<<blocks, kColThreads, 0, stream>>>(st, p, n, minScore);
    return hipGetLastError();
}

template <int M>
hipError_t finishWith(const ColumnsState& st, const ColumnsOut& out, int64_t n, int m, hipStream_t stream) {
    const unsigned blocks = (unsigned)((n + kColThreads - 1) / kColThreads);
    if (out.endI) columns_finish_kernel<M, true><<<blocks, kColThreads, 0, stream>>>(st, out, n, m);
    else columns_finish_kernel<M, false><<<blocks, kColThreads, 0, stream>>>(st, out, n, m);
    return hipGetLastError();
}

bool columnsShapeOk(int64_t n, int m) { return n >= 1 && n <= INT32_MAX && m >= 1 && m <= kColumnsMaxM; }

}  // namespace

size_t columnsStateBytes(int64_t n, int m, bool ends) {
    const size_t cells = (size_t)columnsSlots(m) * (size_t)n;
    return align256(sizeof(uint64_t) * cells) + (ends ? 2 * align256(sizeof(int32_t) * cells) : 0);
}

ColumnsState columnsStateLayout(void* base, int64_t n, int m, bool ends) {
    const size_t cells = (size_t)columnsSlots(m) * (size_t)n;
    char* p = (char*)base;
    ColumnsState s{};
    s.key = (uint64_t*)p;
    p += align256(sizeof(uint64_t) * cells);
    if (ends) {
        s.endI = (int32_t*)p;
        p += align256(sizeof(int32_t) * cells);
        s.endJ = (int32_t*)p;
    }
    return s;
}

size_t columnsOutBytes(int64_t n, int m, bool ends) {
    const size_t cells = (size_t)m * (size_t)n;
    return align256(sizeof(int32_t) * (size_t)n) + (ends ? 4 : 2) * align256(sizeof(int32_t) * cells);
}

ColumnsOut columnsOutLayout(void* base, int64_t n, int m, bool ends) {
    const size_t cells = (size_t)m * (size_t)n;
    char* p = (char*)base;
    ColumnsOut o{};
    o.count = (int32_t*)p;
    p += align256(sizeof(int32_t) * (size_t)n);
    o.row = (int32_t*)p;
    p += align256(sizeof(int32_t) * cells);
    o.score = (int32_t*)p;
    p += align256(sizeof(int32_t) * cells);
    if (ends) {
        o.endI = (int32_t*)p;
        p += align256(sizeof(int32_t) * cells);
        o.endJ = (int32_t*)p;
    }
    return o;
}

hipError_t launchColumnsFold(const ColumnsState& st, const ColumnsPiece& p, int64_t n, int m, int minScore,
                             hipStream_t stream) {
    if (!columnsShapeOk(n, m) || p.rows < 1 || p.firstRow < 0 || p.firstRow > INT32_MAX - p.rows) return hipErrorInvalidValue;
    if ((p.endI != nullptr) != (st.endI != nullptr) || (p.endI == nullptr) != (p.endJ == nullptr)) return hipErrorInvalidValue;
    switch (columnsSlots(m)) {
        case 1: return foldWith<1>(st, p, n, minScore, stream);
        case 2: return foldWith<2>(st, p, n, minScore, stream);
        case 4: return foldWith<4>(st, p, n, minScore, stream);
        default: return foldWith<8>(st, p, n, minScore, stream);
    }
}

hipError_t launchColumnsFinish(const ColumnsState& st, const ColumnsOut& out, int64_t n, int m, hipStream_t stream) {
    if (!columnsShapeOk(n, m) || (out.endI != nullptr) != (st.endI != nullptr)) return hipErrorInvalidValue;
    switch (columnsSlots(m)) {
        case 1: return finishWith<1>(st, out, n, m, stream);
        case 2: return finishWith<2>(st, out, n, m, stream);
        case 4: return finishWith<4>(st, out, n, m, stream);
        default: return finishWith<8>(st, out, n, m, stream);
    }
}

}  // namespace miopal
