// The m best rows of every column of rows of int32 scores, folded on the device piece by piece (select_columns.hip):
// miopalSearchBatchTargetTop runs it on the [queries][targets] rows the batch leaves in HBM - the best queries of
// every target - where select_top.hip selects along the rows.
//
// Order: score descending, then row (query index) ascending - a total order, so the state after any number of
// folds is the m best of the rows folded so far, in whatever order the pieces came. The state is device memory of
// the caller: M = columnsSlots(m) entries per column, zero-initialised ("empty"); one fold per piece, every fold
// complete before the next starts; one finish turns it into count[n] and [n][m] arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace miopal {

constexpr int kColumnsMaxM = 8;   // (MIOPAL_MAX_TARGET_TOP)

// slots per column of the state: m rounded up to 1, 2, 4 or 8 (the kernels keep them in registers)
inline int columnsSlots(int m) { return m <= 1 ? 1 : m <= 2 ? 2 : m <= 4 ? 4 : 8; }

// The running state of n columns: slot j of column t at [j * n + t]. key = (score ^ 0x80000000) << 32 |
// (0x7fffffff - row): "better" is one unsigned compare; 0 = empty (row <= INT32_MAX - 1 keeps the low word >= 1, so
// a score of INT_MIN is still an entry).
struct ColumnsState {
    uint64_t* key;    // [M][n]
    int32_t* endI;    // [M][n] each (null: scores only)
    int32_t* endJ;
};
size_t columnsStateBytes(int64_t n, int m, bool ends);
ColumnsState columnsStateLayout(void* base, int64_t n, int m, bool ends);

struct ColumnsPiece {
    const int32_t* score;   // [rows][n], device: row r of the piece starts at r * n
    const int32_t* endI;    // end locations beside them (null: scores only)
    const int32_t* endJ;
    int rows;
    int32_t firstRow;       // row r of the piece is row (query) firstRow + r of the answer
    const int32_t* skip;    // [rows], device (null: no row is skipped): non-zero - the row holds nothing, never read
};

// the piece folded into the state: entries >= minScore that beat a column's worst kept entry are inserted
hipError_t launchColumnsFold(const ColumnsState& st, const ColumnsPiece& p, int64_t n, int m, int minScore,
                             hipStream_t stream);

// the answer, device: count[n]; the others [n][m], best first, -1 in slots count .. m - 1
struct ColumnsOut {
    int32_t* count;
    int32_t* row;
    int32_t* score;
    int32_t* endI;    // (null without end locations)
    int32_t* endJ;
};
size_t columnsOutBytes(int64_t n, int m, bool ends);
ColumnsOut columnsOutLayout(void* base, int64_t n, int m, bool ends);
hipError_t launchColumnsFinish(const ColumnsState& st, const ColumnsOut& out, int64_t n, int m, hipStream_t stream);

}  // namespace miopal
