// The row figures of the panel occurrence sweeps (occurrences_batch.h), in a header of their own that includes nothing
// of HIP: the kernels and the host's chunk plan (occurrence_plan.h, which a plain host compiler builds) share one copy.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define MIOPAL_ROWS_HD __host__ __device__
#else
#define MIOPAL_ROWS_HD
#endif

namespace miopal {

// the pad residue of a chunk's row list: a row behind its query, up to the next multiple of eight
constexpr int kBatchOccurrencePadRow = 255;

// rows a query of Q rows takes in the row list and in LDS
MIOPAL_ROWS_HD constexpr int batchOccurrenceRows(int Q) { return (Q + 7) / 8 * 8; }
// bytes of LDS of `rows` table rows
MIOPAL_ROWS_HD constexpr size_t batchOccurrenceLdsBytes(int64_t rows, int alphabet) {
    return (size_t)rows * (size_t)(alphabet + 1) * sizeof(int);
}

}  // namespace miopal
