// Score statistics by target length, gathered on the device from rows of int32 scores (select_stats.hip), and the
// compaction of select_hits.h with one threshold per length bin in the place of one per row: miopalSearchSignificant
// and its PSSM and batch forms run them on the score rows the search kernels leave in HBM (host_stats.inc).
//
// Length bins: quarter octaves, exact in integers (lengthBin). A handle keeps one uint8 bin per target; a row's column
// i has the bin bin[i]. Per (row, bin) the statistics are n, the sum and the sum of squares of the scores, 64-bit
// two's complement (wrapping): integer sums, the same in any order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "select_hits.h"

namespace miopal {

constexpr int kStatBins = 128;   // MIOPAL_STAT_BINS

// The bin of a target of length L: 0 for L = 0; otherwise 1 + 4 e + m with e = floor(log2 L) and m the two bits below
// the leading one (124 for 2^31 - 1; lengths beyond 32 bits end in the last bin)
__host__ __device__ inline int lengthBin(int64_t L) {
    if (L <= 0) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    const int e = 63 - __clzll((long long)L);
#else
    const int e = 63 - __builtin_clzll((unsigned long long)L);
#endif
    const int m = (int)(e >= 2 ? (L >> (e - 2)) & 3 : (L << (2 - e)) & 3);
    const int b = 1 + 4 * e + m;
    return b < kStatBins ? b : kStatBins - 1;
}

struct StatsArgs {
    const int32_t* score;      // [rows][stride], device
    int64_t stride;            // entries per row (>= 1)
    int rows;
    const uint8_t* bin;        // [stride]: the bin of column i
    const int32_t* skip;       // [rows]: non-zero - the row is not read (null: no row is skipped)
    const int32_t* ceiling;    // [rows][kStatBins]: entries with score > ceiling[row][bin] are left out (null: none)
    int64_t* stats;            // [rows][kStatBins][3], zero-filled before the launch: n, sum, sum of squares
};

// bin[i] = lengthBin(offsets[i + 1] - offsets[i]) (offsets given) or lengthBin(length[i]), i < n
hipError_t launchLengthBins(const int64_t* offsets, const int32_t* length, int64_t n, uint8_t* bin, hipStream_t stream);
// out[b][0] += targets of bin b, out[b][1] += their lengths, over targets [0, n) of `offsets` (out zero-filled before)
hipError_t launchLengthSums(const int64_t* offsets, int64_t n, int64_t* out, hipStream_t stream);
// the statistics of every row, in groups of kTopRowsPerLaunch rows (no host synchronisation)
hipError_t launchRowsStats(const StatsArgs& a, hipStream_t stream);

// launchHitsCount / launchHitsWrite (select_hits.h: the same HitsArgs, scratch, order and capacity rule; minScore of
// the scratch is not read) with entry i of row r a hit iff score >= threshold[r][bin[i]]
struct BinnedArgs {
    const uint8_t* bin;          // [stride]
    const int32_t* threshold;    // [rows][kStatBins], device
};
hipError_t launchHitsBinnedCount(const HitsArgs& a, const BinnedArgs& t, hipStream_t stream);
hipError_t launchHitsBinnedWrite(const HitsArgs& a, const BinnedArgs& t, hipStream_t stream);

}  // namespace miopal
