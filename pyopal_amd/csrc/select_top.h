// The k best entries of rows of int32 scores, chosen on the device (select_top.hip): miopalSearchTop and
// miopalSearchBatchTop run it on the score rows the search kernels leave in HBM.
//
// Order: score descending, then index ascending. Entries below minScore do not count. Row r's answer is its
// first min(k, hits) entries in that order; slots past the count hold -1 in every output.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace miopal {

constexpr int kTopBins = 4096;                                   // histogram bins of a round (16 KB of LDS)
constexpr int kTopThreads = 256;                                 // threads of a block of the passes over the scores
constexpr int kTopVecs = 4;                                      // 16-byte loads per thread and block
constexpr int kTopBlockSlots = kTopThreads * kTopVecs;           // 16-byte slots per block (4096 scores)
constexpr int kTopRounds = 3;                                    // 12 + 12 + 8 bits: any int32 range
constexpr int kTopMaxK = 4096;                                   // MIOPAL_MAX_TOP
constexpr int kTopRowsPerLaunch = 1024;                          // rows per sequence of launches (bounds the scratch)

struct TopArgs {
    const int32_t* score;   // [rows][stride], device
    const int32_t* endI;    // end locations beside them (null: scores only)
    const int32_t* endJ;
    int64_t stride;         // entries per row (>= 1)
    int rows;
    int k;                  // 1 .. kTopMaxK
    int minScore;
    int64_t start;          // absolute index of entry 0 of a row
    void* scratch;          // topScratchBytes(rows, stride, k) bytes, device
    // outputs, device: count [rows]; [rows][k] row-major
    int32_t* count;
    int64_t* target;
    int32_t* outScore;
    int32_t* outEndQ;       // (null without end locations)
    int32_t* outEndT;
    int* error;             // incremented by a block that gave up waiting for the blocks before it (never seen)
};

size_t topScratchBytes(int rows, int64_t stride, int k);
// enqueues the whole selection on `stream` (no host synchronisation); rows in groups of kTopRowsPerLaunch
hipError_t launchSelectTop(const TopArgs& a, hipStream_t stream);

}  // namespace miopal
