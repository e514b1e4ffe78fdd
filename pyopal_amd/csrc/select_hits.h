// Every entry at or above a per-row threshold of rows of int32 scores, compacted on the device (select_hits.hip):
// miopalSearchHits and its PSSM and batch forms run it on the score rows the search kernels leave in HBM.
//
// Order: row by row, index ascending inside a row (database order). Three launches per group of rows - count,
// offsets, write - with the host between the second and the third: it reads rowOffset, sizes the outputs to the
// total and only then enqueues the write.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "select_top.h"

namespace miopal {

struct HitsArgs {
    const int32_t* score;      // [rows][stride], device
    const int32_t* endI;       // end locations beside them (null: scores only)
    const int32_t* endJ;
    int64_t stride;            // entries per row (>= 1)
    int rows;
    int64_t start;             // absolute index of entry 0 of a row
    void* scratch;             // hitsScratchBytes(rows, stride) bytes, device (hitsScratchLayout)
    // outputs of the write, device: `capacity` entries each; entry rowOffset[r] + (rank inside row r)
    int64_t capacity;
    int64_t* target;
    int32_t* outScore;
    int32_t* outEndQ;          // (null without end locations)
    int32_t* outEndT;
};

// The scratch of a selection, all rows of it (a few bytes per block of 4096 scores): what the host uploads
// (minScore, skip) and downloads (rowOffset) sits at fixed places.
struct HitsScratch {
    int64_t* rowOffset;        // [rows + 1]: entries before row r; [rows]: the total
    int32_t* minScore;         // [rows]: row r keeps its entries >= minScore[r]
    int32_t* skip;             // [rows]: non-zero - the row holds nothing and keeps nothing
    int64_t* blockOffset;      // [rows][blocks]: entries before the block, absolute
    int32_t* blockCount;       // [rows][blocks]
};
size_t hitsScratchBytes(int rows, int64_t stride);
HitsScratch hitsScratchLayout(void* base, int rows, int64_t stride);

// count and offsets of every group of kTopRowsPerLaunch rows, enqueued on `stream` (no host synchronisation);
// afterwards rowOffset is complete
hipError_t launchHitsCount(const HitsArgs& a, hipStream_t stream);
// the offsets scan alone, of the group of `rows` rows from r0 whose blockCount is complete (nb: blocksPerRow): for a
// count pass of another file (select_stats.hip)
hipError_t launchHitsOffsets(const HitsScratch& sc, int nb, int r0, int rows, hipStream_t stream);
// the write of every group; never writes at or beyond a.capacity
hipError_t launchHitsWrite(const HitsArgs& a, hipStream_t stream);

}  // namespace miopal
