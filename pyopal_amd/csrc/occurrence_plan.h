// The plan of a panel occurrence search's chunks (host_batch_occurrences.inc): how many of the panel's queries a chunk
// takes and, for one chunk, the row list (plain) or the row-source map (PSSM), the entries of its queries, the groups of
// the count sweep, the tallest query and the widest group - what decides the grid and the LDS size of every launch, by
// occurrences_batch.h's rules. Host only, pure integer arithmetic: no HIP, no workspace, no tuned() - a switch comes in
// as a number. occurrence_plan_selftest.h checks it on the CPU (miopalSelfTest(7), tools/occurrence_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "occurrence_rows.h"

namespace miopal {

// queries of a chunk at most (every group holds at least one: the count sweep's grid has one row of workgroups per group)
constexpr int64_t kBatchOccurrenceChunkQueries = 32768;

struct OccurrenceMeta {   // an entry of the chunk's meta array as the kernels read it (an int4: asserted where it is uploaded)
    int x, y, z, w;
};

// queries a chunk takes: its count array [queries][n] stays within `entries`, one query when the slice alone has more
inline int64_t occurrenceChunkQueries(int64_t entries, int64_t n) {
    return std::max<int64_t>(1, std::min<int64_t>(kBatchOccurrenceChunkQueries, entries / n));
}
// ... and the chunks of a panel of `panelSize` queries, in order: the queries of each (none is empty)
inline std::vector<int> occurrenceChunkSizes(int64_t perChunk, size_t panelSize) {
    std::vector<int> sizes;
    for (size_t p0 = 0; p0 < panelSize; p0 += (size_t)sizes.back())
        sizes.push_back((int)std::min<int64_t>(perChunk, (int64_t)(panelSize - p0)));
    return sizes;
}

// Groups a chunk is spread over at least. A group is as many consecutive queries as fit the LDS - unless that leaves
// the count sweep fewer than `perCu` workgroups per compute unit: then the queries are spread over more, smaller groups,
// down to one query a group (occurrences_batch.h). Few targets: the panel fills the GPU side by side. Many: the launch ends evenly.
// (launchTargets: targets of one launch of the count sweep at most)
inline int64_t occurrenceWantGroups(int64_t n, int64_t launchTargets, int64_t perCu, int computeUnits) {
    const int64_t targetBlocks = (std::min<int64_t>(n, launchTargets) + 255) / 256;
    return std::max<int64_t>(1, (perCu * (int64_t)std::max(computeUnits, 1) + targetBlocks - 1) / targetBlocks);
}

struct OccurrenceChunkPlan {
    std::vector<uint8_t> rowResidue;    // plain: the residue of every table row, kBatchOccurrencePadRow behind each query
    std::vector<int32_t> rowSource;     // PSSM: the row of the chunk's rows (end to end, unpadded) each table row holds, -1: a pad row
    std::vector<OccurrenceMeta> meta;   // [cq] queries {first row, rows, cut, window}, then the groups {first query, queries, first row, rows}
    int groups = 0;
    int tallest = 0;          // padded rows of the tallest query: the write sweep's LDS table
    int64_t widest = 0;       // rows of the widest group: the count sweep's
    int64_t mostQueries = 0;  // queries of the largest group
};

// The chunk of the panel queries panel[0 .. cq) of the call's list (`offsets` delimits its queries, 1 .. 64 rows each;
// `residues`: the plain form's queries, null for a PSSM panel; ldsBytes: the LDS a group's rows may fill).
inline void planOccurrenceChunk(const unsigned char* residues, const int64_t* offsets, const int* minScore, const int* window,
                                const int* panel, int cq, int A, int64_t wantGroups, int64_t ldsBytes, OccurrenceChunkPlan* p) {
    p->rowResidue.clear();
    p->rowSource.clear();
    p->meta.clear();
    p->groups = p->tallest = 0;
    p->widest = p->mostQueries = 0;
    int32_t origin = 0;   // (PSSM: the query's first row among the chunk's unpadded rows)
    size_t tableRows = 0;
    for (int q = 0; q < cq; ++q) {
        const int i = panel[q];
        const int Q = (int)(offsets[i + 1] - offsets[i]);
        const size_t padded = (size_t)batchOccurrenceRows(Q);
        p->meta.push_back(OccurrenceMeta{(int)tableRows, Q, minScore[i], window[i]});
        if (residues) {
            p->rowResidue.insert(p->rowResidue.end(), residues + offsets[i], residues + offsets[i + 1]);
            p->rowResidue.resize(tableRows + padded, (uint8_t)kBatchOccurrencePadRow);
        } else {
            for (int r = 0; r < Q; ++r) p->rowSource.push_back(origin + r);
            p->rowSource.resize(tableRows + padded, -1);
            origin += Q;
        }
        tableRows += padded;
        p->tallest = std::max(p->tallest, (int)padded);
    }
    const int64_t perGroup = std::max<int64_t>(1, (cq + wantGroups - 1) / wantGroups);
    for (int q = 0; q < cq;) {
        int e = q;
        int64_t rows = 0;
        while (e < cq && e - q < perGroup &&
               (int64_t)batchOccurrenceLdsBytes(rows + batchOccurrenceRows(p->meta[(size_t)e].y), A) <= ldsBytes) {
            rows += batchOccurrenceRows(p->meta[(size_t)e].y);
            ++e;
        }
        p->meta.push_back(OccurrenceMeta{q, e - q, p->meta[(size_t)q].x, (int)rows});
        p->mostQueries = std::max<int64_t>(p->mostQueries, e - q);
        p->widest = std::max(p->widest, rows);
        ++p->groups;
        q = e;
    }
}

}  // namespace miopal
