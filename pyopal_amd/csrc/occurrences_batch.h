// Every occurrence of every query of a panel in each target (occurrences_batch.hip; miopalSearchBatchOccurrences,
// host_batch_occurrences.inc): occurrences.h's two sweeps with the host between them, for queries of 1 .. 64 rows
// (one strip), many of them per launch.
//
// A CHUNK is a run of panel queries whose count array [queries of the chunk][n] (n: the targets of the slice) stays
// within kBatchOccurrenceEntries; entry q * n + t is query q of the chunk against target t. occurrences.h's scan runs
// on that array unchanged: its list of the entries with occurrences is query-major, target ascending - the order of
// the answer. A GROUP is a run of the chunk's queries whose rows fit one compute unit's LDS side by side: a workgroup
// of the count sweep builds its group's rows once and every lane walks its target once per query of the group.
//
// The write sweep runs over the scan's list alone: a wavefront takes 64 consecutive listed entries of ONE query, so
// what its lanes look up stays wave-uniform. first[q] = the position in the list of query q's first entry
// (occurrences_batch_bounds_kernel); wavefront w belongs to the query q with the largest base(q) <= w, base(q) =
// first[q] / 64 + q, and takes the entries first[q] + 64 (w - base(q)) ... - base(q + 1) - base(q) is at least the
// wavefronts q needs, so the host sizes the grid as listed / 64 + queries without another look at the device, and
// the wavefronts left over exit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.h"
#include "occurrence_rows.h"
#include "occurrences.h"

namespace miopal {

// entries of a chunk's count array at most (one query when the slice alone has more). What it bounds: the scratch of
// occurrenceScratchBytes (16 bytes an entry: 512 MB at the bound) and the scan's list, whose entries are int32.
// The tuning switch BATCH_OCCURRENCE_ENTRIES sets another bound (tests: chunks on a small panel).
constexpr int64_t kBatchOccurrenceEntries = int64_t(1) << 25;
// Workgroups of the count sweep per compute unit that the host forms the groups for: a group is as many consecutive
// queries as fit the LDS, but where that leaves fewer workgroups than this (targets / 256 x groups), the chunk's queries
// are spread over more, smaller groups. It rests on ONE measurement and no counters (profiles/batch_occurrences_timing.txt:
// 96 queries of 8 .. 24 rows, 200 000 reads - one LDS-filling group, 782 workgroups that each walk the whole panel,
// three to a compute unit by registers: a full round and a round of 14, 23.2 ms; 11 groups: 14.9 ms; 2 000 reads, 48
// groups 0.29 ms, 96 groups 0.19 ms). The tuning switch BATCH_OCCURRENCE_WORKGROUPS_PER_CU sets another value; 0
// keeps every group as large as the LDS allows (tests: several queries a group, groups that fill the LDS).
constexpr int kBatchOccurrenceWorkgroupsPerCu = 32;
struct BatchOccurrenceArgs {
    // count sweep: the chunk of targets, sorted by length (job.out = the target's position in the slice)
    const PairJob* jobs;
    int nJobs;
    const uint8_t* residues;
    // the chunk's queries: rowResidue[r] = the residue of table row r (kBatchOccurrencePadRow: a pad row), every
    // query's rows padded to a multiple of eight; query[q] = {first row, rows of the query, minScore, window};
    // group[g] = {first query, queries, first row, rows} (count sweep: blockIdx.y = g)
    // PSSM form (occurrences_batch_pssm.hip): rowSource[r] = the row of `rows` that table row r holds (-1: a pad row),
    // rows = the chunk's PSSM rows end to end, [rows][alphabet]; query[] and group[] as above
    union {
        const uint8_t* rowResidue;
        const int32_t* rowSource;
    };
    const int4* query;
    const int4* group;
    int nQueries;
    union {
        const int32_t* matrix; // [A][A]
        const int32_t* rows;   // PSSM form
    };
    int alphabet, gapOpen, gapExt;
    int64_t n;                 // targets of the slice: the stride of the count array
    int32_t* count;            // count sweep: [nQueries][n]
    // write sweep: the scan's offsets and list over the count array, first[nQueries + 1], the handle's offsets
    const int64_t* offsets;
    const int32_t* list;
    const int32_t* first;
    const int64_t* dbOffsets;
    int64_t start;             // absolute index of slice position 0
    int64_t* outTarget;
    int32_t *outScore, *outColumn, *outRow;
};

// region: kLastRow (HW) or kAllCells (SW). groups: the grid's y of the count sweep; ldsBytes: the largest group's
// table (count) / the tallest query's (write); listed: the scan's total of entries with occurrences.
hipError_t launchBatchOccurrencesCount(const BatchOccurrenceArgs& a, int region, int groups, size_t ldsBytes, hipStream_t stream);
hipError_t launchBatchOccurrencesWrite(const BatchOccurrenceArgs& a, int region, int64_t listed, size_t ldsBytes, hipStream_t stream);
// the same sweeps with the table filled from PSSM rows (occurrences_batch_pssm.hip)
hipError_t launchBatchOccurrencesCountPssm(const BatchOccurrenceArgs& a, int region, int groups, size_t ldsBytes, hipStream_t stream);
hipError_t launchBatchOccurrencesWritePssm(const BatchOccurrenceArgs& a, int region, int64_t listed, size_t ldsBytes, hipStream_t stream);
// first[q] (q = 0 .. nQueries) and head[q] = offsets[q * n] - the occurrences in front of query q, the chunk's total
// at nQueries - then head[nQueries + 1 ..] = the scan's totals {occurrences, listed entries}: one small download
hipError_t launchBatchOccurrencesBounds(const OccurrenceScratch& sc, int64_t n, int nQueries, int32_t* first, int64_t* head,
                                        hipStream_t stream);

}  // namespace miopal
