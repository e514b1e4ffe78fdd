// CPU-only checks of occurrence_plan.h: miopalSelfTest(7) (host.hip) and tools/occurrence_plan_check.cpp (the same under
// the host sanitizers). 0 = fine, else the number of the check that failed. The expectations are literals worked out by
// hand from occurrences_batch.h's rules: a query takes its rows padded to a multiple of eight, a table row takes
// (letters + 1) x 4 bytes, and a group's rows fit a compute unit's 160 KB = 163840 bytes of LDS.
#pragma once
#include "occurrence_plan.h"

namespace miopal {

namespace occurrence_plan_selftest {

constexpr int64_t kLds = 163840, kLaunch = int64_t(1) << 22;   // a compute unit's LDS; targets of one count launch

// a list of queries of the given heights, residue r of query i = (i + r) % 4, cuts 10 + i and windows i
struct Panel {
    std::vector<unsigned char> residues;
    std::vector<int64_t> offsets{0};
    std::vector<int> minScore, window, all;
    explicit Panel(const std::vector<int>& heights) {
        for (size_t i = 0; i < heights.size(); ++i) {
            for (int r = 0; r < heights[i]; ++r) residues.push_back((unsigned char)((i + (size_t)r) % 4));
            offsets.push_back((int64_t)residues.size());
            minScore.push_back(10 + (int)i);
            window.push_back((int)i);
            all.push_back((int)i);
        }
    }
    OccurrenceChunkPlan plan(int A, int64_t wantGroups, bool pssm) const {
        OccurrenceChunkPlan p;
        planOccurrenceChunk(pssm ? nullptr : residues.data(), offsets.data(), minScore.data(), window.data(), all.data(),
                            (int)all.size(), A, wantGroups, kLds, &p);
        return p;
    }
};

inline bool same(const OccurrenceMeta& m, int x, int y, int z, int w) { return m.x == x && m.y == y && m.z == z && m.w == w; }

}  // namespace occurrence_plan_selftest

inline int occurrencePlanSelfTest() {
    using namespace occurrence_plan_selftest;
    // ---- the figures ----
    if (batchOccurrenceRows(1) != 8 || batchOccurrenceRows(8) != 8 || batchOccurrenceRows(9) != 16 || batchOccurrenceRows(64) != 64) return 1;
    // 4 letters: 20 bytes a row, 8192 rows fill the LDS to the byte; 32 letters: 132 bytes, 1240 rows = 163680, 1248 = 164736
    if (batchOccurrenceLdsBytes(8192, 4) != 163840 || batchOccurrenceLdsBytes(1240, 32) != 163680 || batchOccurrenceLdsBytes(1248, 32) != 164736) return 2;
    // ---- the chunks ----
    // 2^25 entries: 16777 queries against 2000 targets; the cap of 32768 against 100; one query when the slice alone has
    // more entries than the bound (the switch at 100 against 1000 targets)
    if (occurrenceChunkQueries(int64_t(1) << 25, 2000) != 16777 || occurrenceChunkQueries(int64_t(1) << 25, 100) != 32768) return 10;
    if (occurrenceChunkQueries(100, 1000) != 1 || occurrenceChunkQueries(int64_t(1) << 25, (int64_t(1) << 25) + 1) != 1) return 11;
    // the chunks of a panel of 4 and of 5 queries, two a chunk: 2 + 2 and 2 + 2 + 1 - an empty trailing chunk is never
    // produced; a panel that fits one chunk, one query a chunk, no panel at all
    if (occurrenceChunkSizes(2, 4) != std::vector<int>{2, 2} || occurrenceChunkSizes(2, 5) != std::vector<int>{2, 2, 1}) return 12;
    if (occurrenceChunkSizes(32768, 3) != std::vector<int>{3} || occurrenceChunkSizes(1, 3) != std::vector<int>{1, 1, 1} ||
        !occurrenceChunkSizes(2, 0).empty()) return 13;
    // ---- the groups the count sweep wants ----
    // 256 compute units x 32 workgroups = 8192; 2000 targets are 8 blocks of 256: 1024 groups; 200 000 are 782: 11 groups;
    // a launch of the count sweep takes 2^22 targets at most (16384 blocks): 1 group; perCu = 0: 1; no compute units known: 1 CU
    if (occurrenceWantGroups(2000, kLaunch, 32, 256) != 1024 || occurrenceWantGroups(200000, kLaunch, 32, 256) != 11) return 20;
    if (occurrenceWantGroups(int64_t(1) << 30, kLaunch, 32, 256) != 1 || occurrenceWantGroups(2000, kLaunch, 0, 256) != 1 || occurrenceWantGroups(256, kLaunch, 32, 0) != 32) return 21;
    // ---- one chunk ----
    {
        // pad rows to a multiple of eight: queries of 6 and 9 rows take table rows 0 .. 7 and 8 .. 23
        const Panel panel({6, 9});
        const OccurrenceChunkPlan p = panel.plan(4, 1, false);
        const std::vector<uint8_t> want = {0, 1, 2, 3, 0, 1, 255, 255, 1, 2, 3, 0, 1, 2, 3, 0, 1, 255, 255, 255, 255, 255, 255, 255};
        if (p.rowResidue != want || !p.rowSource.empty() || p.meta.size() != 3) return 30;
        if (!same(p.meta[0], 0, 6, 10, 0) || !same(p.meta[1], 8, 9, 11, 1) || !same(p.meta[2], 0, 2, 0, 24)) return 31;
        if (p.groups != 1 || p.tallest != 16 || p.widest != 24 || p.mostQueries != 2) return 32;
        // the PSSM form: the same entries; table row r holds row r of the 15 unpadded rows, -1 on the pad rows
        const OccurrenceChunkPlan s = panel.plan(4, 1, true);
        const std::vector<int32_t> source = {0, 1, 2, 3, 4, 5, -1, -1, 6, 7, 8, 9, 10, 11, 12, 13, 14, -1, -1, -1, -1, -1, -1, -1};
        if (s.rowSource != source || !s.rowResidue.empty() || s.meta.size() != 3) return 33;
        if (!same(s.meta[0], 0, 6, 10, 0) || !same(s.meta[1], 8, 9, 11, 1) || !same(s.meta[2], 0, 2, 0, 24)) return 34;
        if (s.groups != 1 || s.tallest != 16 || s.widest != 24) return 35;
    }
    {
        // 4 letters: 128 queries of 64 rows are 8192 rows, one group that fills the LDS exactly ...
        std::vector<int> heights(128, 64);
        const OccurrenceChunkPlan p = Panel(heights).plan(4, 1, false);
        if (p.groups != 1 || p.meta.size() != 129 || !same(p.meta[128], 0, 128, 0, 8192) || p.widest != 8192 || p.tallest != 64) return 40;
        if (batchOccurrenceLdsBytes(p.widest, 4) != (size_t)kLds || !same(p.meta[127], 8128, 64, 137, 127)) return 41;
        // ... and one row more (a query of one row: eight table rows) splits it
        heights.push_back(1);
        const OccurrenceChunkPlan q = Panel(heights).plan(4, 1, true);
        if (q.groups != 2 || q.meta.size() != 131 || !same(q.meta[129], 0, 128, 0, 8192) || !same(q.meta[130], 128, 1, 8192, 8)) return 42;
        if (q.widest != 8192 || q.mostQueries != 128 || q.rowSource.size() != 8200 || q.rowSource[8192] != 8192 || q.rowSource[8193] != -1) return 43;
    }
    {
        // 32 letters: 1240 rows at most - 19 queries of 64 rows and one of 24 ...
        std::vector<int> heights(19, 64);
        heights.push_back(24);
        const OccurrenceChunkPlan p = Panel(heights).plan(32, 1, false);
        if (p.groups != 1 || !same(p.meta[20], 0, 20, 0, 1240) || p.widest != 1240 || p.mostQueries != 20) return 50;
        // ... and with a row more on the last (25 rows: 32 table rows, 1248) it has a group of its own
        heights.back() = 25;
        const OccurrenceChunkPlan q = Panel(heights).plan(32, 1, false);
        if (q.groups != 2 || !same(q.meta[20], 0, 19, 0, 1216) || !same(q.meta[21], 19, 1, 1216, 32) || q.widest != 1216 || q.tallest != 64) return 51;
        if (q.rowResidue.size() != 1248 || q.rowResidue[1216 + 24] != (19 + 24) % 4 || q.rowResidue[1216 + 25] != 255) return 52;
    }
    {
        // more groups wanted than there are queries: one query a group; 2 wanted for 5: three queries a group at most
        const Panel panel({6, 9, 64, 1, 8});
        const OccurrenceChunkPlan p = panel.plan(4, 10, false);
        if (p.groups != 5 || p.meta.size() != 10 || p.mostQueries != 1 || p.widest != 64 || p.tallest != 64) return 60;
        if (!same(p.meta[5], 0, 1, 0, 8) || !same(p.meta[6], 1, 1, 8, 16) || !same(p.meta[7], 2, 1, 24, 64) ||
            !same(p.meta[8], 3, 1, 88, 8) || !same(p.meta[9], 4, 1, 96, 8)) return 61;
        const OccurrenceChunkPlan q = panel.plan(4, 2, false);
        if (q.groups != 2 || !same(q.meta[5], 0, 3, 0, 88) || !same(q.meta[6], 3, 2, 88, 16) || q.widest != 88 || q.mostQueries != 3) return 62;
    }
    {
        // a chunk of panel positions 1 and 3 of a longer list: the entries carry those queries' cuts and windows
        const Panel panel({5, 7, 3, 12});
        const int chunk[2] = {1, 3};
        OccurrenceChunkPlan p;
        planOccurrenceChunk(panel.residues.data(), panel.offsets.data(), panel.minScore.data(), panel.window.data(), chunk, 2, 4, 1, kLds, &p);
        if (!same(p.meta[0], 0, 7, 11, 1) || !same(p.meta[1], 8, 12, 13, 3) || !same(p.meta[2], 0, 2, 0, 24)) return 70;
        if (p.rowResidue[0] != 1 || p.rowResidue[7] != 255 || p.rowResidue[8] != 3 || p.rowResidue[19] != 2 || p.rowResidue[20] != 255) return 71;
        // ... and a plan object that is used again starts over
        planOccurrenceChunk(nullptr, panel.offsets.data(), panel.minScore.data(), panel.window.data(), chunk, 1, 4, 1, kLds, &p);
        if (!p.rowResidue.empty() || p.rowSource.size() != 8 || p.meta.size() != 2 || p.groups != 1 || p.widest != 8 || p.tallest != 8) return 72;
    }
    return 0;
}

}  // namespace miopal
