// The plan of the passes behind the score / end pass of a `full` search (host_full.inc) and of a pair list
// (host_pairs.inc): the bits of the routing word, the lane-against-wavefront cost model, the geometry of a pair's
// slots, and the traceback batch plan. One copy of every formula. Host only, pure functions: no HIP runtime call, no
// workspace, no tuned() - switches come in as flags, what a .hip file decides (packedTraceFits) as a bool.
// full_plan_selftest.h checks it on the CPU (miopalSelfTest(5), tools/full_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace miopal {

// ---- miopalLastFullRouting (include/miopal.h) ---------------------------------------------------------------------
enum FullRoute : int {
    kRouteScanLane = 1,        // start cells: one lane per pair
    kRouteScanProfile = 2,     // ... in the query-profile form
    kRouteTraceLane = 4,       // directions: one lane per pair
    kRouteTraceProfile = 8,    // ... in the query-profile form
    kRouteOverlapOps = 16,     // operations copied to the host batch by batch beside the next batch
    kRouteScanRefill = 32,     // start cells by persistent wavefronts whose lanes take the next pair (one strip)
    kRouteTracePacked = 64,    // directions: two pairs per lane on 16-bit halves
    kRouteScanPacked = 128,    // start cells: two pairs per lane on 16-bit halves
    kRouteOneLaunch = 256,     // the packed direction pass of a group of batches in one launch
};

constexpr int kPlanLanes = 64;                       // (common.h's kLanes: host.hip asserts that they agree)
constexpr int64_t kDirBudget = 2ll << 30;            // direction workspace: 2 x this per device-resident traceback batch, 1 x per host-built batch
constexpr int64_t kDirBudgetOneLaunch = 8ll << 30;   // directions of a group of batches of a `full` search at once

// ---- the cost model: rough time of a pass, in ms, on one lane per pair or one wavefront per pair -------------------
// One lane per pair: ~14 instructions per cell of the scan (21 of the direction pass), but a wavefront lasts as long as
// its longest lane. One wavefront per pair spends 64 lanes on a 64-row column step: ~225 instructions per step when the
// chip is full, 250 along one pair's chain of steps.
constexpr int kScanLaneInstr = 14, kTraceLaneInstr = 21;
constexpr double kWaveStepInstr = 225.0, kWaveChainInstr = 250.0;
constexpr double kCyclesPerInstr = 4.5;
constexpr double kCyclesPerMs = 2.4e6;
constexpr int kScanWaveSlots = 1024;        // wavefronts the chip runs side by side in the estimates of the scan ...
constexpr double kTraceWaveSlots = 2048.0;  // ... and of the lane-per-pair direction pass (two of 64 pairs per SIMD)

// The scan. `cols`: 64-row column steps of all pairs (strips x columns, summed); `chain`: those of the longest pair.
// (the one-query search passes n x strips x the mean length and strips x the longest target - the wavefront's columns
// with 63 steps of skew each; a pair list passes its sums and its longest chains)
inline double scanLaneMs(double cols, double chain) {
    return std::max(cols * (kScanLaneInstr * kCyclesPerInstr) / (kScanWaveSlots * kCyclesPerMs),
                    chain * (kPlanLanes * kScanLaneInstr * kCyclesPerInstr) / kCyclesPerMs);
}
inline double scanWaveMs(double cols, double chain) {
    return std::max(cols * kWaveStepInstr / (kScanWaveSlots * kCyclesPerMs), chain * kWaveChainInstr / kCyclesPerMs);
}
// The direction pass. `cells`: column steps of one slot, strips x (longest window + 63); `pairs`: of one batch;
// `batches`: how many such batches follow each other (a pair list's chunk: 1).
inline double traceLaneMs(double batches, double pairs, double cells) {
    return batches * std::ceil(pairs / kPlanLanes / kTraceWaveSlots) * cells * (kPlanLanes * kTraceLaneInstr * kCyclesPerInstr) /
           kCyclesPerMs;
}
inline double traceWaveMs(double batches, double pairs, double cells) {
    return batches * std::max(pairs * cells * kWaveStepInstr / (kScanWaveSlots * kCyclesPerMs), cells * kWaveChainInstr / kCyclesPerMs);
}
inline double traceCells(int64_t windowStrips, int64_t maxWindow) {
    return (double)windowStrips * (double)(maxWindow + kPlanLanes - 1);
}

// ---- slot geometry: what one pair takes in the traceback's workspaces -------------------------------------------------
inline int64_t round4(int64_t columns) { return (columns + 3) & ~(int64_t)3; }
inline int64_t roundLanes(int64_t pairs) { return (pairs + kPlanLanes - 1) / kPlanLanes * kPlanLanes; }
// direction bytes of one pair (either 32-bit layout: anti-diagonals of 64 lanes per strip, or 64 rows per column)
inline int64_t slotDir(int64_t windowStrips, int64_t maxWindow) { return windowStrips * (maxWindow + kPlanLanes - 1) * kPlanLanes; }
// operations of one pair (they leave 16 bytes at a time). `rows`: the query's length in a search, the tallest window
// of a pair list's chunk
inline int64_t slotOps(int64_t rows, int64_t maxWindow) { return (rows + maxWindow + 15) & ~(int64_t)15; }
inline int64_t slotOpsMost(int64_t rows, int64_t columns) { return rows + columns + 16; }   // (above slotOps, whatever the windows)
// bytes of direction bits per pair as the pass writes them: the lane-per-pair layouts pack two rows per byte (half of
// slotDir); the packed kernel's lines need the window's columns rounded up to four, not the 63 columns of slack of the
// anti-diagonal layout
enum DirLayout { kDirWave, kDirLane, kDirPacked };
inline int64_t slotDirUsed(DirLayout layout, int64_t windowStrips, int64_t maxWindow) {
    return layout == kDirPacked ? windowStrips * round4(maxWindow) * (kPlanLanes / 2)
           : layout == kDirLane ? slotDir(windowStrips, maxWindow) / 2
                                : slotDir(windowStrips, maxWindow);
}
// columns reserved per strip in the lane layouts (the bit planes come in blocks of four columns: a multiple of 4, within
// the slot's maxWindow + 63)
inline int64_t dirStripColumns(bool planes, int64_t maxWindow) { return planes ? round4(maxWindow) : maxWindow + kPlanLanes - 1; }
// strip boundaries of a group of lane-per-pair jobs: 8 bytes (an int2) per column and pair, whole wavefronts
inline size_t boundaryBytes(int64_t pairs, int64_t columns) { return (size_t)roundLanes(pairs) * columns * 8; }

// ---- the traceback batch plan --------------------------------------------------------------------------------------
struct PlanSwitches {
    bool forceLanePerPair = false;   // FORCE_LANE_PER_PAIR
    bool noHybridTrace = false;      // NO_HYBRID_TRACE
    bool noOneLaunch = false;        // NO_ONE_LAUNCH
    bool groupSet = false;           // ONE_LAUNCH_GROUP is set, to ...
    int group = 0;                   // ... this many batches per direction launch
};

struct TracePlan {
    int64_t slotDir, slotOps, slotDirUsed;
    bool fits;                 // n x slotOps within 16 GB (else: host-built batches)
    int64_t opsCap;            // n x slotOps
    int64_t dirBudget, chipRound, batchLane, batchWave;
    bool traceLanePerPair, packedTrace, overlapOps;
    int64_t batch;             // pairs per batch (before the allocation of the directions had its say)
    int64_t maxHead;           // wavefronts of outliers a wavefront-per-pair pass may take per batch, at most (0: no hybrid)
    int64_t nBatchesPlanned, allSlots, dirGroup, groupSlots;
    bool oneLaunch;            // ... if its directions are granted
    int routing;               // bits 4, 8, 16, 64 of the routing word
};

// Traceback in batches of whole direction slots and whole wavefronts of 64 pairs.
// `packedOk`: two pairs per lane on 16-bit halves would do for the scoring scheme and the windows (packedTraceFits).
inline TracePlan planTrace(int64_t n, int64_t queryLength, int64_t windowStrips, int64_t maxWindow, int computeUnits,
                           bool lanePerPair, bool profiled, bool packedOk, const PlanSwitches& sw) {
    TracePlan p{};
    p.slotDir = slotDir(windowStrips, maxWindow);
    p.slotOps = slotOps(queryLength, maxWindow);
    p.opsCap = n * p.slotOps;
    p.fits = p.opsCap <= (16ll << 30);
    // (a round of the chip is twice the pairs with two in a lane, and the budget follows: Q = 300 on 1M x 300
    // asks for 58 KB of directions per pair - 15 GB per round)
    // OPEN (ADVICE.md's second finding): budget and round follow packedOk, not packedTrace - the wavefront route's
    // batches are sized against 16 GB when the packed kernel WOULD fit. Changing it changes batch sizes: to be measured.
    p.dirBudget = packedOk ? kDirBudget * 8 : kDirBudget * 2;
    auto batchFor = [&](int64_t slotBytes) {
        return std::max<int64_t>(kPlanLanes, std::min<int64_t>(n + kPlanLanes - 1, p.dirBudget / slotBytes) / kPlanLanes * kPlanLanes);
    };
    // lane per pair: whole rounds of the chip (two wavefronts of 64 pairs per SIMD; a batch of 1.1 rounds lasts as
    // long as one of two). The slots are budgeted at a quarter of slotDir and written at half of it (packed: less):
    // within 2 x dirBudget of directions, 8 GB unpacked and 32 GB packed. Q = 300 on 1M x 300 took 14 batches of 1117
    // wavefronts, 5.2 ms each, where 8 of 2048 take 5.2 ms as well
    p.chipRound = (int64_t)computeUnits * 4 * 2 * kPlanLanes * (packedOk ? 2 : 1);
    p.batchLane = batchFor(std::max<int64_t>(p.slotDir / 4, 1));
    if (p.batchLane >= p.chipRound) p.batchLane = p.batchLane / p.chipRound * p.chipRound;
    else if (p.batchLane >= p.chipRound / 2 && n > p.batchLane) p.batchLane = p.chipRound / 2;
    p.batchWave = batchFor(p.slotDir);
    // (the pinned staging buffer holds the worst case, n x slotOps: Q = 300 on 1M x 300 asks for 664 MB)
    // (within it the operations leave batch by batch, two bits each; a larger result is downloaded whole, in bytes,
    // after the last batch)
    p.overlapOps = p.opsCap <= (1024ll << 20);
    // Direction pass: one lane per pair needs ~64 x fewer instructions per cell but a lane walks its whole window
    // alone (strips x columns x 64 rows, ~0.4 us per strip column); with few pairs per batch or huge windows (global
    // alignments of long targets) a wavefront per pair is done sooner.
    p.traceLanePerPair = lanePerPair;
    if (lanePerPair) {
        const double cells = traceCells(windowStrips, maxWindow);
        const double pairsL = (double)std::min<int64_t>(p.batchLane, n), pairsW = (double)std::min<int64_t>(p.batchWave, n);
        const double perLane = traceLaneMs(std::ceil((double)n / (double)p.batchLane), pairsL, cells);
        const double perWave = traceWaveMs(std::ceil((double)n / (double)p.batchWave), pairsW, cells);
        p.traceLanePerPair = perLane <= perWave || sw.forceLanePerPair;
    }
    p.packedTrace = p.traceLanePerPair && packedOk;
    if (p.traceLanePerPair) p.routing |= kRouteTraceLane | (profiled ? kRouteTraceProfile : 0) | (p.packedTrace ? kRouteTracePacked : 0);
    if (p.overlapOps) p.routing |= kRouteOverlapOps;
    p.batch = p.traceLanePerPair ? p.batchLane : p.batchWave;
    if (p.overlapOps && n >= 4 * 65536) {
        // (four batches, the last one half a batch: its operations are what the host unpacks with the device idle)
        int64_t target = std::max<int64_t>(65536, roundLanes(n * 2 / 7));
        // (a batch a little above a round of the chip lasts two: rather one round)
        // (not when the direction pass runs over groups of batches anyway: oneLaunch)
        const bool grouped = p.packedTrace && !sw.noOneLaunch &&
                             std::min<int64_t>(n + kPlanLanes, 2 * target) * slotDirUsed(kDirPacked, windowStrips, maxWindow) <= kDirBudgetOneLaunch;
        if (p.traceLanePerPair && !grouped && target > p.chipRound && target < p.chipRound * 3 / 2) target = p.chipRound;
        p.batch = std::min(p.batch, target);
    }
    // hybrid: up to 1 GB of direction bytes for the outliers a wavefront-per-pair pass takes
    if (p.traceLanePerPair && !sw.noHybridTrace)
        p.maxHead = std::min<int64_t>((1ll << 30) / p.slotDir / kPlanLanes, (p.batch + kPlanLanes - 1) / kPlanLanes);
    p.nBatchesPlanned = (n + p.batch - 1) / p.batch;
    p.allSlots = roundLanes(n);
    // (batches per direction launch: the walks - whose operations the host unpacks - must not all come at the end; two
    // launches of two batches leave the host the second launch's time for the first's shares. The direction bits of
    // ONE group stay in HBM at a time)
    p.dirGroup = p.nBatchesPlanned >= 4 ? (p.nBatchesPlanned + 1) / 2 : p.nBatchesPlanned;
    if (sw.groupSet) p.dirGroup = std::max(1, sw.group);
    p.slotDirUsed = slotDirUsed(p.packedTrace ? kDirPacked : p.traceLanePerPair ? kDirLane : kDirWave, windowStrips, maxWindow);
    p.groupSlots = std::min(p.allSlots, p.dirGroup * p.batch);
    p.oneLaunch = p.packedTrace && p.nBatchesPlanned > 1 && !sw.noOneLaunch && p.groupSlots * p.slotDirUsed <= kDirBudgetOneLaunch;
    return p;
}

// The pinned staging a search with overlapped copies reserves in one go (a later drain would reset the buffer): the
// running totals in front, the operations at two bits each, and room for the small per-target arrays that follow
// (with the scores and end locations when they are still to be sent).
struct StagingPlan {
    size_t head, stagedOps, reserve;
};
inline StagingPlan planStaging(int64_t n, int64_t opsCap, int64_t nBatches, bool resultsPending) {
    StagingPlan s{};
    s.head = 256 + (((size_t)nBatches * 8 + 255) & ~(size_t)255);
    s.stagedOps = ((size_t)opsCap + 63) / 64 * 16;
    s.reserve = s.head + s.stagedOps + 256 + (size_t)n * (resultsPending ? 36 : 20) + 8192 + (size_t)nBatches * 1024;
    return s;
}

}  // namespace miopal
