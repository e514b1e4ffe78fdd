// CPU-only checks of full_plan.h: miopalSelfTest(5) (host.hip) and tools/full_plan_check.cpp (the same under the host
// sanitizers). 0 = fine, else the number of the check that failed. The expectations are literals worked out from the
// expressions as host_full.inc and host_pairs.inc wrote them out before they had one home.
#pragma once
#include "full_plan.h"

namespace miopal {

inline int fullPlanSelfTest() {
    const PlanSwitches none;
    // ---- the routing word: include/miopal.h ----
    if (kRouteScanLane != 1 || kRouteScanProfile != 2 || kRouteTraceLane != 4 || kRouteTraceProfile != 8 || kRouteOverlapOps != 16 ||
        kRouteScanRefill != 32 || kRouteTracePacked != 64 || kRouteScanPacked != 128 || kRouteOneLaunch != 256)
        return 1;
    // ---- slot geometry ----
    // one strip, windows of 61 columns: (61 + 63) x 64 = 7936 direction bytes, half of it on lanes, 64 x 32 packed;
    // operations (53 + 61 + 15) & ~15 = 128
    if (slotDir(1, 61) != 7936 || slotDirUsed(kDirWave, 1, 61) != 7936 || slotDirUsed(kDirLane, 1, 61) != 3968 || slotDirUsed(kDirPacked, 1, 61) != 2048) return 10;
    if (slotOps(53, 61) != 128 || slotOps(300, 300) != 608 || slotOps(1, 1) != 16 || slotOps(2000, 35000) != 37008) return 11;
    // five strips of 300 columns: 5 x 363 x 64 = 116160; packed 5 x 300 x 32 = 48000; two strips of 120: 2 x 183 x 64
    if (slotDir(5, 300) != 116160 || slotDirUsed(kDirLane, 5, 300) != 58080 || slotDirUsed(kDirPacked, 5, 300) != 48000) return 12;
    if (slotDir(2, 120) != 23424 || slotDirUsed(kDirPacked, 2, 120) != 7680) return 13;
    if (dirStripColumns(true, 61) != 64 || dirStripColumns(false, 61) != 124 || dirStripColumns(true, 300) != 300 || dirStripColumns(true, 1) != 4) return 14;
    // boundaries: whole wavefronts x columns x 8 bytes
    if (boundaryBytes(1, 300) != 64u * 300 * 8 || boundaryBytes(64, 300) != 64u * 300 * 8 || boundaryBytes(65, 300) != 128u * 300 * 8) return 15;
    if (slotOpsMost(53, 61) != 130 || slotOpsMost(53, 61) <= slotOps(53, 61)) return 16;
    // ---- the cost model ----
    // Q = 300 on 1M x 300, five strips: lanes 1.5e9 steps x 63 / (1024 x 2.4e6) = 38.45 ms (the chain: 1500 x 4032 / 2.4e6
    // = 2.52); wavefronts 1.815e9 x 225 / (1024 x 2.4e6) = 166.17 ms
    if (scanLaneMs(1e6 * 5 * 300.0, 5 * 300.0) != 38.4521484375 || scanWaveMs(1e6 * 5 * 363.0, 5 * 363.0) != 166.168212890625) return 20;
    // 1000 global alignments of 2000 residues against targets of 3000, one of 35 000: the lane's chain of 32 x 35 000
    // steps decides (1881.6 ms against 116.9): the wavefront route
    if (!(scanLaneMs(1000 * 32 * 3000.0, 32 * 35000.0) > 1881.59 && scanLaneMs(1000 * 32 * 3000.0, 32 * 35000.0) < 1881.61)) return 21;
    if (!(scanWaveMs(1000 * 32 * 3063.0, 32 * 35063.0) > 116.87 && scanWaveMs(1000 * 32 * 3063.0, 32 * 35063.0) < 116.88)) return 22;
    // the direction pass of a 64-pair chunk of one-strip windows: a lane 124 x 6048 / 2.4e6 = 0.31248 ms, a wavefront
    // per pair 124 x 250 / 2.4e6 = 0.0129 ms
    if (!(traceLaneMs(1, 64, traceCells(1, 61)) > 0.31247 && traceLaneMs(1, 64, traceCells(1, 61)) < 0.31249)) return 23;
    if (!(traceWaveMs(1, 64, traceCells(1, 61)) > 0.012916 && traceWaveMs(1, 64, traceCells(1, 61)) < 0.012917)) return 24;
    // ---- the batch plan ----
    {
        // cfg3: 53 residues against 1M x 300, windows of 61 columns, 256 CUs, everything packed. Budget 16 GB: the
        // lane batch is the whole list, cut to 3 rounds of 262144; four batches of roundLanes(2/7 n) = 285760 (grouped:
        // no snap to the chip's round); two launches of two batches (571520 slots x 2048 B within 8 GB)
        const TracePlan p = planTrace(1000000, 53, 1, 61, 256, true, true, true, none);
        if (p.slotDir != 7936 || p.slotOps != 128 || p.slotDirUsed != 2048 || !p.fits || p.opsCap != 128000000) return 30;
        if (p.dirBudget != (16ll << 30) || p.chipRound != 262144 || p.batchLane != 786432 || p.batchWave != 1000000) return 31;
        if (!p.traceLanePerPair || !p.packedTrace || !p.overlapOps || p.batch != 285760 || p.maxHead != 2114) return 32;
        if (p.nBatchesPlanned != 4 || p.allSlots != 1000000 || p.dirGroup != 2 || p.groupSlots != 571520 || !p.oneLaunch) return 33;
        if (p.routing != (kRouteTraceLane | kRouteTraceProfile | kRouteOverlapOps | kRouteTracePacked)) return 34;
        // the switches: no hybrid head, no group launch (then the target snaps: 285760 is within 1.5 rounds of 262144),
        // a group of every batch
        PlanSwitches sw;
        sw.noHybridTrace = true;
        if (planTrace(1000000, 53, 1, 61, 256, true, true, true, sw).maxHead != 0) return 35;
        sw = PlanSwitches{};
        sw.noOneLaunch = true;
        const TracePlan q = planTrace(1000000, 53, 1, 61, 256, true, true, true, sw);
        if (q.oneLaunch || q.batch != 262144 || q.nBatchesPlanned != 4) return 36;
        sw = PlanSwitches{};
        sw.groupSet = true;
        sw.group = 4;
        const TracePlan g = planTrace(1000000, 53, 1, 61, 256, true, true, true, sw);
        if (g.dirGroup != 4 || g.groupSlots != 1000000 || !g.oneLaunch) return 37;
        sw.group = 0;
        if (planTrace(1000000, 53, 1, 61, 256, true, true, true, sw).dirGroup != 1) return 38;
        // 240 CUs: a round of 245760
        if (planTrace(1000000, 53, 1, 61, 240, true, true, true, none).chipRound != 245760) return 39;
    }
    {
        // Q = 300 on 1M x 300, five strips of 300 columns. Packed: 16 GB / 29040 = 591593 -> 2 rounds = 524288; the
        // target 285760 is not grouped (571520 x 48000 B is beyond 8 GB) and snaps to one round, 262144; a group of two
        // batches is 25 GB: a launch per batch
        const TracePlan p = planTrace(1000000, 300, 5, 300, 256, true, true, true, none);
        if (p.slotDir != 116160 || p.slotOps != 608 || p.slotDirUsed != 48000 || p.opsCap != 608000000 || !p.overlapOps) return 40;
        if (p.batchLane != 524288 || p.batchWave != 147840 || p.batch != 262144 || p.maxHead != 144) return 41;
        if (p.nBatchesPlanned != 4 || p.dirGroup != 2 || p.groupSlots != 524288 || p.oneLaunch || p.routing != 92) return 42;
        // the scheme does not fit the halves: 4 GB, rounds of 131072, eight batches
        const TracePlan u = planTrace(1000000, 300, 5, 300, 256, true, true, false, none);
        if (u.dirBudget != (4ll << 30) || u.chipRound != 131072 || u.batchLane != 131072 || u.batchWave != 36928) return 43;
        if (u.packedTrace || u.slotDirUsed != 58080 || u.batch != 131072 || u.nBatchesPlanned != 8 || u.dirGroup != 4 || u.oneLaunch || u.routing != 28) return 44;
    }
    {
        // two strips: 270 000 pairs, windows of 100 rows x 120 columns
        const TracePlan p = planTrace(270000, 100, 2, 120, 256, true, true, true, none);
        if (p.slotDir != 23424 || p.slotOps != 224 || p.slotDirUsed != 7680 || p.batchLane != 262144 || p.batchWave != 270016) return 50;
        if (p.batch != 77184 || p.maxHead != 716 || p.nBatchesPlanned != 4 || p.allSlots != 270016 || p.groupSlots != 154368 || !p.oneLaunch) return 51;
    }
    {
        // n = 1, 64, 65: one batch of whole wavefronts; so few pairs are done sooner by a wavefront each (0.0129 ms
        // against a lane's 0.3125) unless lanes are forced
        const TracePlan a = planTrace(1, 53, 1, 61, 256, true, true, true, none);
        const TracePlan b = planTrace(64, 53, 1, 61, 256, true, true, true, none);
        const TracePlan c = planTrace(65, 53, 1, 61, 256, true, true, true, none);
        if (a.batch != 64 || b.batch != 64 || c.batch != 128 || a.allSlots != 64 || b.allSlots != 64 || c.allSlots != 128) return 60;
        if (a.traceLanePerPair || b.traceLanePerPair || c.traceLanePerPair || a.routing != 16 || c.slotDirUsed != 7936 || c.maxHead != 0) return 61;
        if (a.nBatchesPlanned != 1 || c.nBatchesPlanned != 1 || c.dirGroup != 1 || c.oneLaunch || a.opsCap != 128 || c.opsCap != 8320) return 62;
        PlanSwitches sw;
        sw.forceLanePerPair = true;
        const TracePlan f = planTrace(65, 53, 1, 61, 256, true, true, true, sw);
        if (!f.traceLanePerPair || !f.packedTrace || f.routing != 92 || f.slotDirUsed != 2048 || f.maxHead != 2 || f.oneLaunch) return 63;
        // n = 270 000 (the tests' four batches): 2/7 n in whole wavefronts = 77184, two launches of two batches
        const TracePlan d = planTrace(270000, 53, 1, 61, 256, true, true, true, none);
        if (d.batchLane != 262144 || d.batchWave != 270016 || d.batch != 77184 || d.maxHead != 1206 || d.nBatchesPlanned != 4) return 64;
        if (d.dirGroup != 2 || d.groupSlots != 154368 || !d.oneLaunch || d.routing != 92) return 65;
    }
    {
        // global alignments, windows of 32 strips x 35 000 columns: 71.8 MB of directions per pair; sixteen batches of one
        // wavefront, and the wavefront route wins (1870 ms against 16965) whether or not lanes were possible
        const TracePlan p = planTrace(1000, 2000, 32, 35000, 256, true, false, false, none);
        if (p.slotDir != 71809024 || p.slotOps != 37008 || p.batchLane != 192 || p.batchWave != 64) return 70;
        if (p.traceLanePerPair || p.batch != 64 || p.nBatchesPlanned != 16 || p.dirGroup != 8 || p.groupSlots != 512 || p.routing != 16) return 71;
        if (p.slotDirUsed != 71809024 || p.maxHead != 0 || p.oneLaunch || p.allSlots != 1024) return 72;
        const TracePlan w = planTrace(1000, 2000, 32, 35000, 256, false, false, false, none);
        if (w.traceLanePerPair || w.batch != 64 || w.routing != 16) return 73;
        // operations beyond 1 GB stay on the device until the end; beyond 16 GB the batches are built on the host
        if (planTrace(4000000, 300, 5, 300, 256, true, true, true, none).overlapOps) return 74;
        if (planTrace(4000000, 4097, 65, 35000, 256, false, false, false, none).fits) return 75;
    }
    {
        // staging: 256 + the totals in whole 256 bytes, the operations at 16 bytes per 64, 20 or 36 bytes per target
        const StagingPlan s = planStaging(1000000, 128000000, 4, true);
        if (s.head != 512 || s.stagedOps != 32000000 || s.reserve != 512 + 32000000 + 256 + 36000000 + 8192 + 4096) return 80;
        if (planStaging(1, 128, 1, false).reserve != 512 + 32 + 256 + 20 + 8192 + 1024) return 81;
    }
    return 0;
}

}  // namespace miopal
