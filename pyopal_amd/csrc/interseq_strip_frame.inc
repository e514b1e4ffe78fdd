// The unit frame of the two multi-strip pair-table kernels (interseq_pair_strips_kernel,
// interseq_pair_global_strips_kernel), included as text in four parts; each kernel keeps its own sweep (cell, borders,
// answers) and its own answer fold between them. (Text, not functions: as structs or functions every form of the
// frame changed the kernels' code objects, profiles/pair_table_parts_device_code.txt.)
//   #define MIOPAL_STRIP_FRAME_PART 1   once, in front of the unit loop `for (;;) {`: the frame's state
//   #define MIOPAL_STRIP_FRAME_PART 2   at the top of the loop's body: takes a unit (breaks out of the loop when none
//                                       is left), rebuilds the table when the strip changes, picks the wavefront's
//                                       group (continues when the batch has none for it) and sets up the feed from
//                                       the strip above: s, g, gIdx, pack, nChunks, longGroup, fromAbove, toBelow,
//                                       rowsIn, rowsOut, progOut, lastCol, kLag, dead, waitFor(need)
//   #define MIOPAL_STRIP_FRAME_PART 3   behind the kernel's `sweep` lambda: runs sweep(from above, to below) for the
//                                       kind of strip
//   #define MIOPAL_STRIP_FRAME_PART 4   behind part 3, with `base` (the group's first result) declared: ends a dead
//                                       unit (continue)
// The including kernel sets, for all parts,
//   MIOPAL_STRIP_FRAME_ABORTS 1 / 0     the launch also watches a.stripAbort (Smith-Waterman: lanes that left the range)
//   MIOPAL_PAIR_ENTRY(v)                its table's entry transform (interseq_pair_table_build.inc)
//   MIOPAL_STRIP_FRAME_STATE            declarations of its own among the frame's state, or nothing (they stand where
//                                       they stood before the frame was shared: their place is part of the code object)
// and provides pairs, a, lane, nSym, R, SLOTS.
//
// A pair table holds one strip of the query and fills the CU's LDS, so all twelve wavefronts of a workgroup work on
// the same strip: a workgroup takes units (batch of up to 12 groups, strip) from a counter, rebuilds the table when the
// strip changes (150 KB of LDS writes, a few microseconds) and each wavefront sweeps its group through that strip.
#if MIOPAL_STRIP_FRAME_PART == 1
    const int nStrips = a.nStrips;
    const int perBatch = a.batchGroups;   // 12, or fewer when the groups are few (more CUs, faster wavefronts)
    const int nBatches = (a.nGroups + perBatch - 1) / perBatch;
    int* ctl = reinterpret_cast<int*>(pairs + nSym * nSym * SLOTS);   // 16 bytes behind the table
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int tableStrip = -1;
    const int spinCap = a.stripSpinCap > 0 ? a.stripSpinCap : kStripSpinCap;
    MIOPAL_STRIP_FRAME_STATE
    SimdPace pace;
    pace.init(ctl + 4, lane);
    StripTimer timer;
#elif MIOPAL_STRIP_FRAME_PART == 2
        timer.start(0);
        if (threadIdx.x == 0) {
            int next = atomicAdd(a.unitCounter, 1);
#if MIOPAL_STRIP_FRAME_ABORTS
            // Too many lanes have left the exact range: the host will redo the whole view on the next
            // rung whatever this launch still computes (end locations of long queries against long
            // targets under cheap gaps: scores in the thousands, a range of 384) - stop here.
            if (a.stripAbort && __hip_atomic_load(a.stripAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.stripAbortAt) {
                if (next < nBatches * nStrips) atomicAdd(a.stripGaveUp, a.stripAbortAt);
                next = INT32_MAX;
            }
#endif
            ctl[0] = next;
        }
        __syncthreads();   // (and: every wavefront has left the table of the unit before)
        const int u = __builtin_amdgcn_readfirstlane(ctl[0]);
        if (u >= nBatches * nStrips) {
            timer.stop(0);
            break;
        }
        // strip-major: strip s of every batch before strip s + 1 of any. The wavefront above is then
        // (number of batches) units ahead - usually finished, never just started: with batch-major
        // order every unit began by waiting for the unit taken a moment before it to get two chunks
        // ahead, and a chain of 20 strips idled a fifth of the time - and a workgroup keeps its table
        // until the strip changes.
        const int s = u / nBatches, b = u - s * nBatches;
        if (s != tableStrip) {
            const int16_t* gp = a.profile + s * R;
            constexpr int kBuildThreads = kPairWavesPerGroup * kLanes;
#include "interseq_pair_table_build.inc"
            tableStrip = s;
        }
        __syncthreads();   // table ready; ctl[0] read by everybody
        timer.stop(0);
        const int gIdx = b * perBatch + wave;
        if (wave >= perBatch || gIdx >= a.nGroups) continue;
        const int g = gIdx + a.groupBase;
        const uint2* pack = a.pack + a.groupOff[g];
        // (a leading group whose longest targets were handed to the int32 kernel stops at the longest that stays)
        const int nChunks = gIdx < a.capGroups ? min(a.groupChunks[g], a.capChunks) : a.groupChunks[g];
        // (a long group is the launch's critical path: it wins the SIMD's issue arbitration)
        const bool longGroup = groupPriority(nChunks, a.priorityChunks);
        const bool fromAbove = s > 0, toBelow = s + 1 < nStrips;
        // The last row of a strip reaches the strip below through HBM: per column and lane the pair (H, F) as patterns
        // on that column's scale - all strips rebase their column shift at the same chunks, so a pattern means the same
        // in either - 512 bytes per column and wavefront, written once and read once: [column pair][lane] (StripRows).
        // (wave-uniform bases and 32-bit element offsets: scalar base + one offset register per access)
        // The producer and the consumer of a row usually sit in different XCDs, whose L2 caches do not
        // see each other: the rows travel as agent-scope relaxed atomics (write-through stores, loads
        // that bypass the local L2), ordered against the progress counter by waiting for the memory
        // operations themselves - release / acquire FENCES at agent scope write back and invalidate
        // the whole L2 each time, 80 us per chunk when every wavefront of the chip does it.
        const StripRows rowsIn(a.boundary[(s + 1) & 1] + a.boundaryOff[g]), rowsOut(a.boundary[s & 1] + a.boundaryOff[g]);
        int* progOut = a.unitFlags + (size_t)gIdx * nStrips + s;
        const int* progIn = progOut - 1;
        const int lastCol = nChunks * 4 - 1;
        // The wavefront of (group, s) follows the wavefront of (group, s - 1) - which may still be running in another
        // workgroup when the batches are few - kLag chunks behind: the producer publishes the number of finished
        // chunks, the consumer waits for it before it fetches rows it has not seen published (stripPublish /
        // stripPoll, common.h). Chunks the strip above must be ahead: the rows of columns up to j + (rows ahead) are fetched
        constexpr int kLag = 1 + (MIOPAL_STRIP_ROWS_AHEAD + 3) / 4;
        int avail = fromAbove ? 0 : nChunks;   // chunks of the strip above known to be published
        // (test hook, host.hip miopalTestInjectFault: this unit behaves like one that died - no sweep, no
        // progress published, its lanes flagged - so that the strip below runs into its time-out)
        const bool injected = u + 1 == a.faultUnit1;
        bool dead = injected;
        // Every taken unit's producer was taken before it and strip 0 waits for nobody, so the chain always moves; a
        // consumer that nevertheless waits longer than about a second gives up (dead): its lanes are flagged and the
        // next rung recomputes them, and the strip below is told (poison).
        auto waitFor = [&](int need) {
#ifdef MIOPAL_ABL_NO_POLL
            avail = nChunks;
#endif
            if (avail >= need) return;
            timer.start(1);
            // (wave-uniform: every lane reads the same counter)
            int spins = 0;
            while (avail < need) {
                avail = stripPoll(progIn);
                if (avail >= need) break;
                __builtin_amdgcn_s_sleep(MIOPAL_STRIP_SLEEP);
                if (++spins > spinCap) avail = kStripPoison;
#if MIOPAL_STRIP_FRAME_ABORTS
                // (the unit above may never be taken once the launch has given up)
                if (a.stripAbort && __hip_atomic_load(a.stripAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.stripAbortAt)
                    avail = kStripPoison;
#endif
            }
            timer.stop(1);
            if (avail >= kStripPoison) dead = true;
        };
        if (!dead) waitFor(min(kLag + MIOPAL_STRIP_SLACK, nChunks));
#elif MIOPAL_STRIP_FRAME_PART == 3
        // the sweep is compiled for the three kinds of strip (first / inner / last): no selects between border and
        // row above, no stores from the last strip
        if (!dead) {
            pace.begin(lane);
            timer.start(3);
#if MIOPAL_STRIP_FRAME_ABORTS
            if (!fromAbove) sweep(std::false_type{}, std::true_type{});
            else if (toBelow) sweep(std::true_type{}, std::true_type{});
            else sweep(std::true_type{}, std::false_type{});
#else
            // (a lone strip is the one-strip kernel's business and is not swept: the launcher refuses it. The
            // Smith-Waterman form above would sweep it as a first strip; its launcher refuses it too.)
            if (!fromAbove && toBelow) sweep(std::false_type{}, std::true_type{});
            else if (fromAbove && toBelow) sweep(std::true_type{}, std::true_type{});
            else if (fromAbove) sweep(std::true_type{}, std::false_type{});
#endif
            timer.stop(3);
            pace.end(lane);
        }
#elif MIOPAL_STRIP_FRAME_PART == 4
        if (dead) {
            // the strip above never got here: leave the answers to the next rung, tell the strip below
            if (toBelow && lane == 0 && !injected) __hip_atomic_store(progOut, kStripPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.overflow) a.overflow[base + lane] = a.overflow[base + kLanes + lane] = 1;
            continue;
        }
#else
#error "MIOPAL_STRIP_FRAME_PART: 1, 2, 3 or 4"
#endif
#undef MIOPAL_STRIP_FRAME_PART
