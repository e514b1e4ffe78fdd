// What the pair-table kernels share (overview of the families: interseq_impl.h): the representation's constants, the
// compile-time knobs, the table's layout and the address of a row, the boundary rows between strips, the pacing of a
// SIMD's wavefronts, the priority step, the dynamic rounds of the one-strip hand-out and the publish step of the strips.
// (The table build, the hand-out of the one-strip kernels and the unit frame of the multi-strip kernels are written
// once too, as text the kernels include: interseq_pair_table_build.inc, interseq_pair_handout.inc,
// interseq_strip_frame.inc. As functions or structs of this header they changed the kernels' code objects - the order
// of phi nodes and of reassociated sums, and the register allocation with them; see
// profiles/pair_table_parts_device_code.txt.)
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace miopal {

// ---- biased integer halves, column-shifted ----------------------------------------
// Third arithmetic for the pair-table kernel. A half holds the unsigned integer
//     kBiasedZero + x + shift(j),      shift(j) = (j - j0) * ext,
// for a true value x of column j, and is COMPARED as a half float: between 0x0400 (smallest
// normal) and 0x7BFF (largest finite) the order of the bit patterns is the order of the
// numbers, so v_pk_maximum3_f16 still folds two max per cell while every addition is a plain
// 32-bit integer add over both halves at once: the pair table holds
// (sB' << 16) + sA' as ONE signed integer, so the borrow of a negative low score is undone by
// the carry of the sum as long as each half stays in [0, 65535]. The column shift makes
// extending E free (the next column's shift absorbs the ext) and lets E and F open with the same
// h - (open - ext); the Smith-Waterman floor becomes the column's own zero `fl`:
//     h    = max3(Hdiag + s', E, F)                s' = s + ext (one column to the right)
//     hmo  = h - (open - ext)
//     E    = max3(E, hmo, fl + ext)                (already on the next column's scale)
//     F    = max3(F, hmo, fl + ext) - ext
// 3 integer adds + 3.5 max3 per cell pair instead of 4 packed half adds + 3.5 max3, and the exact
// range grows from 2048 to kBiasedScoreLimit. Measured mix: tools/ubench_mix.hip. Every kBiasedMaxShift
// of accumulated shift the state is rebased (112 subtractions). A half that reaches 0x7C00
// (inf / NaN patterns) makes the column maximum inf / NaN (maximum3 propagates NaN, payloads stay
// below 0x8000), the running best is an INTEGER max of (column maximum - fl) and therefore ends
// at or above kBiasedScoreLimit: the lane is flagged and redone by the next rung.
// (kBiasedScoreLimit, kBiasedMaxShift, kBiasedPad - the padding symbol / padding rows of the profile, a true value -
// and the host's bounds on scores and gap costs: common.h)
constexpr int kBiasedZero = 0x0800;      // pattern of a true 0 at shift 0; 0x0400 of room below
constexpr int kBiasedGuard = 0x0400;     // how far a value may dip below the column's zero
static_assert(kBiasedScoreLimit == 0x7C00 - kBiasedZero - kBiasedMaxShift, "the exact range ends where inf / NaN begin");
static_assert(kBiasedPad == -kBiasedGuard, "padding sits as far below the column's zero as the guard band allows");
static_assert(kBiasedMaxMagnitude <= kBiasedGuard && 5 * kBiasedMaxExt <= kBiasedMaxShift, "guard band");

// End locations (LOC): every value is scaled by 2^kBits (kBits = 4, 5 or 6: enough for the strip's
// rows), so the low bits of a cell are free, and the key  h + (2^kBits - 1 - row)  is folded instead
// of h: the column maximum then carries the FIRST row that holds it, for one more integer add per
// cell pair, and the running best (an integer max against best | rowmask, i.e. strictly greater
// scores only) carries the row of the first maximum in column-major order. No row scan. The exact
// range shrinks to kLocLimit(kBits) - 384 for 64 rows, above what a 64-residue query can score with
// the usual protein matrices short of near-identity; flagged lanes take the next rung as always.
// (kLocZeroPattern, kLocGuardBand, locRowBits: common.h)
__host__ __device__ constexpr int locLimit(int bits) { return (0x7C00 - kLocZeroPattern - kBiasedMaxShift) >> bits; }

// ---- compile-time knobs of the pair-table kernels (tools/ab_build.sh sets them; the product build sets none) ----
// Pacing of the wavefronts that share a SIMD (round 3). The twelve wavefronts of a unit sweep groups of
// (nearly) equal length and meet at the unit's barrier, but a SIMD serves its OLDEST ready wavefront
// first: of three with equal work the first is done after little more than half the unit's time, the
// last sweeps the rest of its group alone on a SIMD it cannot fill, and meanwhile the others wait at the
// barrier (PMC of the round-2 kernel on BASELINE configs[3]: wavefronts parked 47 % of their life,
// 15 % in the one-strip kernel whose wavefronts fetch new groups on their own). Each wavefront
// therefore publishes the chunk it is on in LDS, per hardware SIMD, and the one furthest behind runs at
// a higher priority: the three advance together and reach the barrier together.
#ifndef MIOPAL_STRIP_PACE
#define MIOPAL_STRIP_PACE 1
#endif
// The same pacing in the one-strip kernels, by what is left of each wavefront's current group: the last
// groups of a SIMD end together instead of one after the other (round 3; 393k / 500k targets x 300 at
// Q = 53: 0.634 -> 0.574 / 0.816 -> 0.742 ms, nothing lost at other sizes: profiles/r03_headline_pace_ab.txt)
#ifndef MIOPAL_HEADLINE_PACE
#define MIOPAL_HEADLINE_PACE 1
#endif

// Diagnostic builds of the strips kernels (tools/ab_build.sh; never the product build):
//   -DMIOPAL_STRIP_TIMING=1   every wavefront adds up s_memtime deltas around its wait sites and leaves them in
//                             InterseqArgs::stripTiming: [0] taking a unit (counter, the two barriers, the table
//                             when the strip changes), [1] polling the strip above, [2] the s_waitcnt before
//                             progress is published, [3] the sweeps (polls and publishes included), [4] the
//                             wavefront's life, [5] wavefronts (s_memtime comes back through lgkmcnt, so the LDS
//                             reads in flight are waited for at every mark: the build is slower than the product's)
//   -DMIOPAL_ABL_NO_POLL / _NO_ROW_LOADS / _NO_ROW_STORES / _NO_PUBLISH_WAIT
//                             ablations: the same instruction stream without one of the hand-over's parts (wrong
//                             results, honest timing: what that part costs)
#ifndef MIOPAL_STRIP_TIMING
#define MIOPAL_STRIP_TIMING 0
#endif
// Diagnostic build of the one-strip Smith-Waterman kernel (tools/ab_build.sh; never the product build):
//   -DMIOPAL_HEADLINE_TIMING=1   every wavefront stamps s_memrealtime (100 MHz, one clock for the whole device)
//                                when it starts and when it leaves; with MIOPAL_STRIP_TIMING=1 the host hands over
//                                InterseqArgs::stripTiming: [0] the earliest start (min), [1 + 4 * block + simd] the
//                                last exit on that SIMD (max), and prints how the SIMDs' finish times spread; behind
//                                them (from slot 1 + 4 * gridDim.x) when the pair table stood: the latest
//                                workgroup (max) and the sum over the workgroups - the prologue, launch to first column
#ifndef MIOPAL_HEADLINE_TIMING
#define MIOPAL_HEADLINE_TIMING 0
#endif
// The first two 4-row blocks of a column are fetched while the column before it is still
// being computed, the others two blocks ahead of their use: an LDS read waits behind the
// other eleven wavefronts' (bank-conflicted) reads, and a column that starts by waiting
// for its first scores leaves the SIMD to two wavefronts. MIOPAL_PAIR_AHEAD: blocks fetched ahead where the
// registers allow (three is the best of 1..3 on cfg2; the kernels' kWant takes fewer for tall strips);
// MIOPAL_PAIR_XCOL: 0 = no fetch across the column's end.
#ifndef MIOPAL_PAIR_AHEAD
#define MIOPAL_PAIR_AHEAD 3
#endif
#ifndef MIOPAL_PAIR_XCOL
#define MIOPAL_PAIR_XCOL 1
#endif
// The hand-over between strips (the multi-strip kernels' waitFor): how many columns ahead the row above is fetched, the s_sleep
// between two polls, and how many chunks more than needed the strip above must be ahead before a unit starts
#ifndef MIOPAL_STRIP_ROWS_AHEAD
#define MIOPAL_STRIP_ROWS_AHEAD 2
#endif
#ifndef MIOPAL_STRIP_SLEEP
#define MIOPAL_STRIP_SLEEP 8
#endif
#ifndef MIOPAL_STRIP_SLACK
#define MIOPAL_STRIP_SLACK 0
#endif
// progress is published every (mask + 1) chunks and at the end of the sweep (round 3: every 8 chunks
// instead of 4, and the counter fetched a chunk before it is needed, change nothing measurable - the
// hand-over is not what the wavefronts wait for: profiles/r03_handover_experiments.txt)
#ifndef MIOPAL_STRIP_PUBLISH_MASK
#define MIOPAL_STRIP_PUBLISH_MASK 3
#endif
constexpr int kStripPoison = 1 << 30;
constexpr int kStripSpinCap = 1 << 21;    // x s_sleep 8 (512 cycles): about half a second

// Boundary rows between strips travel 16 bytes a lane (round 4): {H, F} of TWO neighbouring columns per store /
// load, [column pair][lane] - the same bytes as before, half the memory instructions. An 8-byte sc1 store is one
// fabric write per lane at 2.7 x the time per byte of a 16-byte one, an 8-byte sc1 load runs at 0.54-0.70 x the
// 16-byte rate (MI355X_MICROARCH.md, "stores of each flavour"); the ablation builds (MIOPAL_ABL_*, above) showed each direction of
// the hand-over costing a cfg4 search 9 % (profiles/r04_strips_ablation.txt). buffer_load / buffer_store
// dwordx4 with sc1 (the atomics of common.h stop at 8 bytes); the compiler tracks them in vmcnt like any load.
typedef unsigned int StripU4 __attribute__((ext_vector_type(4)));
struct StripRows {
    __amdgpu_buffer_rsrc_t rsrc;
    __device__ __forceinline__ explicit StripRows(void* base)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7ffffff0, 0x00020000)) {}
    __device__ __forceinline__ StripU4 load(int pair, int lane) const {
#ifdef MIOPAL_ABL_NO_ROW_LOADS
        return StripU4{0x0a000a00u + (uint32_t)pair, 0x08000800u, 0x0a000a00u, 0x08000800u};
#else
        return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (pair * kLanes + lane) * 16, 0, 16 /* sc1 */);
#endif
    }
    __device__ __forceinline__ void store(int pair, int lane, StripU4 v) const {
#ifndef MIOPAL_ABL_NO_ROW_STORES
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (pair * kLanes + lane) * 16, 0, 16 /* sc1 */);
#else
        asm volatile("" ::"v"(v));
#endif
    }
};
struct StripTimer {
#if MIOPAL_STRIP_TIMING
    unsigned long long t[4] = {0, 0, 0, 0}, mark[4] = {0, 0, 0, 0}, born = __builtin_amdgcn_s_memtime();
    __device__ __forceinline__ void start(int k) { mark[k] = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void stop(int k) { t[k] += __builtin_amdgcn_s_memtime() - mark[k]; }
    __device__ __forceinline__ void flush(unsigned long long* out, int lane) {
        if (!out || lane != 0) return;
        for (int k = 0; k < 4; ++k) atomicAdd(out + k, t[k]);
        atomicAdd(out + 4, __builtin_amdgcn_s_memtime() - born);
        atomicAdd(out + 5, 1ull);
    }
#else
    __device__ __forceinline__ void start(int) {}
    __device__ __forceinline__ void stop(int) {}
    __device__ __forceinline__ void flush(unsigned long long*, int) {}
#endif
};
// Pacing of the wavefronts that share a SIMD (MIOPAL_STRIP_PACE / MIOPAL_HEADLINE_PACE above); kPaceInts: common.h
struct SimdPace {
    int* mine = nullptr;        // this wavefront's progress word
    const int4* simdRow = nullptr;
    // (once per kernel; `lds` = kPaceInts ints, every thread of the workgroup calls this)
    __device__ __forceinline__ void init(int* lds, int lane) {
        if (threadIdx.x < kPaceInts) lds[threadIdx.x] = threadIdx.x < 16 ? INT32_MAX : 0;
        __syncthreads();
        // HW_REG_HW_ID (4), SIMD_ID = bits 5:4
        const int simd = (int)__builtin_amdgcn_s_getreg(4 | (4 << 6) | ((2 - 1) << 11)) & 3;
        int slot = 0;
        if (lane == 0) slot = atomicAdd(&lds[16 + simd], 1);
        slot = __builtin_amdgcn_readfirstlane(slot) & 3;
        mine = lds + simd * 4 + slot;
        simdRow = reinterpret_cast<const int4*>(lds + simd * 4);
    }
    __device__ __forceinline__ void begin(int lane) const {
        if (MIOPAL_STRIP_PACE && lane == 0) *mine = 0;
    }
    __device__ __forceinline__ void end(int lane) const {
        if (MIOPAL_STRIP_PACE && lane == 0) *mine = INT32_MAX;   // (at the barrier: nobody waits for this one)
    }
    // at the top of chunk c; `fixed`: the wavefront keeps the priority it has (a long group)
    __device__ __forceinline__ void step(int c, int lane, bool fixed) const {
        if (!MIOPAL_STRIP_PACE || fixed) return;
        if (lane == 0) *mine = c;
        const int4 p = *simdRow;
        const int behind = __builtin_amdgcn_readfirstlane(min(min(p.x, p.y), min(p.z, p.w)));
        if (c <= behind) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
    }
};

// ---- the pair table -----------------------------------------------------------------
// pairs[tA * nSymbols + tB][r] in 16-byte slots of four rows (pairRowSlots, common.h)
template <int R>
struct PairLayout {
    static constexpr int kRowSlots = pairRowSlots(R);
    static __host__ __device__ constexpr size_t bytes(int nSymbols) { return pairLdsBytes(R, nSymbols); }
};

// LDS row of a residue pair (24-bit multiplies: v_mul_lo_u32 is a quarter-rate instruction)
// (interseq_pair_global_kernel calls this directly; the other three kernels through a one-line closure
// `rowOf`: called directly there, the phi nodes of the column loop change their order in some instantiations, and
// the register numbers with them - profiles/pair_table_parts_device_code.txt. An artefact of this compiler build:
// once the digests are re-based on another ROCm, the closures can go and the kernels call pairRowOf directly.)
template <int SLOTS>
static __device__ __forceinline__ const uint4* pairRowOf(const uint4* pairs, int nSym, uint32_t tA, uint32_t tB) {
    const uint32_t rowIdx = __umul24(tA, (uint32_t)nSym) + tB;
    return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(pairs) +
                                          __umul24(rowIdx, (uint32_t)(SLOTS * 16)));
}

// The entry transforms of the table build (interseq_pair_table_build.inc), true score v -> what the kernel adds to a
// half, by the names of the including kernel. Smith-Waterman: one column to the right (+ ext in pattern units), scaled
// by 2^kBits with end locations; kPadPattern: the padding symbol / padding rows, as far below the column's zero as the
// guard band allows. NW / HW / OV: s'' = s + 2 ext + c = s + ext + open (the diagonal step crosses two anti-diagonals,
// and H is kept in its stored form, c = open - ext below its plain form); padding adds c: the pattern of a padding
// cell is the one of its diagonal neighbour.
#define MIOPAL_SW_PAIR_ENTRY(v) (((v) == kBiasedPad ? kPadPattern : (v) << kBits) + ext)
#define MIOPAL_GLOBAL_PAIR_ENTRY(v) ((v) == kBiasedPad ? open - ext : (v) + ext + open)

// a group much longer than a wavefront's balanced share is on the launch's critical path: it wins the SIMD's issue
// arbitration against its co-resident wavefronts. Returns whether the group is such a one.
static __device__ __forceinline__ bool groupPriority(int nChunks, int priorityChunks) {
    const bool longGroup = nChunks > priorityChunks;
    if (longGroup) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(0);
    return longGroup;
}

// ---- hand-out of groups in the one-strip kernels: the dynamic rounds ---------------------
// Whoever finishes pulls the next group from a shared counter (behind the firstDynamic groups of the static first
// round). Groups of similar length (tailThrottle = groups per SIMD, rounded up; else 0): a SIMD that takes one
// group more than its share works a whole extra round while its neighbours idle, so every SIMD stops at its
// share - counted in LDS per hardware SIMD (simdTaken) - and the last round runs two wavefronts (or one) per
// SIMD, each faster for it. Shares add up to at least the number of groups, and a SIMD below its share keeps
// asking, so every group is taken. Returns the group's index in the launch; at or beyond nGroups: none is left.
static __device__ __forceinline__ int nextGroup(int* simdTaken, int simd, int tailThrottle, int* workCounter, int firstDynamic, int lane) {
    int g = 0;
    if (lane == 0) {
        bool take = true;
        if (tailThrottle > 0) take = atomicAdd(&simdTaken[simd], 1) < tailThrottle;
        g = take ? atomicAdd(workCounter, 1) : INT32_MAX - firstDynamic;
    }
    return __builtin_amdgcn_readfirstlane(g) + firstDynamic;
}

// ---- the hand-over between strips in the multi-strip kernels: the publish step -------------
// after chunk c of a strip that has one below: progress moves every (mask + 1) chunks and at the last (the wait inside
// also waits for the loads in flight); every row store of the chunks has COMPLETED before the counter moves
static __device__ __forceinline__ void stripPublishStep(int* progOut, int c, int nChunks, int lane, StripTimer& timer) {
    if (((c + 1) & MIOPAL_STRIP_PUBLISH_MASK) == 0 || c + 1 == nChunks) {
        timer.start(2);
        stripPublish(progOut, c + 1, lane);
        timer.stop(2);
    }
}
}  // namespace miopal
