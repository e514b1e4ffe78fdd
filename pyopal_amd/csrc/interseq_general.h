// The general inter-sequence kernel (any query length, all four modes) with its arithmetic flavours, and the first
// pair-table kernel, interseq_pair_kernel (int16 / half floats). Overview: interseq_impl.h.
#pragma once
#include <algorithm>

#include <type_traits>

#include "common.h"
#include "interseq_packed_ops.h"
#include "interseq_pair_parts.h"

namespace miopal {

// ---- arithmetic flavours --------------------------------------------------------
struct ArithSwI16 {
    static constexpr bool kFloor = true;    // Smith-Waterman
    static constexpr bool kDiag = false;
    static constexpr int kLimit = 0x7fff;   // a best at or above this may have clipped
    static constexpr bool kColShift = false;    // values of column j carry j * ext (ArithSwU16)
    static constexpr bool kStoresOpen = false;  // H[r] keeps h (true: h - (open - ext), ArithU16Diag)
    static constexpr bool kWeakPad = false;     // padding scores cannot win a max on their own
    static __device__ __forceinline__ uint32_t answerLowest() { return lowest(); }
    __device__ __forceinline__ uint32_t toTrue(uint32_t v, uint32_t) const { return v; }
    uint32_t open2, ext2;
    __device__ __forceinline__ ArithSwI16(int open, int ext) : open2(dup16(min(open, 32767))), ext2(dup16(min(ext, 32767))) {}
    __device__ __forceinline__ uint32_t addScore(uint32_t h, uint32_t s) const { return pk_add_sat_i16(h, s); }
    __device__ __forceinline__ uint32_t hmax(uint32_t d, uint32_t e, uint32_t f) const { return pk_max_i16(pk_max_i16(d, e), f); }
    __device__ __forceinline__ void track(uint32_t& best, uint32_t& held, uint32_t h, int r) const {
        (void)held; (void)r;
        best = pk_max_i16(best, h);
    }
    __device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) const { return pk_max_i16(a, b); }
    __device__ __forceinline__ uint32_t afterOpen(uint32_t h) const { return pk_sub_sat_u16(h, open2); }
    __device__ __forceinline__ uint32_t cellOpen(uint32_t h) const { return pk_sub_sat_u16(h, open2); }
    __device__ __forceinline__ uint32_t gap(uint32_t x, uint32_t hmo) const { return pk_max_i16(pk_sub_sat_u16(x, ext2), hmo); }
    __device__ __forceinline__ uint32_t fromInt(int v) const { return dup16(max(v, 0)); }
    static __device__ __forceinline__ uint32_t lowest() { return 0u; }
    static __device__ __forceinline__ int toInt(uint32_t half) { return (int)(short)half; }
};

struct ArithSwF16 {
    static constexpr bool kFloor = true;
    static constexpr bool kDiag = false;
    static constexpr int kLimit = 2048;
    static constexpr bool kColShift = false;    // values of column j carry j * ext (ArithSwU16)
    static constexpr bool kStoresOpen = false;  // H[r] keeps h (true: h - (open - ext), ArithU16Diag)
    static constexpr bool kWeakPad = false;     // padding scores cannot win a max on their own
    static __device__ __forceinline__ uint32_t answerLowest() { return lowest(); }
    __device__ __forceinline__ uint32_t toTrue(uint32_t v, uint32_t) const { return v; }
    uint32_t negOpen2, negExt2;
    static __device__ __forceinline__ uint32_t pack(int v) {
        const _Float16 h = (_Float16)(float)v;
        return (uint32_t)__builtin_bit_cast(unsigned short, h) * 0x00010001u;
    }
    __device__ __forceinline__ ArithSwF16(int open, int ext) : negOpen2(pack(-min(open, 2048))), negExt2(pack(-min(ext, 2048))) {}
    __device__ __forceinline__ uint32_t addScore(uint32_t h, uint32_t s) const { return pk_add_f16(h, s); }
    __device__ __forceinline__ uint32_t hmax(uint32_t d, uint32_t e, uint32_t f) const { return pk_max3_f16(d, e, f); }
    __device__ __forceinline__ void track(uint32_t& best, uint32_t& held, uint32_t h, int r) const {
        if (r & 1) best = pk_max3_f16(best, held, h);
        else held = h;
    }
    __device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) const { return pk_max3_f16(a, b, b); }
    __device__ __forceinline__ uint32_t afterOpen(uint32_t h) const { return pk_max3_f16(pk_add_f16(h, negOpen2), 0u, 0u); }
    // inside a cell the floor comes with the max3 of gap(), so the open step needs none
    __device__ __forceinline__ uint32_t cellOpen(uint32_t h) const { return pk_add_f16(h, negOpen2); }
    __device__ __forceinline__ uint32_t gap(uint32_t x, uint32_t hmo) const { return pk_max3_f16(pk_add_f16(x, negExt2), hmo, 0u); }
    __device__ __forceinline__ uint32_t fromInt(int v) const { return pack(max(v, 0)); }
    static __device__ __forceinline__ uint32_t lowest() { return 0u; }
    static __device__ __forceinline__ int toInt(uint32_t half) {
        return (int)(float)__builtin_bit_cast(_Float16, (unsigned short)half);
    }
};

struct ArithI16 {
    static constexpr bool kFloor = false;   // NW / HW / OV / anchored reverse pass
    static constexpr bool kDiag = false;
    static constexpr int kLimit = 0x7fff;   // ranges are checked statically by the host
    static constexpr bool kColShift = false;    // values of column j carry j * ext (ArithSwU16)
    static constexpr bool kStoresOpen = false;  // H[r] keeps h (true: h - (open - ext), ArithU16Diag)
    static constexpr bool kWeakPad = false;     // padding scores cannot win a max on their own
    static __device__ __forceinline__ uint32_t answerLowest() { return lowest(); }
    __device__ __forceinline__ uint32_t toTrue(uint32_t v, uint32_t) const { return v; }
    uint32_t open2, ext2;
    __device__ __forceinline__ ArithI16(int open, int ext) : open2(dup16(min(open, 32767))), ext2(dup16(min(ext, 32767))) {}
    __device__ __forceinline__ uint32_t addScore(uint32_t h, uint32_t s) const { return pk_add_sat_i16(h, s); }
    __device__ __forceinline__ uint32_t hmax(uint32_t d, uint32_t e, uint32_t f) const { return pk_max_i16(pk_max_i16(d, e), f); }
    __device__ __forceinline__ void track(uint32_t& best, uint32_t& held, uint32_t h, int r) const {
        (void)held; (void)r;
        best = pk_max_i16(best, h);
    }
    __device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) const { return pk_max_i16(a, b); }
    __device__ __forceinline__ uint32_t afterOpen(uint32_t h) const { return pk_sub_sat_i16(h, open2); }
    __device__ __forceinline__ uint32_t cellOpen(uint32_t h) const { return pk_sub_sat_i16(h, open2); }
    __device__ __forceinline__ uint32_t gap(uint32_t x, uint32_t hmo) const { return pk_max_i16(pk_sub_sat_i16(x, ext2), hmo); }
    __device__ __forceinline__ uint32_t fromInt(int v) const { return dup16(max(v, -32768)); }
    static __device__ __forceinline__ uint32_t lowest() { return 0x80008000u; }  // acts as -infinity
    static __device__ __forceinline__ int toInt(uint32_t half) { return (int)(short)half; }
};

// Signed int16 on anti-diagonally shifted values: every cell holds X + (i + j) * ext.
// Extending a gap then costs nothing (the shift of the next cell absorbs the ext), both
// gap kinds open with the same h + (ext - open), and the diagonal step's 2 * ext is
// folded into the query profile: 6 ops per cell pair instead of 8. Answers are shifted
// back where they are read. Needs (Q + L) * ext of extra head-room (checked by the host).
struct ArithI16Diag {
    static constexpr bool kFloor = false;
    static constexpr bool kDiag = true;
    static constexpr int kLimit = 0x7fff;
    static constexpr bool kColShift = false;    // values of column j carry j * ext (ArithSwU16)
    static constexpr bool kStoresOpen = false;  // H[r] keeps h (true: h - (open - ext), ArithU16Diag)
    static constexpr bool kWeakPad = false;     // padding scores cannot win a max on their own
    static __device__ __forceinline__ uint32_t answerLowest() { return lowest(); }
    // packed true values of stored cells whose shift is `shift2`
    __device__ __forceinline__ uint32_t toTrue(uint32_t v, uint32_t shift2) const { return pk_sub_sat_i16(v, shift2); }
    uint32_t extMinusOpen2;
    __device__ __forceinline__ ArithI16Diag(int open, int ext) : extMinusOpen2(dup16(max(ext - open, -32768))) {}
    __device__ __forceinline__ uint32_t addScore(uint32_t h, uint32_t s) const { return pk_add_sat_i16(h, s); }
    __device__ __forceinline__ uint32_t hmax(uint32_t d, uint32_t e, uint32_t f) const { return pk_max_i16(pk_max_i16(d, e), f); }
    __device__ __forceinline__ void track(uint32_t& best, uint32_t& held, uint32_t h, int r) const {
        (void)held; (void)r;
        best = pk_max_i16(best, h);
    }
    __device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) const { return pk_max_i16(a, b); }
    __device__ __forceinline__ uint32_t afterOpen(uint32_t h) const { return pk_add_sat_i16(h, extMinusOpen2); }
    __device__ __forceinline__ uint32_t cellOpen(uint32_t h) const { return pk_add_sat_i16(h, extMinusOpen2); }
    __device__ __forceinline__ uint32_t gap(uint32_t x, uint32_t hmo) const { return pk_max_i16(x, hmo); }
    __device__ __forceinline__ uint32_t fromInt(int v) const { return dup16(max(v, -32768)); }
    static __device__ __forceinline__ uint32_t lowest() { return 0x80008000u; }
    static __device__ __forceinline__ int toInt(uint32_t half) { return (int)(short)half; }
};

// NW / HW / OV on anti-diagonally shifted values like ArithI16Diag, as unsigned patterns compared as
// half floats (see "biased integer halves" further down; same idea in the general kernel, round 2).
// Plain form of a value x of cell (i, j): P(x) = kUnsignedDiagZero + x + (i + j) * ext. H[r] keeps the STORED
// form S(h) = P(h) - c, c = open - ext >= 0, which is at once the value both gap kinds open with, so:
//     d = S(Hd) + s''          s'' = s + 2 ext + c >= 0 (host: open + ext >= -min S): a plain integer add
//     h = max3(d, E, F)         one v_pk_maximum3_f16
//     hmo = h - c               integer subtract; also the next column's stored H
//     E = max(E, hmo), F = max(F, hmo)
// 2 integer adds + 3 half-float max + 1 v_perm per cell pair, against 2 saturating packed adds + 4
// packed max + 1 v_perm. Padding (symbol and rows) scores c after the shift, so that chains of padding
// cells never sink below lowest() + c and `h - c` can neither borrow from the other half nor leave the
// normal half floats; it can therefore reach real
// magnitudes, and the places that read answers mask rows and columns beyond the pair explicitly
// (kWeakPad). The host checks the static range (every pattern within [0, 0x7BFF]); answers are turned
// into packed true int16 values where they are read (toTrue).
// (kUnsignedDiagZero, the pattern of a true 0: common.h)
struct ArithU16Diag {
    static constexpr bool kFloor = false;
    static constexpr bool kDiag = true;
    static constexpr int kLimit = 0x7fff;
    static constexpr bool kColShift = false;    // values of column j carry j * ext (ArithSwU16)
    static constexpr bool kStoresOpen = true;
    static constexpr bool kWeakPad = true;
    int c;
    uint32_t c2, trueBias2;
    __device__ __forceinline__ ArithU16Diag(int open, int ext)
        : c(open - ext), c2((uint32_t)(open - ext) * 0x00010001u), trueBias2(dup16(kUnsignedDiagZero - (open - ext))) {}
    __device__ __forceinline__ uint32_t addScore(uint32_t h, uint32_t s) const { return h + s; }
    __device__ __forceinline__ uint32_t hmax(uint32_t d, uint32_t e, uint32_t f) const { return pk_max3_f16(d, e, f); }
    __device__ __forceinline__ void track(uint32_t& best, uint32_t& held, uint32_t h, int r) const {
        (void)held; (void)r;
        best = pk_max3_f16(best, h, h);
    }
    __device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) const { return pk_max_i16(a, b); }  // answers: true values
    __device__ __forceinline__ uint32_t afterOpen(uint32_t h) const { return h; }   // stored form = opened plain form
    __device__ __forceinline__ uint32_t cellOpen(uint32_t h) const { return h - c2; }
    __device__ __forceinline__ uint32_t gap(uint32_t x, uint32_t hmo) const { return pk_max3_f16(x, hmo, hmo); }
    __device__ __forceinline__ uint32_t fromInt(int v) const { return (uint32_t)(kUnsignedDiagZero + v - c) * 0x00010001u; }
    // ("minus infinity" of the cells: the smallest NORMAL half-float pattern. Patterns below 0x0400 are
    // denormals: they compare correctly, but a database with ragged groups - a third of its cells
    // padding, all of them down there - ran 20 % slower with 0 here.)
    static __device__ __forceinline__ uint32_t lowest() { return 0x04000400u; }
    static __device__ __forceinline__ uint32_t answerLowest() { return 0x80008000u; }
    static __device__ __forceinline__ int toInt(uint32_t half) { return (int)(short)half; }
    __device__ __forceinline__ uint32_t toTrue(uint32_t v, uint32_t shift2) const {
        const u16x2 r = __builtin_bit_cast(u16x2, v) - (__builtin_bit_cast(u16x2, shift2) + __builtin_bit_cast(u16x2, trueBias2));
        return __builtin_bit_cast(uint32_t, r);
    }
};

// Smith-Waterman in the general kernel on the representation of the pair-table kernel ("biased
// integer halves" further down), round 2: unsigned patterns compared as half floats, values of
// column j shifted by j * ext. Plain form of a value x of column j: P(x) = kSwShiftZero + x + j ext;
// H[r] keeps the stored form S(h) = P(h) - K with K >= 0 chosen by the host so that the profile
// entries s'' = s + ext + K are not negative (v_perm builds the pair of scores from 16-bit halves:
// a plain integer add over both halves needs them non-negative):
//     d = S(Hd) + s''                     plain form, on this column's scale
//     h = max3(d, E, F)
//     S(h) = h - K;  hmo = h - (open - ext)
//     E = max3(E, hmo, zero');  F = max3(F, hmo, zero') - ext        zero' = the next column's zero
// 4 integer adds + 3.5 max3 + 1 v_perm against 4 v_pk_add_f16 + 3.5 max3 + 1 v_perm, and an exact
// range of a.biasedLimit (tens of thousands minus ext x the longest packed target) instead of 2048:
// a 300-residue query's strong hits no longer send the whole view to the int16 rung. The all-cells
// maximum is folded per column and unshifted there (an integer max of true values, sticky for the
// inf / NaN patterns of a lane that left the range). No rebasing: the host only picks this flavour
// when zero + ext x (longest packed target) leaves a range worth having. Scores only (the end-location
// form keeps ArithSwF16: its row scans compare packed values of different columns).
// (kSwShiftZero, the pattern of a true 0 at shift 0: common.h)
struct ArithSwU16 {
    static constexpr bool kFloor = true;
    static constexpr bool kDiag = false;
    static constexpr int kLimit = 0x7fff;       // (unused: the limit of this flavour is a.biasedLimit)
    static constexpr bool kColShift = true;
    static constexpr bool kStoresOpen = false;
    static constexpr bool kWeakPad = false;
    uint32_t c2, k2, ext2;
    __device__ __forceinline__ ArithSwU16(int open, int ext, int K = 0)
        : c2((uint32_t)(open - ext) * 0x00010001u), k2((uint32_t)K * 0x00010001u), ext2((uint32_t)ext * 0x00010001u) {}
    __device__ __forceinline__ uint32_t addScore(uint32_t h, uint32_t s) const { return h + s; }
    __device__ __forceinline__ uint32_t hmax(uint32_t d, uint32_t e, uint32_t f) const { return pk_max3_f16(d, e, f); }
    __device__ __forceinline__ void track(uint32_t& cm, uint32_t& held, uint32_t h, int r) const {
        if (r & 1) cm = pk_max3_f16(cm, held, h);
        else held = h;
    }
    __device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) const {   // answers: true values
        const u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
        return __builtin_bit_cast(uint32_t, r);
    }
    __device__ __forceinline__ uint32_t afterOpen(uint32_t h) const { return h; }   // (borders are set up by hand)
    __device__ __forceinline__ uint32_t cellOpen(uint32_t h) const { return h - c2; }
    __device__ __forceinline__ uint32_t gap(uint32_t x, uint32_t hmo) const { return pk_max3_f16(x, hmo, hmo); }
    __device__ __forceinline__ uint32_t stored(uint32_t h) const { return h - k2; }
    __device__ __forceinline__ uint32_t fromInt(int v) const { return (uint32_t)v * 0x00010001u; }
    static __device__ __forceinline__ uint32_t lowest() { return 0u; }             // of the answers: true values
    static __device__ __forceinline__ uint32_t answerLowest() { return 0u; }
    static __device__ __forceinline__ int toInt(uint32_t half) { return (int)(half & 0xffffu); }
    __device__ __forceinline__ uint32_t toTrue(uint32_t v, uint32_t) const { return v; }
};

// 16-byte slots per profile row in LDS: odd, so that the 16 lanes of a
// ds_read_b128 lane group that hold different symbols land on different slots.
template <int R>
struct ProfileLayout {
    static constexpr int kSlots = (R / 8) | 1;
};

// take the halves of `v` named by the 0 / 0xffff masks in `m`, keep `dst` elsewhere
static __device__ __forceinline__ uint32_t selectHalves(uint32_t dst, uint32_t v, uint32_t m) {
    return (dst & ~m) | (v & m);
}

template <typename Arith>
static __device__ __forceinline__ Arith makeArith(const InterseqArgs& a) {
    if constexpr (Arith::kColShift) return Arith(a.gapOpen, a.gapExt, a.scoreBias);
    else return Arith(a.gapOpen, a.gapExt);
}

// MULTI = false: the query fits one strip (no boundary traffic, no rounds).
// LOC = true: also report where the answer was found (OPAL_SEARCH_SCORE_END): the
// first maximum when candidates are visited target column by target column and,
// inside a column, query row by query row (oracle/opal_oracle.c).
template <int R, typename Arith, int W, bool TRACK_ALL, bool MULTI, bool LOC, bool UNITS = false>
__global__ __launch_bounds__(W * kLanes)
void interseq_kernel(InterseqArgs a) {
    static_assert(MULTI || W == 1, "a single strip needs a single wavefront");
    static_assert(!UNITS || (MULTI && !LOC), "unit mode: scores of multi-strip queries");
    constexpr int kLowInt = Arith::kFloor ? 0 : INT32_MIN;
    static_assert(!(Arith::kDiag && TRACK_ALL), "the shifted flavour has no all-cells maximum");
    constexpr bool kRegions = !Arith::kFloor;  // Smith-Waterman flavours only know the all-cells maximum
    constexpr int SLOTS = ProfileLayout<R>::kSlots;
    constexpr int NB = R / 8;
    constexpr int WB = W > 1 ? W : 1;
    __shared__ uint4 ldsProf[W][(kMaxAlphabet + 1) * SLOTS];
    __shared__ uint2 ldsBnd[WB][2][W > 1 ? 4 * kLanes : 1];
    __shared__ uint32_t ldsOut[WB][W > 1 ? kLanes : 1];
    __shared__ int ldsLoc[(LOC && W > 1) ? W : 1][(LOC && W > 1) ? 10 : 1][(LOC && W > 1) ? kLanes : 1];

    const int wave = W > 1 ? (int)(threadIdx.x >> 6) : 0;
    const int lane = threadIdx.x & 63;
    const int nStrips = MULTI ? a.nStrips : 1;
    const int nRounds = (nStrips + W - 1) / W;
    // Unit mode (scores only, several rounds of strips per group): a workgroup does not own a group
    // for all its rounds but takes (group, round) units from a counter, rounds in order. The rounds
    // of a group already hand their last row over through HBM; a group of a 2000-residue query is
    // 4 rounds, and 782 such groups on 256 resident workgroups are 3.05 workgroup-lifetimes, i.e. 4:
    // with units of one round the last quarter of the launch is no longer three quarters idle.
    // The few answers a wavefront carries from round to round travel through a.unitPartial.
    __shared__ int ldsUnit;
    // (a template parameter: the extra scalars it keeps alive cost the classic form 5 % when both
    // shared one instantiation)
    constexpr bool unitMode = UNITS;
    int unitRound = 0;
next_unit:
    int groupIndex = blockIdx.x;
    if (unitMode) {
        if (threadIdx.x == 0) ldsUnit = atomicAdd(a.unitCounter, 1);
        __syncthreads();
        const int u = ldsUnit;
        __syncthreads();
        if (u >= a.nGroups * nRounds) return;
        groupIndex = u % a.nGroups;     // rounds in order: round r of every group before round r + 1 of any
        unitRound = u / a.nGroups;
        if (unitRound > 0) {
            // the round before this one, done by whoever took that unit (earlier than this one)
            if (threadIdx.x == 0)
                while (__hip_atomic_load(a.unitFlags + groupIndex, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < unitRound)
                    __builtin_amdgcn_s_sleep(4);
            __syncthreads();
        }
    }
    const int g = groupIndex + a.groupBase;  // one group of 128 targets per workgroup (and unit)

    uint4* prof = ldsProf[wave];
    const uint2* pack = a.pack + a.groupOff[g];
    // (a leading group whose longest targets were handed to the int32 kernel stops at the longest that stays)
    const int nChunks = groupIndex < a.capGroups ? min(a.groupChunks[g], a.capChunks) : a.groupChunks[g];
    if (nChunks > a.priorityChunks) __builtin_amdgcn_s_setprio(3);  // long group: critical path
    else if (unitMode) __builtin_amdgcn_s_setprio(0);
    const Arith ar = makeArith<Arith>(a);
    const uint4* gprof = reinterpret_cast<const uint4*>(a.profile);
    const int rowSlotsGlobal = a.qPad / 8;
    const int Q = a.qLen;
    const bool topGap = a.topGap, leftGap = a.leftGap;
    const int region = kRegions ? a.region : (int)kAllCells;
    const int open = a.gapOpen, ext = a.gapExt;
    // value of a border cell k residues into a border (the other index is -1); the shifted
    // flavour stores X + (i + j) * ext (the other index is -1 here)
    auto border = [&](bool gap, int k) -> int {
        const int v = gap ? borderGap(k, open, ext) : 0;
        return Arith::kDiag ? v + (k - 1) * ext : v;
    };
    // shift a stored value of cell (i, j) back to its true value
    auto unshift = [&](uint32_t v, int i, int j) -> uint32_t {
        if (Arith::kDiag) return ar.toTrue(v, dup16((i + j) * ext));
        return v;
    };

    // per-lane target lengths (NW / OV take answers at each target's own last column)
    const size_t base = (size_t)g * kGroupTargets;
    int lenA = 0, lenB = 0;
    if (LOC || (kRegions && (!TRACK_ALL || region != kAllCells))) {
        lenA = a.lens[base + lane];
        lenB = a.lens[base + kLanes + lane];
    }

    uint32_t best = Arith::lowest(), held = Arith::lowest();  // maximum over all cells (TRACK_ALL)
    uint32_t ans = Arith::answerLowest();                      // answer of the other regions (true values)
    uint32_t H[R], E[R];
    // LOC state, one set per packed half (A = low, B = high): running best score with
    // its column / row, the same for the strip in flight (all-cells region), and the
    // last-column candidate of OV
    int runA = kLowInt, runB = kLowInt, colA = -1, colB = -1, rowA = -1, rowB = -1;
    int scolA = -1, scolB = -1, srowA = -1, srowB = -1;
    int cbA = kLowInt, cbB = kLowInt, crowA = -1, crowB = -1;
    uint32_t bestPrev = Arith::lowest();

    const int lastStrip = nStrips - 1;
    const int rl = Q - 1 - lastStrip * R;  // row of the last query residue inside the last strip
    const int nSteps = nChunks + (W - 1);
    if (unitMode && unitRound > 0) {
        // what this wavefront's strips of the earlier rounds found
        const uint2 p = a.unitPartial[((size_t)groupIndex * W + wave) * kLanes + lane];
        best = p.x;
        ans = p.y;
    }

    for (int rho = unitMode ? unitRound : 0; rho < (unitMode ? unitRound + 1 : nRounds); ++rho) {
        const int s = rho * W + wave;
        const bool active = s < nStrips;
        const bool isLast = s == lastStrip;
        const bool inGlobal = MULTI && active && s > 0 && wave == 0;  // boundary of the previous round, from HBM
        const bool inLds = MULTI && active && s > 0 && wave > 0;      // boundary of the wavefront above, from LDS
        const bool outGlobal = MULTI && active && s + 1 < nStrips && wave == W - 1;
        const bool outLds = MULTI && active && s + 1 < nStrips && wave < W - 1;
        const uint2* bin = nullptr;
        uint2* bout = nullptr;
        if (MULTI && nRounds > 1) {
            bin = a.boundary[(rho + 1) & 1] + a.boundaryOff[g];
            bout = a.boundary[rho & 1] + a.boundaryOff[g];
        }

        uint32_t hdiagTop = Arith::lowest();
        // column-shifted flavour: the zero of the last column done (column -1 at a round's start)
        uint32_t fl = 0u;
        if (active) {
            // stage this strip's slice of the query profile into the wavefront's LDS region
            for (int idx = lane; idx < a.nSymbols * (R / 8); idx += kLanes) {
                const int t = idx / (R / 8), k = idx - t * (R / 8);
                prof[t * SLOTS + k] = gprof[t * rowSlotsGlobal + s * (R / 8) + k];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // column -1: left border H[i][-1] and the E it induces in column 0
            const int i0 = s * R;
            if constexpr (Arith::kColShift) {
                // H[r][-1] = 0 on column -1's scale (stored form), E[r][0] = 0 on column 0's
                fl = ar.fromInt(kSwShiftZero) - ar.ext2;
                const uint32_t h0 = ar.stored(fl), e0 = fl + ar.ext2;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    H[r] = h0;
                    E[r] = e0;
                }
                hdiagTop = h0;
            } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                uint32_t hl;
                if (Arith::kFloor) hl = 0u;
                else if (i0 + r >= Q) hl = Arith::lowest();
                else hl = ar.fromInt(border(leftGap, i0 + r));
                H[r] = hl;
                E[r] = ar.afterOpen(hl);
            }
            // H[i0-1][-1]: diagonal of the strip's first row in column 0
            if (Arith::kFloor) hdiagTop = 0u;
            else hdiagTop = s == 0 ? ar.fromInt(Arith::kDiag ? -2 * ext : 0) : ar.fromInt(border(leftGap, i0 - 1));
            }
        }

        uint2 cur = {0, 0}, nxt = {0, 0};
        uint2 n0 = {0, 0}, n1 = {0, 0}, n2 = {0, 0}, n3 = {0, 0};
        if (active) {
            cur = pack[lane];
            if (inGlobal) {
                n0 = bin[0 * kLanes + lane];
                n1 = bin[1 * kLanes + lane];
                n2 = bin[2 * kLanes + lane];
                n3 = bin[3 * kLanes + lane];
            }
        }

        for (int tau = 0; tau < nSteps; ++tau) {
            const int c = tau - wave;
            if (active && c >= 0 && c < nChunks) {
                uint2 b0 = n0, b1 = n1, b2 = n2, b3 = n3;
                if (W > 1 && inLds) {
                    const uint2* p = ldsBnd[wave - 1][c & 1] + lane;
                    b0 = p[0 * kLanes];
                    b1 = p[1 * kLanes];
                    b2 = p[2 * kLanes];
                    b3 = p[3 * kLanes];
                }
                if (c + 1 < nChunks) {
                    nxt = pack[(size_t)(c + 1) * kLanes + lane];
                    if (MULTI && inGlobal) {
                        const uint2* p = bin + (size_t)(c + 1) * 4 * kLanes + lane;
                        n0 = p[0 * kLanes];
                        n1 = p[1 * kLanes];
                        n2 = p[2 * kLanes];
                        n3 = p[3 * kLanes];
                    }
                }
                uint32_t ra = cur.x, rb = cur.y;
#pragma unroll 1
                for (int cc = 0; cc < 4; ++cc) {
                    const int j = c * 4 + cc;
                    const uint32_t tA = ra & 0xffu, tB = rb & 0xffu;
                    ra >>= 8;
                    rb >>= 8;
                    const uint4* pa = prof + tA * SLOTS;
                    const uint4* pb = prof + tB * SLOTS;
                    // row above the strip: H[i0-1][j-1] (diagonal) and the F entering row i0
                    uint32_t diag = hdiagTop;
                    uint32_t f;
                    uint32_t fl1 = 0u, cm = 0u, cheld = 0u;   // column-shifted flavour only
                    if constexpr (Arith::kColShift) {
                        fl += ar.ext2;                    // this column's zero
                        fl1 = fl + ar.ext2;               // the next column's
                        asm volatile("" : "+v"(fl1));     // (a VGPR: max3 with a scalar operand issues slower)
                        cm = cheld = fl;
                    }
                    if (!MULTI || s == 0) {
                        uint32_t topH = Arith::kFloor ? 0u : ar.fromInt(border(topGap, j));  // H[-1][j]
                        if constexpr (Arith::kColShift) topH = ar.stored(fl);                 // 0 on this column's scale
                        hdiagTop = topH;
                        f = ar.afterOpen(topH);
                        if constexpr (Arith::kColShift) f = fl;                               // F entering row 0: the floor
                    } else {
                        hdiagTop = b0.x;
                        f = b0.y;
                    }
                    // Profile rows are fetched one 8-row block ahead of their use; the compiler
                    // barrier at the end of each block keeps hipcc from hoisting every
                    // ds_read_b128 and v_perm to the top of the column (~60 VGPRs, one wave
                    // of occupancy).
                    uint4 va[NB], vb[NB];
                    va[0] = pa[0];
                    vb[0] = pb[0];
                    // {A's score, B's score} for query row r
                    auto score = [&](int r) -> uint32_t {
                        const uint4 x = va[r >> 3], y = vb[r >> 3];
                        const int k = (r & 7) >> 1;
                        const uint32_t wa = k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w;
                        const uint32_t wb = k == 0 ? y.x : k == 1 ? y.y : k == 2 ? y.z : y.w;
                        return __builtin_amdgcn_perm(wb, wa, (r & 1) ? 0x07060302u : 0x05040100u);
                    };
                    uint32_t dsum = ar.addScore(diag, score(0));
#pragma unroll
                    for (int r8 = 0; r8 < NB; ++r8) {
                        if (r8 + 1 < NB) {
                            va[r8 + 1] = pa[r8 + 1];
                            vb[r8 + 1] = pb[r8 + 1];
                        }
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const int r = r8 * 8 + k;
                            // consume the old H[r] (diagonal of row r+1) before H[r] is rewritten
                            uint32_t dnext = 0;
                            if (r + 1 < R) dnext = ar.addScore(H[r], score(r + 1));
                            const uint32_t h = ar.hmax(dsum, E[r], f);
                            const uint32_t hmo = ar.cellOpen(h);
                            if constexpr (Arith::kColShift) {
                                ar.track(cm, cheld, h, r);                     // this column's maximum
                                E[r] = pk_max3_f16(E[r], hmo, fl1);
                                asm volatile("" : "+v"(E[r]));
                                f = pk_max3_f16(f, hmo, fl1) - ar.ext2;
                                H[r] = ar.stored(h);
                            } else {
                            if (TRACK_ALL) ar.track(best, held, h, r);
                            E[r] = ar.gap(E[r], hmo);
                            // (at its row: E is off the critical path, and hipcc defers the R updates to
                            // the end of the block, each holding on to its hmo)
                            asm volatile("" : "+v"(E[r]));
                            f = ar.gap(f, hmo);
                            H[r] = Arith::kStoresOpen ? hmo : h;
                            }
                            dsum = dnext;
                        }
                        // pins the schedule: the block's cells are finished before the loads
                        // (and v_perm) of the block after next may start
                        asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
                    }
                    if constexpr (Arith::kColShift) {
                        // true values of this column's maximum: an integer max (sticky for inf / NaN patterns)
                        if (R & 1) cm = pk_max3_f16(cm, cheld, cheld);
                        best = ar.max2(best, cm - fl);
                    }
                    if (outGlobal) bout[((size_t)c * 4 + cc) * kLanes + lane] = make_uint2(H[R - 1], f);
                    if (W > 1 && outLds) ldsBnd[wave][c & 1][cc * kLanes + lane] = make_uint2(H[R - 1], f);
                    if (MULTI) {
                        b0 = b1;
                        b1 = b2;
                        b2 = b3;
                    }

                    if constexpr (LOC && TRACK_ALL) {
                        // a half of `best` that changed in this column holds a new strict
                        // maximum: its row is the first row of the column with that value
                        const uint32_t ch = best ^ bestPrev;
                        if (region == kAllCells && __builtin_amdgcn_ballot_w64(ch != 0) != 0) {
                            const uint32_t nbA = best & 0xffffu, nbB = best >> 16;
                            int ra = 0, rb = 0;
#pragma unroll
                            for (int r = R - 1; r >= 0; --r) {
                                if ((H[r] & 0xffffu) == nbA) ra = r;
                                if ((H[r] >> 16) == nbB) rb = r;
                            }
                            if (ch & 0xffffu) {
                                scolA = j;
                                srowA = s * R + ra;
                            }
                            if (ch >> 16) {
                                scolB = j;
                                srowB = s * R + rb;
                            }
                            bestPrev = best;
                        }
                    }
                    if constexpr (LOC && kRegions) {
                        if (region != kAllCells) {
                            const uint32_t lastMask = ((j == lenA - 1) ? 0x0000ffffu : 0u) |
                                                      ((j == lenB - 1) ? 0xffff0000u : 0u);
                            if (isLast) {
                                uint32_t hq = H[0];
#pragma unroll
                                for (int r = 1; r < R; ++r)
                                    if (r == rl) hq = H[r];
                                hq = unshift(hq, Q - 1, j);
                                const int qA = Arith::toInt(hq & 0xffffu), qB = Arith::toInt(hq >> 16);
                                if (region == kLastCell) {
                                    if (j == lenA - 1) { runA = qA; colA = j; }
                                    if (j == lenB - 1) { runB = qB; colB = j; }
                                } else {
                                    // last row: HW scans columns < len, OV columns < len - 1 (its
                                    // last column is scanned row by row below)
                                    const int cut = region == kLastRowCol ? 1 : 0;
                                    if (j < lenA - cut && qA > runA) { runA = qA; colA = j; }
                                    if (j < lenB - cut && qB > runB) { runB = qB; colB = j; }
                                }
                            }
                            if (region == kLastRowCol && __builtin_amdgcn_ballot_w64(lastMask != 0) != 0) {
                                int mA = INT32_MIN, mB = INT32_MIN, ra = 0, rb = 0;
                                uint32_t off = Arith::kDiag ? dup16((s * R + R - 1 + j) * ext) : 0u;
                                const uint32_t step = Arith::kDiag ? dup16(ext) : 0u;
#pragma unroll
                                for (int r = R - 1; r >= 0; --r) {
                                    const uint32_t offR = off;
                                    if (Arith::kDiag) {
                                        off -= step;  // running shift of the row above
                                        asm volatile("" : "+v"(off));
                                    }
                                    if (s * R + r < Q) {
                                        const uint32_t hv = Arith::kDiag ? ar.toTrue(H[r], offR) : H[r];
                                        const int hA = Arith::toInt(hv & 0xffffu), hB = Arith::toInt(hv >> 16);
                                        if (hA >= mA) { mA = hA; ra = r; }
                                        if (hB >= mB) { mB = hB; rb = r; }
                                    }
                                }
                                if ((lastMask & 0xffffu) && mA > cbA) { cbA = mA; crowA = s * R + ra; }
                                if ((lastMask >> 16) && mB > cbB) { cbB = mB; crowB = s * R + rb; }
                            }
                        }
                    }
                    // ---- answers on the last query row / each target's last column ----
                    if (!LOC && kRegions && (!TRACK_ALL || region != kAllCells)) {
                        const uint32_t lastMask = ((j == lenA - 1) ? 0x0000ffffu : 0u) |
                                                  ((j == lenB - 1) ? 0xffff0000u : 0u);
                        if (isLast) {
                            uint32_t hq = H[0];
#pragma unroll
                            for (int r = 1; r < R; ++r)
                                if (r == rl) hq = H[r];
                            hq = unshift(hq, Q - 1, j);
                            if (region == kLastCell) {
                                ans = selectHalves(ans, hq, lastMask);
                            } else if (Arith::kWeakPad) {
                                // last row, columns of the target only
                                const uint32_t inside = ((j < lenA) ? 0x0000ffffu : 0u) | ((j < lenB) ? 0xffff0000u : 0u);
                                ans = selectHalves(ans, ar.max2(ans, hq), inside);
                            } else {
                                ans = ar.max2(ans, hq);  // last row; padded columns never exceed real ones
                            }
                        }
                        if (region == kLastRowCol && __builtin_amdgcn_ballot_w64(lastMask != 0) != 0) {
                            // some lane is on its target's last column: maximum over this strip's rows
                            // (the shift of row r is kept as a running packed value: one add per row
                            // here instead of R live offsets)
                            uint32_t off = Arith::kDiag ? dup16((s * R + j) * ext) : 0u;
                            const uint32_t step = Arith::kDiag ? dup16(ext) : 0u;
                            uint32_t cm = Arith::kDiag ? ar.toTrue(H[0], off) : H[0];
#pragma unroll
                            for (int r = 1; r < R; ++r) {
                                if (Arith::kDiag) {
                                    off += step;  // halves stay below 32000: no carry between them
                                    asm volatile("" : "+v"(off));
                                    // (rows beyond the query only matter when padding can score: kWeakPad)
                                    if (!Arith::kWeakPad || s * R + r < Q) cm = ar.max2(cm, ar.toTrue(H[r], off));
                                } else {
                                    cm = ar.max2(cm, H[r]);
                                }
                            }
                            ans = selectHalves(ans, ar.max2(ans, cm), lastMask);
                        }
                    }
                }
                cur = nxt;
            }
            if (W > 1) __syncthreads();
        }
        if constexpr (LOC && TRACK_ALL) {
            if (region == kAllCells && active) {
                // fold this strip's first maximum into the running one: higher score wins,
                // then the smaller column (rows of later strips are larger)
                const int sA = Arith::toInt(best & 0xffffu), sB = Arith::toInt(best >> 16);
                if (scolA >= 0 && (sA > runA || (sA == runA && scolA < colA))) { runA = sA; colA = scolA; rowA = srowA; }
                if (scolB >= 0 && (sB > runB || (sB == runB && scolB < colB))) { runB = sB; colB = scolB; rowB = srowB; }
                best = Arith::lowest();
                held = Arith::lowest();
                bestPrev = Arith::lowest();
                scolA = scolB = srowA = srowB = -1;
            }
        }
        if (MULTI && nRounds > 1) {
            // the next round's first strip reads what this round's last strip wrote to HBM
            __threadfence();
            if (W > 1) __syncthreads();
        }
    }

    // ---- combine the wavefronts' partial answers ---------------------------------
    if constexpr (LOC) {
        if (W > 1) {
            ldsLoc[wave][0][lane] = runA;
            ldsLoc[wave][1][lane] = runB;
            ldsLoc[wave][2][lane] = colA;
            ldsLoc[wave][3][lane] = colB;
            ldsLoc[wave][4][lane] = rowA;
            ldsLoc[wave][5][lane] = rowB;
            ldsLoc[wave][6][lane] = cbA;
            ldsLoc[wave][7][lane] = cbB;
            ldsLoc[wave][8][lane] = crowA;
            ldsLoc[wave][9][lane] = crowB;
            __syncthreads();
            if (wave != 0) return;
            for (int w = 1; w < W; ++w) {
                const int oA = ldsLoc[w][0][lane], oB = ldsLoc[w][1][lane];
                const int ocA = ldsLoc[w][2][lane], ocB = ldsLoc[w][3][lane];
                const int orA = ldsLoc[w][4][lane], orB = ldsLoc[w][5][lane];
                // same order as the scan: score, then column, then row
                if (ocA >= 0 && (colA < 0 || oA > runA || (oA == runA && (ocA < colA || (ocA == colA && orA < rowA))))) {
                    runA = oA; colA = ocA; rowA = orA;
                }
                if (ocB >= 0 && (colB < 0 || oB > runB || (oB == runB && (ocB < colB || (ocB == colB && orB < rowB))))) {
                    runB = oB; colB = ocB; rowB = orB;
                }
                const int pA = ldsLoc[w][6][lane], pB = ldsLoc[w][7][lane];
                const int prA = ldsLoc[w][8][lane], prB = ldsLoc[w][9][lane];
                if (prA >= 0 && (crowA < 0 || pA > cbA || (pA == cbA && prA < crowA))) { cbA = pA; crowA = prA; }
                if (prB >= 0 && (crowB < 0 || pB > cbB || (pB == cbB && prB < crowB))) { cbB = pB; crowB = prB; }
            }
        }
        if (region != kAllCells) {
            // answers of the last-row regions sit on query row Q - 1
            rowA = colA >= 0 ? Q - 1 : -1;
            rowB = colB >= 0 ? Q - 1 : -1;
        }
        if (region == kLastRowCol) {
            // OV: the last column is scanned after the last row, strictly greater wins
            if (crowA >= 0 && (colA < 0 || cbA > runA)) { runA = cbA; rowA = crowA; colA = lenA - 1; }
            if (crowB >= 0 && (colB < 0 || cbB > runB)) { runB = cbB; rowB = crowB; colB = lenB - 1; }
        }
        a.score[base + lane] = runA;
        a.score[base + kLanes + lane] = runB;
        a.endI[base + lane] = rowA;
        a.endI[base + kLanes + lane] = rowB;
        a.endJ[base + lane] = colA;
        a.endJ[base + kLanes + lane] = colB;
        if (a.overflow) {
            a.overflow[base + lane] = runA >= Arith::kLimit;
            a.overflow[base + kLanes + lane] = runB >= Arith::kLimit;
        }
        return;
    }
    if (unitMode && unitRound + 1 < nRounds) {
        // not the group's last round: leave the partial answers and the round's boundary row (HBM,
        // fenced above) to whoever takes the next round of this group
        a.unitPartial[((size_t)groupIndex * W + wave) * kLanes + lane] = make_uint2(best, ans);
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(a.unitFlags + groupIndex, unitRound + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        goto next_unit;
    }
    {
        uint32_t res = (TRACK_ALL && region == kAllCells) ? best : ans;
        if (W > 1) {
            ldsOut[wave][lane] = res;
            __syncthreads();
            if (wave == 0)
                for (int w = 1; w < W; ++w) res = ar.max2(res, ldsOut[w][lane]);
        }
        if (wave == 0) {
            const int lo = Arith::toInt(res & 0xffffu), hi = Arith::toInt(res >> 16);
            a.score[base + lane] = lo;
            a.score[base + kLanes + lane] = hi;
            if (a.overflow) {
                const int limit = Arith::kColShift ? a.biasedLimit : Arith::kLimit;
                a.overflow[base + lane] = lo >= limit;
                a.overflow[base + kLanes + lane] = hi >= limit;
            }
        }
    }
    if (unitMode) goto next_unit;   // (the barriers of the hand-out keep ldsOut safe)
}

template <int R, typename Arith, bool TRACK_ALL, bool LOC>
static hipError_t launchW(const InterseqArgs& a, int waves, hipStream_t stream) {
    const dim3 grid(a.nGroups);
    if (a.nStrips == 1) {
        hipLaunchKernelGGL((interseq_kernel<R, Arith, 1, TRACK_ALL, false, LOC>), grid, dim3(kLanes), 0, stream, a);
        return hipGetLastError();
    }
    if constexpr (!LOC) {
        if (a.unitCounter != nullptr) {
            switch (waves) {
                case 1: hipLaunchKernelGGL((interseq_kernel<R, Arith, 1, TRACK_ALL, true, false, true>), grid, dim3(1 * kLanes), 0, stream, a); break;
                case 2: hipLaunchKernelGGL((interseq_kernel<R, Arith, 2, TRACK_ALL, true, false, true>), grid, dim3(2 * kLanes), 0, stream, a); break;
                case 4: hipLaunchKernelGGL((interseq_kernel<R, Arith, 4, TRACK_ALL, true, false, true>), grid, dim3(4 * kLanes), 0, stream, a); break;
                case 8: hipLaunchKernelGGL((interseq_kernel<R, Arith, 8, TRACK_ALL, true, false, true>), grid, dim3(8 * kLanes), 0, stream, a); break;
                default: return hipErrorInvalidValue;
            }
            return hipGetLastError();
        }
    }
    switch (waves) {
        case 1: hipLaunchKernelGGL((interseq_kernel<R, Arith, 1, TRACK_ALL, true, LOC>), grid, dim3(1 * kLanes), 0, stream, a); break;
        case 2: hipLaunchKernelGGL((interseq_kernel<R, Arith, 2, TRACK_ALL, true, LOC>), grid, dim3(2 * kLanes), 0, stream, a); break;
        case 4: hipLaunchKernelGGL((interseq_kernel<R, Arith, 4, TRACK_ALL, true, LOC>), grid, dim3(4 * kLanes), 0, stream, a); break;
        case 8: hipLaunchKernelGGL((interseq_kernel<R, Arith, 8, TRACK_ALL, true, LOC>), grid, dim3(8 * kLanes), 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// Rows per strip are a multiple of 8 (one ds_read_b128 = 8 16-bit scores);
// `waves` (1, 2, 4 or 8) is the number of strips of a group in flight.
template <typename Arith, bool TRACK_ALL, bool LOC>
hipError_t launchFlavour(const InterseqArgs& a, int rowsPerStrip, int waves, hipStream_t stream) {
    return dispatchRows<8, 8, 8>(rowsPerStrip, [&](auto r) { return launchW<r, Arith, TRACK_ALL, LOC>(a, waves, stream); });
}


// ---- single-strip Smith-Waterman with a pair-indexed profile --------------------
// The {A's score, B's score} pair of a query row depends on the query row and on the
// two residues (tA, tB) only, so for a query that fits one strip the whole table
//     pairs[tA * nSymbols + tB][r] = { S[q_r][tA], S[q_r][tB] }
// fits the CU's 160 KB of LDS (625 rows x 60 dwords for the 24-letter protein
// alphabet and R = 56). One ds_read_b128 then delivers four ready-made operands and
// the v_perm_b32 per cell pair disappears (about 11 % of the VALU work). The table
// is built once per workgroup, so workgroups are persistent: kPairWavesPerGroup wavefronts
// each pull groups from a shared counter until none is left. (PairLayout: interseq_pair_parts.h)
template <int R, typename Arith>
__global__ __launch_bounds__(kPairWavesPerGroup * kLanes) void interseq_pair_kernel(InterseqArgs a) {
    constexpr int SLOTS = PairLayout<R>::kRowSlots;
    constexpr int NB4 = R / 4;
    extern __shared__ uint4 pairs[];

    const int lane = threadIdx.x & 63;
    const int nSym = a.nSymbols;
    const Arith ar(a.gapOpen, a.gapExt);

    // build the table: one thread per (pair row, 2 query rows)
    {
        const uint32_t* gw = reinterpret_cast<const uint32_t*>(a.profile);
        uint32_t* pw = reinterpret_cast<uint32_t*>(pairs);
        const int rowWords = a.qPad / 2;
        const int total = nSym * nSym * (R / 2);
        for (int idx = threadIdx.x; idx < total; idx += kPairWavesPerGroup * kLanes) {
            const int row = idx / (R / 2), k = idx - row * (R / 2);
            const int tA = row / nSym, tB = row - tA * nSym;
            const uint32_t wa = gw[tA * rowWords + k], wb = gw[tB * rowWords + k];
            pw[row * (SLOTS * 4) + 2 * k] = __builtin_amdgcn_perm(wb, wa, 0x05040100u);
            pw[row * (SLOTS * 4) + 2 * k + 1] = __builtin_amdgcn_perm(wb, wa, 0x07060302u);
        }
    }
    __syncthreads();

    // Hand-out of groups (sorted longest first). First round: static and striped, so that
    // every CU, and every SIMD inside it (wavefronts w, w+4, w+8 share one), starts with
    // a mix of long and short groups: wavefront w takes tier kTier[w % 4][w / 4] of
    // gridDim.x groups each, in snake order across workgroups. Later rounds: whoever
    // finishes pulls the next group from a shared counter, so wavefronts finish together.
    const int wave = threadIdx.x >> 6;
    constexpr int kTier[4][3] = {{0, 6, 11}, {1, 7, 8}, {2, 5, 9}, {3, 4, 10}};
    const int tier = kTier[wave & 3][wave >> 2];
    const int firstDynamic = kPairWavesPerGroup * gridDim.x;
    bool firstRound = true;
    for (;;) {
        int g;
        if (firstRound) {
            g = tier * gridDim.x + ((tier & 1) ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x);
            firstRound = false;
            if (g >= a.nGroups) continue;
            g += a.groupBase;
        } else {
            g = 0;
            if (lane == 0) g = atomicAdd(a.workCounter, 1);
            g = __builtin_amdgcn_readfirstlane(g) + firstDynamic;
            if (g >= a.nGroups) break;
            g += a.groupBase;
        }
        const uint2* pack = a.pack + a.groupOff[g];
        const int nChunks = a.groupChunks[g];
        // a group much longer than a wavefront's balanced share is on the critical path:
        // let it win the SIMD's issue arbitration against its co-resident wavefronts
        if (nChunks > a.priorityChunks) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(0);
        uint32_t best = 0u, held = 0u;
        uint32_t H[R], E[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            H[r] = 0u;
            E[r] = 0u;
        }
        uint2 cur = pack[lane];
        for (int c = 0; c < nChunks; ++c) {
            uint2 nxt = {0, 0};
            if (c + 1 < nChunks) nxt = pack[(size_t)(c + 1) * kLanes + lane];
            uint32_t ra = cur.x, rb = cur.y;
#pragma unroll 1
            for (int cc = 0; cc < 4; ++cc) {
                const uint32_t tA = ra & 0xffu, tB = rb & 0xffu;
                ra >>= 8;
                rb >>= 8;
                const uint4* prow = pairs + (tA * nSym + tB) * SLOTS;
                uint32_t f = 0u;
                uint4 v[NB4];
                v[0] = prow[0];
                auto score = [&](int r) -> uint32_t {
                    const uint4 x = v[r >> 2];
                    const int k = r & 3;
                    return k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w;
                };
                uint32_t dsum = ar.addScore(0u, score(0));
#pragma unroll
                for (int r4 = 0; r4 < NB4; ++r4) {
                    if (r4 + 1 < NB4) v[r4 + 1] = prow[r4 + 1];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int r = r4 * 4 + k;
                        uint32_t dnext = 0;
                        if (r + 1 < R) dnext = ar.addScore(H[r], score(r + 1));
                        const uint32_t h = ar.hmax(dsum, E[r], f);
                        ar.track(best, held, h, r);
                        const uint32_t hmo = ar.cellOpen(h);
                        E[r] = ar.gap(E[r], hmo);
                        f = ar.gap(f, hmo);
                        H[r] = h;
                        dsum = dnext;
                    }
                    if (r4 & 1) asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
                }
            }
            cur = nxt;
        }
        const int lo = Arith::toInt(best & 0xffffu), hi = Arith::toInt(best >> 16);
        const size_t base = (size_t)g * kGroupTargets;
        a.score[base + lane] = lo;
        a.score[base + kLanes + lane] = hi;
        if (a.overflow) {
            a.overflow[base + lane] = lo >= Arith::kLimit;
            a.overflow[base + kLanes + lane] = hi >= Arith::kLimit;
        }
    }
}

template <int R, typename Arith>
static hipError_t launchPairR(const InterseqArgs& a, int computeUnits, hipStream_t stream) {
    const size_t lds = PairLayout<R>::bytes(a.nSymbols);
    if (const hipError_t e = allowFullLds<&interseq_pair_kernel<R, Arith>>(); e != hipSuccess) return e;
    // (every CU takes part even when the groups are fewer than its wavefronts: the first round hands
    // out group g to wavefront tier g / blocks of workgroup g % blocks, and a wavefront alone on its
    // SIMD sweeps its group three times faster than one of three)
    const int blocks = std::max(1, std::min(computeUnits, a.nGroups));
    hipLaunchKernelGGL((interseq_pair_kernel<R, Arith>), dim3(blocks), dim3(kPairWavesPerGroup * kLanes), lds, stream, a);
    return hipGetLastError();
}

// Smith-Waterman, one strip, pair-indexed profile. Returns hipErrorInvalidValue when
// the table does not fit LDS (the caller then uses the v_perm variant).
template <typename Arith>
hipError_t launchPairFlavour(const InterseqArgs& a, int rowsPerStrip, int computeUnits, hipStream_t stream) {
    if (a.nStrips != 1) return hipErrorInvalidValue;
    return dispatchRows<8, 8, 8>(rowsPerStrip, [&](auto r) { return launchPairR<r, Arith>(a, computeUnits, stream); });
}

}  // namespace miopal
