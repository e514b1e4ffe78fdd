// One-strip Smith-Waterman on the pair table, on biased integer halves (the representation: interseq_pair_parts.h),
// with end locations (LOC) or as the column split (SPLIT).
#pragma once
#include "interseq_packed_ops.h"
#include "interseq_pair_parts.h"

namespace miopal {

// Column split (SPLIT; scores only). The dynamic hand-out's unit is a whole group, so a launch of G groups on S
// SIMDs lasts ceil(G / S) group-times whatever G is. With SPLIT the chunk sequence of all the launch's groups is
// cut into W = gridDim.x * kPairWavesPerGroup equal intervals, one per resident wavefront: wavefront w owns the chunks
// [w C / W, (w + 1) C / W) of that sequence, and the host says where each interval begins (a.splitPlan: group, chunks
// into it, chunk number - no search on the device). A group cut by an interval's end is BEGUN by that wavefront (the
// producer, first thing it does) and FINISHED by the next one (the consumer, last thing it does); between the two
// the whole groups of the interval. At the cut the producer leaves H[R], E[R] and the running best - rebased to
// shift 0, so that no scalar state travels - in a.splitState (slot w + 1: [quad][lane] x 16 bytes, the sc1 buffer
// stores of StripRows) and publishes a.splitFlags[w + 1] (stripPublish / stripPoll, common.h) with the launch's
// epoch a.splitEpoch, which no flag of an earlier launch or plan can equal: the host zeroes the flags when it
// allocates them and when its counter wraps, never per launch. Only the wavefront that reaches the group's last chunk
// writes its scores. The host takes this mode when an interval is at least as long as the longest group (no group is
// cut twice, and a consumer arrives nearly a whole interval after its producer has left); forced on smaller launches
// (MIOPAL_COLUMN_SPLIT) an interval may lie inside one group, whose
// wavefront then consumes and produces. A consumer polls kSplitPolls times at most, then - or at once with
// a.splitMode == 2 - sweeps the group from column 0 itself: always correct, no launch can hang on a flag.
// The wavefronts of a SIMD are paced by what is left of their INTERVALS: equal shares that end together.
// (the state's quads: StripRows' accesses with the quad in the scalar offset - one lane offset for all of them, where
// a vector offset per quad is hoisted out of the group loop into as many registers)
struct SplitState {
    __amdgpu_buffer_rsrc_t rsrc;
    __device__ __forceinline__ explicit SplitState(void* base)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7ffffff0, 0x00020000)) {}
    // (the offset made where it is used: as a constant it would be hoisted out of the group loop too, into a scalar
    // register per quad)
    static __device__ __forceinline__ int at(int quad) {
        int offset = quad * (kLanes * 16);
        asm volatile("" : "+s"(offset));
        return offset;
    }
    __device__ __forceinline__ StripU4 load(int quad, int lane) const {
        return __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16, at(quad), 16 /* sc1 */);
    }
    __device__ __forceinline__ void store(int quad, int lane, StripU4 v) const {
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, lane * 16, at(quad), 16 /* sc1 */);
    }
};
constexpr int kSplitPolls = 256;

template <int R, bool LOC, bool SPLIT = false>
__global__ __launch_bounds__(kPairWavesPerGroup * kLanes) void interseq_pair_biased_kernel(InterseqArgs a) {
    static_assert(!(SPLIT && LOC), "the column split carries no end locations");
    constexpr int SLOTS = PairLayout<R>::kRowSlots;
    constexpr int NB4 = (R + 3) / 4;   // R need not be a multiple of 4: the last read is partly used
    constexpr int kBits = LOC ? locRowBits(R) : 0;
    constexpr int kRowMask = (1 << kBits) - 1;
    extern __shared__ uint4 pairs[];
#if MIOPAL_HEADLINE_TIMING
    const unsigned long long born = __builtin_amdgcn_s_memrealtime();
#endif

    const int lane = threadIdx.x & 63;
    const int nSym = a.nSymbols;
    const int ext = a.gapExt << kBits;   // pattern units
    const uint32_t ext2 = both(ext), openMinusExt2 = both((a.gapOpen << kBits) - ext);
    const uint32_t zero2 = both(LOC ? kLocZeroPattern : kBiasedZero);

    // build the table: one thread per (pair row, query row); profile = true scores as int16
    if constexpr (SPLIT) {
        // The split form's prologue: the profile comes into LDS with one coalesced load per thread (it may lie in the
        // host's pinned staging buffer: read once, no copy in front of the launch), then wavefront w builds the pair
        // rows w, w + 12, ... with lane = query row - two LDS reads and one LDS write per entry, (tA, tB) stepped
        // along, no division. Same table bytes as the loop below.
        uint32_t* pw = reinterpret_cast<uint32_t*>(pairs);
        uint32_t* lw = pw + nSym * nSym * (SLOTS * 4) + kPairTailInts;
        const uint32_t* gw = reinterpret_cast<const uint32_t*>(a.profile);
        const int words = nSym * a.qPad / 2;
#pragma unroll 1
        for (int idx = threadIdx.x; idx < words; idx += kPairWavesPerGroup * kLanes) lw[idx] = gw[idx];
        __syncthreads();
        const int16_t* lp = reinterpret_cast<const int16_t*>(lw);
        const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        // (four pair rows at a time: their eight reads are in flight together - one row at a time the loop is a chain of
        // LDS round trips)
        constexpr int kAtOnce = 4;
        const int nRows = nSym * nSym;
        int tA = 0, tB = w;
        for (int row = w; row < nRows; row += kPairWavesPerGroup * kAtOnce) {
            int vA[kAtOnce], vB[kAtOnce];
#pragma unroll
            for (int k = 0; k < kAtOnce; ++k) {
                for (; tB >= nSym; tB -= nSym) ++tA;
                // (rows behind the table's end and lanes behind the query's rows: entry 0, not used)
                const bool on = lane < R && row + k * kPairWavesPerGroup < nRows;
                vA[k] = lp[on ? tA * a.qPad + lane : 0];
                vB[k] = lp[on ? tB * a.qPad + lane : 0];
                tB += kPairWavesPerGroup;
            }
#pragma unroll
            for (int k = 0; k < kAtOnce; ++k) {
                // (scores only: no row bits, and the padding score is its own pattern)
                const int sA = vA[k] + ext, sB = vB[k] + ext;
                if (lane < R && row + k * kPairWavesPerGroup < nRows)
                    pw[(row + k * kPairWavesPerGroup) * (SLOTS * 4) + lane] = (uint32_t)(sB * 65536 + sA);
            }
        }
    } else {
        const int16_t* gp = a.profile;
        constexpr int kBuildThreads = kPairWavesPerGroup * kLanes;
        // (padding symbol / padding rows: as far below the column's zero as the guard band allows)
        constexpr int kPadPattern = LOC ? -kLocGuardBand : kBiasedPad;
#define MIOPAL_PAIR_ENTRY MIOPAL_SW_PAIR_ENTRY
#include "interseq_pair_table_build.inc"
#undef MIOPAL_PAIR_ENTRY
    }
    // groups handed to the wavefronts of each SIMD (end game: nextGroup, interseq_pair_parts.h): 16 bytes behind the table
    int* simdTaken = reinterpret_cast<int*>(pairs + nSym * nSym * SLOTS);
    if (threadIdx.x < 4) simdTaken[threadIdx.x] = 0;
    __syncthreads();
#if MIOPAL_HEADLINE_TIMING
    // (the table stands: the latest workgroup, and the sum over the workgroups for their mean)
    if (a.stripTiming && threadIdx.x == 0) {
        const unsigned long long built = __builtin_amdgcn_s_memrealtime();
        atomicMax(a.stripTiming + 1 + 4 * gridDim.x, built);
        atomicAdd(a.stripTiming + 2 + 4 * gridDim.x, built);
    }
#endif
    // (the wavefronts of a SIMD paced by what is left of their groups: MIOPAL_HEADLINE_PACE, interseq_pair_parts.h)
    SimdPace pace;
    if (MIOPAL_HEADLINE_PACE) pace.init(simdTaken + 4, lane);

    constexpr int kHandoutWaves = kPairWavesPerGroup;
#define MIOPAL_PAIR_HANDOUT_PART 1
#include "interseq_pair_handout.inc"
    // SPLIT: this wavefront's interval [lo, hi) of the launch's chunks, the groups gLo / gHi that hold its two ends
    // and how far into them the ends lie (0: not cut); phase 0 = the piece that begins gHi, 1 = the whole groups,
    // 2 = the piece that finishes gLo
    int splitW = 0, gLo = 0, gHi = 0, cutLo = 0, cutHi = 0, gWhole = 0, phase = 0, paceAfter = 0;
    if constexpr (SPLIT) {
        // the host's plan (host_search.inc, splitPlanOf; made once per view and launch width, for the forced test
        // plans too): the two boundaries of the interval, {group, chunks into it, chunk number}
        splitW = kPairWavesPerGroup * (int)blockIdx.x + wave;
        const int4 from = a.splitPlan[splitW], to = a.splitPlan[splitW + 1];
        // (wave-uniform, and said so: what a vector load returns would keep all that follows in VGPRs)
        gLo = __builtin_amdgcn_readfirstlane(from.x);
        gHi = __builtin_amdgcn_readfirstlane(to.x);
        cutLo = __builtin_amdgcn_readfirstlane(from.y);
        cutHi = __builtin_amdgcn_readfirstlane(to.y);
        gWhole = cutLo > 0 ? gLo + 1 : gLo;
        paceAfter = __builtin_amdgcn_readfirstlane(to.z - from.z);
        if (paceAfter == 0) phase = 3;
    }
    for (;;) {
        int g;
        int cBegin = 0, cEnd = 0;               // SPLIT: the piece's chunks of group g (cEnd = 0: to the group's end)
        bool consume = false, produce = false;  // SPLIT: the piece starts from / leaves the state of a cut
        if constexpr (SPLIT) {
            if (phase == 0) {
                phase = 1;
                if (gLo == gHi) {               // the interval lies inside one group (forced launches only)
                    phase = 3;
                    g = gLo;
                    cBegin = cutLo;
                    cEnd = cutHi;
                    consume = cutLo > 0;
                    produce = true;
                } else if (cutHi > 0) {
                    g = gHi;
                    cEnd = cutHi;
                    produce = true;
                } else {
                    continue;
                }
            } else if (phase == 1) {
                if (gWhole < gHi) {
                    g = gWhole++;
                } else {
                    phase = 2;
                    continue;
                }
            } else if (phase == 2) {
                phase = 3;
                if (cutLo == 0) break;
                g = gLo;
                cBegin = cutLo;
                consume = true;
            } else {
                break;
            }
            g += a.groupBase;
        } else
#define MIOPAL_PAIR_HANDOUT_PART 2
#include "interseq_pair_handout.inc"
        const uint2* pack = a.pack + a.groupOff[g];
        const int nChunks = a.groupChunks[g];
        groupPriority(nChunks, a.priorityChunks);
        uint32_t best = 0u;                 // true values (LOC: keys), integer order
        int colA = -1, colB = -1;           // LOC: column of the first maximum of each half
        uint32_t fl = zero2 - ext2;         // zero of column -1
        int shift = -ext;                   // fl = zero2 + both(shift); wave-uniform
        uint32_t H[R], E[R];
        if constexpr (SPLIT) {
            if (cEnd == 0) cEnd = nChunks;
            paceAfter -= cEnd - cBegin;     // (a piece swept again from column 0 counts as what it was)
            if (consume) {
                bool there = false;
                if (a.splitMode != 2) {
                    for (int poll = 0; poll < kSplitPolls && !there; ++poll) {
                        there = stripPoll(a.splitFlags + splitW) == (int)a.splitEpoch;   // (a flag of an earlier launch never is)
                        if (!there) __builtin_amdgcn_s_sleep(16);
                    }
                }
                if (!there) {
                    consume = false;
                    cBegin = 0;
                }
            }
        }
        if (SPLIT && consume) {
            // the producer's state at shift 0: H on the last column's scale, E on the next one's, fl = zero2
            fl = zero2;
            shift = 0;
            const SplitState mine(a.splitState + (size_t)splitW * splitStateQuads(R) * kLanes);
            // (seven loads in flight at a time: each lands in four registers of its own before it moves into H / E)
#pragma unroll
            for (int q = 0; q < splitStateQuads(R); ++q) {
                if (q % 7 == 0 && q > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const StripU4 v = mine.load(q, lane);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = 4 * q + k;
                    const uint32_t x = k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
                    if (i < R) H[i] = x;
                    else if (i < 2 * R) E[i - R] = x;
                    else if (i == 2 * R) best = x;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                H[r] = fl;                      // H[r][-1] = 0 on column -1's scale
                E[r] = zero2;                   // E[r][0]  = 0 on column 0's scale
            }
        }
        const int cFirst = SPLIT ? cBegin : 0, cLast = SPLIT ? cEnd : nChunks;
        uint2 cur = pack[(size_t)cFirst * kLanes + lane];
        // (through a closure: see pairRowOf)
        auto rowOf = [&](uint32_t tA, uint32_t tB) -> const uint4* { return pairRowOf<SLOTS>(pairs, nSym, tA, tB); };
        // (blocks of table rows fetched ahead, across the column's end: MIOPAL_PAIR_AHEAD / MIOPAL_PAIR_XCOL,
        // interseq_pair_parts.h; 64 rows leave registers for two)
        constexpr int kWant = LOC ? (R > 62 ? 1 : R > 58 ? 2 : MIOPAL_PAIR_AHEAD) : (R > 60 ? 2 : MIOPAL_PAIR_AHEAD);
        constexpr int kAhead = NB4 > kWant ? kWant : 1;
        constexpr bool kAcross = MIOPAL_PAIR_XCOL != 0;
        const uint4* prowNext = rowOf(cur.x & 0xffu, cur.y & 0xffu);
        uint4 vn[kAhead];
        if (kAcross) {
#pragma unroll
            for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
        }
        for (int c = cFirst; c < cLast; ++c) {
            uint2 nxt = {0, 0};
            if (c + 1 < nChunks) nxt = pack[(size_t)(c + 1) * kLanes + lane];
            // (SPLIT: by what is left of the interval)
            if (MIOPAL_HEADLINE_PACE) pace.step(c - cLast - (SPLIT ? paceAfter : 0), lane, nChunks > a.priorityChunks);
            uint32_t ra = cur.x, rb = cur.y;
#pragma unroll 1
            for (int cc = 0; cc < 4; ++cc) {
                const uint4* prow = prowNext;
                uint4 v[NB4];
#pragma unroll
                for (int k = 0; k < kAhead; ++k) v[k] = kAcross ? vn[k] : prow[k];
                // the column after this one (past the group's end: row 0, never used)
                ra = cc < 3 ? ra >> 8 : nxt.x;
                rb = cc < 3 ? rb >> 8 : nxt.y;
                prowNext = rowOf(ra & 0xffu, rb & 0xffu);
                auto score = [&](int r) -> uint32_t {
                    const uint4 x = v[r >> 2];
                    const int k = r & 3;
                    return k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w;
                };
                uint32_t dsum = fl + score(0);      // H[-1][j-1] = 0 on the previous column's scale
                fl += ext2;                         // this column's zero
                uint32_t fl1 = fl + ext2;           // the next column's
                // (wave-uniform, so hipcc would keep it in an SGPR: v_pk_maximum3_f16 with a scalar
                // operand issues ~10 % slower, profiles/r01_valu_issue_rates.txt)
                asm volatile("" : "+v"(fl1));
                uint32_t f = fl, cm = fl, held = fl;
#pragma unroll
                for (int r4 = 0; r4 < NB4; ++r4) {
                    if (r4 + kAhead < NB4) v[r4 + kAhead] = prow[r4 + kAhead];
                    if (kAcross && r4 == (NB4 > 3 ? NB4 - 3 : 0)) {
#pragma unroll
                        for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int r = r4 * 4 + k;
                        if (r >= R) continue;
                        uint32_t dnext = 0;
                        if (r + 1 < R) dnext = H[r] + score(r + 1);
                        const uint32_t h = pk_max3_f16(dsum, E[r], f);
                        // what the column maximum folds: h, or h with the row in its free low bits
                        const uint32_t hk = LOC ? h + both(kRowMask - r) : h;
                        if (r & 1) cm = pk_max3_f16(cm, held, hk);
                        else held = hk;
                        const uint32_t hmo = h - openMinusExt2;
                        E[r] = pk_max3_f16(E[r], hmo, fl1);
                        if (r + 1 < R) f = pk_max3_f16(f, hmo, fl1) - ext2;
                        H[r] = h;
                        dsum = dnext;
                    }
                    // pins the schedule: hipcc would otherwise hoist every ds_read to the column's top
                    asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
                }
                if (R & 1) cm = pk_max3_f16(cm, held, held);
                if constexpr (LOC) {
                    // strictly greater scores only: compare against best with its row bits all set
                    const uint32_t cand = cm - fl, thr = best | both(kRowMask);
                    const uint32_t ch = pk_max_u16(thr, cand) ^ thr;   // nonzero half: new maximum
                    const int j = c * 4 + cc;
                    if (ch & 0xffffu) {
                        best = (best & 0xffff0000u) | (cand & 0xffffu);
                        colA = j;
                    }
                    if (ch >> 16) {
                        best = (best & 0xffffu) | (cand & 0xffff0000u);
                        colB = j;
                    }
                } else {
                    best = pk_max_u16(best, cm - fl);
                }
            }
            cur = nxt;
            shift += 4 * ext;
            if (shift + 4 * ext > kBiasedMaxShift) {
                // rebase: H is on the last column's scale, E on the next one's, both relative to fl
                const uint32_t d = both(shift);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    H[r] -= d;
                    E[r] -= d;
                }
                fl -= d;
                shift = 0;
            }
        }
        if constexpr (SPLIT) {
            if (produce) {
                // the cut: the state leaves at shift 0 (the rebase above, whatever the shift has come to)
                const uint32_t d = both(shift);
                const SplitState next(a.splitState + (size_t)(splitW + 1) * splitStateQuads(R) * kLanes);
#pragma unroll
                for (int q = 0; q < splitStateQuads(R); ++q) {
                    auto word = [&](int i) -> uint32_t {
                        if (i < R) return H[i] - d;
                        if (i < 2 * R) return E[i - R] - d;
                        return i == 2 * R ? best : 0u;
                    };
                    next.store(q, lane, StripU4{word(4 * q), word(4 * q + 1), word(4 * q + 2), word(4 * q + 3)});
                }
                stripPublish(a.splitFlags + splitW + 1, (int)a.splitEpoch, lane);
                continue;                   // (the consumer writes the group's scores)
            }
        }
        const int lo = (int)(best & 0xffffu) >> kBits, hi = (int)(best >> 16) >> kBits;
        const size_t base = (size_t)g * kGroupTargets;
        if (a.directOut) {
            // database order at once (the host has made sure that no lane can leave its range and that
            // nothing else writes these results): no view-order array, no scatter kernel
            const int posA = (int)base + lane, posB = posA + kLanes;
            if (posA < a.directN) {
                const int id = a.directIds[posA];
                a.directOut[id] = lo;
                if constexpr (LOC) {
                    a.directEndI[id] = colA < 0 ? -1 : kRowMask - (int)(best & kRowMask);
                    a.directEndJ[id] = colA;
                }
            }
            if (posB < a.directN) {
                const int id = a.directIds[posB];
                a.directOut[id] = hi;
                if constexpr (LOC) {
                    a.directEndI[id] = colB < 0 ? -1 : kRowMask - (int)((best >> 16) & kRowMask);
                    a.directEndJ[id] = colB;
                }
            }
            continue;
        }
        a.score[base + lane] = lo;
        a.score[base + kLanes + lane] = hi;
        if constexpr (LOC) {
            a.endI[base + lane] = colA < 0 ? -1 : kRowMask - (int)(best & kRowMask);
            a.endI[base + kLanes + lane] = colB < 0 ? -1 : kRowMask - (int)((best >> 16) & kRowMask);
            a.endJ[base + lane] = colA;
            a.endJ[base + kLanes + lane] = colB;
        }
        if (a.overflow) {
            // (at most locLimit(kBits) / kBiasedScoreLimit; lower when single steps are large, host.hip)
            a.overflow[base + lane] = lo >= a.biasedLimit;
            a.overflow[base + kLanes + lane] = hi >= a.biasedLimit;
        }
    }
    if (MIOPAL_HEADLINE_PACE && lane == 0) *pace.mine = INT32_MAX;   // (done: nobody waits for this one)
#if MIOPAL_HEADLINE_TIMING
    if (a.stripTiming && lane == 0) {
        atomicMin(a.stripTiming, born);
        atomicMax(a.stripTiming + 1 + blockIdx.x * 4 + simd, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
#endif
}

template <int R, bool LOC>
static hipError_t launchPairBiasedR(const InterseqArgs& a, int computeUnits, hipStream_t stream) {
    const size_t lds = PairLayout<R>::bytes(a.nSymbols) + 16 + kPaceInts * sizeof(int);  // table + per-SIMD counters (+ pacing)
    if (const hipError_t e = allowFullLds<&interseq_pair_biased_kernel<R, LOC>>(); e != hipSuccess) return e;
    // (every CU takes part even when the groups are fewer than its wavefronts: the first round hands
    // out group g to wavefront tier g / blocks of workgroup g % blocks, and a wavefront alone on its
    // SIMD sweeps its group three times faster than one of three)
    const int blocks = std::max(1, std::min(computeUnits, a.nGroups));
    hipLaunchKernelGGL((interseq_pair_biased_kernel<R, LOC>), dim3(blocks), dim3(kPairWavesPerGroup * kLanes), lds, stream, a);
    return hipGetLastError();
}

// the column-split form (a.splitMode != 0; scores only): a.splitBlocks workgroups, whose wavefronts the host's plan
// (flags, state slots, the interval's length) was made for
template <int R>
static hipError_t launchPairBiasedSplitR(const InterseqArgs& a, hipStream_t stream) {
    // (table + per-SIMD counters + pacing as above, and the profile the table is built from)
    const size_t lds = pairSplitLdsBytes(R, a.nSymbols, a.qPad);
    if (lds > kCuLdsBytes || a.qPad < R || (a.qPad & 7)) return hipErrorInvalidValue;
    if (const hipError_t e = allowFullLds<&interseq_pair_biased_kernel<R, false, true>>(); e != hipSuccess) return e;
    if (a.splitBlocks < 1 || !a.splitState || !a.splitFlags || !a.splitPlan || a.splitEpoch == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((interseq_pair_biased_kernel<R, false, true>), dim3(a.splitBlocks), dim3(kPairWavesPerGroup * kLanes), lds, stream, a);
    return hipGetLastError();
}

template <int kLo, bool LOC>
hipError_t launchPairBiased(const InterseqArgs& a, int rowsPerStrip, int computeUnits, hipStream_t stream) {
    if (a.nStrips != 1) return hipErrorInvalidValue;
    // rows: kLo, kLo + 2, ..., kLo + 14; the translation units interseq_swb16_{a,b,c,d}[_loc].hip share the
    // even counts 2..64, interseq_swb16_{a,b,c,d}[_loc]_odd.hip the odd ones 1..63
    if constexpr (!LOC) {
        if (a.splitMode != 0)
            return dispatchRows<kLo, 2, kPairUnitCounts>(rowsPerStrip, [&](auto r) { return launchPairBiasedSplitR<r>(a, stream); });
    }
    return dispatchRows<kLo, 2, kPairUnitCounts>(rowsPerStrip, [&](auto r) { return launchPairBiasedR<r, LOC>(a, computeUnits, stream); });
}

}  // namespace miopal
