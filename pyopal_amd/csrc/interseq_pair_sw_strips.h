#pragma once
#include "interseq_packed_ops.h"
#include "interseq_pair_parts.h"

namespace miopal {

// ---- Smith-Waterman scores of SEVERAL strips on the pair table (round 2) -----------
// The biased-halves kernel of interseq_pair_sw.h for queries of more than one strip. A pair table holds one strip
// of the query and fills the CU's LDS, so all twelve wavefronts of a workgroup work on the same
// strip: a workgroup takes units (batch of 12 groups, strip) from a counter, strip-major, rebuilds
// the table when the strip changes (150 KB of LDS writes, a few microseconds) and each wavefront
// sweeps its group through that strip. The last row of a strip reaches the strip below through HBM: per column and
// lane the pair (H, F) as patterns on that column's scale - both strips rebase their column shift at
// the same chunks, so a pattern means the same in either - 512 bytes per column and wavefront,
// written once and read once. The wavefront of (group, s) follows the wavefront of (group, s - 1) -
// which may still be running in another workgroup when the batches are few - two chunks behind: the producer publishes the
// number of finished chunks (release), the consumer acquires it before it fetches rows it has not
// seen published. Every taken unit's producer was taken before it and strip 0 waits for nobody, so
// the chain always moves; a consumer that nevertheless waits longer than about a second poisons its
// own progress counter and flags its lanes, and the next rung recomputes them.
// A group's maximum is the maximum over its strips: atomicMax into the (zeroed) view scores.

// KNOWN (round 3, second pass of an `end` search whose scores are beyond the row keys' range): the optimum
// of every lane half is known (a.known, view order, from the scores-only pass of this very kernel); the
// sweep is the same, but instead of a running maximum every column's maximum is compared with the optimum,
// and the first time they are equal - once per lane half and strip at most - a scan of the column's rows
// finds the first row that holds it. The (score, column, row) keys are the ones of LOC.
template <int R, bool LOC, bool KNOWN = false>
__global__ __launch_bounds__(kPairWavesPerGroup * kLanes) void interseq_pair_strips_kernel(InterseqArgs a) {
    static_assert(!(LOC && KNOWN), "row keys or a known optimum");
    constexpr int SLOTS = PairLayout<R>::kRowSlots;
    constexpr int NB4 = (R + 3) / 4;
    // end locations (LOC): values scaled by 2^kBits, the row inside the strip in the low bits of what
    // the column maximum folds - the one-strip kernel's scheme, per strip
    constexpr int kBits = LOC ? locRowBits(R) : 0;
    constexpr int kRowMask = (1 << kBits) - 1;
    extern __shared__ uint4 pairs[];

    const int lane = threadIdx.x & 63;
    const int nSym = a.nSymbols;
    const int ext = a.gapExt << kBits;   // pattern units
    const uint32_t ext2 = both(ext), openMinusExt2 = both((a.gapOpen << kBits) - ext);
    const uint32_t zero2 = both(LOC ? kLocZeroPattern : kBiasedZero);
    constexpr int kPadPattern = LOC ? -kLocGuardBand : kBiasedPad;   // (padding symbol / padding rows)
    // units, table rebuild and the hand-over between strips: interseq_strip_frame.inc, with the watch on a.stripAbort
#define MIOPAL_STRIP_FRAME_ABORTS 1
#define MIOPAL_STRIP_FRAME_STATE
#define MIOPAL_PAIR_ENTRY MIOPAL_SW_PAIR_ENTRY
#define MIOPAL_STRIP_FRAME_PART 1
#include "interseq_strip_frame.inc"

    for (;;) {
#define MIOPAL_STRIP_FRAME_PART 2
#include "interseq_strip_frame.inc"

        uint32_t best = 0u;                 // true values (LOC: keys), integer order
        int colA = -1, colB = -1;           // LOC: column of the first maximum of each half in this strip
        // KNOWN: the optimum of both halves as one packed value; a half without a positive optimum, or whose
        // optimum is beyond the exact range (redone by the next rung), has nothing to find
        uint32_t target2 = 0u;
        bool foundA = true, foundB = true;
        if constexpr (KNOWN) {
            const size_t kbase = (size_t)g * kGroupTargets;
            const int kA = a.known[kbase + lane], kB = a.known[kbase + kLanes + lane];
            foundA = kA <= 0 || kA >= a.biasedLimit;
            foundB = kB <= 0 || kB >= a.biasedLimit;
            target2 = ((uint32_t)(foundB ? 0xffff : kB) << 16) | (uint32_t)(foundA ? 0xffff : kA);
        }
        // the sweep, compiled for the three kinds of strip (first / inner / last): no selects between
        // border and row above, no stores from the last strip
        auto sweep = [&](auto fromAboveC, auto toBelowC) {
            constexpr bool kFromAbove = decltype(fromAboveC)::value, kToBelow = decltype(toBelowC)::value;
            uint32_t fl = zero2 - ext2;         // zero of column -1
            int shift = -ext;                   // fl = zero2 + both(shift); wave-uniform
            uint32_t H[R], E[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                H[r] = fl;
                E[r] = zero2;
            }
            // row above: column j in hand, the next kRowsAhead columns on their way (the loads go to
            // memory, past the L2: a microsecond or two, a column takes about one)
            // (two columns per load: the pair in use and the next one on its way - it is asked for at the pair's
            // first column and first read two columns later)
            StripU4 pq0 = {fl, zero2, fl, zero2}, pq1 = pq0;
            uint32_t keepH = 0, keepF = 0;      // the even column's {H, F} waiting for its neighbour's
            uint32_t hbPrev = fl;               // H of the row above at column j - 1 (left border: 0)
            if constexpr (kFromAbove) pq0 = rowsIn.load(0, lane);
            uint2 cur = pack[lane];
            // (through a closure: see pairRowOf)
            auto rowOf = [&](uint32_t tA, uint32_t tB) -> const uint4* { return pairRowOf<SLOTS>(pairs, nSym, tA, tB); };
            // (the second pass of an `end` search has a row scan inside the column loop: it gives the
            // registers of two prefetched blocks of pair-table rows for it)
            // (round 4: the boundary rows in 16-byte pairs cost four registers: tall strips give a prefetched block for them)
            constexpr int kWant = KNOWN ? 1 : R > (LOC ? 38 : 44) ? 2 : MIOPAL_PAIR_AHEAD;
            constexpr int kAhead = NB4 > kWant ? kWant : 1;
            const uint4* prowNext = rowOf(cur.x & 0xffu, cur.y & 0xffu);
            uint4 vn[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
            for (int c = 0; c < nChunks && !dead; ++c) {
                uint2 nxt = {0, 0};
                if (c + 1 < nChunks) nxt = pack[(size_t)(c + 1) * kLanes + lane];
                pace.step(c, lane, longGroup);
                if constexpr (kFromAbove) {
                    waitFor(min(c + kLag, nChunks));
                    // (a unit that has given up computes nothing more: what it would publish from rows that
                    // never arrived could be taken for real by a strip below that needs no further poll)
                    if (dead) break;
                }
                uint32_t ra = cur.x, rb = cur.y;
                // (the two columns of a pair as two copies of the body: which half of the pair a column reads and
                // whether it stores are compile-time then - as run-time selects they cost the kernel 24 registers)
                auto column = [&](auto oddC, int cc) {
                    constexpr bool odd = decltype(oddC)::value;
                    const int j = c * 4 + cc;
                    const uint4* prow = prowNext;
                    uint4 v[NB4];
#pragma unroll
                    for (int k = 0; k < kAhead; ++k) v[k] = vn[k];
                    if constexpr (kFromAbove && !odd) pq1 = rowsIn.load(min(j / 2 + 1, lastCol / 2), lane);
                    const uint32_t hAbove = odd ? pq0.z : pq0.x, fAbove = odd ? pq0.w : pq0.y;
                    ra = cc < 3 ? ra >> 8 : nxt.x;
                    rb = cc < 3 ? rb >> 8 : nxt.y;
                    prowNext = rowOf(ra & 0xffu, rb & 0xffu);
                    auto score = [&](int r) -> uint32_t {
                        const uint4 x = v[r >> 2];
                        const int k = r & 3;
                        return k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w;
                    };
                    // the row above at column j - 1, one column to the right; strip 0: the border's 0
                    uint32_t dsum = (kFromAbove ? hbPrev : fl) + score(0);
                    fl += ext2;                         // this column's zero
                    uint32_t fl1 = fl + ext2;           // the next column's
                    asm volatile("" : "+v"(fl1));
                    uint32_t f = kFromAbove ? fAbove : fl, cm = fl, held = fl;
#pragma unroll
                    for (int r4 = 0; r4 < NB4; ++r4) {
                        if (r4 + kAhead < NB4) v[r4 + kAhead] = prow[r4 + kAhead];
                        if (r4 == (NB4 > 3 ? NB4 - 3 : 0)) {
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
                            const uint32_t hk = LOC ? h + both(kRowMask - r) : h;
                            if (r & 1) cm = pk_max3_f16(cm, held, hk);
                            else held = hk;
                            const uint32_t hmo = h - openMinusExt2;
                            E[r] = pk_max3_f16(E[r], hmo, fl1);
                            f = pk_max3_f16(f, hmo, fl1) - ext2;   // (after the last row: what the strip below starts from)
                            H[r] = h;
                            dsum = dnext;
                        }
                        asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
                    }
                    if (R & 1) cm = pk_max3_f16(cm, held, held);
                    if constexpr (LOC) {
                        // strictly greater scores only: compare against best with its row bits all set
                        const uint32_t cand = cm - fl, thr = best | both(kRowMask);
                        const uint32_t ch = pk_max_u16(thr, cand) ^ thr;   // nonzero half: new maximum
                        if (ch & 0xffffu) {
                            best = (best & 0xffff0000u) | (cand & 0xffffu);
                            colA = j;
                        }
                        if (ch >> 16) {
                            best = (best & 0xffffu) | (cand & 0xffff0000u);
                            colB = j;
                        }
                    } else if constexpr (KNOWN) {
                        const uint32_t x = (cm - fl) ^ target2;
                        const bool hitA = !foundA && (x & 0xffffu) == 0, hitB = !foundB && (x >> 16) == 0;
                        if (__builtin_amdgcn_ballot_w64(hitA || hitB) != 0) {
                            // the first row of this column that holds the optimum of its half
                            int ia = 0, ib = 0;
#pragma unroll
                            for (int r = R - 1; r >= 0; --r) {
                                const uint32_t d = (H[r] - fl) ^ target2;
                                if ((d & 0xffffu) == 0) ia = r;
                                if ((d >> 16) == 0) ib = r;
                                asm volatile("" : "+v"(ia), "+v"(ib));
                            }
                            // (only remembered here: the keys leave after the sweep, when the DP state is dead -
                            // anything more inside the column loop costs registers the loop does not have)
                            if (hitA) {
                                colA = (j << 6) | ia;
                                foundA = true;
                            }
                            if (hitB) {
                                colB = (j << 6) | ib;
                                foundB = true;
                            }
                        }
                    } else {
                        best = pk_max_u16(best, cm - fl);
                    }
                    // (compiled per kind of strip: a run-time branch here costs 27 registers)
                    if constexpr (kToBelow) {
                        if constexpr (odd) {
                            rowsOut.store(j / 2, lane, StripU4{keepH, keepF, H[R - 1], f});
                        } else {
                            keepH = H[R - 1];
                            keepF = f;
                        }
                    }
                    hbPrev = hAbove;
                    if constexpr (odd) pq0 = pq1;
                };
#pragma unroll 1
                for (int cp = 0; cp < 4; cp += 2) {
                    column(std::false_type{}, cp);
                    column(std::true_type{}, cp + 1);
                }
                cur = nxt;
                shift += 4 * ext;
                if (shift + 4 * ext > kBiasedMaxShift) {
                    // rebase (the strip above did the same after this chunk: the rows it wrote from
                    // the next chunk on are already on the new scale, the one kept in hbPrev is not)
                    const uint32_t d = both(shift);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        H[r] -= d;
                        E[r] -= d;
                    }
                    hbPrev -= d;
                    fl -= d;
                    shift = 0;
                }
                if (kToBelow) stripPublishStep(progOut, c, nChunks, lane, timer);
            }
        };
#define MIOPAL_STRIP_FRAME_PART 3
#include "interseq_strip_frame.inc"
        const size_t base = (size_t)g * kGroupTargets;
#define MIOPAL_STRIP_FRAME_PART 4
#include "interseq_strip_frame.inc"
        if constexpr (KNOWN) {
            // (score, column, row) of the first cell of this strip that holds the optimum; scores and flags are
            // the first pass's
            auto key = [&](uint32_t score, int where) -> unsigned long long {
                return ((unsigned long long)score << 40) | ((unsigned long long)(0xFFFFFu - (unsigned)(where >> 6)) << 20) |
                       (unsigned long long)(0xFFFFFu - (unsigned)(s * R + (where & 63)));
            };
            if (colA >= 0) atomicMax(a.stripKeys + base + lane, key(target2 & 0xffffu, colA));
            if (colB >= 0) atomicMax(a.stripKeys + base + kLanes + lane, key(target2 >> 16, colB));
            continue;
        }
        const int lo = (int)(best & 0xffffu) >> kBits, hi = (int)(best >> 16) >> kBits;
        if constexpr (LOC) {
            // first maximum in column-major order over the strips: highest score, then smallest column,
            // then smallest row, as one 64-bit key (a strip without a positive cell contributes nothing)
            auto key = [&](int score, int col, uint32_t half) -> unsigned long long {
                const int row = s * R + (kRowMask - (int)(half & kRowMask));
                return ((unsigned long long)(unsigned)score << 40) | ((unsigned long long)(0xFFFFFu - (unsigned)col) << 20) |
                       (unsigned long long)(0xFFFFFu - (unsigned)row);
            };
            if (colA >= 0) atomicMax(a.stripKeys + base + lane, key(lo, colA, best));
            if (colB >= 0) atomicMax(a.stripKeys + base + kLanes + lane, key(hi, colB, best >> 16));
        } else {
            atomicMax(a.score + base + lane, lo);
            atomicMax(a.score + base + kLanes + lane, hi);
        }
        if (a.overflow) {
            // (first flags only are counted: a lane that left the range in this strip usually does in the next)
            const bool fa = lo >= a.biasedLimit && a.overflow[base + lane] == 0;
            const bool fb = hi >= a.biasedLimit && a.overflow[base + kLanes + lane] == 0;
            if (fa) a.overflow[base + lane] = 1;
            if (fb) a.overflow[base + kLanes + lane] = 1;
            if (a.stripAbort) {
                const int fresh = __popcll(__builtin_amdgcn_ballot_w64(fa)) + __popcll(__builtin_amdgcn_ballot_w64(fb));
                if (fresh > 0 && lane == 0) atomicAdd(a.stripAbort, fresh);
            }
        }
    }
    timer.flush(a.stripTiming, lane);
#undef MIOPAL_STRIP_FRAME_ABORTS
#undef MIOPAL_STRIP_FRAME_STATE
#undef MIOPAL_PAIR_ENTRY
}

template <int R, bool LOC, bool KNOWN = false>
static hipError_t launchPairStripsR(const InterseqArgs& a, int computeUnits, hipStream_t stream) {
    const size_t lds = PairLayout<R>::bytes(a.nSymbols) + 16 + kPaceInts * sizeof(int);  // table + the unit in flight + pacing
    if (const hipError_t e = allowFullLds<&interseq_pair_strips_kernel<R, LOC, KNOWN>>(); e != hipSuccess) return e;
    const int nBatches = (a.nGroups + a.batchGroups - 1) / a.batchGroups;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(computeUnits, (int64_t)nBatches * a.nStrips));
    hipLaunchKernelGGL((interseq_pair_strips_kernel<R, LOC, KNOWN>), dim3(blocks), dim3(kPairWavesPerGroup * kLanes), lds, stream, a);
    return hipGetLastError();
}

// (the tallest strips, kPairStripsMaxRows*: taller ones spill - the boundary rows cost 9 registers, the row scan of
// the known-optimum pass sits inside the column loop - and are not even instantiated)
template <int kLo, bool LOC, bool KNOWN>
hipError_t launchPairStrips(const InterseqArgs& a, int rowsPerStrip, int computeUnits, hipStream_t stream) {
    if (a.nStrips < 2 || !a.unitCounter || !a.unitFlags || !a.boundary[0] || !a.boundary[1] || a.batchGroups < 1 ||
        a.batchGroups > kPairWavesPerGroup || ((LOC || KNOWN) && !a.stripKeys) || (KNOWN && !a.known))
        return hipErrorInvalidValue;
    constexpr int kMax = KNOWN ? kPairStripsMaxRowsKnown : LOC ? kPairStripsMaxRowsLoc : kPairStripsMaxRows;
    return dispatchRows<kLo, 2, kPairUnitCounts, kMax>(
        rowsPerStrip, [&](auto r) { return launchPairStripsR<r, LOC, KNOWN>(a, computeUnits, stream); });
}

}  // namespace miopal
