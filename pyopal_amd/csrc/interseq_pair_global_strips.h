#pragma once
#include "interseq_packed_ops.h"
#include "interseq_pair_parts.h"

namespace miopal {

// H[row] for a wave-uniform, run-time `row` in [LO, HI]: a binary tree of scalar branches (the opaque
// move in the leaves keeps the compiler from turning the tree into HI - LO selects on hoisted predicates)
template <int LO, int HI, int N>
static __device__ __forceinline__ uint32_t pickRow(const uint32_t (&H)[N], int row) {
    if constexpr (LO >= HI) {
        uint32_t v = H[LO];
        asm volatile("" : "+v"(v));
        return v;
    } else {
        constexpr int MID = (LO + HI) / 2;
        if (row <= MID) return pickRow<LO, MID>(H, row);
        return pickRow<MID + 1, HI>(H, row);
    }
}

// ---- NW / HW / OV of SEVERAL strips on the pair table (round 3) ---------------------
// The one-strip kernel's cell (interseq_pair_global.h: 3 integer adds + 3 max per cell pair, no v_perm) in the unit
// scheme of interseq_pair_strips_kernel: a workgroup takes (batch of up to 12 groups, strip) units from a
// counter, strip-major, rebuilds its pair table when the strip changes, and the last row of a strip
// reaches the strip below through HBM as relaxed agent-scope atomics behind a progress counter
// (stripPublish / stripPoll, common.h). What the modes without a floor need on top:
//  * borders: the left border H[i][-1] of the strip's own rows as running sums, the top border only in
//    strip 0 (the other strips start from the row above), both as wave-uniform patterns;
//  * the scale: a half holds zero + x + sigma(j). With a free top border (HW, OV) x is bounded by the
//    QUERY (not the strip) and sigma is rebased at the same chunks in every strip, so a pattern means
//    the same on both sides of a boundary; with a penalised one (NW) x + j ext is bounded and sigma
//    just grows. The host checks the static range for the whole query (host.hip, globalStrips);
//  * answers: only the last strip holds the last query row (NW: its value at each lane's own last
//    column; HW / OV: maximum over the columns), and OV also takes the maximum over the rows of each
//    target's last column, strip by strip.
//    Scores only (LOC = false): the last strip stores the last-row answer (NW, HW) or every strip folds
//    its candidates into the view scores with atomicMax (OV; the host fills them with INT32_MIN).
//    With end locations (LOC = true) every candidate becomes a 64-bit key
//      (score + 2^31) << 32 | last-row candidate << 31 | 0x7FFFFFFF - (column | row)
//    merged with atomicMax: highest score; at equal scores the last row before the last column (the scan
//    order of oracle/opal_oracle.c), then the smallest column / row. decode_global_keys_kernel
//    (pack.hip) turns the keys into view-order scores and end locations. The row and column
//    bookkeeping costs registers: strips of at most 48 rows (52 without);
//  * nothing leaves its range, so nothing is flagged - except the lanes of a unit whose strip above
//    never arrived (time-out escape, as in the Smith-Waterman kernel): they are flagged for the int32
//    kernel and the strip below is told (poison).
template <int R, bool LOC>
__global__ __launch_bounds__(kPairWavesPerGroup * kLanes) void interseq_pair_global_strips_kernel(InterseqArgs a) {
    constexpr int SLOTS = PairLayout<R>::kRowSlots;
    constexpr int NB4 = (R + 3) / 4;
    extern __shared__ uint4 pairs[];

    const int lane = threadIdx.x & 63;
    const int nSym = a.nSymbols;
    const int ext = a.gapExt, open = a.gapOpen, Q = a.qLen;
    const int zero = a.biasedZero;
    const bool topGap = a.topGap, leftGap = a.leftGap;
    const int region = a.region;
    const uint32_t ext2 = both(ext), openMinusExt2 = both(open - ext);
    // units, table rebuild and the hand-over between strips: interseq_strip_frame.inc
#define MIOPAL_STRIP_FRAME_ABORTS 0
// (row of the last query residue inside the last strip)
#define MIOPAL_STRIP_FRAME_STATE const int rl = Q - 1 - (nStrips - 1) * R;
#define MIOPAL_PAIR_ENTRY MIOPAL_GLOBAL_PAIR_ENTRY
#define MIOPAL_STRIP_FRAME_PART 1
#include "interseq_strip_frame.inc"

    for (;;) {
#define MIOPAL_STRIP_FRAME_PART 2
#include "interseq_strip_frame.inc"

        const size_t base = (size_t)g * kGroupTargets;
        const int lenA = a.lens[base + lane], lenB = a.lens[base + kLanes + lane];
        // candidates (true values) of this unit: last query row (last strip), last column (OV, any strip);
        // their columns / rows only with LOC
        int runA = INT32_MIN, runB = INT32_MIN, colA = -1, colB = -1;
        int cbA = INT32_MIN, cbB = INT32_MIN, crowA = -1, crowB = -1;

        // the sweep, compiled for the three kinds of strip (first / inner / last)
        auto sweep = [&](auto fromAboveC, auto toBelowC) {
            constexpr bool kFromAbove = decltype(fromAboveC)::value, kToBelow = decltype(toBelowC)::value;
            int sigma = zero - ext;             // zero + sigma(j) of the last column done (column -1 here)
            int shift = -ext;                   // part of sigma accumulated since the last rebase
            uint32_t H[R], E[R];
            {
                // H[i][-1], i = s R + r: one gap of i + 1 residues or i + 1 one-residue gaps (borderGap), as
                // running sums in VECTOR registers (wave-uniform values: left to itself the compiler keeps
                // all 2 R of them in scalar registers first, and spills hundreds)
                const int i0 = s * R;
                int one = open + i0 * ext, many = (i0 + 1) * open;
                int rowShift = 0;                                      // r ext: the anti-diagonal part of the scale
                asm volatile("" : "+v"(one), "+v"(many), "+v"(rowShift));
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int left = (leftGap ? -min(one, many) : 0) + rowShift;
                    H[r] = both(zero - ext + left - (open - ext));    // stored form, on the scale of (r, -1)
                    E[r] = both(zero + left - open);                  // E[i][0], plain form on the scale of (r, 0)
                    one += ext;
                    many += open;
                    rowShift += ext;
                }
            }
            StripU4 pq0 = {0u, 0u, 0u, 0u}, pq1 = pq0;   // the pair of columns in use, the next one on its way
            uint32_t keepH = 0, keepF = 0;
            // H of the row above at column j - 1, on that column's scale: the left border of row s R - 1
            uint32_t hbPrev = 0u;
            if constexpr (kFromAbove) {
                // (stored form on the scale of (-1, -1): one row above the strip's row 0)
                hbPrev = both(zero - ext + (leftGap ? borderGap(s * R - 1, open, ext) : 0) - ext - (open - ext));
                pq0 = rowsIn.load(0, lane);
            }
            uint2 cur = pack[lane];
            // (through a closure: see pairRowOf)
            auto rowOf = [&](uint32_t tA, uint32_t tB) -> const uint4* { return pairRowOf<SLOTS>(pairs, nSym, tA, tB); };
            constexpr int kWant = R > 50 ? 1 : R > (LOC ? 38 : 44) ? 2 : MIOPAL_PAIR_AHEAD;
            constexpr int kAhead = NB4 > kWant ? kWant : 1;
            const uint4* prowNext = rowOf(cur.x & 0xffu, cur.y & 0xffu);
            uint4 vn[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
            // top border of the matrix (strip 0), as running values: H[-1][j - 1] and H[-1][j]
            int topPrev = 0, topHere = topGap ? borderGap(0, open, ext) : 0;
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
                // (the two columns of a pair as two copies of the body: see interseq_pair_strips_kernel)
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
                    uint32_t dsum, f;
                    if constexpr (kFromAbove) {
                        dsum = hbPrev + score(0);       // the row above at column j - 1, one column to the right
                        sigma += ext;
                        f = fAbove;                     // F entering the strip's first row, on this column's scale
                    } else {
                        // row above the matrix: H[-1][j-1] in stored form on the scale of (-1, j - 1), the F that
                        // H[-1][j] opens in plain form on the scale of (0, j)
                        dsum = both(sigma + topPrev - open) + score(0);
                        sigma += ext;
                        f = both(sigma + topHere - open);
                        asm volatile("" : "+v"(f));
                        topPrev = topHere;
                        if (topGap) topHere = borderGap(j + 1, open, ext);
                    }
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
                            // 2 integer adds + 1 max3 + 2 max: every cell (r, j) is on the scale zero + sigma(j) +
                            // r ext, so extending either gap costs nothing, both open with hmo = h - c, and hmo is
                            // at once the stored form of h that the next column's diagonal sum starts from
                            const uint32_t h = pk_max3_f16(dsum, E[r], f);
                            const uint32_t hmo = h - openMinusExt2;
                            E[r] = pk_max2_f16(E[r], hmo);
                            asm volatile("" : "+v"(E[r]));
                            // (after the last row: what the strip below starts from)
                            if (kToBelow || r + 1 < R) f = pk_max2_f16(f, hmo);
                            H[r] = hmo;
                            dsum = dnext;
                        }
                        asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
#pragma unroll
                        for (int k = 1; k <= 4; ++k)
                            if (r4 * 4 + 3 + k < R) asm volatile("" : "+v"(H[r4 * 4 + 3 + k]));
                    }
                    if constexpr (kToBelow) {
                        // (row R of this strip is row 0 of the strip below, whose scale starts again at r = 0)
                        const uint32_t down = both(R * ext);
                        if constexpr (odd) {
                            rowsOut.store(j / 2, lane, StripU4{keepH, keepF, H[R - 1] - down, f - down});
                        } else {
                            keepH = H[R - 1] - down;
                            keepF = f - down;
                        }
                    }
                    if constexpr (kFromAbove) {
                        hbPrev = hAbove;
                        if constexpr (odd) pq0 = pq1;
                    }
                    // ---- answers
                    if constexpr (!kToBelow) {
                        // the last query row: row rl of this strip, the same for the whole launch - usually
                        // the strip's last (the host prefers strip heights that divide the query). Otherwise a
                        // tree of wave-uniform BRANCHES finds it (selects would be R hoisted scalar predicates).
                        uint32_t hq = H[R - 1];
                        if (rl != R - 1) hq = pickRow<0, R - 2>(H, rl);
                        // (stored form on the scale of (rl, j): true value = pattern - sigma - rl ext + c)
                        const int back = sigma + rl * ext - (open - ext);
                        const int qA = (int)(hq & 0xffffu) - back, qB = (int)(hq >> 16) - back;
                        if (region == kLastCell) {
                            if (j == lenA - 1) { runA = qA; if (LOC) colA = j; }
                            if (j == lenB - 1) { runB = qB; if (LOC) colB = j; }
                        } else {
                            // HW scans columns < len, OV columns < len - 1 (its last column is scanned row by row)
                            const int cut = region == kLastRowCol ? 1 : 0;
                            if (j < lenA - cut && qA > runA) { runA = qA; if (LOC) colA = j; }
                            if (j < lenB - cut && qB > runB) { runB = qB; if (LOC) colB = j; }
                        }
                    }
                    if (region == kLastRowCol) {
                        const bool lastA = j == lenA - 1, lastB = j == lenB - 1;
                        if (__builtin_amdgcn_ballot_w64(lastA || lastB) != 0) {
                            // some lane is on its target's last column: maximum over this strip's query rows. The
                            // patterns of one column share a scale, so the packed maximum is a chain of max3 on
                            // both halves at once. (Rows beyond the query exist in the last strip only; their
                            // bound is made opaque HERE so that the row predicates are not hoisted out of the
                            // column loop into scalar register pairs.)
                            int rows = kToBelow ? R : rl + 1;
                            if (!kToBelow) asm volatile("" : "+v"(rows));
                            // (row r is on the scale of column j plus r ext: taken off with a running offset)
                            uint32_t off = 0u;
                            auto rowValue = [&](int r) -> uint32_t {
                                uint32_t v = H[r];
                                if (!kToBelow && r > 0) v = r < rows ? H[r] : H[0] + off;
                                return v - off;
                            };
                            uint32_t m2 = H[0];
#pragma unroll
                            for (int r = 1; r < R; ++r) {
                                off += ext2;
                                asm volatile("" : "+v"(off));
                                m2 = pk_max2_f16(m2, rowValue(r));
                            }
                            const int mA = (int)(m2 & 0xffffu), mB = (int)(m2 >> 16);
                            const int back = sigma - (open - ext);
                            if (lastA) cbA = mA - back;
                            if (lastB) cbB = mB - back;
                            if constexpr (LOC) {
                                // first row that holds the maximum of its half
                                int ia = 0, ib = 0;
#pragma unroll
                                for (int r = R - 1; r >= 0; --r) {
                                    const uint32_t d = rowValue(r) ^ m2;
                                    if ((d & 0xffffu) == 0) ia = r;
                                    if ((d >> 16) == 0) ib = r;
                                    asm volatile("" : "+v"(ia), "+v"(ib), "+v"(off));
                                    off -= ext2;
                                }
                                if (lastA) crowA = s * R + ia;
                                if (lastB) crowB = s * R + ib;
                            }
                        }
                    }
                };
#pragma unroll 1
                for (int cp = 0; cp < 4; cp += 2) {
                    column(std::false_type{}, cp);
                    column(std::true_type{}, cp + 1);
                }
                cur = nxt;
                shift += 4 * ext;
                if (!topGap && shift + 4 * ext > kBiasedMaxShift) {
                    // rebase (every strip does it after the same chunks: the rows the strip above wrote from
                    // the next chunk on are already on the new scale, the one kept in hbPrev is not)
                    const uint32_t d = both(shift);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        H[r] -= d;
                        E[r] -= d;
                    }
                    if constexpr (kFromAbove) hbPrev -= d;
                    sigma -= shift;
                    shift = 0;
                }
                if (kToBelow) stripPublishStep(progOut, c, nChunks, lane, timer);
            }
        };
#define MIOPAL_STRIP_FRAME_PART 3
#include "interseq_strip_frame.inc"
#define MIOPAL_STRIP_FRAME_PART 4
#include "interseq_strip_frame.inc"
        if constexpr (LOC) {
            auto key = [](int score, bool onLastRow, int index) -> unsigned long long {
                return ((unsigned long long)((uint32_t)score ^ 0x80000000u) << 32) | (onLastRow ? 0x80000000ull : 0ull) |
                       (unsigned long long)(0x7FFFFFFFu - (uint32_t)index);
            };
            if (!toBelow) {
                if (colA >= 0) atomicMax(a.stripKeys + base + lane, key(runA, true, colA));
                if (colB >= 0) atomicMax(a.stripKeys + base + kLanes + lane, key(runB, true, colB));
            }
            if (region == kLastRowCol) {
                if (crowA >= 0) atomicMax(a.stripKeys + base + lane, key(cbA, false, crowA));
                if (crowB >= 0) atomicMax(a.stripKeys + base + kLanes + lane, key(cbB, false, crowB));
            }
        } else if (region == kLastRowCol) {
            // OV: every strip's last-column maximum and the last strip's last-row maximum (INT32_MIN: none)
            atomicMax(a.score + base + lane, max(runA, cbA));
            atomicMax(a.score + base + kLanes + lane, max(runB, cbB));
        } else if (!toBelow) {
            a.score[base + lane] = runA;
            a.score[base + kLanes + lane] = runB;
        }
    }
    timer.flush(a.stripTiming, lane);
#undef MIOPAL_STRIP_FRAME_ABORTS
#undef MIOPAL_STRIP_FRAME_STATE
#undef MIOPAL_PAIR_ENTRY
}

template <int R, bool LOC>
static hipError_t launchPairGlobalStripsR(const InterseqArgs& a, int computeUnits, hipStream_t stream) {
    const size_t lds = PairLayout<R>::bytes(a.nSymbols) + 16 + kPaceInts * sizeof(int);  // table + the unit in flight + pacing
    if (const hipError_t e = allowFullLds<&interseq_pair_global_strips_kernel<R, LOC>>(); e != hipSuccess) return e;
    const int nBatches = (a.nGroups + a.batchGroups - 1) / a.batchGroups;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(computeUnits, (int64_t)nBatches * a.nStrips));
    hipLaunchKernelGGL((interseq_pair_global_strips_kernel<R, LOC>), dim3(blocks), dim3(kPairWavesPerGroup * kLanes), lds, stream, a);
    return hipGetLastError();
}

template <int kLo, bool LOC>
hipError_t launchPairGlobalStrips(const InterseqArgs& a, int rowsPerStrip, int computeUnits, hipStream_t stream) {
    if (a.nStrips < 2 || !a.unitCounter || !a.unitFlags || !a.boundary[0] || !a.boundary[1] || a.batchGroups < 1 ||
        a.batchGroups > kPairWavesPerGroup || (LOC && !a.stripKeys) || a.region == kAllCells)
        return hipErrorInvalidValue;
    return dispatchRows<kLo, 2, kPairUnitCounts, LOC ? kPairStripsMaxRowsLoc : kPairStripsMaxRows>(
        rowsPerStrip, [&](auto r) { return launchPairGlobalStripsR<r, LOC>(a, computeUnits, stream); });
}

}  // namespace miopal
