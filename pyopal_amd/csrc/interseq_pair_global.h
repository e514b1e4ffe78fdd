#pragma once
#include "interseq_packed_ops.h"
#include "interseq_pair_parts.h"

namespace miopal {

// ---- one-strip NW / HW / OV on biased integer halves, column-shifted --------------
// The pair-table kernel for the modes without a floor (round 2). Same representation as the Smith-Waterman kernels'
// (interseq_pair_parts.h) - a
// half holds zero + x + sigma(j) and is compared as a half float, additions are 32-bit integer adds,
// values of column j carry sigma(j) = j * ext so that extending E is free - with what the other
// modes need:
//  * borders: H[-1][j], H[i][-1] = 0 or the gap of j + 1 / i + 1 residues (borderGap), entered per
//    column as wave-uniform patterns;
//  * no floor: E = max(E, hmo), F = max(F, hmo) - ext; 3 integer adds + 3 max per cell pair (the
//    general kernel's shifted int16 flavour: 6 packed operations + 1 v_perm);
//  * the answer of a lane half is read at its own last column / on the last query row, turned into a
//    true 32-bit value x = pattern - (zero + sigma(j)): the lanes never leave their range because of
//    a target's length (NW scores of 35000-residue targets are far below -32768, the pattern is not),
//    so nothing is flagged and no target is redone at 32 bit. The host checks the static bounds
//    (zero covers 2 open + (Q + 2) ext + |min S|, Q (max S + ext) + zero + kBiasedMaxShift < 0x7C00);
//  * with a free top border (HW, OV) x is bounded and sigma is rebased like the Smith-Waterman
//    kernel's; with a penalised one (NW) x + j ext is bounded and sigma just grows (as an int).
// End locations (optional): the scan rules of oracle/opal_oracle.c on those per-column values.
// Twelve wavefronts per workgroup (three per SIMD, 168 VGPRs) up to 54 rows, eight (256 VGPRs) beyond:
// beside H[R], E[R] this kernel keeps per-lane answers, lengths and locations.
__host__ __device__ constexpr int globalWaves(int rows) { return rows <= 54 ? 12 : 8; }

template <int R>
__global__ __launch_bounds__(globalWaves(R) * kLanes) void interseq_pair_global_kernel(InterseqArgs a) {
    constexpr int kGlobalWaves = globalWaves(R);
    constexpr int SLOTS = PairLayout<R>::kRowSlots;
    constexpr int NB4 = (R + 3) / 4;
    extern __shared__ uint4 pairs[];

    const int lane = threadIdx.x & 63;
    const int nSym = a.nSymbols;
    const int ext = a.gapExt, open = a.gapOpen, Q = a.qLen;
    const int zero = a.biasedZero;
    const bool topGap = a.topGap, leftGap = a.leftGap;
    const int region = a.region;
    const bool locate = a.endI != nullptr;
    const uint32_t openMinusExt2 = both(open - ext);

    // table: s'' = s + 2 ext + c = s + ext + open of both targets as one integer (round 3: every cell (r, j) is
    // on the scale zero + sigma(j) + r ext, H kept c = open - ext below its plain form: 2 integer adds + 3
    // max per cell pair, see interseq_pair_global_strips_kernel); padding symbol / rows add c
    {
        const int16_t* gp = a.profile;
        constexpr int kBuildThreads = kGlobalWaves * kLanes;
#define MIOPAL_PAIR_ENTRY MIOPAL_GLOBAL_PAIR_ENTRY
#include "interseq_pair_table_build.inc"
#undef MIOPAL_PAIR_ENTRY
    }
    int* simdTaken = reinterpret_cast<int*>(pairs + nSym * nSym * SLOTS);
    if (threadIdx.x < 4) simdTaken[threadIdx.x] = 0;
    __syncthreads();
    SimdPace pace;
    if (MIOPAL_HEADLINE_PACE) pace.init(simdTaken + 4, lane);

    constexpr int kHandoutWaves = kGlobalWaves;
#define MIOPAL_PAIR_HANDOUT_PART 1
#include "interseq_pair_handout.inc"
    for (;;) {
        int g;
#define MIOPAL_PAIR_HANDOUT_PART 2
#include "interseq_pair_handout.inc"
        const uint2* pack = a.pack + a.groupOff[g];
        const int nChunks = a.groupChunks[g];
        groupPriority(nChunks, a.priorityChunks);
        const size_t base = (size_t)g * kGroupTargets;
        const int lenA = a.lens[base + lane], lenB = a.lens[base + kLanes + lane];

        // answers (true values) and where they were found
        int runA = INT32_MIN, runB = INT32_MIN, colA = -1, colB = -1, rowA = -1, rowB = -1;
        int cbA = INT32_MIN, cbB = INT32_MIN, crowA = -1, crowB = -1;   // OV: best of the last column

        int sigma = zero - ext;             // zero + sigma(j) of the last column done (column -1 here)
        int shift = -ext;                   // part of sigma accumulated since the last rebase
        uint32_t H[R], E[R];
        {
            // (opaque to the optimiser: the 2 R border values are the same for every group, and hoisting
            // them out of the group loop would cost 2 R registers for the whole kernel)
            int zeroHere = zero, openHere = open, extHere = ext;
            asm volatile("" : "+s"(zeroHere), "+s"(openHere), "+s"(extHere));
            // H[r][-1]: one gap of r + 1 residues or r + 1 one-residue gaps (borderGap), as running sums
            int one = openHere, many = openHere, rowShift = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int left = (leftGap ? -min(one, many) : 0) + rowShift;
                H[r] = both(zeroHere - extHere + left - (openHere - extHere));   // stored form, scale of (r, -1)
                E[r] = both(zeroHere + left - openHere);                  // E[r][0], plain form, scale of (r, 0)
                one += extHere;
                many += openHere;
                rowShift += extHere;
            }
        }
        uint2 cur = pack[lane];
        constexpr int kWant = 3;
        constexpr int kAhead = NB4 > kWant ? kWant : 1;
        const uint4* prowNext = pairRowOf<SLOTS>(pairs, nSym, cur.x & 0xffu, cur.y & 0xffu);
        uint4 vn[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) vn[k] = prowNext[k];
        for (int c = 0; c < nChunks; ++c) {
            uint2 nxt = {0, 0};
            if (c + 1 < nChunks) nxt = pack[(size_t)(c + 1) * kLanes + lane];
            if (MIOPAL_HEADLINE_PACE) pace.step(c - nChunks, lane, nChunks > a.priorityChunks);
            uint32_t ra = cur.x, rb = cur.y;
#pragma unroll 1
            for (int cc = 0; cc < 4; ++cc) {
                const int j = c * 4 + cc;
                const uint4* prow = prowNext;
                uint4 v[NB4];
#pragma unroll
                for (int k = 0; k < kAhead; ++k) v[k] = vn[k];
                ra = cc < 3 ? ra >> 8 : nxt.x;
                rb = cc < 3 ? rb >> 8 : nxt.y;
                prowNext = pairRowOf<SLOTS>(pairs, nSym, ra & 0xffu, rb & 0xffu);
                auto score = [&](int r) -> uint32_t {
                    const uint4 x = v[r >> 2];
                    const int k = r & 3;
                    return k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w;
                };
                // row above the strip: H[-1][j-1] on the previous column's scale, H[-1][j] on this one's
                const int topPrev = (j == 0 || !topGap) ? 0 : borderGap(j - 1, open, ext);
                const int topHere = topGap ? borderGap(j, open, ext) : 0;
                // (H[-1][j-1] in stored form on the scale of (-1, j - 1))
                uint32_t dsum = both(sigma + topPrev - open) + score(0);
                sigma += ext;
                uint32_t f = both(sigma + topHere - open);      // F entering row 0
                asm volatile("" : "+v"(f));
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
                        const uint32_t hmo = h - openMinusExt2;
                        E[r] = pk_max2_f16(E[r], hmo);
                        // (here, not whenever the scheduler likes: E is off the critical path, and the R
                        // deferred updates would each hold on to their hmo)
                        asm volatile("" : "+v"(E[r]));
                        if (r + 1 < R) f = pk_max2_f16(f, hmo);
                        H[r] = hmo;
                        dsum = dnext;
                    }
                    // pins the schedule: no ds_read and none of the NEXT blocks' diagonal sums (they only
                    // need last column's H, all of it available at the column's top: hoisting them costs
                    // R registers) may start before this block's cells are done
                    asm volatile("" : "+v"(f), "+v"(dsum)::"memory");
#pragma unroll
                    for (int k = 1; k <= 4; ++k)
                        if (r4 * 4 + 3 + k < R) asm volatile("" : "+v"(H[r4 * 4 + 3 + k]));
                }
                // ---- answers: the last query row is row R - 1 or R - 2 (R = Q rounded up to even)
                const uint32_t hq = (Q & 1) ? H[R >= 2 ? R - 2 : 0] : H[R - 1];
                // (stored form on the scale of (Q - 1, j): true value = pattern - sigma - (Q - 1) ext + c)
                const int back = sigma + (Q - 1) * ext - (open - ext);
                const int qA = (int)(hq & 0xffffu) - back, qB = (int)(hq >> 16) - back;
                if (region == kLastCell) {
                    if (j == lenA - 1) { runA = qA; colA = j; }
                    if (j == lenB - 1) { runB = qB; colB = j; }
                } else {
                    // last row: HW scans columns < len, OV columns < len - 1 (its last column is
                    // scanned row by row below)
                    const int cut = region == kLastRowCol ? 1 : 0;
                    if (j < lenA - cut && qA > runA) { runA = qA; colA = j; }
                    if (j < lenB - cut && qB > runB) { runB = qB; colB = j; }
                    const bool lastA = j == lenA - 1, lastB = j == lenB - 1;
                    if (region == kLastRowCol && __builtin_amdgcn_ballot_w64(lastA || lastB) != 0) {
                        // some lane is on its target's last column: first maximum over the query rows
                        int mA = INT32_MIN, mB = INT32_MIN, ia = 0, ib = 0;
                        int off = (R - 1) * ext;   // row r is on the scale of column j plus r ext
                        asm volatile("" : "+v"(off));
#pragma unroll
                        for (int r = R - 1; r >= 0; --r) {
                            // (rows beyond the query: only row R - 1, when Q is odd; one test, not one
                            // per row - per-row predicates would be hoisted into a hundred SGPRs)
                            if (!(r == R - 1 && (Q & 1))) {
                                const int hA = (int)(H[r] & 0xffffu) - off, hB = (int)(H[r] >> 16) - off;
                                if (hA >= mA) { mA = hA; ia = r; }
                                if (hB >= mB) { mB = hB; ib = r; }
                            }
                            off -= ext;
                            // (row by row: the scheduler would otherwise unpack all 2 R halves up front)
                            asm volatile("" : "+v"(mA), "+v"(mB), "+v"(off));
                        }
                        const int back = sigma - (open - ext);
                        if (lastA) { cbA = mA - back; crowA = ia; }
                        if (lastB) { cbB = mB - back; crowB = ib; }
                    }
                }
            }
            cur = nxt;
            shift += 4 * ext;
            if (!topGap && shift + 4 * ext > kBiasedMaxShift) {
                const uint32_t d = both(shift);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    H[r] -= d;
                    E[r] -= d;
                }
                sigma -= shift;
                shift = 0;
            }
        }
        if (region != kLastCell || true) {
            rowA = colA >= 0 ? Q - 1 : -1;
            rowB = colB >= 0 ? Q - 1 : -1;
        }
        if (region == kLastRowCol) {
            // OV: the last column is scanned after the last row's earlier columns, strictly greater wins
            if (crowA >= 0 && (colA < 0 || cbA > runA)) { runA = cbA; rowA = crowA; colA = lenA - 1; }
            if (crowB >= 0 && (colB < 0 || cbB > runB)) { runB = cbB; rowB = crowB; colB = lenB - 1; }
        }
        if (a.directOut) {
            // database order at once (nothing else writes these results: see the Smith-Waterman kernel)
            const int posA = (int)base + lane, posB = posA + kLanes;
            if (posA < a.directN) {
                const int id = a.directIds[posA];
                a.directOut[id] = runA;
                if (locate) {
                    a.directEndI[id] = rowA;
                    a.directEndJ[id] = colA;
                }
            }
            if (posB < a.directN) {
                const int id = a.directIds[posB];
                a.directOut[id] = runB;
                if (locate) {
                    a.directEndI[id] = rowB;
                    a.directEndJ[id] = colB;
                }
            }
            continue;
        }
        a.score[base + lane] = runA;
        a.score[base + kLanes + lane] = runB;
        if (locate) {
            a.endI[base + lane] = rowA;
            a.endI[base + kLanes + lane] = rowB;
            a.endJ[base + lane] = colA;
            a.endJ[base + kLanes + lane] = colB;
        }
        if (a.overflow) {
            a.overflow[base + lane] = 0;
            a.overflow[base + kLanes + lane] = 0;
        }
    }
    if (MIOPAL_HEADLINE_PACE && lane == 0) *pace.mine = INT32_MAX;   // (done: nobody waits for this one)
}

template <int R>
static hipError_t launchPairGlobalR(const InterseqArgs& a, int computeUnits, hipStream_t stream) {
    const size_t lds = PairLayout<R>::bytes(a.nSymbols) + 16 + kPaceInts * sizeof(int);
    if (const hipError_t e = allowFullLds<&interseq_pair_global_kernel<R>>(); e != hipSuccess) return e;
    constexpr int kGlobalWaves = globalWaves(R);
    const int blocks = std::max(1, std::min(computeUnits, a.nGroups));   // (see launchPairBiasedR)
    hipLaunchKernelGGL((interseq_pair_global_kernel<R>), dim3(blocks), dim3(kGlobalWaves * kLanes), lds, stream, a);
    return hipGetLastError();
}

template <int kLo>
hipError_t launchPairGlobal(const InterseqArgs& a, int rowsPerStrip, int computeUnits, hipStream_t stream) {
    if (a.nStrips != 1) return hipErrorInvalidValue;
    return dispatchRows<kLo, 2, kPairUnitCounts>(rowsPerStrip, [&](auto r) { return launchPairGlobalR<r>(a, computeUnits, stream); });
}

}  // namespace miopal
