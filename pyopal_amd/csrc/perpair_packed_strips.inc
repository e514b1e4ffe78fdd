// Part of perpair_packed.hip (included inside its anonymous namespace): the start-cell scan with two pairs per lane
// for queries of several strips - the lanes of a wavefront in step.
//
// (Halves on schedules of their own, as in perpair_packed_scan_kernel, would hand a strip's last row to the next
// through a private line of HBM per half: 4 bytes used of every 128-byte line moved, 33 MB of lines in flight -
// tried, 37 ms where the 32-bit kernel takes 23.) Jobs sorted by length, 128 to a wavefront, which sweeps strip
// after strip; the last row of a strip reaches the next as [column][lane] rows of 8 bytes - {stored H, F} of both
// halves - written and read back whole. A half leaves a strip at the column where it met its optimum; the strips
// below then only need the columns up to it (their rows are larger: they can only beat it in a smaller column).
// Cells, keys and hits as in perpair_packed_scan_kernel.
// (OV - the pair's own last row, wherever its strip, or any row of its last column - is an instantiation of its own:
// perpair_packed_scan_kernel)
template <bool BIASED, bool OV>
__global__ __launch_bounds__(kScanBlock, 2) void perpair_packed_scan_strips_kernel(PerPairArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pkLds[];
    uint8_t* const prof = pkLds;
    const int A = a.alphabet;
    const int Qtot = a.queryLength;
    const int pstride = a.profileStride;
    const int open = a.gapOpen, ext = a.gapExt;
    const int Z = a.packedZero;
    for (int idx = threadIdx.x; idx < (A + 1) * pstride; idx += kScanBlock) {
        const int t = idx / pstride, y = idx - t * pstride;
        int v = 0;
        if (t < A && y < Qtot) v = 8 * (scoreAt(a.matrix, a.query, a.rows, A, Qtot - 1 - y, t) + open + a.packedBias);
        prof[idx] = (uint8_t)v;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int W = blockIdx.x * kScanWaves + wave;
    const int idxA = W * 128 + lane, idxB = idxA + kLanes;
    const bool activeA = idxA < a.nJobs, activeB = idxB < a.nJobs;
    if (__builtin_amdgcn_ballot_w64(activeA || activeB) == 0) return;
    PairJob jobA{}, jobB{};
    if (activeA) jobA = a.jobs[idxA];
    if (activeB) jobB = a.jobs[idxB];
    const int QA = jobA.qLen, LA = jobA.tLen, QB = jobB.qLen, LB = jobB.tLen;
    int maxQ = max(QA, QB);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxQ = max(maxQ, __shfl_xor(maxQ, off));
    maxQ = __builtin_amdgcn_readfirstlane(maxQ);
    const int nStrips = (maxQ + kLanes - 1) / kLanes;

    const uint32_t ext2 = both(8 * ext), c2 = both(8 * (open - ext));
    const uint32_t negBias2 = 0u - both(8 * a.packedBias);
    const uint32_t top2 = both(Z - 8 * (2 * open - ext));   // row -1 in stored form, any column but -1
    const uint32_t padWord = (uint32_t)A * 0x01010101u;
    const uint8_t* const dbLo = a.residues;
    const uint8_t* const dbHi = a.residues + a.residueCount - 4;
    const uint8_t* const tptrA = a.residues + jobA.tOff;
    const uint8_t* const tptrB = a.residues + jobB.tOff;
    auto fetchRaw = [&](const uint8_t* tptr, int j0) -> uint32_t {
        const uint8_t* at = tptr - j0 - 3;
        at = at < dbLo ? dbLo : at;
        at = at > dbHi ? dbHi : at;
        uint32_t w;
        __builtin_memcpy(&w, at, 4);
        return w;
    };
    auto inPlace = [&](const uint8_t* tptr, int L, uint32_t raw, int j0) -> uint32_t {
        const uint8_t* at = tptr - j0 - 3;
        const int64_t below = dbLo - at, above = at - dbHi;
        uint32_t w = raw;
        if (below > 0) w = below >= 4 ? 0u : raw << (8 * (int)below);
        if (above > 0) w = above >= 4 ? 0u : raw >> (8 * (int)above);
        w = __builtin_bswap32(w);
        const int valid = L - j0;
        const uint32_t keep = valid >= 4 ? 0xffffffffu : valid <= 0 ? 0u : (1u << (8 * valid)) - 1u;
        return (w & keep) | (padWord & ~keep);
    };
    uint2* const bnd = reinterpret_cast<uint2*>(a.boundary) + (int64_t)W * a.boundaryStride * kLanes + lane;
    int needA = (QA > 0 && LA > 0) ? LA : 0, needB = (QB > 0 && LB > 0) ? LB : 0;
    int bcolA = -1, browA = -1, bcolB = -1, browB = -1;
    const int y0A = Qtot - 1 - jobA.qOff, y0B = Qtot - 1 - jobB.qOff;
    const uint32_t tgt0 = ((uint32_t)(Z + 8 * jobA.stop) & 0xffffu) | ((uint32_t)(Z + 8 * jobB.stop) << 16);
    const bool lastRowOnly = !OV && a.scanLastRow == 1;   // (wave-uniform)

    for (int s = 0; s < nStrips; ++s) {
        const int row0 = s * kLanes;
        const int rowsHere = min(maxQ - row0, kLanes);  // wave-uniform
        auto sweepStrip = [&](auto groupsTag) {
            constexpr int GROUPS = decltype(groupsTag)::value, ROWS = GROUPS * 8;
            const bool toNext = s + 1 < nStrips;
            // (HW: the query's last row, if this strip holds it - every HW prefix has all the query's rows)
            const int lastRowLocal = (lastRowOnly && Qtot - 1 >= row0 && Qtot - 1 < row0 + kLanes) ? Qtot - 1 - row0 : -1;
            // halves this strip matters to, and the columns it has to sweep for them
            bool stillA = row0 < QA && needA > 0, stillB = row0 < QB && needB > 0;
            int maxNeed = max(stillA ? needA : 0, stillB ? needB : 0);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) maxNeed = max(maxNeed, __shfl_xor(maxNeed, off));
            maxNeed = __builtin_amdgcn_readfirstlane(maxNeed);
            const int ysA = min(y0A + row0, Qtot), ysB = min(y0B + row0, Qtot);
            const uint32_t shiftA = (uint32_t)ysA & 3u, shiftB = (uint32_t)ysB & 3u;
            const int yAlA = ysA & ~3, yAlB = ysB & ~3;
            uint32_t HS[ROWS], E[ROWS];
#pragma unroll
            for (int i = 0; i < ROWS; ++i) HS[i] = E[i] = both(Z - 8 * (2 * open + (row0 + i) * ext));   // column -1
            uint32_t aboveHsPrev = s == 0 ? both(Z - 8 * open) : both(Z - 8 * (2 * open + (row0 - 1) * ext));
            uint32_t tgt2 = tgt0;
            uint32_t wcurA = padWord, rawNextA = fetchRaw(tptrA, 0), wcurB = padWord, rawNextB = fetchRaw(tptrB, 0);
            // (the row above, TWO columns ahead: a column of 64 rows lasts about as long as a load from HBM - one ahead
            // 13.3 ms at Q = 300, two 12.2, three 12.3)
            uint2 aboveNext = make_uint2(top2, top2), aboveNext2 = aboveNext;
            if (s > 0 && maxNeed > 0) {
                aboveNext = bnd[0];
                aboveNext2 = bnd[(int64_t)min(1, maxNeed - 1) * kLanes];
            }
            for (int j = 0; j < maxNeed; ++j, tgt2 += ext2) {
                if ((j & 3) == 0) {
                    wcurA = inPlace(tptrA, LA, rawNextA, j);
                    rawNextA = fetchRaw(tptrA, j + 4);
                    wcurB = inPlace(tptrB, LB, rawNextB, j);
                    rawNextB = fetchRaw(tptrB, j + 4);
                }
                const uint32_t tA = (wcurA >> (8 * (j & 3))) & 0xffu, tB = (wcurB >> (8 * (j & 3))) & 0xffu;
                const uint32_t* prowA = reinterpret_cast<const uint32_t*>(prof + tA * pstride + yAlA);
                const uint32_t* prowB = reinterpret_cast<const uint32_t*>(prof + tB * pstride + yAlB);
                uint32_t hsUp = top2, F = top2;
                if (s > 0) {
                    const uint2 above = aboveNext;
                    aboveNext = aboveNext2;
                    aboveNext2 = bnd[(int64_t)min(j + 2, maxNeed - 1) * kLanes];   // (unconditional: no copy behind the load)
                    hsUp = above.x;
                    F = above.y;
                }
                uint32_t hsDiag = aboveHsPrev;
                aboveHsPrev = hsUp;
                uint32_t gm[GROUPS];
                uint32_t held = 0;
                uint32_t hLast = 0;   // (scanLastRow: the cell of the query's last row, in the last strip's last group of eight)
                uint32_t wloA = prowA[0], wloB = prowB[0], n1A = prowA[1], n1B = prowB[1], fourA = 0, fourB = 0;
#pragma unroll
                for (int i = 0; i < ROWS; ++i) {
                    if ((i & 3) == 0) {
                        const int blk = i >> 2;
                        const uint32_t whiA = n1A, whiB = n1B;
                        fourA = __builtin_amdgcn_alignbyte(whiA, wloA, shiftA);
                        fourB = __builtin_amdgcn_alignbyte(whiB, wloB, shiftB);
                        wloA = whiA;
                        wloB = whiB;
                        if (blk + 2 <= ROWS / 4) {
                            n1A = prowA[blk + 2];
                            n1B = prowB[blk + 2];
                        }
                    }
                    const uint32_t ub2 = __builtin_amdgcn_perm(fourB, fourA, 0x0c040c00u + (uint32_t)(i & 3) * 0x00010001u);
                    uint32_t d = hsDiag + ub2;
                    if (BIASED) d += negBias2;
                    const uint32_t e = pkMax(E[i], HS[i]);
                    const uint32_t f = pkMax(F, hsUp) - ext2;
                    const uint32_t h = pkMax3(d, e, f);
                    if (i >= ROWS - 8) hLast = i == lastRowLocal ? h : hLast;   // (wave-uniform)
                    const int r = i & 7, g = i >> 3;
                    if (r == 1) gm[g] = pkMax(held, h);
                    else if (r & 1) gm[g] = pkMax3(gm[g], held, h);
                    else held = h;
                    const uint32_t hs = h - c2;
                    hsDiag = HS[i];
                    HS[i] = hs;
                    E[i] = e;
                    F = f;
                    hsUp = hs;
                    if ((i & 3) == 3) asm volatile("" : "+v"(F), "+v"(hsDiag)::"memory");
                }
                if (ROWS == kLanes && toNext) bnd[(int64_t)j * kLanes] = make_uint2(hsUp, F);
                uint32_t cmk = gm[0] + both(7);
#pragma unroll
                for (int g = 1; g < GROUPS; g += 2) {
                    if (g + 1 < GROUPS) cmk = pkMax3(cmk, gm[g] + both(7 - g), gm[g + 1] + both(6 - g));
                    else cmk = pkMax(cmk, gm[g] + both(7 - g));
                }
                // (HW, scanLastRow: only the cell of the query's last row answers - in the last strip - and cells above it
                // may well be larger; the strips above sweep the whole prefix for it)
                uint32_t x = lastRowOnly ? (lastRowLocal >= 0 ? hLast ^ tgt2 : 0xffffffffu) : (cmk & 0xfff8fff8u) ^ tgt2;
                // OV: the prefix's last column answers in every row (the test above), every other column only in the pair's own
                // last row - when this strip holds it
                const bool lastColA = j == LA - 1, lastColB = j == LB - 1;
                if (OV) {
                    // (the halves' rows inside this strip, each on its own: a packed subtraction would borrow across them)
                    const uint32_t local2 = ((uint32_t)(QA - 1 - row0) & 0x3fu) | (((uint32_t)(QB - 1 - row0) & 0x3fu) << 16);
                    uint32_t own = pickRowOfEither<ROWS>(HS, local2) ^ (tgt2 - c2);   // (HS holds h - c2)
                    const bool holdsA = (QA - 1) >= row0 && (QA - 1) < row0 + ROWS, holdsB = (QB - 1) >= row0 && (QB - 1) < row0 + ROWS;
                    own |= (holdsA ? 0u : 0x0000ffffu) | (holdsB ? 0u : 0xffff0000u);
                    x = (lastColA ? x & 0xffffu : own & 0xffffu) | (lastColB ? x & 0xffff0000u : own & 0xffff0000u);
                }
                const bool hitA = stillA && (x & 0xffffu) == 0, hitB = stillB && (x >> 16) == 0;
                if (__builtin_amdgcn_ballot_w64(hitA || hitB) != 0) {
                    const int gstarA = 7 - (int)(cmk & 7u), gstarB = 7 - (int)((cmk >> 16) & 7u);
                    int rowA = OV ? QA - 1 - row0 : max(lastRowLocal, 0), rowB = OV ? QB - 1 - row0 : max(lastRowLocal, 0);
#pragma unroll
                    for (int g = 0; g < GROUPS && !lastRowOnly; ++g) {
                        const bool inA = hitA && gstarA == g && (!OV || lastColA), inB = hitB && gstarB == g && (!OV || lastColB);
                        if (__builtin_amdgcn_ballot_w64(inA || inB) == 0) continue;
                        uint32_t m = pkMax(HS[8 * g] + both(7), HS[8 * g + 1] + both(6));
                        m = pkMax3(m, HS[8 * g + 2] + both(5), HS[8 * g + 3] + both(4));
                        m = pkMax3(m, HS[8 * g + 4] + both(3), HS[8 * g + 5] + both(2));
                        m = pkMax3(m, HS[8 * g + 6] + both(1), HS[8 * g + 7]);
                        if (inA) rowA = 8 * g + 7 - (int)(m & 7u);
                        if (inB) rowB = 8 * g + 7 - (int)((m >> 16) & 7u);
                    }
                    // of the strips' hits the smallest column wins, then the smallest row: an earlier strip's at the
                    // same column
                    if (hitA && (bcolA < 0 || j < bcolA)) {
                        bcolA = j;
                        browA = row0 + rowA;
                    }
                    if (hitB && (bcolB < 0 || j < bcolB)) {
                        bcolB = j;
                        browB = row0 + rowB;
                    }
                }
                stillA = stillA && !hitA && j + 1 < needA;
                stillB = stillB && !hitB && j + 1 < needB;
                if (__builtin_amdgcn_ballot_w64(stillA || stillB) == 0) break;
            }
            if (bcolA >= 0) needA = min(needA, bcolA + 1);
            if (bcolB >= 0) needB = min(needB, bcolB + 1);
        };
        using std::integral_constant;
        switch ((rowsHere + 7) >> 3) {   // wave-uniform
            case 1: sweepStrip(integral_constant<int, 1>{}); break;
            case 2: sweepStrip(integral_constant<int, 2>{}); break;
            case 3: sweepStrip(integral_constant<int, 3>{}); break;
            case 4: sweepStrip(integral_constant<int, 4>{}); break;
            case 5: sweepStrip(integral_constant<int, 5>{}); break;
            case 6: sweepStrip(integral_constant<int, 6>{}); break;
            case 7: sweepStrip(integral_constant<int, 7>{}); break;
            default: sweepStrip(integral_constant<int, 8>{}); break;
        }
    }
    int windowMax = 0, rowsMax = 0;
    auto finish = [&](bool active, const PairJob& job, int bcol, int brow) {
        if (!active) return;
        if (a.startQ != nullptr) {
            // the start cell itself (perpair_packed_scan_kernel: what start_cells_kernel makes of the reverse pass)
            int sq = -1, st = -1;
            if (job.qLen > 0 && job.tLen > 0) {
                const bool found = bcol >= 0;
                // (HW: the whole query in one gap - a border cell of the reversed problem: perpair_packed_scan_kernel)
                const bool border = !found && (lastRowOnly || OV) && job.stop == borderGap(job.qLen - 1, open, ext);
                // (OV: ... or the whole target prefix in one gap: start_cells_kernel asks in this order)
                const bool borderT = OV && !found && !border && job.stop == borderGap(job.tLen - 1, open, ext);
                if (!found && !border && !borderT) atomicExch(a.startChecks, job.out + 1);
                sq = found ? job.qLen - 1 - brow : borderT ? job.qLen : 0;
                st = found ? job.tLen - 1 - bcol : border ? job.tLen : 0;
                windowMax = max(windowMax, job.tLen - st);
                rowsMax = max(rowsMax, job.qLen - sq);
            }
            a.startQ[job.out] = sq;
            a.startT[job.out] = st;
            return;
        }
        int v = bcol >= 0 ? job.stop : INT32_MIN;
        if (!(job.qLen > 0 && job.tLen > 0)) {
            // degenerate pair: closed forms of the border (oracle/opal_oracle.c, dp_pass)
            v = 0;
            if (job.qLen > 0) v = borderGap(job.qLen - 1, open, ext);
            if (job.tLen > 0) v = borderGap(job.tLen - 1, open, ext);
        }
        a.score[job.out] = v;
        if (a.endI) a.endI[job.out] = bcol >= 0 ? brow : -1;
        if (a.endJ) a.endJ[job.out] = bcol;
    };
    finish(activeA, jobA, bcolA, browA);
    finish(activeB, jobB, bcolB, browB);
    if (a.startQ != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            windowMax = max(windowMax, __shfl_xor(windowMax, off));
            rowsMax = max(rowsMax, __shfl_xor(rowsMax, off));
        }
        if (lane == 0 && windowMax > 0) {
            atomicMax(a.startChecks + 1, windowMax);
            atomicMax(a.startChecks + 2, rowsMax);
        }
    }
}
