// CPU-only checks of score_ranges.h: miopalSelfTest(4) (host.hip) and tools/score_ranges_check.cpp (the same under the
// host sanitizers). 0 = fine, else the number of the check that failed. The expectations are literals worked out by
// hand from the rules as the router wrote them out before they had one home; BLOSUM62 (min -4, max 11), open 3, ext 1.
#pragma once
#include "score_ranges.h"

namespace miopal {

inline int scoreRangesSelfTest() {
    const ScoreModel b62{3, 1, 11, -4};
    // ---- mode -> rules ----
    {
        DpRules r{};
        if (!rulesForMode(OPAL_MODE_NW, &r) || r.topGap != 1 || r.leftGap != 1 || r.floor0 != 0 || r.region != kLastCell) return 1;
        if (!rulesForMode(OPAL_MODE_HW, &r) || r.topGap != 0 || r.leftGap != 1 || r.floor0 != 0 || r.region != kLastRow) return 2;
        if (!rulesForMode(OPAL_MODE_OV, &r) || r.topGap != 0 || r.leftGap != 0 || r.floor0 != 0 || r.region != kLastRowCol) return 3;
        if (!rulesForMode(OPAL_MODE_SW, &r) || r.topGap != 0 || r.leftGap != 0 || r.floor0 != 1 || r.region != kAllCells) return 4;
        if (rulesForMode(7, &r) || rulesForMode(-1, &r)) return 5;
    }
    // ---- (a) the biased band ----
    // step up max(11 + 1, 1 - 3) = 12, step down max(-(-4 + 1), 3 - 1) = 3, 5 ext = 5: far inside; no excess over 0x0400
    if (stepUp(b62) != 12 || stepDown(b62) != 3) return 10;
    if (!biasedBandFits(b62, 0, false) || biasedLimit(b62, 0, false) != 25600) return 11;
    // row keys: (0x7C00 - 0x0C00 - 4096) = 24576, >> 4 / 5 / 6 bits for <= 16 / <= 32 / more rows
    if (rowKeyBits(16, true) != 4 || rowKeyBits(17, true) != 5 || rowKeyBits(32, true) != 5 || rowKeyBits(33, true) != 6 ||
        rowKeyBits(48, false) != 0)
        return 12;
    if (!biasedBandFits(b62, 4, true) || !biasedBandFits(b62, 5, true) || !biasedBandFits(b62, 6, true)) return 13;
    if (biasedLimit(b62, rowKeyBits(16, true), true) != 1536 || biasedLimit(b62, rowKeyBits(32, true), true) != 768 ||
        biasedLimit(b62, rowKeyBits(48, true), true) != 384)
        return 14;
    // a step up beyond 0x0400 lowers the limit by the excess, shifted back:
    //   max S = 99: 100 << 4 = 1600, 576 too many: (24576 - 576) >> 4 = 1500 = 1536 - (576 >> 4)
    //   max S = 1123, no keys: 1124, 100 too many: 25600 - 100
    if (!biasedBandFits({3, 1, 99, -4}, 4, true) || biasedLimit({3, 1, 99, -4}, 4, true) != 1500) return 15;
    if (!biasedBandFits({3, 1, 1123, -4}, 0, false) || biasedLimit({3, 1, 1123, -4}, 0, false) != 25500) return 16;
    // each of the four conditions alone, at its boundary and one beyond:
    //   step up: max S + ext = 4096 = 0x1000 holds, 4097 does not (step down 3, 5 ext = 5)
    if (!biasedBandFits({3, 1, 4095, -4}, 0, false) || biasedBandFits({3, 1, 4096, -4}, 0, false)) return 17;
    //   step down, no keys: open - ext = 1024 holds, 1025 does not (step up max(12, -1024) = 12)
    if (!biasedBandFits({1025, 1, 11, -4}, 0, false) || biasedBandFits({1026, 1, 11, -4}, 0, false)) return 18;
    //   step down, row keys of 16 rows: (open - ext) << 4 = 128 << 4 = 0x0800 holds, 129 << 4 does not
    if (!biasedBandFits({129, 1, 11, -4}, 4, true) || biasedBandFits({130, 1, 11, -4}, 4, true)) return 19;
    //   5 ext: 5 x 819 = 4095 holds, 5 x 820 = 4100 does not (open = ext: step down 0; step up 830 / 831)
    if (!biasedBandFits({819, 819, 11, -4}, 0, false) || biasedBandFits({820, 820, 11, -4}, 0, false)) return 20;
    //   min S above the padding score: -1023 holds (step down 1022), -1024 does not (step down 1023 still would)
    if (!biasedBandFits({3, 1, 11, -1023}, 0, false) || biasedBandFits({3, 1, 11, -1024}, 0, false)) return 21;
    // ---- (b) NW / HW / OV of several strips ----
    // zero = 0x0400 + 9 + (Q + 4) + 4 = Q + 1041; NW: above = 12 Q + 56 + 3, + 5 + 11: 13 Q + 1116 < 31744: Q <= 2355
    // HW / OV: above = 11 Q + 4096 + 59, + 16: 12 Q + 5212 < 31744: Q <= 2210
    if (!globalStripsFit(b62, 2355, true) || globalStripsFit(b62, 2356, true)) return 30;
    if (!globalStripsFit(b62, 2210, false) || globalStripsFit(b62, 2211, false)) return 31;
    // open < ext refuses NW only
    if (globalStripsFit({1, 2, 11, -4}, 100, true) || !globalStripsFit({1, 2, 11, -4}, 100, false)) return 32;
    if (globalOneStripFits({1, 2, 11, -4}, 50, true, false) || !globalOneStripFits({1, 2, 11, -4}, 50, false, false)) return 33;
    // ---- (c) the one-strip zero ----
    // 0x0400 + 9 + 68 + 4 = 1105; the batch form (floor 2 ext = 2 < 4) the same; ext = 3: 1024 + 9 + 204 + max(4, 6) = 1243
    if (globalZeroPattern(b62, 64, false) != 1105 || globalZeroPattern(b62, 64, true) != 1105) return 40;
    if (globalZeroPattern({3, 3, 11, -4}, 64, false) != 1241 || globalZeroPattern({3, 3, 11, -4}, 64, true) != 1243) return 41;
    // 1105 + 64 x 12 + 4096 + 5 + 11 + 68 + 3 = 6056 < 31744
    if (!globalOneStripFits(b62, 64, true, false) || !globalOneStripFits(b62, 64, false, true)) return 42;
    // 5 ext beyond the rebase shift, min S at the padding score: refused in every mode
    if (globalOneStripFits({820, 820, 11, -4}, 8, false, false) || globalOneStripFits({3, 1, 11, -1024}, 8, false, false)) return 43;
    // ---- (d) the 32-bit bound ----
    // 2 x 3 + (53 + 1000) + 53 x 11 + 11 = 1653; the signs of the gap costs do not matter (llabs, as miopalSearch had it)
    if (int32Bound(b62, 53, 1000) != 1653 || int32Bound({-3, -1, 11, -4}, 53, 1000) != 1653) return 50;
    // scores of 0, ext 1: the bound is Q + L; 2^29 - 1 fits, 2^29 does not
    if (!int32Fits(int32Bound({0, 1, 0, 0}, 1, (1ll << 29) - 2)) || int32Fits(int32Bound({0, 1, 0, 0}, 1, (1ll << 29) - 1))) return 51;
    if (int32Bound({0, 1, 0, 0}, 1, (1ll << 29) - 1) != kInt32Safe) return 52;
    // |min S| counts where it is the larger: 6 + 20 + 10 x 30 + 30
    if (int32Bound({3, 1, 11, -30}, 10, 10) != 356) return 53;
    // every other term of the bound alone, one unit inside and one outside (52 is ext's row), Q = 1, L = 1:
    //   2 open: 2 x (2^28 - 1) = 2^29 - 2 fits, 2 x 2^28 does not
    if (!int32Fits(int32Bound({(1 << 28) - 1, 0, 0, 0}, 1, 1)) || int32Fits(int32Bound({1 << 28, 0, 0, 0}, 1, 1))) return 54;
    //   min(Q, L) mag + mag, the largest score: 2 x (2^28 - 1) fits, 2 x 2^28 does not; and the lowest, by its magnitude
    if (!int32Fits(int32Bound({0, 0, (1 << 28) - 1, 0}, 1, 1)) || int32Fits(int32Bound({0, 0, 1 << 28, 0}, 1, 1))) return 55;
    if (!int32Fits(int32Bound({0, 0, 0, -(1 << 28) + 1}, 1, 1)) || int32Fits(int32Bound({0, 0, 0, -(1 << 28)}, 1, 1))) return 56;
    //   min(Q, L) counts the shorter side: mag 2^19 at Q = 1023 against L = 2000 is 2^29 exactly, at Q = 1022 2^19 less;
    //   and it is the target that is the shorter side when the query is long
    if (int32Bound({0, 0, 1 << 19, 0}, 1023, 2000) != kInt32Safe || !int32Fits(int32Bound({0, 0, 1 << 19, 0}, 1022, 2000))) return 57;
    if (int32Bound({0, 0, 1 << 19, 0}, 2000, 1023) != kInt32Safe || !int32Fits(int32Bound({0, 0, 1 << 19, 0}, 2000, 1022))) return 58;
    //   (Q + L) ext counts both sides: ext 2^19, Q + L = 1024 is 2^29 exactly, one row less fits
    if (int32Bound({0, 1 << 19, 0, 0}, 24, 1000) != kInt32Safe || !int32Fits(int32Bound({0, 1 << 19, 0, 0}, 23, 1000))) return 59;
    // ---- (e) NW / HW / OV in the general kernel, Q = 53 ----
    // plain: 9 + 53 + L < 32000: L <= 31937 (53 x 11 = 583 is far below)
    if (!fitsPlain(b62, 53, 31937) || fitsPlain(b62, 53, 31938) || fitsPlain(b62, 53, 0)) return 60;
    // shifted: 583 + 53 + L < 32000: L <= 31363 (9 + 55 + L < 32000 allows more)
    if (!fitsDiag(b62, 53, 31363) || fitsDiag(b62, 53, 31364) || fitsDiag(b62, 53, 0)) return 61;
    // unsigned: 4096 + 583 + (55 + L) + 11 + 2 + 2 < 31744: L <= 26994
    if (!fitsUnsigned(b62, 53, 26994) || fitsUnsigned(b62, 53, 26995) || fitsUnsigned(b62, 53, 0)) return 62;
    // its model: open >= ext, min S + ext + open = 0 >= 0, 0x0400 + (9 + 2 + 4 + 2) + 64 <= 0x1000
    if (!unsignedDiagUsable(b62) || unsignedDiagUsable({3, 1, 11, -5}) || unsignedDiagUsable({1, 2, 11, -3})) return 63;
    // ---- the rest ----
    {
        // every residue with its best partner, nothing below 0: rows (1, -1), (-2, -3), (1, -1)
        const int matrix[4] = {1, -1, -2, -3};
        const unsigned char query[3] = {0, 1, 0};
        if (queryBest(3, 2, [&](int i, int t) { return matrix[query[i] * 2 + t]; }) != 2) return 70;
        if (queryBest(0, 2, [&](int, int) { return 5; }) != 0) return 71;
    }
    {
        // strips: tables of up to 44 rows fit
        auto fits = [](int rows, int) { return rows <= 44; };
        if (tallestStrip(52, 25, fits) != 44 || tallestStrip(40, 25, fits) != 40) return 72;
        if (tallestStrip(52, 25, [](int, int) { return false; }) >= 32) return 73;
        if (pairTableRows(53) != 54 || pairTableRows(64) != 64 || pairTableRows(0) != 2) return 74;
        if (!oneStripFits(44, 25, fits) || oneStripFits(45, 25, fits) || oneStripFits(65, 25, [](int, int) { return true; })) return 75;
    }
    {
        // column-shifted Smith-Waterman: bias 3 (-(-4 + 1)), limit 0x7C00 - 0x1000 - (1000 + 8) = 26640
        const SwShiftPlan s = swShiftPlan(b62, 1000);
        if (!s.usable || s.bias != 3 || s.limit != 26640) return 76;
        // 27648 - (23541 + 8) = 4099 is worth having, 4095 (four columns more) is not; the bias is told either way
        if (!swShiftPlan(b62, 23541).usable || swShiftPlan(b62, 23545).usable || swShiftPlan(b62, 23545).bias != 3) return 77;
    }
    // half floats: min(Q, L) x 11 below 60000: 5454 x 11 = 59994, 5455 x 11 = 60005; scores within +-1024
    if (!halfFloatFits(b62, 5454, 6000) || halfFloatFits(b62, 5455, 6000) || !halfFloatFits(b62, 6000, 53)) return 78;
    if (halfFloatFits({3, 1, 1025, -4}, 10, 10) || halfFloatFits({3, 1, 11, -1025}, 10, 10)) return 79;
    return 0;
}

}  // namespace miopal
