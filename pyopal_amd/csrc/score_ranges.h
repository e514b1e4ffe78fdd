// The range model of the host router: whether a scoring model fits a kernel's number range, and with which limit.
// One copy of every rule, for miopalSearch (host_search.inc), the batch path (host_batch.inc: "the answer miopalSearch
// gives for that query alone"), the pair lists (host_pairs.inc), the alignment passes (host_full.inc) and the PSSM
// entry points. Host only, pure functions: no HIP runtime call, no workspace, no view, no globals - what is defined
// in a .hip file (interseqPairFits) comes in as a callable. score_ranges_selftest.h checks it on the CPU
// (miopalSelfTest(4), tools/score_ranges_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include "../../include/opal.h"
#include "common.h"

namespace miopal {

// what every rule below reads of a scoring system: the gap costs and the extreme substitution scores
struct ScoreModel {
    int open, ext, maxScore, minScore;
};

// ---- mode -> border / answer rules ------------------------------------------------------------------------------
inline bool rulesForMode(int mode, DpRules* r) {   // false: no such mode
    switch (mode) {
        case OPAL_MODE_NW: *r = {1, 1, 0, kLastCell}; return true;
        case OPAL_MODE_HW: *r = {0, 1, 0, kLastRow}; return true;
        case OPAL_MODE_OV: *r = {0, 0, 0, kLastRowCol}; return true;
        case OPAL_MODE_SW: *r = {0, 0, 1, kAllCells}; return true;
    }
    return false;
}

// ---- the 32-bit kernels ---------------------------------------------------------------------------------------
// Conservative range check for the 32-bit kernels (the reference returns
// OPAL_ERR_OVERFLOW when its widest lanes overflow, pyx.in:104-105).
// (miopalSearch and the pair lists took the gap costs' magnitudes, the batch path the costs as they are, after
// refusing negative ones: one form, the same answer wherever the batch path got to)
constexpr int64_t kInt32Safe = 1ll << 29;
inline int64_t int32Bound(const ScoreModel& m, int64_t Q, int64_t maxLen) {
    const int64_t mag = std::max<int64_t>(std::llabs((long long)m.maxScore), std::llabs((long long)m.minScore));
    return 2 * (int64_t)std::llabs((long long)m.open) + (Q + maxLen) * std::llabs((long long)m.ext) +
           std::min<int64_t>(Q, maxLen) * mag + mag;
}
inline bool int32Fits(int64_t bound) { return bound < kInt32Safe; }

// ---- the query's own best -------------------------------------------------------------------------------------
// every residue is aligned at most once, at best with its most favourable partner; at(i, t) = the score of query
// position i against residue t (a matrix indexed by the query's residues, or the rows of a PSSM)
template <typename At>
inline int64_t queryBest(int Q, int A, At&& at) {
    int64_t best = 0;
    for (int i = 0; i < Q; ++i) {
        int rowMax = 0;
        for (int t = 0; t < A; ++t) rowMax = std::max(rowMax, (int)at(i, t));
        best += rowMax;
    }
    return best;
}

// ---- Smith-Waterman on biased integer halves (pair-table kernels) ------------------------------------------------
// The biased halves are exact below 25600 (interseq_impl.h) when the scores and gap costs leave the guard band alone:
// a step up (score + ext, or ext - open) of at most 0x0400 so that a finite half cannot jump over the NaN patterns,
// a step down (score + ext, open - ext) within the room below zero. With end locations every value is scaled by
// 2^bits (row keys in the low bits: bits = locRowBitsHost(rows of the strip), 0 without row keys).
inline int64_t stepUp(const ScoreModel& m) { return std::max<int64_t>((int64_t)m.maxScore + m.ext, (int64_t)m.ext - m.open); }
inline int64_t stepDown(const ScoreModel& m) { return std::max<int64_t>(-((int64_t)m.minScore + m.ext), (int64_t)m.open - m.ext); }
inline int rowKeyBits(int rows, bool rowKeys) { return rowKeys ? locRowBitsHost(rows) : 0; }
inline bool biasedBandFits(const ScoreModel& m, int bits, bool rowKeys) {
    return (stepUp(m) << bits) <= kBiasedMaxStepUp && (stepDown(m) << bits) <= (rowKeys ? kLocGuardBand : kBiasedMaxMagnitude) &&
           5 * ((int64_t)m.ext << bits) <= kLocMaxShift && m.minScore > kBiasedPad;
}
// (A step up of more than 0x0400 could carry a finite half past the NaN patterns, 0x7C00 to
// 0x7FFF, into the negative ones, where the max would drop it: the limit is then lowered
// by the excess, so that the cell it would jump from is itself flagged.)
inline int biasedLimit(const ScoreModel& m, int bits, bool rowKeys) {
    return (int)(((rowKeys ? 0x7C00 - kLocZeroPattern - kLocMaxShift : kBiasedScoreLimit) -
                  std::max<int64_t>(0, (stepUp(m) << bits) - 0x0400)) >> bits);
}

// ---- NW / HW / OV on biased integer halves (pair-table kernels) --------------------------------------------------
// The true values around a pattern's zero are bounded by the query, not by the targets' lengths, so no target is
// redone at 32 bit; the bounds are static:
//   below zero: 3 open + (rows + 4) ext + |min S|,   above: rows (max S + ext) + the rebase shift
// `rows`: the query's length on the single-query path; the batch path passes the row class (padding rows included),
// whose padding rows score -2 ext, which the room below zero covers as well (padFloor).
inline int64_t globalZeroPattern(const ScoreModel& m, int64_t rows, bool padFloor) {
    return 0x0400 + 3 * (int64_t)m.open + (rows + 4) * m.ext +
           std::max<int64_t>({0, -(int64_t)m.minScore, padFloor ? 2 * (int64_t)m.ext : 0});
}
inline bool globalModelFits(const ScoreModel& m, bool topGap) {   // what both kernels ask of the model alone
    return m.minScore > kBiasedPad && (topGap ? m.open >= m.ext : true) && 5 * (int64_t)m.ext <= kLocMaxShift;
}
// the one-strip kernel
inline bool globalOneStripFits(const ScoreModel& m, int64_t rows, bool topGap, bool padFloor) {
    const int64_t pos = std::max(m.maxScore, 0);
    // (+ the strip's rows and an opening: the cells are on anti-diagonally shifted scales, round 3)
    return globalModelFits(m, topGap) &&
           globalZeroPattern(m, rows, padFloor) + rows * (pos + m.ext) + kLocMaxShift + 5 * (int64_t)m.ext + pos +
                   (rows + 4) * m.ext + m.open < 0x7C00;
}
// the multi-strip kernel (all of the query: the strips share one scale):
//   above: NW Q (max S + ext), HW / OV Q max S + the rebase shift.
// (the cells of a strip are on anti-diagonally shifted scales - row r carries r ext more - and H is
// kept open - ext below its plain form: one strip's rows and an opening more on either side; the
// kernel's zero is the one-strip kernel's, which has this room below it: 3 open cover 2)
inline bool globalStripsFit(const ScoreModel& m, int64_t Q, bool topGap) {
    const int64_t pos = std::max(m.maxScore, 0);
    const int64_t above = (topGap ? Q * (pos + m.ext) : Q * pos + kLocMaxShift) + ((int64_t)kPairStripsMaxRows + 4) * m.ext + m.open;
    return globalModelFits(m, topGap) && globalZeroPattern(m, Q, false) + above + 5 * (int64_t)m.ext + pos < 0x7C00;
}

// ---- strips of the pair-table kernels ----------------------------------------------------------------------------
// fits(rows, nSymbols): does a pair table of that many rows fit LDS (interseqPairFits)
inline int pairTableRows(int Q) { return std::max(2, (Q + 1) / 2 * 2); }   // (the NW / HW / OV kernel sweeps rows in pairs)
template <typename Fits>
inline bool oneStripFits(int Q, int nSymbols, Fits&& fits) {
    return Q <= kLanes && fits(pairTableRows(Q), nSymbols);
}
// the tallest strip (even, at most maxRows) whose table fits; below 32: none
template <typename Fits>
inline int tallestStrip(int maxRows, int nSymbols, Fits&& fits) {
    while (maxRows >= 32 && !fits(maxRows, nSymbols)) maxRows -= 2;
    return maxRows;
}

// ---- Smith-Waterman scores in the general kernel -----------------------------------------------------------------
// column-shifted unsigned patterns (ArithSwU16) when the longest packed target leaves a range worth having -
// zero + ext x columns + score below 0x7C00
struct SwShiftPlan {
    bool usable = false;
    int bias = 0;    // profile entries s + ext + bias >= 0
    int limit = 0;
};
inline SwShiftPlan swShiftPlan(const ScoreModel& m, int64_t maxPackedLen) {
    SwShiftPlan s;
    s.bias = std::max(0, -(m.minScore + m.ext));
    const int64_t up = stepUp(m);
    const int64_t lim = 0x7C00 - kSwShiftZero - (int64_t)m.ext * (maxPackedLen + 8) - std::max<int64_t>(0, up - 0x0400);
    if (lim >= 4096 && s.bias + m.ext <= 0x0800 && m.open - m.ext <= 0x0800 && up <= 0x1000 &&
        (int64_t)m.maxScore + m.ext + s.bias < 0x4000) {
        s.usable = true;
        s.limit = (int)lim;
    }
    return s;
}
// Half floats turn a sum above 65504 into +inf, and inf + (-inf padding) into NaN, which
// the flag `best >= 2048` would miss (NaN converts to 0): only matrices whose best
// possible score stays finite take the half-float rung.
inline bool halfFloatFits(const ScoreModel& m, int64_t Q, int64_t maxLen) {
    return m.maxScore <= 1024 && m.minScore >= -1024 && std::min<int64_t>(Q, maxLen) * std::max(m.maxScore, 0) < 60000;
}

// ---- NW / HW / OV in the general kernel: whether a target of L columns fits the signed int16 lanes --------------
//   every true H, E, F >= -(3*open + (Q + L)*ext)   and   H <= min(Q, L)*maxScore
inline bool fitsPlain(const ScoreModel& m, int64_t Q, int64_t L) {
    const int64_t pos = std::max(m.maxScore, 0);
    return L > 0 && 3 * (int64_t)m.open + (Q + L) * m.ext < 32000 && std::min<int64_t>(Q, L) * pos < 32000;
}
// the shifted flavour stores X + (i + j) * ext: (Q + L) * ext more head-room
inline bool fitsDiag(const ScoreModel& m, int64_t Q, int64_t L) {
    const int64_t pos = std::max(m.maxScore, 0);
    return L > 0 && 3 * (int64_t)m.open + (Q + L + 2) * m.ext < 32000 && std::min<int64_t>(Q, L) * pos + (Q + L) * m.ext < 32000;
}
// The same shift on unsigned patterns compared as half floats (ArithU16Diag: integer
// adds, one max3 for h): scores after the shift must not be negative
// (s + ext + open >= 0), open >= ext, and every pattern
// zero + x + (i + j) ext within [0, 0x7BFF] for the longest target that stays packed.
inline bool unsignedDiagUsable(const ScoreModel& m) {
    const int64_t c = (int64_t)m.open - m.ext;
    const int64_t below = 3 * (int64_t)m.open + 2 * (int64_t)m.ext + std::max(0, -m.minScore) + c;
    return c >= 0 && (int64_t)m.minScore + m.ext + m.open >= 0 &&
           0x0400 + below + 64 <= kUnsignedDiagZero;   // real cells stay above the padding cells' floor
}
inline bool fitsUnsigned(const ScoreModel& m, int64_t Q, int64_t L) {
    const int64_t pos = std::max(m.maxScore, 0), c = (int64_t)m.open - m.ext;
    return L > 0 && kUnsignedDiagZero + std::min<int64_t>(Q, L) * pos + (Q + L + 2) * (int64_t)m.ext + pos + 2 * (int64_t)m.ext + c < 0x7C00;
}

}  // namespace miopal
