// Dispatcher of the inter-sequence kernel flavours (kernels: interseq_impl.h).
#include "common.h"

namespace miopal {

template <bool LOC>
static hipError_t launchInterseqAs(const InterseqArgs& a, int rowsPerStrip, int waves, InterseqFlavour flavour, hipStream_t stream) {
    switch (flavour) {
        case kSwHalf: return launchFlavour<ArithSwF16, true, LOC>(a, rowsPerStrip, waves, stream);
        case kSwInt16: return launchFlavour<ArithSwI16, true, LOC>(a, rowsPerStrip, waves, stream);
        case kSignedInt16: return launchFlavour<ArithI16, false, LOC>(a, rowsPerStrip, waves, stream);
        case kSignedInt16AllCells: return launchFlavour<ArithI16, true, LOC>(a, rowsPerStrip, waves, stream);
        case kSignedInt16Diag: return launchFlavour<ArithI16Diag, false, LOC>(a, rowsPerStrip, waves, stream);
        case kUnsignedDiag: return launchFlavour<ArithU16Diag, false, LOC>(a, rowsPerStrip, waves, stream);
        case kSwShifted:   // scores only
            if constexpr (!LOC) return launchFlavour<ArithSwU16, true, false>(a, rowsPerStrip, waves, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launchInterseq(const InterseqArgs& a, int rowsPerStrip, int waves, InterseqFlavour flavour,
                          bool locate, hipStream_t stream) {
    if (a.nGroups <= 0) return hipSuccess;
    return locate ? launchInterseqAs<true>(a, rowsPerStrip, waves, flavour, stream)
                  : launchInterseqAs<false>(a, rowsPerStrip, waves, flavour, stream);
}

bool interseqPairFits(int rowsPerStrip, int nSymbols) {
    return pairLdsBytes(rowsPerStrip, nSymbols) <= 158 * 1024;  // leaves the runtime a little of the 160 KB
}

// The translation units of a pair-table family hold kPairUnitSpan consecutive row counts each (those of one parity),
// the first one from `first` on, kUnits of them: launch(kLo) for the unit that holds `rows`. A count that no unit
// holds ends as hipErrorInvalidValue, here or in the unit's own dispatch (the wrong parity, above a family's maximum).
template <int first, int kUnits, typename Launch>
static hipError_t inUnitOf(int rows, Launch&& launch) {
    return dispatchRows<first, kPairUnitSpan, kUnits>(first + (rows - first) / kPairUnitSpan * kPairUnitSpan, launch);
}

hipError_t launchInterseqPair(const InterseqArgs& a, int rowsPerStrip, PairFlavour flavour, int computeUnits,
                              hipStream_t stream, bool locate) {
    if (a.nGroups <= 0) return hipSuccess;
    if (locate && flavour != kPairSwBiased && flavour != kPairGlobalBiased && flavour != kPairSwStrips && flavour != kPairGlobalStrips)
        return hipErrorInvalidValue;
    if (a.nStrips != 1 && flavour != kPairSwStrips && flavour != kPairGlobalStrips) return hipErrorInvalidValue;
    const int rows = rowsPerStrip;
    constexpr int kStripUnits = (kPairStripsMaxRows - kPairStripsFirst) / kPairUnitSpan + 1;
    switch (flavour) {
        case kPairGlobalBiased:
            // even counts 2..64 (end locations are a run-time option of this kernel: a.endI != nullptr)
            return inUnitOf<2, 4>(rows, [&](auto lo) { return launchPairGlobal<lo>(a, rows, computeUnits, stream); });
        case kPairSwBiased: {
            // 1..64 rows: the query's length, odd ones included (a padding row is 1 / Q of the work)
            auto launch = [&](auto lo) {
                return locate ? launchPairBiased<lo, true>(a, rows, computeUnits, stream)
                              : launchPairBiased<lo, false>(a, rows, computeUnits, stream);
            };
            return (rows & 1) ? inUnitOf<1, 4>(rows, launch) : inUnitOf<2, 4>(rows, launch);
        }
        case kPairSwStrips:
            // even counts kPairStripsFirst..kPairStripsMaxRows (..MaxRowsLoc with end locations)
            if (a.known) {
                // (second pass of an `end` search: the known optimum is looked for, no row keys; ..MaxRowsKnown)
                if (locate) return hipErrorInvalidValue;
                return inUnitOf<kPairStripsFirst, 1>(rows, [&](auto lo) { return launchPairStrips<lo, false, true>(a, rows, computeUnits, stream); });
            }
            return inUnitOf<kPairStripsFirst, kStripUnits>(rows, [&](auto lo) {
                return locate ? launchPairStrips<lo, true>(a, rows, computeUnits, stream)
                              : launchPairStrips<lo, false>(a, rows, computeUnits, stream);
            });
        case kPairGlobalStrips:
            // the same counts (end locations leave as keys: decode_global_keys_kernel)
            return inUnitOf<kPairStripsFirst, kStripUnits>(rows, [&](auto lo) {
                return locate ? launchPairGlobalStrips<lo, true>(a, rows, computeUnits, stream)
                              : launchPairGlobalStrips<lo, false>(a, rows, computeUnits, stream);
            });
        case kPairSwHalf: return launchPairFlavour<ArithSwF16>(a, rows, computeUnits, stream);
        case kPairSwInt16: return launchPairFlavour<ArithSwI16>(a, rows, computeUnits, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace miopal
