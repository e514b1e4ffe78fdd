// Query-anchored profile columns from the alignments of a pair list (profile_columns.hip): the members' rows are
// projected from the walk's operation slots on the device, then counted and weighted in integers. miopalProfileColumns
// and its PSSM form run the kernels on what alignPairsImpl leaves in HBM (host_profile.inc); only the [Q][A + 1] tables
// and one weight per member cross PCIe.
//
// The multiple alignment: msa[member][Q] bytes, member 0 the query. An entry is a letter (< A), the gap letter (A) or
// 255, not covered. Per column i: counts[i][a] members with letter a (a <= A); k_i letters a < A that occur;
// term[i][a] = floor(2^32 / (k_i counts[i][a])) for the letters that occur, 0 otherwise and for the gap;
// memberWeight[s] = the sum of term[i][msa[s][i]] over the rows with a letter (Henikoff position-based weights,
// 32.32 fixed point); weighted[i][a] = the sum of memberWeight[s] over the members with msa[s][i] == a (a <= A).
// Integer sums: the same in any order. No sum exceeds Q * 2^32.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace miopal {

constexpr uint8_t kProfileUncovered = 255;
constexpr int kProfileSpan = 128;   // members a wavefront of the count / weighted kernels takes

// What the walk of a chunk of a pair list left (alignPairsImpl): slot k of `slots` holds the operations of the chunk's
// pair k, filled from the back - they begin at (k + 1) * slotOps - opsLen[k] - and start at cell (startQ[k], startT[k])
// of the pair; the target's residues begin at residues[tOff[k]]. member[k]: the row of `msa` pair k fills.
struct ProjectArgs {
    const uint8_t* slots;
    int64_t slotOps;
    const int32_t* opsLen;
    const int32_t* startQ;
    const int32_t* startT;
    const int64_t* tOff;
    const int64_t* member;
    int nPairs;
    const uint8_t* residues;
    int64_t residueCount;
    uint8_t* msa;            // [members][Q], every row of a pair all kProfileUncovered before the launch
    int queryLength;
    int alphabet;
};
hipError_t launchProfileProject(const ProjectArgs& a, hipStream_t stream);

// bytes of the scratch of launchProfileColumns (the terms)
inline size_t profileScratchBytes(int queryLength, int alphabet) {
    return sizeof(int64_t) * (size_t)queryLength * (size_t)(alphabet + 1);
}
// counts, weighted: [Q][A + 1], zero-filled before the launch; memberWeight: [members]; all device. Count, terms,
// member weights and weighted columns, one after the other on `stream`.
hipError_t launchProfileColumns(const uint8_t* msa, int64_t members, int queryLength, int alphabet, int64_t* counts,
                                int64_t* weighted, int64_t* memberWeight, void* scratch, hipStream_t stream);

}  // namespace miopal
