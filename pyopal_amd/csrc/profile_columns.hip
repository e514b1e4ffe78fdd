// Member rows from operation slots, and the counted and weighted columns of the multiple alignment they form
// (profile_columns.h).
//   profile_project   one wavefront per pair of a chunk: 64 operations a step, the row and the target residue of each
//                     from a ballot / popcount prefix over "consumes a query row" / "consumes a target residue"
//   columns_count     a lane owns a column, a wavefront 64 columns x kProfileSpan members: [letter][lane] counters in
//                     LDS that no two lanes share, then one 64-bit atomicAdd per non-zero (column, letter)
//   columns_terms     one thread per (column, letter): k_i of the column and floor(2^32 / (k_i count))
//   member_weights    one wavefront per member: its terms summed over the columns, reduced with shuffles
//   columns_weighted  columns_count with the member's weight in the place of 1 (64-bit counters)
// Integers throughout: the sums are the same in any order.
#include "profile_columns.h"

namespace miopal {
namespace {

typedef unsigned long long u64;

constexpr int kProfileMaxAlphabet = 32;                 // kMaxAlphabet (common.h)
constexpr int kColumnSlots = kProfileMaxAlphabet + 2;   // the letters, the gap, and one slot for what is not counted
constexpr int kWavesPerBlock = 4;                       // profile_project, member_weights: wavefronts side by side

__global__ __launch_bounds__(64 * kWavesPerBlock) void profile_project_kernel(ProjectArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (k >= a.nPairs) return;   // (the whole wavefront)
    const int len = a.opsLen[k];
    if (len <= 0 || len > a.slotOps) return;   // an empty alignment: the row stays uncovered
    const uint8_t* ops = a.slots + ((k + 1) * a.slotOps - len);
    uint8_t* row = a.msa + a.member[k] * (int64_t)a.queryLength;
    int i = a.startQ[k];
    int64_t t = a.tOff[k] + a.startT[k];
    const u64 below = (1ull << lane) - 1;
    for (int base = 0; base < len; base += 64) {
        const int p = base + lane;
        const unsigned op = p < len ? ops[p] : 4u;    // 0 match, 1 deletion, 2 insertion, 3 mismatch (opal.h)
        const bool both = op == 0 || op == 3;
        const bool onQuery = both || op == 1, onTarget = both || op == 2;
        const u64 q = __ballot(onQuery), r = __ballot(onTarget);
        const int ri = i + __popcll(q & below);
        const int64_t ti = t + __popcll(r & below);
        if (onQuery && ri >= 0 && ri < a.queryLength) {
            uint8_t v = (uint8_t)a.alphabet;          // a query residue against a gap
            if (both) v = ti >= 0 && ti < a.residueCount ? a.residues[ti] : kProfileUncovered;
            row[ri] = v;
        }
        i += __popcll(q);
        t += __popcll(r);
    }
}

// The block's 64 columns x its span of members into acc[slot][lane]; a lane touches its own counters only.
template <typename Counter, bool WEIGHTED>
__device__ inline void foldColumns(Counter* acc, const uint8_t* msa, int64_t members, int Q, int A, int colBlocks,
                                   const int64_t* memberWeight, int64_t* out) {
    const int lane = threadIdx.x;
    for (int x = 0; x < A + 2; ++x) acc[x * 64 + lane] = 0;
    const int i = (int)(blockIdx.x % (unsigned)colBlocks) * 64 + lane;
    const int64_t s0 = (int64_t)(blockIdx.x / (unsigned)colBlocks) * kProfileSpan;
    const int64_t s1 = s0 + kProfileSpan < members ? s0 + kProfileSpan : members;
    if (i >= Q) return;
#pragma unroll 4
    for (int64_t s = s0; s < s1; ++s) {
        const int e = msa[s * Q + i];
        const int slot = e <= A ? e : A + 1;
        acc[slot * 64 + lane] += WEIGHTED ? (Counter)memberWeight[s] : (Counter)1;
    }
    for (int x = 0; x <= A; ++x) {
        const Counter c = acc[x * 64 + lane];
        if (c != 0) atomicAdd((u64*)&out[(int64_t)i * (A + 1) + x], (u64)c);
    }
}

__global__ __launch_bounds__(64) void columns_count_kernel(const uint8_t* msa, int64_t members, int Q, int A, int colBlocks,
                                                           int64_t* counts) {
    __shared__ uint32_t acc[kColumnSlots * 64];
    foldColumns<uint32_t, false>(acc, msa, members, Q, A, colBlocks, nullptr, counts);
}

__global__ __launch_bounds__(64) void columns_weighted_kernel(const uint8_t* msa, int64_t members, int Q, int A, int colBlocks,
                                                              const int64_t* memberWeight, int64_t* weighted) {
    __shared__ u64 acc[kColumnSlots * 64];
    foldColumns<u64, true>(acc, msa, members, Q, A, colBlocks, memberWeight, weighted);
}

__global__ __launch_bounds__(256) void columns_terms_kernel(const int64_t* counts, int Q, int A, int64_t* term) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (int64_t)Q * (A + 1)) return;
    const int64_t i = at / (A + 1);
    const int a = (int)(at - i * (A + 1));
    const int64_t* col = counts + i * (A + 1);
    u64 k = 0;
    for (int x = 0; x < A; ++x) k += col[x] > 0 ? 1 : 0;
    const u64 c = (u64)col[a];
    term[at] = a < A && c > 0 ? (int64_t)((1ull << 32) / (k * c)) : 0;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void member_weights_kernel(const uint8_t* msa, int64_t members, int Q, int A,
                                                                             const int64_t* term, int64_t* memberWeight) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (s >= members) return;   // (the whole wavefront)
    const uint8_t* row = msa + s * Q;
    u64 sum = 0;
    for (int i = lane; i < Q; i += 64) {
        const int e = row[i];
        if (e < A) sum += (u64)term[(int64_t)i * (A + 1) + e];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) memberWeight[s] = (int64_t)sum;
}

}  // namespace

hipError_t launchProfileProject(const ProjectArgs& a, hipStream_t stream) {
    if (a.nPairs <= 0) return hipSuccess;
    if (!a.slots || !a.opsLen || !a.startQ || !a.startT || !a.tOff || !a.member || !a.residues || !a.msa ||
        a.slotOps <= 0 || a.queryLength <= 0 || a.alphabet <= 0 || a.alphabet > kProfileMaxAlphabet)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.nPairs + kWavesPerBlock - 1) / kWavesPerBlock);
    profile_project_kernel<<<blocks, 64 * kWavesPerBlock, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launchProfileColumns(const uint8_t* msa, int64_t members, int queryLength, int alphabet, int64_t* counts,
                                int64_t* weighted, int64_t* memberWeight, void* scratch, hipStream_t stream) {
    const int Q = queryLength, A = alphabet;
    if (!msa || !counts || !weighted || !memberWeight || !scratch || members < 1 || Q < 1 || A < 1 ||
        A > kProfileMaxAlphabet)
        return hipErrorInvalidValue;
    const int colBlocks = (Q + 63) / 64;
    const int64_t spans = (members + kProfileSpan - 1) / kProfileSpan;
    const int64_t waves = (members + kWavesPerBlock - 1) / kWavesPerBlock;
    if (spans * colBlocks > INT32_MAX || waves > INT32_MAX) return hipErrorInvalidValue;
    const unsigned foldBlocks = (unsigned)(spans * colBlocks);
    const unsigned termBlocks = (unsigned)(((int64_t)Q * (A + 1) + 255) / 256);
    int64_t* term = (int64_t*)scratch;
    columns_count_kernel<<<foldBlocks, 64, 0, stream>>>(msa, members, Q, A, colBlocks, counts);
    columns_terms_kernel<<<termBlocks, 256, 0, stream>>>(counts, Q, A, term);
    member_weights_kernel<<<(unsigned)waves, 64 * kWavesPerBlock, 0, stream>>>(msa, members, Q, A, term, memberWeight);
    columns_weighted_kernel<<<foldBlocks, 64, 0, stream>>>(msa, members, Q, A, colBlocks, memberWeight, weighted);
    return hipGetLastError();
}

}  // namespace miopal
