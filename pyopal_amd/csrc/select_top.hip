// Device selection of the k best entries of score rows (select_top.h). A fixed sequence of launches, no host
// round trip between them:
//   A  range    every (row, block): min and max of its scores -> two integer atomics per block and row
//   B  hist     kTopRounds rounds of (histogram of the row's current range in 4096 LDS bins, summed per row
//               with global atomics; one workgroup per row scans it from the top). Round 0 counts [max(min,
//               minScore), max]; when the range spans 4096 or more, the bin that holds the k-th entry is
//               counted again, 12 bits finer, by the next round. A row that is settled skips the later rounds.
//               Result per row: threshold T and tieTake - every entry > T is chosen, and the first tieTake
//               entries == T in index order. (When every entry of the range is chosen, T = lo - 1 and no ties;
//               a range that starts at INT_MIN has no such T and takes its entries == INT_MIN as ties instead.)
//   C  gather   every (row, block) counts its entries > T and == T, takes its offsets from a single-pass
//               scan over the row's blocks in the order they started (look-back), and writes its chosen
//               entries as (score, index) keys: at most k candidates per row, at fixed places.
//   D  sort     one workgroup per row: bitonic sort of the <= k keys in LDS, end locations gathered at the
//               chosen positions only, the row of outputs written.
// Scores are read three times in the common case (A, B round 0, C) with 16-byte loads; the rounds after the
// first read them again only for rows whose range spans 4096 or more.
#include <climits>

#include "select_rows.h"
#include "select_top.h"

namespace miopal {
namespace {

struct TopRow {
    unsigned maxKey, minKey;   // A: order-preserving key of the row's max, complemented key of its min
    int lo, hi, shift;         // the range the next round counts: scores in [lo, hi], bins of 2^shift
    int active;                // 1: the next round is needed
    int need;                  // entries still to choose inside [lo, hi]
    int above;                 // entries chosen above hi
    int T, tieTake, count;     // settled: every score > T and the first tieTake entries == T
    unsigned ticket;           // C: blocks of the row in the order they started
    int pad[4];
};
static_assert(sizeof(TopRow) == 64, "TopRow");

constexpr unsigned long long kFlagAggregate = 1ull << 62, kFlagInclusive = 2ull << 62;
constexpr unsigned long long kCountsMask = (1ull << 62) - 1;
constexpr int kLookbackSpinCap = 1 << 21;   // polls x s_sleep 8 before a block gives up (about half a second)

__device__ inline unsigned orderedKey(int s) { return (unsigned)s ^ 0x80000000u; }
__device__ inline int fromKey(unsigned u) { return (int)(u ^ 0x80000000u); }
__device__ inline int shiftFor(int64_t span) {
    int sh = 0;
    while ((span >> sh) >= kTopBins) ++sh;
    return sh;
}

struct Scratch {
    TopRow* rows;
    unsigned* hist;                 // [rows][kTopBins]
    unsigned long long* status;     // [rows][blocks]
    unsigned long long* cand;       // [rows][k]
    size_t zeroBytes;               // rows, hist and status: zeroed before every sequence
};
inline size_t histOffset(int rows) { return align256(sizeof(TopRow) * (size_t)rows); }
inline size_t statusOffset(int rows) { return histOffset(rows) + align256(sizeof(unsigned) * (size_t)rows * kTopBins); }
inline size_t candOffset(int rows, int64_t stride) {
    return statusOffset(rows) + align256(sizeof(unsigned long long) * (size_t)rows * blocksPerRow(stride));
}
inline Scratch scratchLayout(void* base, int rows, int64_t stride) {
    char* p = (char*)base;
    Scratch s;
    s.rows = (TopRow*)p;
    s.hist = (unsigned*)(p + histOffset(rows));
    s.status = (unsigned long long*)(p + statusOffset(rows));
    s.zeroBytes = candOffset(rows, stride);
    s.cand = (unsigned long long*)(p + s.zeroBytes);
    return s;
}

// the range round `round` counts; false: nothing to count (round 0: no entry reaches minScore)
__device__ inline bool roundRange(const TopRow& t, int round, int minScore, int& lo, int& hi, int& sh) {
    if (round == 0) {
        hi = fromKey(t.maxKey);
        if (hi < minScore) return false;
        lo = max(fromKey(~t.minKey), minScore);
        sh = shiftFor((int64_t)hi - lo);
        return true;
    }
    if (!t.active) return false;
    lo = t.lo;
    hi = t.hi;
    sh = t.shift;
    return true;
}

// ---- A: range --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void top_range_kernel(TopArgs a, Scratch sc, int nb) {
    const int r = blockIdx.x / nb, b = blockIdx.x % nb;
    const RowSpan rs = rowSpan(a.stride, r);
    int lo = INT_MAX, hi = INT_MIN;
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
        if (s < rs.slots) {
            unsigned mask;
            const int4 v = loadSlot(a.score, rs, s, mask);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (mask >> c & 1) {
                    lo = min(lo, lane(v, c));
                    hi = max(hi, lane(v, c));
                }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d));
        hi = max(hi, __shfl_xor(hi, d));
    }
    __shared__ int wlo[kTopThreads / 64], whi[kTopThreads / 64];
    const int w = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) {
        wlo[w] = lo;
        whi[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int x = 1; x < kTopThreads / 64; ++x) {
            lo = min(lo, wlo[x]);
            hi = max(hi, whi[x]);
        }
        if (hi >= lo) {
            atomicMax(&sc.rows[r].maxKey, orderedKey(hi));
            atomicMax(&sc.rows[r].minKey, ~orderedKey(lo));
        }
    }
}

// ---- B: histogram of a round -------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void top_hist_kernel(TopArgs a, Scratch sc, int nb, int round) {
    __shared__ unsigned bins[kTopBins];
    const int r = blockIdx.x / nb, b = blockIdx.x % nb;
    const RowSpan rs = rowSpan(a.stride, r);
    int lo, hi, sh;
    if (!roundRange(sc.rows[r], round, a.minScore, lo, hi, sh)) return;
    if ((int64_t)b * kTopBlockSlots >= rs.slots) return;
    for (int x = threadIdx.x; x < kTopBins; x += kTopThreads) bins[x] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
        if (s < rs.slots) {
            unsigned mask;
            const int4 v = loadSlot(a.score, rs, s, mask);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int x = lane(v, c);
                if ((mask >> c & 1) && x >= lo && x <= hi) atomicAdd(&bins[((unsigned)x - (unsigned)lo) >> sh], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* h = sc.hist + (size_t)r * kTopBins;
    for (int x = threadIdx.x; x < kTopBins; x += kTopThreads)
        if (bins[x]) atomicAdd(h + x, bins[x]);
}

// ---- B: scan of a round (one workgroup per row) ------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void top_scan_kernel(TopArgs a, Scratch sc, int round) {
    constexpr int kPer = kTopBins / kTopThreads;   // bins per thread, consecutive
    __shared__ unsigned suffix[kTopThreads];
    const int r = blockIdx.x;
    TopRow& t = sc.rows[r];
    int lo, hi, sh;
    if (!roundRange(t, round, a.minScore, lo, hi, sh)) {
        if (round == 0 && threadIdx.x == 0) {   // no entry reaches minScore
            t.count = 0;
            t.T = INT_MAX;
            t.tieTake = 0;
            t.active = 0;
        }
        return;
    }
    const int need = round == 0 ? a.k : t.need;
    const int above = round == 0 ? 0 : t.above;
    unsigned* h = sc.hist + (size_t)r * kTopBins + threadIdx.x * kPer;
    unsigned mine[kPer];
    unsigned sum = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        mine[q] = h[q];
        sum += mine[q];
        h[q] = 0;   // (for the next round)
    }
    // inclusive suffix sums over the threads (bins from the top)
    suffix[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kTopThreads; d <<= 1) {
        const unsigned add = threadIdx.x + d < kTopThreads ? suffix[threadIdx.x + d] : 0u;
        __syncthreads();
        suffix[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned total = suffix[0];
    const unsigned over = threadIdx.x + 1 < kTopThreads ? suffix[threadIdx.x + 1] : 0u;   // in the bins above mine
    if (total <= (unsigned)need) {
        // every entry of the range is chosen
        if (threadIdx.x == 0) {
            if (lo > INT_MIN) {
                t.T = lo - 1;
                t.tieTake = 0;
                t.count = above + (int)total;
                t.active = 0;
            } else if (sh == 0) {
                // (no int below INT_MIN: the entries equal to lo - bin 0, this thread's - are taken as ties)
                t.T = lo;
                t.tieTake = (int)mine[0];
                t.count = above + (int)total;
                t.active = 0;
            } else {
                // ... and while bin 0 is wider than one score, the next round counts it again with all of it to
                // choose, which ends here with a smaller shift (0 in the last round)
                const int64_t top = (int64_t)lo + ((int64_t)1 << sh) - 1;
                const int64_t nhi = top < hi ? top : (int64_t)hi;
                t.lo = lo;
                t.hi = (int)nhi;
                t.shift = shiftFor(nhi - lo);
                t.need = (int)mine[0];
                t.above = above + (int)(total - mine[0]);
                t.active = 1;
            }
        }
        return;
    }
    if (!(over < (unsigned)need && (unsigned)need <= over + sum)) return;
    // this thread holds the bin of the need-th entry from the top
    unsigned c = over;
    int bin = threadIdx.x * kPer;
    for (int q = kPer - 1; q >= 0; --q) {
        if (c + mine[q] >= (unsigned)need) {
            bin = threadIdx.x * kPer + q;
            break;
        }
        c += mine[q];
    }
    if (sh == 0) {
        t.T = lo + bin;
        t.tieTake = need - (int)c;
        t.count = above + need;
        t.above = above + (int)c;
        t.active = 0;
    } else {
        const int64_t nlo = (int64_t)lo + ((int64_t)bin << sh);
        const int64_t top = nlo + ((int64_t)1 << sh) - 1;
        const int64_t nhi = top < hi ? top : (int64_t)hi;
        t.lo = (int)nlo;
        t.hi = (int)nhi;
        t.shift = shiftFor(nhi - nlo);
        t.need = need - (int)c;
        t.above = above + (int)c;
        t.active = 1;
    }
}

// ---- C: gather -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopThreads) void top_gather_kernel(TopArgs a, Scratch sc, int nb) {
    __shared__ unsigned ticket;
    __shared__ unsigned waveTot[kTopVecs][kTopThreads / 64][2];
    __shared__ unsigned long long prefix;
    const int r = blockIdx.x / nb;
    const TopRow& t = sc.rows[r];
    const int count = t.count;
    if (count == 0) return;
    const int T = t.T, tieTake = t.tieTake, aboveT = count - tieTake;
    if (threadIdx.x == 0) ticket = atomicAdd(&sc.rows[r].ticket, 1u);
    __syncthreads();
    const unsigned b = ticket;   // blocks take their chunks in the order they started: waits only on earlier ones
    const RowSpan rs = rowSpan(a.stride, r);
    const int w = threadIdx.x / 64;
    int4 v[kTopVecs];
    unsigned mask[kTopVecs], preA[kTopVecs], preT[kTopVecs];
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t s = (int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x;
        mask[i] = 0;
        v[i] = make_int4(0, 0, 0, 0);
        if (s < rs.slots) v[i] = loadSlot(a.score, rs, s, mask[i]);
        unsigned ca = 0, ct = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int x = lane(v[i], c);
            ca += (mask[i] >> c & 1) && x > T;
            ct += (mask[i] >> c & 1) && x == T;
        }
        // (both counts in one scan: at most 256 per wavefront, 16 bits each)
        unsigned pre, tot;
        wavePrefix(ca | ct << 16, pre, tot);
        preA[i] = pre & 0xFFFF;
        preT[i] = pre >> 16;
        if (threadIdx.x % 64 == 0) {
            waveTot[i][w][0] = tot & 0xFFFF;
            waveTot[i][w][1] = tot >> 16;
        }
    }
    __syncthreads();
    // offsets of this thread's entries inside the block (order: load i, then wavefront, then lane)
    unsigned totA = 0, totT = 0;
    unsigned baseA[kTopVecs], baseT[kTopVecs];
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        for (int x = 0; x < kTopThreads / 64; ++x) {
            if (x == w) {
                baseA[i] = totA;
                baseT[i] = totT;
            }
            totA += waveTot[i][x][0];
            totT += waveTot[i][x][1];
        }
    }
    if (threadIdx.x < 64) {
        // look-back over the row's earlier blocks, 64 at a time by the first wavefront: (ties << 31) | above per block,
        // flags in the top two bits (aggregate: the block's own counts, inclusive: everything up to it)
        const int ln = threadIdx.x;
        unsigned long long* st = sc.status + (size_t)r * nb;
        const unsigned long long mine = ((unsigned long long)totT << 31) | totA;
        if (b > 0 && ln == 0) __hip_atomic_store(st + b, kFlagAggregate | mine, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        unsigned accA = 0, accT = 0;
        int spins = 0;
        for (int j = (int)b - 1; j >= 0;) {
            const int idx = j - ln;   // (lanes before block 0 read as an inclusive zero)
            const unsigned long long x =
                idx >= 0 ? __hip_atomic_load(st + idx, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) : kFlagInclusive;
            const unsigned long long inc = __ballot((x & ~kCountsMask) == kFlagInclusive);
            const int last = inc ? __builtin_ctzll(inc) : 63;   // lanes 0 .. last are summed
            const unsigned long long upTo = last == 63 ? ~0ull : (2ull << last) - 1;
            if (__ballot((x & ~kCountsMask) == 0) & upTo) {
                if (++spins > kLookbackSpinCap) {
                    if (ln == 0) atomicAdd(a.error, 1);
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
                continue;
            }
            unsigned ca = ln <= last ? (unsigned)(x & 0x7FFFFFFFu) : 0u;
            unsigned ct = ln <= last ? (unsigned)((x >> 31) & 0x7FFFFFFFu) : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                ca += __shfl_xor(ca, d);
                ct += __shfl_xor(ct, d);
            }
            accA += ca;
            accT += ct;
            if (inc) break;
            j -= 64;
        }
        const unsigned long long acc = ((unsigned long long)accT << 31) | accA;
        if (ln == 0) {
            __hip_atomic_store(st + b, kFlagInclusive | (acc + mine), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            prefix = acc;
        }
    }
    __syncthreads();
    const unsigned exA = (unsigned)(prefix & 0x7FFFFFFFu), exT = (unsigned)(prefix >> 31);
    unsigned long long* cand = sc.cand + (size_t)r * a.k;
#pragma unroll
    for (int i = 0; i < kTopVecs; ++i) {
        const int64_t e = rs.a0 + 4 * ((int64_t)b * kTopBlockSlots + i * kTopThreads + threadIdx.x) - rs.first;
        unsigned pa = exA + baseA[i] + preA[i], pt = exT + baseT[i] + preT[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int x = lane(v[i], c);
            if (!(mask[i] >> c & 1)) continue;
            const unsigned long long key = ((unsigned long long)~orderedKey(x) << 32) | (unsigned)(e + c);
            if (x > T) {
                if (pa < (unsigned)aboveT) cand[pa] = key;
                ++pa;
            } else if (x == T) {
                if (pt < (unsigned)tieTake) cand[aboveT + pt] = key;
                ++pt;
            }
        }
    }
}

// ---- D: sort and write (one workgroup per row) ------------------------------------------------------------------
constexpr int kSortThreads = 1024;
__global__ __launch_bounds__(kSortThreads) void top_sort_kernel(TopArgs a, Scratch sc, int r0) {
    __shared__ unsigned long long keys[kTopMaxK];
    const int r = blockIdx.x;
    const int count = sc.rows[r].count;
    int P = 1;
    while (P < count) P <<= 1;
    const unsigned long long* cand = sc.cand + (size_t)r * a.k;
    for (int x = threadIdx.x; x < P; x += kSortThreads) keys[x] = x < count ? cand[x] : ~0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = threadIdx.x; x < P / 2; x += kSortThreads) {
                const int i = 2 * x - (x & (stride - 1));
                const int j = i + stride;
                const unsigned long long ki = keys[i], kj = keys[j];
                if ((ki > kj) == ((i & size) == 0)) {
                    keys[i] = kj;
                    keys[j] = ki;
                }
            }
            __syncthreads();
        }
    }
    const int row = r0 + r;
    const size_t out = (size_t)row * a.k;
    const int32_t* endI = a.endI ? a.endI + (size_t)r * a.stride : nullptr;
    const int32_t* endJ = a.endJ ? a.endJ + (size_t)r * a.stride : nullptr;
    for (int x = threadIdx.x; x < a.k; x += kSortThreads) {
        if (x < count) {
            const unsigned long long key = keys[x];
            const unsigned idx = (unsigned)key;
            a.target[out + x] = a.start + idx;
            a.outScore[out + x] = fromKey(~(unsigned)(key >> 32));
            if (a.outEndQ) {
                a.outEndQ[out + x] = endI[idx];
                a.outEndT[out + x] = endJ[idx];
            }
        } else {
            a.target[out + x] = -1;
            a.outScore[out + x] = -1;
            if (a.outEndQ) {
                a.outEndQ[out + x] = -1;
                a.outEndT[out + x] = -1;
            }
        }
    }
    if (threadIdx.x == 0) a.count[row] = count;
}

}  // namespace

size_t topScratchBytes(int rows, int64_t stride, int k) {
    rows = rows < kTopRowsPerLaunch ? rows : kTopRowsPerLaunch;
    return candOffset(rows, stride) + align256(sizeof(unsigned long long) * (size_t)rows * k);
}

hipError_t launchSelectTop(const TopArgs& full, hipStream_t stream) {
    if (full.rows <= 0 || full.k <= 0 || full.k > kTopMaxK || full.stride <= 0) return hipErrorInvalidValue;
    const int nb = blocksPerRow(full.stride);
    for (int r0 = 0; r0 < full.rows; r0 += kTopRowsPerLaunch) {
        TopArgs a = full;
        a.rows = full.rows - r0 < kTopRowsPerLaunch ? full.rows - r0 : kTopRowsPerLaunch;
        a.score = full.score + (size_t)r0 * full.stride;
        if (full.endI) {
            a.endI = full.endI + (size_t)r0 * full.stride;
            a.endJ = full.endJ + (size_t)r0 * full.stride;
        }
        const Scratch sc = scratchLayout(full.scratch, a.rows, a.stride);
        hipError_t e = hipMemsetAsync(full.scratch, 0, sc.zeroBytes, stream);
        if (e != hipSuccess) return e;
        const unsigned grid = (unsigned)a.rows * (unsigned)nb;
        top_range_kernel<<<grid, kTopThreads, 0, stream>>>(a, sc, nb);
        for (int round = 0; round < kTopRounds; ++round) {
            top_hist_kernel<<<grid, kTopThreads, 0, stream>>>(a, sc, nb, round);
            top_scan_kernel<<<a.rows, kTopThreads, 0, stream>>>(a, sc, round);
        }
        top_gather_kernel<<<grid, kTopThreads, 0, stream>>>(a, sc, nb);
        top_sort_kernel<<<a.rows, kSortThreads, 0, stream>>>(a, sc, r0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace miopal
