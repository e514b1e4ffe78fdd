// Part of host.hip (included there, not a translation unit of its own): per-stream workspace: growable device buffers, the pinned staging buffer, the side stream.
// ---------------------------------------------------------------------------
// per-stream workspace: growable device buffers reused in stream order
// ---------------------------------------------------------------------------
enum Slot {
    kQuery, kMatrix, kProfile, kViewScore, kViewOvf, kCounter, kBoundary0, kBoundary1,
    kScore, kEndI, kEndJ, kJobs, kPairB0, kPairB1, kAuxJobs, kAuxPairB0, kAuxPairB1, kRScore, kRI, kRJ, kDirs, kOps, kOpsOff,
    kOpsLen, kOvfHost, kWorkCounter, kViewEndI, kViewEndJ, kStartQ, kStartT, kMismatch, kCompactOps, kTraceScore, kOpsTotals, kSortBins, kSortedJobs, kScanOrder, kKeys, kHeadWaves, kHeadDirs, kUnitState, kUnitPartial, kStripKeys,
    kPairStripState, kPairStripPartial, kPairStripSpare, kAuxPairStripState, kAuxPairStripPartial, kPairStripError, kStripTiming,
    kBatchProfiles, kBatchMeta, kBatchOverflow,
    // miopalAlignPairs (host_pairs.inc): a chunk's pair list, its pairs' target / query origins, the queries' offsets,
    // and the lane-per-pair kernels' strip boundaries
    kPairListQ, kPairListT, kPairListTOff, kPairListQBase, kPairListQOff, kPairListBoundary,
    kTopScratch,   // miopalSearchTop / miopalSearchBatchTop: the selection's outputs and scratch (rows x (bins + blocks + k))
    // miopalSearchHits and its PSSM and batch forms (host_hits.inc): the compaction's thresholds, counts and offsets
    // (a few bytes per block of 4096 scores), and the written hits, sized to their number
    kHitsScratch, kHitsOut,
    // miopalSearchSignificant and its forms (host_stats.inc): per row the per-bin sums, the ceilings and the thresholds
    kStatsScratch,
    // miopalSearchBatchTargetTop (host_columns.inc): the running state and the answer, in the workspace the call holds
    // throughout; a chunk's skip flags, in the workspace that produced the chunk
    kColumnsState, kColumnsOut, kColumnsSkip,
    kPssmRows,     // miopalSearchPssm: the rows, [Q][A] ints
    kSplitState,   // column split of the one-strip Smith-Waterman kernel: a wavefront's DP state at the cut that starts its interval
    // miopalProfileColumns (host_profile.inc): the multiple alignment and the tables, in the workspace the call holds
    // throughout; a chunk's member indices, in the workspace that produced the chunk
    kProfileMsa, kProfileTables, kProfileMember,
    // column split: the flags of the cuts (epochs: zeroed when allocated, not per launch) and the intervals' plan
    kSplitFlags, kSplitPlan,
    // miopalSearchOccurrences (host_occurrences.inc): per-target counts, offsets and the list of the targets that have
    // occurrences; the written occurrences, sized to their number
    kOccurrenceScratch, kOccurrenceOut,
    // miopalSearchBatchOccurrences (host_batch_occurrences.inc): a chunk's queries and groups; where each query's
    // stretch of the scan's list begins, and the offsets and totals that come down
    kBatchOccurrenceMeta, kBatchOccurrenceBounds,
    // miopalSearchPssmBatchOccurrences: which row of the chunk's PSSM rows (kPssmRows) each table row holds
    kBatchOccurrenceRowSource,
    kSlots
};

// Alignment operations as they cross PCIe - two bits each, operation p in bits 2 (p % 4) of byte p / 4
// (copy_out_packed_kernel) - back into the caller's one byte per operation: operations [from, to) of the
// stream. Whole 16-bit pieces with one `pdep` each where the CPU has it (8 operations an instruction), a
// table otherwise; a few threads side by side for large shares, like the copy this replaces (the pages of
// the caller's buffer are touched here for the first time).
namespace unpack {
#if defined(__x86_64__)
__attribute__((target("bmi2"))) inline void pieces(uint8_t* dst, const uint8_t* packed, int64_t n8) {
    for (int64_t k = 0; k < n8; ++k) {
        uint16_t w;
        memcpy(&w, packed + 2 * k, 2);
        const uint64_t v = __builtin_ia32_pdep_di((uint64_t)w, 0x0303030303030303ull);
        memcpy(dst + 8 * k, &v, 8);
    }
}
inline bool havePdep() {
    static const bool yes = __builtin_cpu_supports("bmi2");
    return yes;
}
// 64 operations an iteration where the CPU has AVX-512 VBMI: eight 16-bit pieces widened to qwords, every byte of a
// qword picked from bit 2k of it by one vpmultishiftqb
// (`stream`: dst is 64-byte aligned and the share is large - non-temporal stores: the caller's buffer is written once,
// front to back, and is larger than the caches; an ordinary store reads every line before it overwrites it)
__attribute__((target("avx512f,avx512bw,avx512vbmi"))) inline void pieces64(uint8_t* dst, const uint8_t* packed, int64_t n64,
                                                                              bool stream) {
    const __m512i from = _mm512_set1_epi64((long long)0x0e0c0a0806040200ull);
    const __m512i low2 = _mm512_set1_epi8(3);
    if (stream) {
        for (int64_t k = 0; k < n64; ++k) {
            const __m128i in = _mm_loadu_si128((const __m128i*)(packed + 16 * k));
            const __m512i spread = _mm512_multishift_epi64_epi8(from, _mm512_cvtepu16_epi64(in));
            _mm512_stream_si512((__m512i*)(dst + 64 * k), _mm512_and_si512(spread, low2));
        }
        _mm_sfence();
        return;
    }
    for (int64_t k = 0; k < n64; ++k) {
        const __m128i in = _mm_loadu_si128((const __m128i*)(packed + 16 * k));
        const __m512i spread = _mm512_multishift_epi64_epi8(from, _mm512_cvtepu16_epi64(in));
        _mm512_storeu_si512((void*)(dst + 64 * k), _mm512_and_si512(spread, low2));
    }
}
inline bool haveVbmi() {
    static const bool yes = __builtin_cpu_supports("avx512vbmi") && __builtin_cpu_supports("avx512bw");
    return yes;
}
#else
inline void pieces(uint8_t*, const uint8_t*, int64_t) {}
inline bool havePdep() { return false; }
inline void pieces64(uint8_t*, const uint8_t*, int64_t, bool) {}
inline bool haveVbmi() { return false; }
#endif
// (the definition, one operation at a time: the self-test's yardstick)
inline void rangePlain(uint8_t* out, const uint8_t* packed, int64_t from, int64_t to) {
    for (int64_t p = from; p < to; ++p) out[p] = (packed[p >> 2] >> (2 * (p & 3))) & 3u;
}
inline void range(uint8_t* out, const uint8_t* packed, int64_t from, int64_t to) {
    int64_t p = from;
    for (; p < to && (p & 7); ++p) out[p] = (packed[p >> 2] >> (2 * (p & 3))) & 3u;
    if (haveVbmi() && to - p >= 64) {
        // (large shares into a buffer whose lines start on multiples of four operations: one by one up to the next
        // 64-byte line of `out`, then whole lines with non-temporal stores)
        const bool stream = to - p >= (1 << 20) && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
        if (stream)
            for (; (reinterpret_cast<uintptr_t>(out + p) & 63) != 0; ++p) out[p] = (packed[p >> 2] >> (2 * (p & 3))) & 3u;
        const int64_t n64 = (to - p) / 64;
        pieces64(out + p, packed + (p >> 2), n64, stream);
        p += 64 * n64;
    }
    const int64_t n8 = (to - p) / 8;
    if (n8 > 0) {
        if (havePdep()) {
            pieces(out + p, packed + (p >> 2), n8);
        } else {
            static const std::vector<uint32_t> table = [] {
                std::vector<uint32_t> t(256);
                for (uint32_t b = 0; b < 256; ++b)
                    t[b] = (b & 3u) | (((b >> 2) & 3u) << 8) | (((b >> 4) & 3u) << 16) | (((b >> 6) & 3u) << 24);
                return t;
            }();
            for (int64_t k = 0; k < 2 * n8; ++k) memcpy(out + p + 4 * k, &table[packed[(p >> 2) + k]], 4);
        }
        p += 8 * n8;
    }
    for (; p < to; ++p) out[p] = (packed[p >> 2] >> (2 * (p & 3))) & 3u;
}
// `out` and `packed` are the bases of the whole streams (operation 0)
// (`most`: threads at most - four beside a device that is still at work, eight for the share that is left
// when it has finished: 2 MB each at least)
inline void ops(uint8_t* out, const uint8_t* packed, int64_t from, int64_t to, int most = 4) {
    const int64_t kPiece = most > 4 ? 2 << 20 : 4 << 20;
    if (to - from < 2 * kPiece) {
        range(out, packed, from, to);
        return;
    }
    const int nThreads = (int)std::min<int64_t>(most, (to - from) / kPiece);
    const int64_t share = (((to - from) / nThreads) + 4095) & ~(int64_t)4095;
    std::vector<std::thread> pool;
    for (int t = 1; t < nThreads; ++t) {
        const int64_t lo = from + share * t, hi = std::min(to, lo + share);
        if (lo >= hi) continue;
        try {
            pool.emplace_back([=] { range(out, packed, lo, hi); });
        } catch (const std::exception&) {   // no thread to be had: this one takes the share
            range(out, packed, lo, hi);
        }
    }
    range(out, packed, from, std::min(to, from + share));
    for (auto& th : pool) th.join();
}
// The same for the share that is left when the device has finished, with the helper threads started BEFOREHAND
// (while the device is still at work) and parked on a condition variable: starting eight threads one after the
// other costs 0.15 ms, a third of what they then do in a cfg3 search.
class Crew {
    std::vector<std::thread> pool;
    std::mutex m;
    std::condition_variable cv;
    bool go = false, cancel = false;
    uint8_t* out = nullptr;
    const uint8_t* packed = nullptr;
    int64_t from = 0, to = 0;
    int members = 1;   // helpers + the caller of run()
    void piece(int t) const {
        const int64_t share = (((to - from + members - 1) / members) + 4095) & ~(int64_t)4095;   // (whole pages; >= 1 page)
        const int64_t lo = from + share * t, hi = std::min(to, lo + share);
        if (lo < hi) range(out, packed, lo, hi);
    }

public:
    explicit Crew(int helpers) {
        pool.reserve((size_t)helpers);   // (emplace_back below can then only throw for the thread itself: no half-built pool of joinable threads)
        for (int t = 1; t <= helpers; ++t) {
            try {
                pool.emplace_back([this, t] {
                    {
                        std::unique_lock<std::mutex> lock(m);
                        cv.wait(lock, [this] { return go || cancel; });
                        if (cancel) return;
                    }
                    piece(t);
                });
                members = t + 1;
            } catch (const std::exception&) {
                break;   // (no thread to be had: the others take its share)
            }
        }
    }
    Crew(const Crew&) = delete;
    Crew& operator=(const Crew&) = delete;
    // operations [from_, to_) of the stream; returns when all of them are in `out_`
    void run(uint8_t* out_, const uint8_t* packed_, int64_t from_, int64_t to_) {
        {
            std::lock_guard<std::mutex> lock(m);
            out = out_;
            packed = packed_;
            from = from_;
            to = to_;
            go = true;
        }
        cv.notify_all();
        piece(0);
        for (auto& th : pool) th.join();
        pool.clear();
    }
    ~Crew() {
        {
            std::lock_guard<std::mutex> lock(m);
            if (!go) cancel = true;
        }
        cv.notify_all();
        for (auto& th : pool)
            if (th.joinable()) th.join();
    }
};
// One helper thread that takes the host's shares of a `full` search - unpacking a batch's operations, copying its
// slices of the per-target arrays - off the thread that feeds the device (round 5: behind the last batch's gather the
// calling thread was still unpacking the batches before it, and the last copy started half a millisecond late).
// Tasks run in the order they were handed in; drain() returns when all of them are done; the destructor drains.
class AsyncWork {
    std::thread th;
    std::mutex m;
    std::condition_variable cv, idleCv;
    std::deque<std::function<void()>> q;
    bool stop = false, busy = false;
    void loop() {
        std::unique_lock<std::mutex> lock(m);
        for (;;) {
            cv.wait(lock, [this] { return stop || !q.empty(); });
            if (q.empty()) return;
            std::function<void()> f = std::move(q.front());
            q.pop_front();
            busy = true;
            lock.unlock();
            f();
            lock.lock();
            busy = false;
            idleCv.notify_all();
        }
    }

public:
    AsyncWork() = default;
    AsyncWork(const AsyncWork&) = delete;
    AsyncWork& operator=(const AsyncWork&) = delete;
    void submit(std::function<void()> f) {
        {
            std::unique_lock<std::mutex> lock(m);
            if (!th.joinable()) {
                try {
                    th = std::thread([this] { loop(); });
                } catch (const std::exception&) {   // no thread to be had: the caller does the work
                    lock.unlock();
                    f();
                    return;
                }
            }
            q.push_back(std::move(f));
        }
        cv.notify_one();
    }
    void drain() {
        std::unique_lock<std::mutex> lock(m);
        idleCv.wait(lock, [this] { return q.empty() && !busy; });
    }
    ~AsyncWork() {
        {
            std::lock_guard<std::mutex> lock(m);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
};
// memcpy of a large piece of results into the caller's memory with non-temporal stores (written once, read by the
// caller later; an ordinary store reads every line first): AVX-512 where the CPU has it, memcpy otherwise
#if defined(__x86_64__)
__attribute__((target("avx512f"))) inline void streamLines(uint8_t* dst, const uint8_t* src, size_t lines) {
    for (size_t k = 0; k < lines; ++k)
        _mm512_stream_si512((__m512i*)(dst + 64 * k), _mm512_loadu_si512((const void*)(src + 64 * k)));
    _mm_sfence();
}
inline bool haveAvx512() {
    static const bool yes = __builtin_cpu_supports("avx512f");
    return yes;
}
#else
inline void streamLines(uint8_t*, const uint8_t*, size_t) {}
inline bool haveAvx512() { return false; }
#endif
inline void copyLarge(void* dst, const void* src, size_t bytes) {
    if (bytes < (256u << 10) || !haveAvx512()) {
        memcpy(dst, src, bytes);
        return;
    }
    uint8_t* d = (uint8_t*)dst;
    const uint8_t* s = (const uint8_t*)src;
    const size_t lead = (64 - (reinterpret_cast<uintptr_t>(d) & 63)) & 63;
    memcpy(d, s, lead);
    const size_t lines = (bytes - lead) / 64;
    streamLines(d + lead, s + lead, lines);
    memcpy(d + lead + 64 * lines, s + lead + 64 * lines, bytes - lead - 64 * lines);
}
}  // namespace unpack

struct Workspace {
    hipStream_t stream = nullptr;
    bool ownsStream = false;
    void* buf[kSlots] = {};
    size_t cap[kSlots] = {};
    // which lease last asked for a slot (trimTo frees what the search that has just ended did NOT use first)
    uint64_t usedBy[kSlots] = {};
    uint64_t leaseStamp = 0;
    // which allocation a slot holds (never 0 once allocated): what a search left in a slot for later searches - the column
    // split's flags and plan - is still there when the number is the one it saw
    uint64_t born[kSlots] = {};
    uint64_t allocations = 0;
    // column split of the one-strip Smith-Waterman kernel (host_search.inc: launchOneStripPair). The flags carry the epoch
    // of the launch that set them, one counter per workspace; the plan in kSplitPlan was made for this view and width
    uint32_t splitEpoch = 0;
    uint64_t splitFlagsBorn = 0, splitPlanBorn = 0, splitPlanView = 0;
    int splitPlanFirstGroup = 0, splitPlanBlocks = 0;
    std::mutex busy;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timings;  // dominant-kernel launches
    // side stream for the intra-sequence recompute that runs beside the inter-sequence kernel
    hipStream_t aux = nullptr;
    hipEvent_t evFork = nullptr, evJoin = nullptr;

    // Results go to the host through a pinned staging buffer: copying straight into the
    // caller's pageable arrays makes the runtime pin and unpin those pages on every call
    // (tens of milliseconds on fresh memory), a pinned bounce buffer does not.
    void* pinned = nullptr;
    size_t pinnedCap = 0, pinnedUsed = 0;
    uint64_t stagingGeneration = 0;   // moves whenever the staging buffer is drained (its contents are void then)
    struct Pending { void* dst; size_t off, bytes; bool onAux = false; };   // (onAux: copied by the side stream)
    std::vector<Pending> pending;
    std::vector<int32_t> hostScratchA, hostScratchB;  // per-target host arrays of a full search

    // Large results land in pages the caller has not touched yet; a few threads fault them in
    // side by side.
    static void copyOut(void* dst, const char* src, size_t bytes) {
        constexpr size_t kPiece = 4u << 20;
        if (bytes < 2 * kPiece) {
            unpack::copyLarge(dst, src, bytes);
            return;
        }
        const int nThreads = (int)std::min<size_t>(4, bytes / kPiece);
        const size_t share = ((bytes / nThreads) + 4095) & ~(size_t)4095;
        std::vector<std::thread> pool;
        for (int t = 1; t < nThreads; ++t) {
            const size_t lo = share * t, hi = std::min(bytes, lo + share);
            if (lo >= hi) continue;
            try {
                pool.emplace_back([=] { unpack::copyLarge((char*)dst + lo, src + lo, hi - lo); });
            } catch (const std::exception&) {   // no thread to be had: this one copies the share
                unpack::copyLarge((char*)dst + lo, src + lo, hi - lo);
            }
        }
        unpack::copyLarge(dst, src, std::min(bytes, share));
        for (auto& th : pool) th.join();
    }

    // staged entries -> the caller's memory
    // (several arrays of a few MB each - scores and end locations of a million targets: 12 MB - are cut
    // into pieces of 2 MB copied by up to four threads side by side; one small array is a plain memcpy)
    void copyOutEntries(const std::vector<Pending>& entries) const {
        size_t total = 0;
        for (const Pending& p : entries) total += p.bytes;
        constexpr size_t kPiece = 2u << 20;
        if (entries.size() > 1 && total >= 3 * kPiece) {
            struct Piece { void* dst; const char* src; size_t bytes; };
            std::vector<Piece> pieces;
            for (const Pending& p : entries)
                for (size_t at = 0; at < p.bytes; at += kPiece)
                    pieces.push_back({(char*)p.dst + at, (const char*)pinned + p.off + at, std::min(kPiece, p.bytes - at)});
            std::atomic<size_t> next{0};
            auto work = [&] {
                for (size_t k; (k = next.fetch_add(1)) < pieces.size();) unpack::copyLarge(pieces[k].dst, pieces[k].src, pieces[k].bytes);
            };
            std::vector<std::thread> pool;
            const int nThreads = (int)std::min<size_t>(4, pieces.size());
            for (int t = 1; t < nThreads; ++t) {
                try {
                    pool.emplace_back(work);
                } catch (const std::exception&) {
                    break;   // (no thread to be had: the others take its pieces)
                }
            }
            work();
            for (auto& th : pool) th.join();
        } else {
            for (const Pending& p : entries) copyOut(p.dst, (const char*)pinned + p.off, p.bytes);
        }
    }
    // The entries the side stream copies, into the caller's memory now: for a caller that has just waited for
    // that stream and has enqueued no download on it since (a `full` search between two batches - the host is
    // waiting for the device there, at its end it is the other way round). Their room in the buffer stays taken.
    // ... the same entries handed to the caller instead (copyOutEntries on a thread of its own)
    std::vector<Pending> takeSideEntries() {
        std::vector<Pending> landed, rest;
        for (const Pending& p : pending) (p.onAux ? landed : rest).push_back(p);
        pending.swap(rest);
        return landed;
    }
    void flushSideEntries() {
        std::vector<Pending> landed, rest;
        for (const Pending& p : pending) (p.onAux ? landed : rest).push_back(p);
        if (landed.empty()) return;
        copyOutEntries(landed);
        pending.swap(rest);
    }

    // Every per-search transfer goes through this pinned buffer, in both directions. Copying
    // from or to the caller's pageable memory makes the runtime pin those pages for the
    // transfer; when the caller later frees or trims that memory (a result buffer, a heap
    // that shrinks) the driver has to quiesce the process's queues to drop the mapping -
    // measured as a 20-30 ms stall of the NEXT search.
    // `deferFrom`: entries of at least that many bytes stay where they are - staged, not yet in the caller's
    // memory - until a later call without the argument (a `full` search has no use for a million scores on
    // the host while its next kernels could be enqueued instead).
    int finishDownloads(size_t deferFrom = SIZE_MAX) {
        if (pending.empty() && pinnedUsed == 0) return 0;
        HIP_TRY(hipStreamSynchronize(stream));
        // (entries that stay staged may still be on their way on the side stream: a `full` search copies its
        // scores and end locations there, beside the start-cell scan)
        bool auxToo = deferFrom == SIZE_MAX;
        for (const Pending& p : pending) auxToo = auxToo || (p.onAux && p.bytes < deferFrom);
        if (aux && auxToo) HIP_TRY(hipStreamSynchronize(aux));
        if (deferFrom != SIZE_MAX) {
            std::vector<Pending> later;
            for (const Pending& p : pending) {
                if (p.bytes >= deferFrom) later.push_back(p);
                else copyOut(p.dst, (const char*)pinned + p.off, p.bytes);
            }
            if (!later.empty()) {
                pending.swap(later);
                return 0;   // (the staging buffer stays as it is: the deferred entries live in it)
            }
            pending.clear();
        }
        copyOutEntries(pending);
        pending.clear();
        pinnedUsed = 0;
        ++stagingGeneration;
        return 0;
    }
    // A search that fails after stageDownload() leaves entries that point at the caller's (or the
    // failed call's local) memory: they must never be copied out by a later search.
    void abandonDownloads() {
        if (pending.empty()) return;
        (void)hipStreamSynchronize(stream);
        if (aux) (void)hipStreamSynchronize(aux);
        pending.clear();
        pinnedUsed = 0;
        ++stagingGeneration;
    }
    // room for `bytes` more in the staging buffer (drains it, and grows it, when needed)
    int reserveStaging(size_t aligned) {
        if (pinnedUsed + aligned <= pinnedCap) return 0;
        RC_TRY(finishDownloads());
        if (aligned > pinnedCap) {
            if (pinned) HIP_TRY(hipHostFree(pinned));
            pinned = nullptr;
            pinnedCap = 0;
            const size_t want = aligned + aligned / 4 + (1u << 20);
            HIP_TRY(hipHostMalloc(&pinned, want, hipHostMallocDefault));
            pinnedCap = want;
        }
        return 0;
    }
    // (`onAux`: by the side stream - the caller has ordered it behind the producer of `deviceSrc`)
    int stageDownload(void* dst, const void* deviceSrc, size_t bytes, bool onAux = false) {
        if (bytes == 0) return 0;
        const size_t aligned = (bytes + 255) & ~(size_t)255;
        RC_TRY(reserveStaging(aligned));
        HIP_TRY(hipMemcpyAsync((char*)pinned + pinnedUsed, deviceSrc, bytes, hipMemcpyDeviceToHost, onAux ? aux : stream));
        pending.push_back({dst, pinnedUsed, bytes, onAux});
        pinnedUsed += aligned;
        return 0;
    }
    // host -> device on `on` (the workspace's stream or its side stream); `src` may be reused
    // as soon as the call returns
    int stageUpload(void* deviceDst, const void* src, size_t bytes, hipStream_t on) {
        if (bytes == 0) return 0;
        const void* staged;
        RC_TRY(stage(src, bytes, &staged));
        HIP_TRY(hipMemcpyAsync(deviceDst, staged, bytes, hipMemcpyHostToDevice, on));
        return 0;
    }
    // The first half of stageUpload alone: `src` copied into the staging buffer. *staged is device-visible (pinned,
    // mapped) and stays as it is until the buffer is drained - finishDownloads(), which waits for `stream` first, on
    // every entry point, the asynchronous ones included - so a kernel enqueued on `stream` before that may read it.
    int stage(const void* src, size_t bytes, const void** staged) {
        const size_t aligned = (bytes + 255) & ~(size_t)255;
        RC_TRY(reserveStaging(aligned));
        memcpy((char*)pinned + pinnedUsed, src, bytes);
        *staged = (const char*)pinned + pinnedUsed;
        pinnedUsed += aligned;
        return 0;
    }

    int ensureAux() {
        if (aux) return 0;
        // A stream of its own PRIORITY: the runtime multiplexes the streams of a process onto four
        // hardware queues per priority level, and two streams that share a queue run in order. With
        // a handful of streams alive (workspaces, view construction, the upload pool) the side stream
        // and its workspace's main stream sometimes landed on one queue: the kernel that should run
        // BESIDE the packed one ran after it (log-normal database, NW at Q = 150: 7.0 instead of 4.0 ms).
        // The work on this stream is the launch's critical path anyway.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
            (void)hipGetLastError();
            least = greatest = 0;
        }
        if (greatest != least) HIP_TRY(hipStreamCreateWithPriority(&aux, hipStreamNonBlocking, greatest));
        else HIP_TRY(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&evFork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&evJoin, hipEventDisableTiming));
        return 0;
    }

    int get(int slot, size_t bytes, void** out) {
        if (bytes == 0) bytes = 16;
        usedBy[slot] = leaseStamp;
        if (cap[slot] < bytes) {
            if (buf[slot]) {
                HIP_TRY(hipStreamSynchronize(stream));
                HIP_TRY(hipFree(buf[slot]));
                buf[slot] = nullptr;
                cap[slot] = 0;
            }
            size_t want = bytes + bytes / 8 + 256;
            HIP_TRY(hipMalloc(&buf[slot], want));
            cap[slot] = want;
            born[slot] = ++allocations;
            if (want > (512u << 20) && tuned(Tune::VERBOSE))
                fprintf(stderr, "miopal: workspace slot %d grows to %zu MiB\n", slot, want >> 20);
        }
        *out = buf[slot];
        return 0;
    }
    // Like get(), but an allocation the device cannot serve is not an error: returns false
    // (the caller asks for less). The slack of get() is left out: these are the big buffers.
    bool tryGet(int slot, size_t bytes, void** out) {
        usedBy[slot] = leaseStamp;
        if (cap[slot] >= bytes) {
            *out = buf[slot];
            return true;
        }
        if (buf[slot]) {
            (void)hipStreamSynchronize(stream);
            (void)hipFree(buf[slot]);
            buf[slot] = nullptr;
            cap[slot] = 0;
        }
        if (hipMalloc(&buf[slot], bytes) != hipSuccess) {
            (void)hipGetLastError();  // out of memory is handled by the caller
            buf[slot] = nullptr;
            return false;
        }
        cap[slot] = bytes;
        born[slot] = ++allocations;
        if (bytes > (512u << 20) && tuned(Tune::VERBOSE))
            fprintf(stderr, "miopal: workspace slot %d grows to %zu MiB\n", slot, bytes >> 20);
        *out = buf[slot];
        return true;
    }
    size_t bytes() const {
        size_t t = 0;
        for (size_t c : cap) t += c;
        return t;
    }
    // Free device buffers, largest first, until at most `keep` bytes are held (an idle workspace: its stream has
    // drained). Streams, events, the pinned staging buffer and the small buffers stay: the next search allocates
    // what it misses - 0.3 ms per multi-GB buffer, against tens of GB parked per thread that once ran a long `full` search.
    size_t trimTo(size_t keep, bool staleOnly = false) {
        size_t freed = 0;
        // (first what the search that has just ended did not touch - the buffers of another kind of search, e.g. the
        // strip boundaries of a long query's score search under a loop of `full` searches of a short one, whose own
        // buffers then stay - then whatever is largest)
        for (int pass = 0; pass < (staleOnly ? 1 : 2); ++pass)
        while (bytes() > keep) {
            int big = -1;
            for (int k = 0; k < kSlots; ++k)
                if (buf[k] && (pass == 1 || usedBy[k] != leaseStamp) && (big < 0 || cap[k] > cap[big])) big = k;
            if (big < 0) break;
            (void)hipFree(buf[big]);
            freed += cap[big];
            buf[big] = nullptr;
            cap[big] = 0;
        }
        return freed;
    }
    ~Workspace() {
        for (auto& ev : timings) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        for (void* p : buf)
            if (p) (void)hipFree(p);
        if (pinned) (void)hipHostFree(pinned);
        if (evFork) (void)hipEventDestroy(evFork);
        if (evJoin) (void)hipEventDestroy(evJoin);
        if (aux) (void)hipStreamDestroy(aux);
        if (ownsStream && stream) (void)hipStreamDestroy(stream);
    }
};

