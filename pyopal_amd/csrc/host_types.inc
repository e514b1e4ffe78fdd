// Part of host.hip (included there, not a translation unit of its own): the packed view of a database slice, the database handle (MiopalDb) and the lease of a workspace.
// ---------------------------------------------------------------------------
// packed view of a database slice
// ---------------------------------------------------------------------------
struct View {
    int64_t start = 0, end = 0;
    int overlap = 0;                 // > 0: long targets are cut into windows overlapping by this much
    int stride = 0;                  // ... starting every `stride` residues
    int32_t* d_segStart = nullptr;   // view position -> first residue of its window (segmented views)
    int nPacked = 0;                 // targets in the packed groups
    int nGroups = 0;
    int maxPackedLen = 0;
    std::vector<int> groupChunksHost;  // 4-column chunks per group (longest group first)
    int64_t totalChunks = 0;
    std::vector<int32_t> ids;        // view position -> database index (packed part)
    std::vector<int32_t> longIds;    // targets always handled by the intra-sequence kernel
    int32_t* d_ids = nullptr;
    int32_t* d_lens = nullptr;       // target lengths in view order, padded to whole groups
    uint2* d_pack = nullptr;
    int64_t* d_groupOff = nullptr;
    int* d_groupChunks = nullptr;
    int64_t* d_boundaryOff = nullptr;
    int64_t* d_chunkPrefix = nullptr;  // [nGroups + 1] running number of chunks (the pack kernel, the column split)
    size_t deviceBytes = 0;
    void* d_meta = nullptr;          // one allocation behind d_ids .. d_boundaryOff (and the pack kernel's prefix)
    bool packPending = false;        // lists built and uploaded, residues not packed yet (prefetched view)
    PackArgs pendingPack{};
    size_t packCap = 0, metaCap = 0; // sizes of the two allocations (a refilled handle re-uses them)
    // one number per view ever built (never 0): what a workspace derived from a view's lists - the column split's plan -
    // is recognised by it, where an address may come back for another view
    const uint64_t serial = [] {
        static std::atomic<uint64_t> last{0};
        return ++last;
    }();
    ~View() {
        if (d_pack) (void)hipFree(d_pack);
        if (d_meta) (void)hipFree(d_meta);
    }
};

}  // namespace

struct MiopalDb {
    int device = 0;                // physical HIP device
    int ordinal = 0;               // the ordinal the caller asked for (differs under miopalTestSetLogicalDevices)
    // per-handle options (miopalDbSetOption); -1: the process-wide default (tuning.h)
    std::atomic<int> optReserveCus{-1};    // CUs kept out of the persistent launches (room for a collective's kernels)
    std::atomic<int> optSmallSearch{-1};   // 0: small searches stay on the lane-per-target kernels
    int alphabet = 0;
    int64_t count = 0;
    int64_t total = 0;
    int64_t maxLen = 0;            // longest sequence (range checks)
    int computeUnits = 256;
    std::vector<int64_t> offsets;  // host copy, [count + 1]
    uint8_t* d_residues = nullptr;
    int64_t* d_offsets = nullptr;
    size_t residueCap = 0, offsetsCap = 0;   // allocated bytes (a handle may be refilled: opalSearchDatabase)
    // the length bin of every target (select_stats.h), built at the first significance search (host_stats.inc:
    // ensureBins) and set, under the mutex, only once the array is complete
    std::mutex binsMutex;
    uint8_t* d_bins = nullptr;
    // device blocks of dropped views, kept for the views of the next filling (at most kSpareBlocks)
    std::vector<std::pair<void*, size_t>> spareBlocks;

    struct ViewSlot {
        int64_t start, end;
        int overlap, stride;
        bool building;                 // placeholder: the view is being built outside the lock
        std::shared_ptr<View> view;
    };
    // view lists built while the residues were still on their way (opalSearchDatabase: fillHandle)
    std::vector<std::shared_ptr<View>> prefetched;   // (one per segment when the call searches under its upload)
    std::mutex viewMutex;
    std::condition_variable viewReady;
    std::list<ViewSlot> views;         // most recent first
    size_t viewBudgetBytes = (size_t)64 << 30;   // set from the device's memory at creation

    // pinned staging buffers + streams for view construction, re-used (hipHostMalloc and
    // hipStreamCreate are slow and serialise between threads)
    struct UploadChannel {
        void* pinned = nullptr;
        size_t cap = 0;
        hipStream_t stream = nullptr;
        ~UploadChannel() {
            if (pinned) (void)hipHostFree(pinned);
            if (stream) (void)hipStreamDestroy(stream);
        }
    };
    std::mutex uploadMutex;
    std::vector<std::unique_ptr<UploadChannel>> uploadFree;

    std::mutex wsMutex;
    std::vector<std::unique_ptr<Workspace>> ownedFree;              // internal streams, idle
    std::map<hipStream_t, std::unique_ptr<Workspace>> external;     // caller streams

    std::atomic<int> profiling{0};
    std::mutex timingMutex;
    Workspace* lastTimed = nullptr;

    MiopalDb() { liveHandles(this, +1); }
    // (every live handle, for miopalReleaseCaches: idle workspaces are caches too)
    static void liveHandles(MiopalDb* db, int what, std::vector<MiopalDb*>* out = nullptr);
    ~MiopalDb() {
        liveHandles(this, -1);
        (void)hipSetDevice(device);
        views.clear();
        uploadFree.clear();
        ownedFree.clear();
        external.clear();
        for (auto& b : spareBlocks) (void)hipFree(b.first);
        if (d_residues) (void)hipFree(d_residues);
        if (d_offsets) (void)hipFree(d_offsets);
        if (d_bins) (void)hipFree(d_bins);
    }
};

namespace {

// idle workspaces a handle may keep (~WorkspaceLease): four times the database, 4 GiB at least
static size_t parkedWorkspaceBound(MiopalDb* db) {
    if (const char* e = tuned(Tune::PARKED_WORKSPACE_MB)) return (size_t)std::max(0ll, atoll(e)) << 20;
    // (the linear database and the offsets; the cached views are bounded on their own)
    const size_t database = (size_t)db->total + (size_t)(db->count + 1) * 8;
    return std::max(kParkedWorkspaceFloor, 4 * database);
}

struct WorkspaceLease {
    MiopalDb* db;
    Workspace* ws = nullptr;
    bool owned = false;
    std::unique_lock<std::mutex> lock;
    explicit WorkspaceLease(MiopalDb* d) : db(d) {}
    int acquireInternal() {
        std::unique_ptr<Workspace> w;
        {
            std::lock_guard<std::mutex> g(db->wsMutex);
            if (!db->ownedFree.empty()) {
                w = std::move(db->ownedFree.back());
                db->ownedFree.pop_back();
            }
        }
        if (!w) {
            w.reset(new Workspace());
            HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
            w->ownsStream = true;
            // The side stream is created WITH the main one, not when a search first needs it. Measured
            // (profiles/r04_late_side_stream.txt): a handle that had only run score searches, then - after a second
            // handle had searched and been closed, its two streams destroyed - ran `full` searches, got a side stream
            // the runtime had recycled; from then on the small kernels of its main stream (fills, histograms, job
            // lists: 5-12 us) took 40-75 us every other time, a 1M x 300 `full` search 9.7 instead of 8.7 ms, for as
            // long as the process ran. Two streams created together - both new or both recycled - do not show it.
            RC_TRY(w->ensureAux());
        }
        ws = w.release();
        ++ws->leaseStamp;
        owned = true;
        return 0;
    }
    int acquireExternal(hipStream_t s) {
        {
            std::lock_guard<std::mutex> g(db->wsMutex);
            auto& slot = db->external[s];
            if (!slot) {
                slot.reset(new Workspace());
                slot->stream = s;
            }
            ws = slot.get();
        }
        lock = std::unique_lock<std::mutex>(ws->busy);
        return 0;
    }
    // a kernel of this search was handed the CALLER's pinned arrays: no way out of the call, error
    // paths included, may leave it running (the caller is free to release the arrays on return)
    bool callerVisibleOutputs = false;
    ~WorkspaceLease() {
        if (ws && callerVisibleOutputs) {
            (void)hipStreamSynchronize(ws->stream);
            if (ws->aux) (void)hipStreamSynchronize(ws->aux);
        }
        // downloads still pending here belong to a search that returned an error
        if (ws) ws->abandonDownloads();
        if (owned && ws) {
            // Idle workspaces keep their buffers for the next search on whatever thread comes
            // first, but not without bound: many threads that each ran one `full` search would
            // otherwise park tens of GB apiece (the reference's thread pools default to one
            // thread per CPU core). Beyond 64 GB of parked buffers this one is released.
            // (round 5: the bound follows the database - four times its device bytes, 4 GiB at least - and it is the
            // OTHER idle workspaces, oldest first, that give back their largest buffers for it: the one that has just
            // searched keeps what it used - up to a quarter of the device's memory - for the next search of its
            // kind. Freeing and re-allocating the 12.6 GB of direction bits of a Q = 300 `full` search every time cost
            // 2 ms per search and, every sixth time or so, TWO SECONDS inside the runtime's allocator
            // (profiles/r05_workspace_trimming.txt). Streams, pinned buffers and small buffers always stay.)
            std::unique_ptr<Workspace> mine(ws);
            std::lock_guard<std::mutex> g(db->wsMutex);
            size_t others = 0;
            for (const auto& w : db->ownedFree) others += w->bytes();
            const size_t bound = parkedWorkspaceBound(db);
            if (others + mine->bytes() > bound) {
                (void)hipSetDevice(db->device);
                size_t excess = others + mine->bytes() - bound;
                for (auto& w : db->ownedFree) {
                    if (excess == 0 || others == 0) break;
                    const size_t held = w->bytes();
                    if (held == 0) continue;
                    (void)hipStreamSynchronize(w->stream);
                    if (w->aux) (void)hipStreamSynchronize(w->aux);
                    ++w->leaseStamp;   // (nothing of an idle workspace is "in use")
                    const size_t freed = w->trimTo(held > excess ? held - excess : 0);
                    excess -= std::min(excess, freed);
                    others -= std::min(others, freed);
                }
                // ... and of its own buffers the ones the search that has just ended did NOT use (a score search behind a
                // `full` one: the direction bits go), all of them beyond a quarter of the device's memory
                const size_t hardCap = std::max(bound, db->viewBudgetBytes / 4 * 3);   // (view budget = a third of the device)
                if (others + mine->bytes() > bound) {
                    (void)hipStreamSynchronize(mine->stream);
                    if (mine->aux) (void)hipStreamSynchronize(mine->aux);
                    mine->trimTo(bound > others ? bound - others : 0, /*staleOnly=*/true);
                    if (mine->bytes() > hardCap) mine->trimTo(hardCap);
                }
            }
            db->ownedFree.emplace_back(std::move(mine));
        }
    }
};

