// Part of host.hip (included there, not a translation unit of its own): argument checks, creation and (re)filling of handles, the exception guard of the C ABI.
int validate(const MiopalDb* db, const unsigned char* query, int Q, const int* matrix, int A,
             int searchType, int mode, int64_t start, int64_t end) {
    if (!db) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null database handle");
    if (mode < OPAL_MODE_NW || mode > OPAL_MODE_SW) return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", mode);
    if (searchType < OPAL_SEARCH_SCORE || searchType > OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "invalid search type %d", searchType);
    if (Q < 0 || (Q > 0 && !query)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad query");
    if (!matrix || A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad score matrix / alphabet length %d", A);
    if (A != db->alphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d differs from the database's %d", A, db->alphabet);
    for (int i = 0; i < Q; ++i)
        if (query[i] >= A) return fail(MIOPAL_ERR_BAD_ARGUMENT, "query residue %d out of range at %d", query[i], i);
    if (start < 0 || end < start || end > db->count) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad slice [%lld, %lld)", (long long)start, (long long)end);
    return 0;
}

// The database's residues as the caller holds them: one flat array, or one pointer per sequence
// (opalSearchDatabase's `unsigned char* db[]`).
struct ResidueSource {
    const unsigned char* flat = nullptr;
    const unsigned char* const* sequences = nullptr;
};

int newHandle(std::unique_ptr<MiopalDb>* out, int device) {
    // (ordinals count the gfx950 devices only: a device of another architecture on the same box is never handed out)
    const std::vector<int>& usable = usableDevices();
    const int ndev = (int)usable.size();
    if (ndev <= 0) return fail(OPAL_ERR_NO_SIMD_SUPPORT, "no gfx950 device available");
    const int logical = g_logicalDevices.load(std::memory_order_relaxed);
    if (device < 0 || device >= (logical > 0 ? logical : ndev)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "device %d out of range", device);
    const int ordinal = device;
    device = usable[(size_t)(logical > 0 ? device % ndev : device)];   // (test hook: several ordinals round-robin over the physical devices)
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<MiopalDb> db(new MiopalDb());
    db->device = device;
    db->ordinal = ordinal;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        db->computeUnits = prop.multiProcessorCount;
    // cached packed views may take a third of the device's memory (MIOPAL_VIEW_CACHE_MB overrides)
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && totalB > 0) db->viewBudgetBytes = totalB / 3;
    if (const char* mb = tuned(Tune::VIEW_CACHE_MB)) db->viewBudgetBytes = (size_t)std::max(0, atoi(mb)) << 20;
    *out = std::move(db);
    return 0;
}

// (Re)fills a handle nobody else is using: the sequences replace whatever it held; device
// allocations that are large enough stay, the blocks of its cached views are kept for the new views.
// `segments` (opalSearchDatabase searching under its own upload): bounds of the slices [segments[k], segments[k + 1])
// that the caller searches one after the other as their residues land - their view lists are built ahead in that
// order; `progress` tells the caller what has landed; `ready` is set (under progress->m) when the handle's host side,
// its device allocations and the offsets on the device are in place, i.e. from when on landed slices may be searched.
int fillHandle(MiopalDb* db, const ResidueSource& src, std::vector<int64_t>&& offsets, int64_t count,
               int alphabetLength, bool prefetchView = false, const std::vector<int64_t>* segments = nullptr,
               UploadProgress* progress = nullptr, bool* ready = nullptr) {
    struct Finish {   // (whatever way this function is left, a waiting caller is told)
        UploadProgress* p;
        ~Finish() { if (p) p->finish(); }
    } finishProgress{progress};
    const int device = db->device;
    HIP_TRY(hipSetDevice(device));
    {
        std::lock_guard<std::mutex> g(db->viewMutex);
        for (auto& slot : db->views) {
            View* v = slot.view.get();
            if (!v || slot.view.use_count() != 1) continue;
            for (auto blk : {std::make_pair((void**)&v->d_pack, v->packCap), std::make_pair(&v->d_meta, v->metaCap)})
                if (*blk.first && db->spareBlocks.size() < kSpareBlocks) {
                    db->spareBlocks.emplace_back(*blk.first, blk.second);
                    *blk.first = nullptr;
                }
        }
        db->views.clear();
        db->prefetched.clear();
    }
    {
        // (the bins of the filling before this one)
        std::lock_guard<std::mutex> g(db->binsMutex);
        if (db->d_bins) HIP_TRY(hipFree(db->d_bins));
        db->d_bins = nullptr;
    }
    db->alphabet = alphabetLength;
    db->count = count;
    db->offsets = std::move(offsets);
    const std::vector<int64_t>& off = db->offsets;
    db->total = off[(size_t)count];
    db->maxLen = 0;
    {
        const int nSlices = hostThreads((size_t)count, 65536);
        std::vector<int64_t> longest((size_t)nSlices, 0);
        parallelSlices(nSlices, [&](int t) {
            int64_t m = 0;
            for (int64_t k = count * t / nSlices; k < count * (t + 1) / nSlices; ++k) m = std::max(m, off[(size_t)k + 1] - off[(size_t)k]);
            longest[(size_t)t] = m;
        });
        for (int64_t m : longest) db->maxLen = std::max(db->maxLen, m);
    }
    const size_t wantRes = (size_t)db->total + 64, wantOff = (size_t)(count + 1) * sizeof(int64_t);
    if (db->residueCap < wantRes || db->residueCap / 4 > wantRes + (1u << 20)) {
        if (db->d_residues) HIP_TRY(hipFree(db->d_residues));
        db->d_residues = nullptr;
        db->residueCap = 0;
        HIP_TRY(hipMalloc(&db->d_residues, wantRes));
        db->residueCap = wantRes;
    }
    if (db->offsetsCap < wantOff || db->offsetsCap / 4 > wantOff + (1u << 20)) {
        if (db->d_offsets) HIP_TRY(hipFree(db->d_offsets));
        db->d_offsets = nullptr;
        db->offsetsCap = 0;
        HIP_TRY(hipMalloc(&db->d_offsets, wantOff));
        db->offsetsCap = wantOff;
    }
    // opalSearchDatabase hands the whole database over on every call and searches all of it at once: the
    // lists of that search's packed view only need the lengths, so they are built (and their small arrays
    // uploaded) by another thread WHILE the residues cross PCIe; the search then only packs. Only for
    // databases whose targets are shorter than any window of a segmented view (the search would ask for
    // another view otherwise). A failure here is no error: the search builds its view itself.
    if (progress) {
        // (the caller searches before the residues are all there: the offsets go first)
        RC_TRY(uploadOnce(device, db->d_offsets, off.data(), wantOff));
        std::lock_guard<std::mutex> g(progress->m);
        if (ready) *ready = true;
        progress->cv.notify_all();
    }
    std::thread viewThread;
    if (prefetchView && count >= 65536 && db->maxLen <= 256 + 128 && !tuned(Tune::NO_VIEW_PREFETCH)) {
        std::vector<int64_t> bounds = segments ? *segments : std::vector<int64_t>{0, count};
        try {
            viewThread = std::thread([db, bounds, device] {
                if (hipSetDevice(device) != hipSuccess) return;
                for (size_t k = 0; k + 1 < bounds.size(); ++k) {
                    if (bounds[k + 1] <= bounds[k]) continue;
                    std::shared_ptr<View> v;
                    try {
                        if (buildView(db, bounds[k], bounds[k + 1], 0, &v, false) != 0) {
                            (void)hipGetLastError();
                            return;
                        }
                    } catch (...) {
                        return;
                    }
                    std::lock_guard<std::mutex> g(db->viewMutex);
                    db->prefetched.push_back(std::move(v));
                }
            });
        } catch (const std::exception&) {
        }
    }
    struct Joiner {
        std::thread& t;
        ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{viewThread};
    // residues: gathered (or copied) piece by piece into the bounce pieces and checked there
    const unsigned limit = (unsigned)alphabetLength;
    int bad = 0;
    RC_TRY(streamedUpload(device, db->d_residues, (size_t)db->total,
        [&](unsigned char* dst, size_t at, size_t n) {
            Bytes16 top = {};
            unsigned topTail = 0;
            if (src.flat) {
                copyWithMax(dst, src.flat + at, n, top, topTail);
            } else {
                // first sequence that ends beyond `at`
                size_t k = (size_t)(std::upper_bound(off.begin(), off.begin() + count + 1, (int64_t)at) - off.begin()) - 1;
                size_t pos = at;
                const size_t stop = at + n;
                while (pos < stop) {
                    const size_t seqEnd = (size_t)off[k + 1];
                    if (seqEnd <= pos) { ++k; continue; }   // (empty sequences)
                    const size_t m = std::min(seqEnd, stop) - pos;
                    copyWithMax(dst + (pos - at), src.sequences[k] + (pos - (size_t)off[k]), m, top, topTail);
                    pos += m;
                }
            }
            const unsigned largest = largestByte(top, topTail);
            return largest >= limit ? (int)largest + 1 : 0;
        }, &bad, progress));
    if (bad) return fail(MIOPAL_ERR_BAD_ARGUMENT, "residue %d out of range for alphabet %d", bad - 1, alphabetLength);
    if (!progress) RC_TRY(uploadOnce(device, db->d_offsets, off.data(), wantOff));
    return 0;
}

int createCommon(MiopalDb** out, const ResidueSource& src, std::vector<int64_t>&& offsets,
                 int64_t count, int alphabetLength, int device) {
    std::unique_ptr<MiopalDb> db;
    RC_TRY(newHandle(&db, device));
    RC_TRY(fillHandle(db.get(), src, std::move(offsets), count, alphabetLength));
    *out = db.release();
    return 0;
}

// Handles of finished opalSearchDatabase calls, kept (with their device memory, bounce buffers and
// streams) for the next call of the process: the reference's entry point hands the whole database
// over on every call, and allocating and releasing a handle's resources costs as much as the search.
// Bounded by count and by the device memory a parked handle may hold (MIOPAL_SPARE_HANDLE_MB,
// default 4096; 0 keeps none); miopalReleaseCaches() drops them.
constexpr size_t kSpareHandles = 4;
struct SpareHandles {
    std::mutex m;
    std::vector<std::unique_ptr<MiopalDb>> idle;
};
SpareHandles& spareHandles() {
    static SpareHandles* s = new SpareHandles();   // never destroyed: the runtime may be gone at exit
    return *s;
}

int64_t handleDeviceBytes(MiopalDb* db) {
    int64_t t = (int64_t)(db->residueCap + db->offsetsCap);
    {
        std::lock_guard<std::mutex> g(db->viewMutex);
        for (auto& v : db->views) t += v.view ? (int64_t)(v.view->packCap + v.view->metaCap) : 0;
        for (auto& b : db->spareBlocks) t += (int64_t)b.second;
    }
    std::lock_guard<std::mutex> g(db->wsMutex);
    for (auto& w : db->ownedFree) t += (int64_t)w->bytes();
    return t;
}


// No C++ exception leaves the C ABI (the callers are C, Cython with the GIL released, ctypes): whatever
// the host code throws - in practice std::bad_alloc from a container of a million entries - becomes
// MIOPAL_ERR_INTERNAL with the reason in miopalLastError().
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
    } catch (const std::exception& e) {
        return fail(MIOPAL_ERR_INTERNAL, "unexpected exception: %s", e.what());
    } catch (...) {
        return fail(MIOPAL_ERR_INTERNAL, "unexpected exception");
    }
}

}  // namespace

