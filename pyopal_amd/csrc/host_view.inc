// Part of host.hip (included there, not a translation unit of its own): construction and cache of packed views.
// ---- view construction -------------------------------------------------------
// Window stride of a segmented view: with overlap O (>= the longest span a local alignment of the
// query can have in the target) every alignment lies inside one window [k S, k S + S + O).
int segmentStride(int overlap) { return std::max(256, (overlap * 3 / 5 + 63) / 64 * 64); }

// Host loops over a million targets (view lists, result structs) are cut into slices worked on by
// a few threads; MIOPAL_HOST_THREADS overrides the count (default: up to 4).
int hostThreads(size_t items, size_t perThread, size_t atMost = 4) {
    int t = (int)std::min<size_t>(atMost, std::max(1u, std::thread::hardware_concurrency()));
    if (const char* env = tuned(Tune::HOST_THREADS)) t = std::max(1, std::min(64, atoi(env)));
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)t, items / std::max<size_t>(perThread, 1)));
}
template <class Body>
void parallelSlices(int nSlices, const Body& body) {
    if (nSlices <= 1) {
        body(0);
        return;
    }
    // (what a slice throws - std::bad_alloc - is carried back to the caller once every thread has ended)
    std::vector<std::exception_ptr> thrown((size_t)nSlices);
    auto run = [&body, &thrown](int t) {
        try {
            body(t);
        } catch (...) {
            thrown[(size_t)t] = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    pool.reserve((size_t)nSlices - 1);
    int started = 1;   // slices [1, started) have a thread of their own
    for (; started < nSlices; ++started) {
        try {
            pool.emplace_back(run, started);
        } catch (const std::exception&) {
            break;
        }
    }
    run(0);
    for (int t = started; t < nSlices; ++t) run(t);   // (no thread to be had for these)
    for (auto& th : pool) th.join();
    for (const auto& e : thrown)
        if (e) std::rethrow_exception(e);
}

// A device block for a view: one left behind by the views of the handle's previous filling when it
// fits without wasting more than half of itself, a fresh allocation otherwise.
constexpr size_t kSpareBlocks = 4;
int viewBlock(MiopalDb* db, size_t bytes, void** out, size_t* cap) {
    {
        std::lock_guard<std::mutex> g(db->viewMutex);
        auto best = db->spareBlocks.end();
        for (auto it = db->spareBlocks.begin(); it != db->spareBlocks.end(); ++it)
            if (it->second >= bytes && it->second / 2 <= bytes + 4096 && (best == db->spareBlocks.end() || it->second < best->second))
                best = it;
        if (best != db->spareBlocks.end()) {
            *out = best->first;
            *cap = best->second;
            db->spareBlocks.erase(best);
            return 0;
        }
    }
    HIP_TRY(hipMalloc(out, bytes));
    *cap = bytes;
    return 0;
}

int finishView(MiopalDb* db, View* v);

// packNow = false: everything but the pack kernel (which reads the residues on the device): the lists,
// the device blocks and the upload of the small arrays - what can be done while the residues are still
// crossing PCIe; finishView() packs.
int buildView(MiopalDb* db, int64_t start, int64_t end, int overlap, std::shared_ptr<View>* out, bool packNow = true,
              int strideWanted = -1) {
    if (packNow) {
        // (lists of this very slice built ahead, beside the upload of the residues: only the packing is left)
        std::shared_ptr<View> ready;
        {
            std::lock_guard<std::mutex> g(db->viewMutex);
            for (auto it = db->prefetched.begin(); it != db->prefetched.end(); ++it)
                if (*it && (*it)->start == start && (*it)->end == end && (*it)->overlap == overlap &&
                    (*it)->stride == (overlap > 0 ? (strideWanted > 0 ? strideWanted : segmentStride(overlap)) : 0)) {
                    ready = std::move(*it);
                    db->prefetched.erase(it);
                    break;
                }
        }
        if (ready) {
            RC_TRY(finishView(db, ready.get()));
            *out = ready;
            return 0;
        }
    }
    PhaseTimer pt;
    auto v = std::make_shared<View>();
    v->start = start;
    v->end = end;
    v->overlap = overlap;
    // The view's entries (targets, or windows of long targets), longest first: the heaviest
    // wavefronts are dispatched first. A stable counting sort by length (windows of one target stay
    // in order), in slices of the target range worked on side by side: count, place, scatter. For
    // a million targets the lists used to cost more than the search itself.
    const int64_t nT = end - start;
    const int stride = overlap > 0 ? (strideWanted > 0 ? strideWanted : segmentStride(overlap)) : 0, window = stride + overlap;
    v->stride = stride;
    const int nSlices = hostThreads((size_t)nT, 65536);
    auto sliceLo = [&](int t) { return start + nT * t / nSlices; };
    auto windowsOf = [&](int L) {   // windows until the tail is inside the overlap of the previous one
        if (L <= window) return 1;
        return 1 + (L - overlap - 1) / stride;
    };
    std::vector<int64_t> sliceEntries((size_t)nSlices + 1, 0);
    std::vector<int> sliceLongest((size_t)nSlices, 0);
    std::vector<std::vector<int32_t>> sliceLong((size_t)nSlices);
    parallelSlices(nSlices, [&](int t) {
        int64_t entries = 0;
        int longest = 0;
        for (int64_t k = sliceLo(t); k < sliceLo(t + 1); ++k) {
            const int L = dbLen(db, k);
            if (overlap > 0) {
                entries += windowsOf(L);
                longest = std::max(longest, std::min(L, window));
            } else if (L > kLongTarget) {
                sliceLong[(size_t)t].push_back((int32_t)k);
            } else {
                ++entries;
                longest = std::max(longest, L);
            }
        }
        sliceEntries[(size_t)t + 1] = entries;
        sliceLongest[(size_t)t] = longest;
    });
    pt.mark("view: count");
    int longest = 0;
    for (int t = 0; t < nSlices; ++t) {
        sliceEntries[(size_t)t + 1] += sliceEntries[(size_t)t];
        longest = std::max(longest, sliceLongest[(size_t)t]);
        v->longIds.insert(v->longIds.end(), sliceLong[(size_t)t].begin(), sliceLong[(size_t)t].end());
    }
    const size_t nEntries = (size_t)sliceEntries[(size_t)nSlices];
    if (nEntries >= (size_t)INT32_MAX) return fail(MIOPAL_ERR_BAD_ARGUMENT, "too many windows in one view");
    const size_t nBins = (size_t)longest + 1;
    // place[t][b]: first sorted position of slice t's entries of length longest - b
    std::vector<int64_t> place((size_t)nSlices * nBins, 0);
    parallelSlices(nSlices, [&](int t) {
        int64_t* mine = place.data() + (size_t)t * nBins;
        for (int64_t k = sliceLo(t); k < sliceLo(t + 1); ++k) {
            const int L = dbLen(db, k);
            if (overlap > 0) {
                if (L <= window) {
                    ++mine[longest - L];
                } else {
                    const int w = windowsOf(L);
                    mine[longest - window] += w - 1;
                    ++mine[longest - std::min(window, L - (w - 1) * stride)];
                }
            } else if (L <= kLongTarget) {
                ++mine[longest - L];
            }
        }
    });
    pt.mark("view: histogram");
    {
        int64_t running = 0;
        for (size_t bin = 0; bin < nBins; ++bin)
            for (int t = 0; t < nSlices; ++t) {
                int64_t& c = place[(size_t)t * nBins + bin];
                const int64_t n = c;
                c = running;
                running += n;
            }
    }
    pt.mark("view: places");
    const int nGroupsAll = (int)((nEntries + kGroupTargets - 1) / kGroupTargets);
    std::vector<int32_t> ids(nEntries), segStart(overlap > 0 ? nEntries : 0);
    std::vector<int32_t> vlen((size_t)nGroupsAll * kGroupTargets);   // padded to whole groups with zeros
    parallelSlices(nSlices, [&](int t) {
        int64_t* mine = place.data() + (size_t)t * nBins;
        for (int64_t k = sliceLo(t); k < sliceLo(t + 1); ++k) {
            const int L = dbLen(db, k);
            if (overlap > 0) {
                const int w = windowsOf(L);
                for (int x = 0; x < w; ++x) {
                    const int s0 = x * stride, len = w == 1 ? L : std::min(window, L - s0);
                    const size_t at = (size_t)mine[longest - len]++;
                    ids[at] = (int32_t)k;
                    segStart[at] = s0;
                    vlen[at] = len;
                }
            } else if (L <= kLongTarget) {
                const size_t at = (size_t)mine[longest - L]++;
                ids[at] = (int32_t)k;
                vlen[at] = L;
            }
        }
    });
    pt.mark("view: scatter");
    v->nPacked = (int)ids.size();
    v->nGroups = (v->nPacked + kGroupTargets - 1) / kGroupTargets;
    std::vector<int64_t> groupOff(v->nGroups + 1, 0), chunkPrefix(v->nGroups + 1, 0), boundaryOff(v->nGroups + 1, 0);
    std::vector<int> groupChunks(std::max(v->nGroups, 1), 0);
    for (int g = 0; g < v->nGroups; ++g) {
        const int maxLen = vlen[(size_t)g * kGroupTargets];  // sorted: first is longest
        v->maxPackedLen = std::max(v->maxPackedLen, maxLen);
        const int chunks = std::max(1, (maxLen + 3) / 4);
        groupChunks[g] = chunks;
        chunkPrefix[g + 1] = chunkPrefix[g] + chunks;
        groupOff[g + 1] = groupOff[g] + (int64_t)chunks * kLanes;
        boundaryOff[g + 1] = boundaryOff[g] + (int64_t)chunks * 4 * kLanes;
    }
    v->totalChunks = chunkPrefix[v->nGroups];
    v->groupChunksHost.assign(groupChunks.begin(), groupChunks.begin() + v->nGroups);
    if (v->nGroups > 0) {
        // Two device allocations and one staged upload per view: the small per-target and per-group
        // arrays share one blob (hipMalloc, hipHostMalloc and stream creation serialise in the
        // runtime, and thread-chunked callers build their slices' views side by side).
        const size_t packBytes = (size_t)groupOff[v->nGroups] * sizeof(uint2);
        struct Part { const void* src; size_t bytes, at; };
        Part parts[] = {
            {ids.data(), ids.size() * sizeof(int32_t), 0},
            {segStart.data(), overlap > 0 ? segStart.size() * sizeof(int32_t) : 0, 0},
            {vlen.data(), vlen.size() * sizeof(int32_t), 0},
            {groupOff.data(), groupOff.size() * sizeof(int64_t), 0},
            {groupChunks.data(), groupChunks.size() * sizeof(int), 0},
            {boundaryOff.data(), boundaryOff.size() * sizeof(int64_t), 0},
            {chunkPrefix.data(), chunkPrefix.size() * sizeof(int64_t), 0},
        };
        size_t metaBytes = 0;
        for (Part& p : parts) {
            p.at = metaBytes;
            metaBytes += (p.bytes + 255) & ~(size_t)255;
        }
        pt.mark("view: host lists");
        RC_TRY(viewBlock(db, std::max<size_t>(metaBytes, 256), &v->d_meta, &v->metaCap));
        RC_TRY(viewBlock(db, packBytes, (void**)&v->d_pack, &v->packCap));
        pt.mark("view: device allocation");
        char* meta = (char*)v->d_meta;
        v->d_ids = (int32_t*)(meta + parts[0].at);
        v->d_segStart = overlap > 0 ? (int32_t*)(meta + parts[1].at) : nullptr;
        v->d_lens = (int32_t*)(meta + parts[2].at);
        v->d_groupOff = (int64_t*)(meta + parts[3].at);
        v->d_groupChunks = (int*)(meta + parts[4].at);
        v->d_boundaryOff = (int64_t*)(meta + parts[5].at);
        v->d_chunkPrefix = (int64_t*)(meta + parts[6].at);
        UploadLease up(db);
        RC_TRY(up.acquire(metaBytes));
        for (const Part& p : parts)
            if (p.bytes) memcpy((char*)up.ch->pinned + p.at, p.src, p.bytes);
        HIP_TRY(hipMemcpyAsync(meta, up.ch->pinned, metaBytes, hipMemcpyHostToDevice, up.ch->stream));
        PackArgs pa{};
        pa.residues = db->d_residues;
        pa.offsets = db->d_offsets;
        pa.ids = v->d_ids;
        pa.segStart = v->d_segStart;
        pa.lens = v->d_lens;
        pa.nTargets = v->nPacked;
        pa.groupOff = v->d_groupOff;
        pa.groupChunks = v->d_groupChunks;
        pa.chunkPrefix = v->d_chunkPrefix;
        pa.nGroups = v->nGroups;
        pa.padSymbol = db->alphabet;
        pa.pack = v->d_pack;
        v->deviceBytes = packBytes + metaBytes;
        if (!packNow) {
            HIP_TRY(hipStreamSynchronize(up.ch->stream));   // (the bounce buffer goes back to the pool)
            v->pendingPack = pa;
            v->packPending = true;
            pt.mark("view: upload (pack later)");
        } else {
            // (the channel's own stream, and a wait for that stream only: other threads' searches go on)
            HIP_TRY(launchPack(pa, v->totalChunks, up.ch->stream));
            HIP_TRY(hipStreamSynchronize(up.ch->stream));
            pt.mark("view: upload + pack");
        }
    }
    v->ids = std::move(ids);
    *out = v;
    return 0;
}

int finishView(MiopalDb* db, View* v) {
    if (!v->packPending) return 0;
    PhaseTimer pt;
    UploadLease up(db);
    RC_TRY(up.acquire(256));
    HIP_TRY(launchPack(v->pendingPack, v->totalChunks, up.ch->stream));
    HIP_TRY(hipStreamSynchronize(up.ch->stream));
    v->packPending = false;
    pt.mark("view: pack (lists built beside the upload)");
    return 0;
}

// Cache of packed views, most recent first. A view is about as large as the slice it packs, so
// the cache is bounded by bytes (a share of the device's memory) as well as by count; thread-chunked
// callers (src/pyopal/_align.py:150-170) re-use their slice on every query, queries of different
// lengths add segmented views of the same slice. A view is built OUTSIDE the lock - other threads
// keep searching their own views meanwhile - behind a placeholder that threads wanting the same
// view wait on. Views in use are kept alive by their shared_ptr whatever the cache drops.
void evictViews(MiopalDb* db, size_t budget, size_t keepCount) {
    size_t total = 0, n = 0;
    for (const auto& s : db->views) {
        total += s.view ? s.view->deviceBytes : 0;
        ++n;
    }
    for (auto it = db->views.end(); it != db->views.begin() && (total > budget || n > keepCount);) {
        --it;
        if (it->building || it == db->views.begin()) continue;   // never the newest, never one being built
        total -= it->view ? it->view->deviceBytes : 0;
        --n;
        it = db->views.erase(it);
    }
}

// `build` fills the view (buildView; the self test of the guard injects its own). Whatever it does -
// return an error, or throw (its vectors have a million entries and parallelSlices rethrows what its
// worker threads threw) - the placeholder is gone and its waiters are woken when this returns: a
// placeholder left behind would block every later search of the same slice forever.
template <class Build>
int getViewWith(MiopalDb* db, int64_t start, int64_t end, int overlap, std::shared_ptr<View>* out, const Build& build,
                int stride = 0) {
    std::unique_lock<std::mutex> lk(db->viewMutex);
    for (;;) {
        auto it = db->views.begin();
        for (; it != db->views.end(); ++it)
            if (it->start == start && it->end == end && it->overlap == overlap && it->stride == stride) break;
        if (it == db->views.end()) break;
        if (!it->building) {
            *out = it->view;
            db->views.splice(db->views.begin(), db->views, it);
            return 0;
        }
        db->viewReady.wait(lk);   // somebody is building this very view
    }
    db->views.push_front(MiopalDb::ViewSlot{start, end, overlap, stride, true, nullptr});
    lk.unlock();
    std::shared_ptr<View> v;
    auto guardedBuild = [&]() -> int {
        try {
            return build(&v);
        } catch (const std::bad_alloc&) {
            return fail(MIOPAL_ERR_INTERNAL, "out of host memory while building a packed view");
        } catch (const std::exception& e) {
            return fail(MIOPAL_ERR_INTERNAL, "building a packed view failed: %s", e.what());
        } catch (...) {
            return fail(MIOPAL_ERR_INTERNAL, "building a packed view failed");
        }
    };
    int rc = guardedBuild();
    if (rc != 0) {
        // most likely out of device memory: drop every idle view and try once more
        v.reset();
        lk.lock();
        evictViews(db, 0, 1);
        lk.unlock();
        (void)hipGetLastError();
        rc = guardedBuild();
    }
    lk.lock();
    auto mine = db->views.begin();
    for (; mine != db->views.end(); ++mine)
        if (mine->building && mine->start == start && mine->end == end && mine->overlap == overlap && mine->stride == stride) break;
    if (rc != 0) {
        if (mine != db->views.end()) db->views.erase(mine);
        db->viewReady.notify_all();
        return rc;
    }
    if (mine == db->views.end()) {   // (cannot happen: placeholders are only removed by their builder)
        db->views.push_front(MiopalDb::ViewSlot{start, end, overlap, stride, false, v});
    } else {
        mine->view = v;
        mine->building = false;
        db->views.splice(db->views.begin(), db->views, mine);
    }
    evictViews(db, db->viewBudgetBytes, kMaxCachedViews);
    db->viewReady.notify_all();
    *out = v;
    return 0;
}

int getView(MiopalDb* db, int64_t start, int64_t end, int overlap, std::shared_ptr<View>* out, int stride = 0) {
    return getViewWith(db, start, end, overlap, out,
                       [&](std::shared_ptr<View>* v) { return buildView(db, start, end, overlap, v, true, stride); }, stride);
}

