// Part of host.hip (included there, not a translation unit of its own): searchImpl: score / end / full alignment search behind miopalSearch, miopalSearchFlat.
// The passes behind the score / end pass of a `full` search are the steps of FullSearch, in the order searchImpl
// calls them; what they decide without the device is full_plan.h's (DESIGN.md 4.9).
namespace {

// the fields every lane-per-pair launch of a search or a pair list shares (`queryLength`: of the whole query buffer)
inline PerPairArgs perPairCommon(const MiopalDb* db, const Search& s, int queryLength, int alphabet, int gapOpen, int gapExt) {
    PerPairArgs a{};
    a.residues = db->d_residues;
    a.query = s.d_query;
    a.queryLength = queryLength;
    a.matrix = s.d_matrix;
    a.rows = s.d_rows;
    a.alphabet = alphabet;
    a.gapOpen = gapOpen;
    a.gapExt = gapExt;
    a.residueCount = db->total;
    return a;
}

// ... and every walk: the jobs, their directions, where the operations and their lengths go (fixed slots of `opsSlot`)
inline void fillWalk(WalkArgs* wa, const PairJob* jobs, int nJobs, const MiopalDb* db, const Search& s, int queryLength,
                     const void* dirs, void* ops, int64_t opsSlot, void* opsLen) {
    wa->jobs = jobs;
    wa->nJobs = nJobs;
    wa->residues = db->d_residues;
    wa->query = s.d_query;
    wa->dirs = (const uint8_t*)dirs;
    wa->ops = (uint8_t*)ops;
    wa->opsSlot = opsSlot;
    wa->queryLength = queryLength;
    wa->opsLen = (int32_t*)opsLen;
}

struct EventSet {
    std::vector<hipEvent_t> ev;
    int create(size_t count) {
        ev.assign(count, nullptr);
        for (auto& e : ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return 0;
    }
    ~EventSet() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

struct JoinedThread {
    std::thread t;
    ~JoinedThread() { if (t.joinable()) t.join(); }
};

// what the caller of searchImpl passed
struct FullCall {
    MiopalDb* db;
    const unsigned char* query;
    int queryLength, gapOpen, gapExt;
    const int* scoreMatrix;
    int alphabetLength, searchType, mode;
    int64_t start, end;
    int *score, *endTarget, *endQuery, *startTarget, *startQuery;
    unsigned char** alignment;
    int* alignmentLength;
    HostBytes* flatOps;
    int64_t* flatOff;
    const int* pssmRows;
    int64_t n;
    bool flat;

    int checkOutputs() const {
        if (!score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score output");
        if (searchType >= OPAL_SEARCH_SCORE_END && (!endTarget || !endQuery))
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
        if (searchType == OPAL_SEARCH_ALIGNMENT &&
            (!startTarget || !startQuery || (flat ? !flatOff : (!alignment || !alignmentLength))))
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "null alignment outputs");
        return 0;
    }
};

struct FullSearch : FullCall {
    PhaseTimer& pt;
    WorkspaceLease& lease;
    Search& s;
    Workspace* const ws;
    const hipStream_t stream;

    // ---- the score / end pass's outputs ----
    void *ps = nullptr, *pi = nullptr, *pj = nullptr;
    const bool wantEnd;
    size_t hostOff = 0;
    const size_t hostBytes;
    const int hostArrays;
    bool callerPinned = false;
    // A `full` search whose later passes stay on the device leaves the scores and end locations in the staging
    // buffer until its end: copying 12 MB into the caller's (fresh) pages here kept the device idle for 0.35 ms
    // between the end pass and the start-cell scan. (Whatever takes the host's paths below flushes first.)
    const bool deferResults;
    static constexpr size_t kDeferFrom = 64u << 10;
    // scores and end locations of a `full` search that have not been sent on their way to the host yet, and the copies
    // themselves: on the side stream, behind whatever the main stream has been given so far
    bool resultsPending = false;

    // ---- the later passes: planLaterPasses, scanStartCells ----
    DpRules fr{};
    const bool oneStrip;
    HostBytes localOps;
    std::vector<int64_t> localOff;
    HostBytes* outOps = nullptr;
    int64_t* outOff = nullptr;
    void *rs = nullptr, *ri = nullptr, *rj = nullptr, *pjobs = nullptr, *psq = nullptr, *pst = nullptr, *pmis = nullptr,
         *plen = nullptr, *pcompact = nullptr, *pts = nullptr;
    bool lanePerPair = false;
    PerPairArgs perPair{};
    int profileStride = 0;
    bool startCellsDone = false;   // (written by the scan itself: perpair_packed.hip)
    struct PackedScan {
        int bias = 0, stride = 0, zero = 0;
        size_t lds = 0;
    };

    // ---- the traceback: readWindowChecks, planTrace, allocTrace ----
    int64_t maxWindow = 1, windowStrips = 1;
    int packedBias = 0, packedStride = 0;
    size_t packedLds = 0;
    TracePlan plan{};
    int64_t batch = 0, maxHead = 0, nBatches = 0;   // (the plan's, after the allocations had their say)
    bool oneLaunch = false;
    int sortRows = 0;
    void *pd = nullptr, *pslots = nullptr, *pbins = nullptr, *psorted = nullptr, *phead = nullptr, *pheadDirs = nullptr,
         *pblock = nullptr, *ptotals = nullptr;
    size_t opsBase = 0;
    int64_t opsFetched = 0;
    int64_t opsCopiedOut = 0;   // of the fetched operations: already in the caller's buffer
    bool copyOutEarly = false;
    int64_t* fetchedTotal = nullptr;   // pinned: running total read back per batch
    int32_t *tscore = nullptr, *lens = nullptr;
    bool sideArrays = false, startsPending = false;
    // operation offsets from the lengths, and the traceback's scores against the search's, of the targets
    // whose arrays are on the host: [done, upTo)
    int64_t prefixDone = 0, wrongAt = -1;
    double shareClock0 = 0;
    PerPairArgs paAll{};
    int64_t preparedGroup = -1;   // first batch of the group whose lists the side stream has been given
    int64_t total = 0;
    // (the last members, in this order: on every way out the helpers go first, then the copier's join, the crew it
    // runs on, and the events)
    EventSet batchDone, traceStart, copyDone, jobsReady;
    std::unique_ptr<unpack::Crew> crew;
    JoinedThread copier;
    unpack::AsyncWork sharer, arrayer;   // (declared behind everything their tasks refer to: drained first on every way out)

    FullSearch(const FullCall& c, PhaseTimer& timer, WorkspaceLease& l, Search& search)
        : FullCall(c), pt(timer), lease(l), s(search), ws(l.ws), stream(l.ws->stream),
          wantEnd(c.searchType >= OPAL_SEARCH_SCORE_END), hostBytes(((size_t)c.n * sizeof(int32_t) + 255) & ~(size_t)255),
          hostArrays(c.searchType == OPAL_SEARCH_SCORE ? 1 : c.searchType == OPAL_SEARCH_SCORE_END ? 3 : 0),
          deferResults(c.searchType == OPAL_SEARCH_ALIGNMENT), oneStrip(c.queryLength <= kLanes) {}

    // ================================================================================================================
    // the score / end pass's outputs
    // ================================================================================================================

    // a caller's array as the device sees it: pinned, device-visible host memory that holds n entries; else null
    int32_t* devicePointerOf(void* p) const {
        // (the n entries must lie inside the pinned range: when the runtime can tell the range's extent and it
        // is too short, the bounce buffer is used instead)
        const size_t wantBytes = (size_t)n * sizeof(int32_t);
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer != nullptr) {
            hipDeviceptr_t base = nullptr;
            size_t extent = 0;
            if (hipMemGetAddressRange(&base, &extent, (hipDeviceptr_t)attr.devicePointer) == hipSuccess) {
                const size_t into = (size_t)((const char*)attr.devicePointer - (const char*)base);
                if (into > extent || extent - into < wantBytes) return nullptr;
            } else {
                (void)hipGetLastError();   // (extent unknown: registered memory on some runtimes)
            }
            return (int32_t*)attr.devicePointer;
        }
        (void)hipGetLastError();   // (an ordinary pointer is "invalid value" to the runtime)
        return nullptr;
    }

    // the device arrays of the pass, and where its kernels may write on the host: scores (and end locations) of a
    // score / end search may leave the kernel straight for pinned host memory
    int bindHostOutputs() {
        RC_TRY(ws->get(kScore, (size_t)n * sizeof(int32_t), &ps));
        if (wantEnd) {
            RC_TRY(ws->get(kEndI, (size_t)n * sizeof(int32_t), &pi));
            RC_TRY(ws->get(kEndJ, (size_t)n * sizeof(int32_t), &pj));
        }
        if (hostArrays == 0) return 0;
        // A caller whose result arrays are themselves pinned, device-visible host memory (hipHostMalloc,
        // hipHostRegister, a pinned torch tensor) gets the results written into them by the kernel: no
        // bounce buffer, no copy on the host.
        int32_t *cs = nullptr, *ci = nullptr, *cj = nullptr;
        if (!tuned(Tune::NO_CALLER_PINNED)) {
            cs = devicePointerOf(score);
            if (cs && hostArrays == 3) {
                ci = devicePointerOf(endQuery);
                cj = devicePointerOf(endTarget);
            }
        }
        if (cs && (hostArrays == 1 || (ci && cj))) {
            s.hostScoreOut = cs;
            s.hostEndIOut = ci;
            s.hostEndJOut = cj;
            s.hostScoreIsCallers = true;
            callerPinned = true;
            lease.callerVisibleOutputs = true;
            return 0;
        }
        // (room for the pass's own small uploads behind it, so that nothing drains or reallocates the
        // buffer before the kernel is launched; if it happens all the same the generation tells)
        RC_TRY(ws->reserveStaging(hostArrays * hostBytes + (1u << 20)));
        hostOff = ws->pinnedUsed;
        ws->pinnedUsed += hostArrays * hostBytes;
        s.hostScoreOut = (int32_t*)((char*)ws->pinned + hostOff);
        if (hostArrays == 3) {
            s.hostEndIOut = (int32_t*)((char*)ws->pinned + hostOff + hostBytes);
            s.hostEndJOut = (int32_t*)((char*)ws->pinned + hostOff + 2 * hostBytes);
        }
        s.hostScoreGeneration = ws->stagingGeneration;
        return 0;
    }

    // (forked: evFork has been recorded where the copies may start - the caller has enqueued more since)
    int sendResults(bool forked = false) {
        if (!resultsPending) return 0;
        resultsPending = false;
        RC_TRY(ws->ensureAux());
        if (!forked) HIP_TRY(hipEventRecord(ws->evFork, stream));
        HIP_TRY(hipStreamWaitEvent(ws->aux, ws->evFork, 0));
        RC_TRY(ws->stageDownload(score, ps, (size_t)n * sizeof(int), true));
        RC_TRY(ws->stageDownload(endQuery, pi, (size_t)n * sizeof(int), true));
        RC_TRY(ws->stageDownload(endTarget, pj, (size_t)n * sizeof(int), true));
        return 0;
    }

    // the pass's results on their way to the caller: written there by the kernel, written to the staging buffer by
    // the kernel, or still in HBM; then the wait for the pass
    int deliverScores() {
        if (s.wroteHost && callerPinned) {
            // (nothing to copy: visible to the host once the stream has drained, below)
        } else if (s.wroteHost) {
            if (s.hostScoreGeneration != ws->stagingGeneration)
                return fail(MIOPAL_ERR_INTERNAL, "the staging buffer was drained under a kernel that writes to it");
            ws->pending.push_back({score, hostOff, (size_t)n * sizeof(int32_t)});
            if (hostArrays == 3) {
                ws->pending.push_back({endQuery, hostOff + hostBytes, (size_t)n * sizeof(int32_t)});
                ws->pending.push_back({endTarget, hostOff + 2 * hostBytes, (size_t)n * sizeof(int32_t)});
            }
        } else {
            // (a `full` search: copied by the side stream, beside the start-cell scan - three copies of 4 MB in the
            // main stream kept the scan waiting for 0.25 ms on a million targets. They start at once, beside the scan's
            // small first kernels, which crawl meanwhile - a 2-us fill 75 us, the 29-us job list 86 us; started WITH the
            // scan kernel instead the first copy waited 1.1 ms for a free compute unit and the scan lasted 1.38 instead
            // of 1.22 ms, and the start cells' copies beside the first direction kernel cost it 0.12 ms: both tried,
            // the device finished 0.4-0.6 ms later)
            const bool beside = deferResults && n * sizeof(int) >= kDeferFrom && !tuned(Tune::NO_SIDE_COPIES);
            // (round 5: LATER still - beside the first direction kernel, which does not mind them; the small kernels between
            // the passes crawl beside a copy: the 30-us job list of the scan took 94 us, a 2-us fill 76 us)
            if (beside) {
                resultsPending = true;
            } else {
                RC_TRY(ws->stageDownload(score, ps, (size_t)n * sizeof(int)));
                if (wantEnd) {
                    RC_TRY(ws->stageDownload(endQuery, pi, (size_t)n * sizeof(int)));
                    RC_TRY(ws->stageDownload(endTarget, pj, (size_t)n * sizeof(int)));
                }
            }
        }
        if (s.d_stripError) RC_TRY(ws->stageDownload(&s.stripErrorHost, s.d_stripError, sizeof(int)));
        RC_TRY(ws->finishDownloads(deferResults ? kDeferFrom : SIZE_MAX));
        HIP_TRY(hipStreamSynchronize(stream));
        RC_TRY(s.checkStripError());
        return 0;
    }

    // ================================================================================================================
    // the later passes on the device: the rest of the pipeline stays in HBM
    // (start cells, traceback jobs, direction bytes and operations are produced and
    // consumed on the device; the host only prefix-sums the alignment lengths)
    // ================================================================================================================

    // which kernels the scan and the direction pass may use: one lane per pair, the query-profile form
    int planLaterPasses() {
        outOps = flatOps;
        outOff = flatOff;
        if (!flat) {
            localOff.assign((size_t)n + 1, 0);
            outOps = &localOps;
            outOff = localOff.data();
        }
        // one lane per pair (perpair.hip) instead of one wavefront per pair (intraseq.hip)
        // (it stages the query in LDS: up to 4096 residues; longer ones keep the wavefront-per-pair kernel)
        lanePerPair = queryLength <= 4096 && !tuned(Tune::NO_PERPAIR) && (n > kSmallSearch || !smallSearchAllowed(db));
        RC_TRY(s.ensurePairInputs());
        perPair = perPairCommon(db, s, queryLength, alphabetLength, gapOpen, gapExt);
        // the query-profile form of the kernel (signed bytes of score + open in LDS, columns on a sliding
        // scale of j x ext): queries whose profile fits 64 KB, matrices and gaps that fit the byte
        const bool profiled = !tuned(Tune::NO_PERPAIR_PROFILE) &&
                              perPairProfileBytes(queryLength, alphabetLength, &profileStride) > 0 &&
                              s.maxScore + gapOpen <= 127 && s.minScore + gapOpen > -128 && gapOpen >= 0 &&
                              gapExt >= 0 && (int64_t)db->maxLen * gapExt < (1 << 27) && db->total >= 4;
        if (!profiled) profileStride = 0;
        // (position-specific scores outside the byte profile: perpair_kernel's row-indexed form stages all the rows
        // in LDS; more rows than fit keep the wavefront-per-pair kernel, as queries beyond 4096 residues do)
        if (!profiled && pssmRows && perPairPssmBytes(queryLength, alphabetLength) == 0) lanePerPair = false;
        return 0;
    }

    // start cells: the reversed prefixes anchored on the end cells, scanned by one of three kernels
    int scanStartCells() {
        RC_TRY(ws->get(kJobs, (size_t)n * sizeof(PairJob), &pjobs));
        RC_TRY(ws->get(kStartQ, (size_t)n * sizeof(int32_t), &psq));
        RC_TRY(ws->get(kStartT, (size_t)n * sizeof(int32_t), &pst));
        RC_TRY(ws->get(kMismatch, 4 * sizeof(int), &pmis));   // [3]: job counter of the persistent start-cell scan
        RC_TRY(ws->get(kOpsLen, (size_t)n * sizeof(int32_t), &plen));
        RC_TRY(ws->get(kRScore, (size_t)n * sizeof(int32_t), &rs));
        HIP_TRY(hipMemsetAsync(pmis, 0, 4 * sizeof(int), stream));
        if (mode != OPAL_MODE_NW) {
            RC_TRY(ws->get(kRI, (size_t)n * sizeof(int32_t), &ri));
            RC_TRY(ws->get(kRJ, (size_t)n * sizeof(int32_t), &rj));
            // Which kernel scans the reversed prefixes. One strip: lane per pair (it stops at the
            // first column that holds the optimum). More strips: no early stop, every job sweeps
            // its whole prefix; a lane walks it alone (14 instructions per cell, but a wavefront
            // lasts as long as its longest lane), a wavefront per pair spends 64 lanes on it
            // (~50 instructions per 64-row column step). Rough cost of either, in ms, from the
            // mean and the longest target of the database:
            bool scanLanePerPair = lanePerPair;
            if (lanePerPair && !oneStrip) {
                const double strips = (double)((queryLength + kLanes - 1) / kLanes);
                const double meanLen = (double)db->total / (double)std::max<int64_t>(db->count, 1);
                const double perLane = scanLaneMs((double)n * strips * meanLen, strips * (double)db->maxLen);
                const double perWave = scanWaveMs((double)n * strips * (meanLen + 63), strips * (double)(db->maxLen + 63));
                // (test switch: one lane per pair whatever the cost estimates say)
                scanLanePerPair = perLane <= perWave || tuned(Tune::FORCE_LANE_PER_PAIR) != nullptr;
            }
            if (scanLanePerPair) g_lastFullRouting |= kRouteScanLane | (profileStride > 0 ? kRouteScanProfile : 0);
            PackedScan packed;
            if (packedScanApplies(scanLanePerPair, &packed)) RC_TRY(scanPacked(packed));
            else if (scanLanePerPair) RC_TRY(scanLanes());
            else RC_TRY(scanWaves());
        }
        if (!startCellsDone)
            HIP_TRY(launchStartCells((int)n, mode, gapOpen, gapExt, (const int32_t*)ps, (const int32_t*)pi,
                                     (const int32_t*)pj, (const int32_t*)rs, (const int32_t*)ri, (const int32_t*)rj,
                                     (int32_t*)psq, (int32_t*)pst, (int*)pmis, stream));
        return 0;
    }

    // Smith-Waterman prefixes with two pairs per lane (perpair_packed.hip): every half of a lane on its own
    // schedule - pair, strip, column - so neither sorted wavefronts nor a boundary line per PAIR are needed
    bool packedScanApplies(bool scanLanePerPair, PackedScan* p) const {
        // (HW too: the same cells, the answer only in the query's last row. OV - last row or last column, the last row
        // another one in every pair: a select tree per column)
        const bool packedRegion = (mode == OPAL_MODE_SW && fr.region == kAllCells) ||
                                  (mode == OPAL_MODE_HW && fr.region == kLastRow && !tuned(Tune::NO_PACKED_HW_SCAN)) ||
                                  (mode == OPAL_MODE_OV && fr.region == kLastRowCol && !tuned(Tune::NO_PACKED_HW_SCAN));
        if (!(scanLanePerPair && profileStride > 0 && packedRegion && !tuned(Tune::NO_PACKED_SCAN))) return false;
        // (no cell of a prefix scan beats the query's own best: every residue against its best partner)
        const int64_t ownBest = queryBest(queryLength, alphabetLength, [&](int y, int t) { return s.at(y, t); });
        const int64_t best = std::min<int64_t>(ownBest, std::min<int64_t>(queryLength, db->maxLen) * std::max(s.maxScore, 0));
        return packedScanFits(queryLength, alphabetLength, gapOpen, gapExt, s.maxScore, s.minScore, db->maxLen, best,
                              &p->bias, &p->zero, &p->stride, &p->lds) &&
               (oneStrip || ((n + 127) / 128) * kLanes * db->maxLen * (int64_t)sizeof(int2) <= (8ll << 30));
    }

    int scanPacked(const PackedScan& packed) {
        const DpRules rr{1, 1, 0, fr.region};
        g_lastFullRouting |= kRouteScanPacked | (oneStrip ? kRouteScanRefill : 0);
        PerPairArgs pa = perPair;
        // (the kernels write the start cells themselves: no reverse-pass arrays, no start_cells_kernel; the
        // one-strip kernel reads the end pass's arrays: no job list either)
        pa.startQ = (int32_t*)psq;
        pa.startT = (int32_t*)pst;
        pa.startChecks = (int*)pmis;
        pa.scanLastRow = mode == OPAL_MODE_HW ? 1 : mode == OPAL_MODE_OV ? 2 : 0;
        startCellsDone = true;
        pa.jobs = nullptr;
        pa.fwdScore = (const int32_t*)ps;
        pa.fwdEndQ = (const int32_t*)pi;
        pa.fwdEndT = (const int32_t*)pj;
        pa.fwdOffsets = db->d_offsets + start;
        if (oneStrip && n >= 4 * kLanes * db->computeUnits && !tuned(Tune::NO_SCAN_ORDER)) {
            // longest prefixes first (intraseq.hip, launchSortIndicesByKey): the scan of a pair ends within its prefix
            void *bins, *porder;
            RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &bins));
            RC_TRY(ws->get(kScanOrder, (size_t)n * sizeof(int), &porder));
            HIP_TRY(launchSortIndicesByKey((const int32_t*)pj, (int)n, (int)db->maxLen, (int*)bins, (int*)porder, stream));
            pa.order = (const int*)porder;
        }
        if (!oneStrip) {
            HIP_TRY(launchReverseJobs((int)n, (const int32_t*)ps, (const int32_t*)pi, (const int32_t*)pj,
                                      db->d_offsets + start, packRules(rr), 0, (PairJob*)pjobs, stream));
            // longest prefixes first: the persistent wavefronts end together
            void *bins, *sorted;
            RC_TRY(ws->get(kSortBins, (size_t)(std::min<int64_t>(db->maxLen, 8191) + 1) * sizeof(int), &bins));
            RC_TRY(ws->get(kSortedJobs, (size_t)n * sizeof(PairJob), &sorted));
            HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, (int)n, (int)db->maxLen, (int*)bins, (PairJob*)sorted, stream));
            pa.jobs = (const PairJob*)sorted;
            void* pb;
            RC_TRY(ws->get(kPairB0, (size_t)((n + 127) / 128) * kLanes * db->maxLen * sizeof(int2), &pb));
            pa.boundary = (int2*)pb;
            pa.boundaryStride = db->maxLen;
        }
        pa.nJobs = (int)n;
        pa.score = (int32_t*)rs;
        pa.endI = (int32_t*)ri;
        pa.endJ = (int32_t*)rj;
        pa.profileStride = packed.stride;
        pa.packedBias = packed.bias;
        pa.packedZero = packed.zero;
        pa.reversed = 1;
        pa.jobCounter = (int*)pmis + 3;
        pa.computeUnits = db->computeUnits;
        HIP_TRY(launchPerPairPackedScan(pa, packed.lds, stream));
        return 0;
    }

    int scanLanes() {
        const DpRules rr{1, 1, 0, fr.region};
        // chunks of whole wavefronts whose strip boundaries (8 B per column and pair) fit 4 GB
        const int64_t chunk = oneStrip ? n : std::max<int64_t>(kLanes, (4ll << 30) / (8 * db->maxLen) / kLanes * kLanes);
        void *pb = nullptr, *bins = nullptr, *sorted = nullptr;
        if (!oneStrip) {
            const int64_t most = std::min(chunk, n);
            RC_TRY(ws->get(kPairB0, boundaryBytes(most, db->maxLen), &pb));
            // prefixes of similar length share a wavefront (results stay addressed by job.out)
            RC_TRY(ws->get(kSortBins, (size_t)(std::min<int64_t>(db->maxLen, 8191) + 1) * sizeof(int), &bins));
            RC_TRY(ws->get(kSortedJobs, (size_t)most * sizeof(PairJob), &sorted));
        }
        for (int64_t c0 = 0; c0 < n; c0 += chunk) {
            const int nc = (int)std::min<int64_t>(chunk, n - c0);
            const PairJob* jobs = (PairJob*)pjobs + c0;
            HIP_TRY(launchReverseJobs(nc, (const int32_t*)ps + c0, (const int32_t*)pi + c0, (const int32_t*)pj + c0,
                                      db->d_offsets + start + c0, packRules(rr), 0, (PairJob*)pjobs + c0, stream));
            if (!oneStrip) {
                HIP_TRY(launchSortJobsByLength(jobs, nc, (int)db->maxLen, (int*)bins, (PairJob*)sorted, stream));
                jobs = (const PairJob*)sorted;
            }
            PerPairArgs pa = perPair;
            pa.jobs = jobs;
            pa.nJobs = nc;
            pa.score = (int32_t*)rs + c0;
            pa.endI = (int32_t*)ri + c0;
            pa.endJ = (int32_t*)rj + c0;
            pa.boundary = (int2*)pb;
            pa.boundaryStride = db->maxLen;
            pa.profileStride = profileStride;
            pa.reversed = 1;
            if (oneStrip && profileStride > 0 && !tuned(Tune::NO_SCAN_REFILL)) {
                // persistent wavefronts whose lanes take the next pair when they are done
                // (one strip: one launch, the counter is still zero)
                pa.jobCounter = (int*)pmis + 3;
                pa.computeUnits = db->computeUnits;
                g_lastFullRouting |= kRouteScanRefill;
            }
            HIP_TRY(launchPerPair(pa, fr.region, stream));
        }
        return 0;
    }

    int scanWaves() {
        const DpRules rr{1, 1, 0, fr.region};
        // chunks of targets whose strip boundaries (16 B per column and pair) fit 4 GB
        const int64_t wsStride = oneStrip ? 0 : db->maxLen;
        const int64_t chunk = oneStrip ? n : std::max<int64_t>(1, (4ll << 30) / (16 * wsStride));
        for (int64_t c0 = 0; c0 < n; c0 += chunk) {
            const int nc = (int)std::min<int64_t>(chunk, n - c0);
            PairJob* jobs = (PairJob*)pjobs + c0;
            HIP_TRY(launchReverseJobs(nc, (const int32_t*)ps + c0, (const int32_t*)pi + c0, (const int32_t*)pj + c0,
                                      db->d_offsets + start + c0, packRules(rr), wsStride, jobs, stream));
            RC_TRY(s.runDeviceJobs(jobs, nc, (int32_t*)rs + c0, (int32_t*)ri + c0, (int32_t*)rj + c0, false, nullptr, wsStride));
        }
        return 0;
    }

    // The slots of the traceback are sized by the longest target window of the slice
    // (local alignments are short whatever the targets' lengths): one small D2H + sync.
    int readWindowChecks() {
        int checks[3] = {0, 0, 0};
        RC_TRY(ws->stageDownload(checks, pmis, sizeof checks));
        RC_TRY(ws->finishDownloads(deferResults ? kDeferFrom : SIZE_MAX));
        if (checks[0])
            return fail(MIOPAL_ERR_INTERNAL, "reverse pass disagrees with the forward score for target %lld",
                        (long long)(start + checks[0] - 1));
        maxWindow = std::max(checks[1], 1);
        windowStrips = (std::max(checks[2], 1) + kLanes - 1) / kLanes;  // tallest query window
        return 0;
    }

    // the batches of the traceback, the kernel of the direction pass and how the operations leave: full_plan.h
    void planTrace() {
        // two pairs per lane on 16-bit halves (perpair_packed.hip) when the scoring scheme and the windows fit
        bool packedOk = false;
        if (lanePerPair && profileStride > 0 && !tuned(Tune::NO_PACKED_TRACE)) {
            const int64_t rows = windowStrips * kLanes, columns = round4(maxWindow);
            const int64_t best = std::min(rows, columns) * std::max(s.maxScore, 0);
            packedOk = packedTraceFits(queryLength, alphabetLength, gapOpen, gapExt, s.maxScore, s.minScore,
                                       rows, columns, best, &packedBias, &packedStride, &packedLds);
        }
        PlanSwitches sw;
        sw.forceLanePerPair = tuned(Tune::FORCE_LANE_PER_PAIR) != nullptr;
        sw.noHybridTrace = tuned(Tune::NO_HYBRID_TRACE) != nullptr;
        sw.noOneLaunch = tuned(Tune::NO_ONE_LAUNCH) != nullptr;
        if (const char* e = tuned(Tune::ONE_LAUNCH_GROUP)) {
            sw.groupSet = true;
            sw.group = atoi(e);
        }
        plan = miopal::planTrace(n, queryLength, windowStrips, maxWindow, db->computeUnits, lanePerPair, profileStride > 0, packedOk, sw);
        if (!plan.fits) return;   // (host-built batches: nothing of the plan is used)
        g_lastFullRouting |= plan.routing;
        if (pt.on)
            fprintf(stderr, "[miopal]   traceback: longest window %lld columns, %lld strip(s) of rows, %lld pairs per batch, %s per pair\n",
                    (long long)maxWindow, (long long)windowStrips, (long long)plan.batch,
                    plan.traceLanePerPair ? "lane" : "wavefront");
    }

    // the traceback's workspaces: what is refused changes the plan (no hybrid head, a launch per batch, smaller batches)
    int allocTrace() {
        const int64_t slotDir = plan.slotDir, slotOps = plan.slotOps;
        // (whole units of 64 operations: copy_out_packed_kernel reads the unit a batch ends in to its end)
        RC_TRY(ws->get(kCompactOps, ((size_t)(n * slotOps) + 63) & ~(size_t)63, &pcompact));
        batch = plan.batch;
        // (the windows' rows as a minor sort key: common.h)
        sortRows = tuned(Tune::NO_SORT_BY_ROWS) ? 0 : queryLength;
        // hybrid: direction bytes for the outliers a wavefront-per-pair pass takes
        maxHead = plan.maxHead;
        if (maxHead > 0) {
            RC_TRY(ws->get(kHeadWaves, sizeof(int), &phead));
            if (!ws->tryGet(kHeadDirs, (size_t)(maxHead * kLanes * slotDir), &pheadDirs)) maxHead = 0;
        }
        // The packed direction pass of EVERY batch in one launch (round 5): a batch of cfg3 is one round of the
        // chip, so its kernel lasted as long as its longest wavefront - 0.5 ms where the work is 0.15 ms - and
        // four of them ran one after the other. The batches' job lists are sorted one by one (the walk, the
        // gather and the copies stay batch by batch), laid end to end, and swept by one launch whose late
        // wavefronts are the last batch's short ones; the directions of a group's pairs stay in HBM meanwhile.
        oneLaunch = plan.oneLaunch;
        void* pdAll = nullptr;
        if (oneLaunch && !ws->tryGet(kDirs, (size_t)(plan.groupSlots * plan.slotDirUsed), &pdAll)) oneLaunch = false;
        if (oneLaunch) g_lastFullRouting |= kRouteOneLaunch;
        if (maxHead > 0 && oneLaunch) RC_TRY(ws->get(kHeadWaves, (size_t)plan.nBatchesPlanned * sizeof(int), &phead));
        if (plan.traceLanePerPair) {
            RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
            RC_TRY(ws->get(kSortedJobs, (size_t)(oneLaunch ? plan.allSlots : batch) * sizeof(PairJob), &psorted));
        }
        // the direction workspace is the one allocation that can be refused on a GPU shared
        // with other work: halve the batch until it fits
        if (oneLaunch) pd = pdAll;
        while (!oneLaunch && !ws->tryGet(kDirs, (size_t)(batch * plan.slotDirUsed), &pd)) {
            if (batch <= kLanes) return fail(MIOPAL_ERR_HIP, "out of device memory for the traceback workspace");
            batch = std::max<int64_t>(kLanes, batch / 2 / kLanes * kLanes);
        }
        RC_TRY(ws->get(kOps, (size_t)(batch * slotOps), &pslots));
        RC_TRY(ws->get(kTraceScore, (size_t)n * sizeof(int32_t), &pts));
        // Operations leave for the host batch by batch, on the side stream, while the next batch
        // is computed: at least four batches when there are enough pairs to fill the chip with
        // each (the copy of the last batch is all that is not hidden). They are staged in
        // pinned memory, contiguously, and copied out once the total is known.
        nBatches = (n + batch - 1) / batch;
        if (plan.overlapOps) RC_TRY(reserveOpsStaging());
        // (host scratch kept on the workspace: no malloc / free of megabytes per search)
        if (ws->hostScratchA.size() < (size_t)n) ws->hostScratchA.resize((size_t)n);
        if (ws->hostScratchB.size() < (size_t)n) ws->hostScratchB.resize((size_t)n);
        tscore = ws->hostScratchA.data();
        lens = ws->hostScratchB.data();
        // The small per-target arrays leave on the side stream as they become final - the start cells now,
        // lengths and traceback scores batch by batch - instead of four copies of 4 MB behind the last batch
        // (0.3 ms of a million targets' search with nothing else left to run beside them).
        sideArrays = plan.overlapOps && !tuned(Tune::NO_SIDE_COPIES);
        startsPending = sideArrays;
        outOff[0] = 0;
        RC_TRY(ws->get(kOpsOff, (size_t)((batch + 255) / 256) * sizeof(int64_t), &pblock));
        RC_TRY(ws->get(kOpsTotals, (size_t)(nBatches + 1) * sizeof(int64_t), &ptotals));
        HIP_TRY(hipMemsetAsync(ptotals, 0, sizeof(int64_t), stream));
        shareClock0 = PhaseTimer::now();
        return 0;
    }

    // the events of the overlapped copies, their room in the staging buffer, and the caller's buffer at its worst case
    int reserveOpsStaging() {
        RC_TRY(ws->ensureAux());
        RC_TRY(batchDone.create((size_t)nBatches));
        RC_TRY(traceStart.create((size_t)nBatches));
        RC_TRY(copyDone.create((size_t)nBatches));
        // room for the operations, the running totals and the small per-target arrays that
        // follow, reserved in one go (a later drain would reset the staging buffer)
        // (the operations cross PCIe two bits each - copy_out_packed_kernel - a quarter of a byte per operation)
        // (with the scores and end locations when they are still to be sent: sendResults)
        const StagingPlan room = planStaging(n, plan.opsCap, nBatches, resultsPending);
        RC_TRY(ws->reserveStaging(room.reserve));
        fetchedTotal = (int64_t*)((char*)ws->pinned + ws->pinnedUsed);
        opsBase = ws->pinnedUsed + room.head;   // (256-byte aligned: pinnedUsed and head are)
        ws->pinnedUsed = opsBase + ((room.stagedOps + 255) & ~(size_t)255);
        // The caller's buffer is filled batch by batch as the operations land (room for the worst
        // case; pages that stay untouched are never committed): only the last batch's share is
        // copied after the device has finished.
        // (a host that refuses the worst case gets its operations in one piece at the end, as before)
        copyOutEarly = outOps->resize((size_t)plan.opsCap);
        return 0;
    }

    // operations of the staged stream -> the caller's buffer (the unpacking of two-bit codes)
    void opsToCaller(uint8_t* out, int64_t from, int64_t to, int threads) const {
        if (to > from) unpack::ops(out, (const uint8_t*)ws->pinned + opsBase, from, to, threads);
    }

    // (beside the first direction kernel, with the scores and end locations)
    int sendEarlyArrays(bool forked = false) {
        RC_TRY(sendResults(forked));
        if (startsPending) {
            startsPending = false;
            if (!forked) HIP_TRY(hipEventRecord(ws->evFork, stream));
            HIP_TRY(hipStreamWaitEvent(ws->aux, ws->evFork, 0));
            RC_TRY(ws->stageDownload(startQuery, psq, (size_t)n * sizeof(int32_t), true));
            RC_TRY(ws->stageDownload(startTarget, pst, (size_t)n * sizeof(int32_t), true));
        }
        return 0;
    }

    // (two loops: the running sum is one add per target and nothing else; the comparison has no chain and
    // vectorises - together, with the branch inside, they took 1.2 ns a target, 0.3-0.4 ms per batch of cfg3 on
    // the thread that was the last to finish)
    void prefixUpTo(int64_t upTo) {
        if (upTo <= prefixDone) return;
        const int32_t* const ln = lens;
        int64_t run = outOff[prefixDone];
        for (int64_t k = prefixDone; k < upTo; ++k) {
            run += ln[k];
            outOff[k + 1] = run;
        }
        if (wrongAt < 0) {
            const int32_t* const ts = tscore;
            int differs = 0;
            for (int64_t k = prefixDone; k < upTo; ++k)
                differs |= (int)((endQuery[k] >= 0) & (endTarget[k] >= 0) & (ts[k] != score[k]));
            if (differs)
                for (int64_t k = prefixDone; k < upTo && wrongAt < 0; ++k)
                    if (endQuery[k] >= 0 && endTarget[k] >= 0 && ts[k] != score[k]) wrongAt = k;
        }
        prefixDone = upTo;
    }

    // The host's own share of a batch - its operations into the caller's buffer, its slices of the per-target
    // arrays into the caller's arrays, its offsets - is done as soon as the batch's copies have LANDED
    // (`copyDone`), while the device is at work on the next batch; it used to wait for the next batch's
    // gather first, so that behind the last gather the host still had two shares to unpack, one after
    // the other (0.4 + 0.5 ms of a cfg3 search with the device idle).
    int hostShare(int64_t landed, int64_t upToBatch) {
        // (up to the last whole unit of what has landed - the unit a batch ends in is written again,
        // complete, by the next batch's copy)
        const int64_t settled = landed & ~(int64_t)63;
        const int64_t from = opsCopiedOut;
        int64_t to = from;
        if (copyOutEarly && settled > opsCopiedOut) {
            to = settled;
            opsCopiedOut = settled;
        }
        // scores, end locations and start cells the first time (20 MB of a million targets), a batch's
        // lengths and traceback scores after that - and the offsets of the batches that are complete
        std::vector<Workspace::Pending> entries;
        if (sideArrays) entries = ws->takeSideEntries();
        const int64_t upTo = std::min<int64_t>(n, upToBatch * batch);
        uint8_t* const out = outOps->data;
        const bool arrays = sideArrays;
        const bool timed = pt.on;
        const double searchT0 = shareClock0;
        // (two helpers: the operations on one, the arrays and the offsets on the other - one after the other
        // they took 0.6-0.7 ms per batch, more than the device needs for a batch, and the thread they shared
        // finished 0.5-1 ms after the device)
        auto workOps = [this, out, from, to, timed, searchT0] {
            const double t0 = timed ? PhaseTimer::now() : 0;
            if (to > from) opsToCaller(out, from, to, 4);
            if (timed)
                fprintf(stderr, "[miopal]     share at %.3f ms: %lld operations %.3f ms\n", (t0 - searchT0) * 1e3,
                        (long long)(to - from), (PhaseTimer::now() - t0) * 1e3);
        };
        auto workArrays = [this, upTo, timed, searchT0, entries = std::move(entries)] {
            const double t0 = timed ? PhaseTimer::now() : 0;
            size_t bytes = 0;
            for (const auto& e : entries) bytes += e.bytes;
            ws->copyOutEntries(entries);
            const double t1 = timed ? PhaseTimer::now() : 0;
            prefixUpTo(upTo);
            if (timed)
                fprintf(stderr, "[miopal]     share at %.3f ms: %.1f MB of arrays %.3f ms, offsets %.3f ms\n",
                        (t0 - searchT0) * 1e3, bytes / 1e6, (t1 - t0) * 1e3, (PhaseTimer::now() - t1) * 1e3);
        };
        if (tuned(Tune::NO_ASYNC_SHARES)) {
            workOps();
            if (arrays) workArrays();
        } else {
            if (to > from) sharer.submit(std::move(workOps));
            if (arrays) arrayer.submit(std::move(workArrays));
        }
        return 0;
    }

    // batch b's compacted operations: wait for its gather on the side stream, read the
    // running total, start the copy of its share
    int fetchOps(int64_t b) {
        if (b > 0 && !tuned(Tune::NO_EARLY_HOST_SHARE)) {
            // (nothing has been staged on the side stream since that event was recorded)
            HIP_TRY(hipEventSynchronize(copyDone.ev[(size_t)b - 1]));
            RC_TRY(hostShare(opsFetched, b));
        }
        HIP_TRY(hipStreamWaitEvent(ws->aux, batchDone.ev[(size_t)b], 0));
        HIP_TRY(hipMemcpyAsync(fetchedTotal + b, (const int64_t*)ptotals + b + 1, sizeof(int64_t),
                               hipMemcpyDeviceToHost, ws->aux));
        HIP_TRY(hipStreamSynchronize(ws->aux));
        // (that wait covers whatever the side stream had been asked to copy before it)
        const int64_t landed = opsFetched;
        const int64_t upTo = fetchedTotal[b];
        if (upTo < opsFetched || upTo > plan.opsCap) return fail(MIOPAL_ERR_INTERNAL, "bad operation count");
        // Two things about a device-to-host copy beside the next batch (kernel traces of cfg3,
        // profiles/r03_full_copy_overlap.txt). The runtime's copy is a kernel that fills the chip: a
        // direction kernel of 0.49 ms beside it lasted 0.78 ms; copy_out_packed_kernel keeps to 64 workgroups.
        // And while either copy runs, the SMALL kernels of the main
        // stream crawl (the 12-us sort and the 12-us outlier pass: 240-350 us each, whichever came
        // first), the direction kernel does not (+ 30 us): so the copy starts with the next batch's
        // direction kernel, not before.
        if (upTo > opsFetched && b + 1 < nBatches)
            HIP_TRY(hipStreamWaitEvent(ws->aux, traceStart.ev[(size_t)b + 1], 0));
        if (upTo > opsFetched) {
            // (whole units of 64 operations: the unit a batch ends in is packed again, complete, with the next)
            HIP_TRY(launchCopyOutPacked(pcompact, (char*)ws->pinned + opsBase, opsFetched / 64, (upTo + 63) / 64, ws->aux));
        }
        opsFetched = upTo;
        // (round 4, first form: the share of the batch before, here - behind this batch's gather)
        if (b == 0 || tuned(Tune::NO_EARLY_HOST_SHARE)) RC_TRY(hostShare(landed, b));
        if (sideArrays) {
            // this batch's slices, behind its operations
            const int64_t b0 = b * batch, nb = std::min<int64_t>(batch, n - b0);
            RC_TRY(ws->stageDownload(lens + b0, (const int32_t*)plen + b0, (size_t)nb * sizeof(int32_t), true));
            RC_TRY(ws->stageDownload(tscore + b0, (const int32_t*)pts + b0, (size_t)nb * sizeof(int32_t), true));
        }
        HIP_TRY(hipEventRecord(copyDone.ev[(size_t)b], ws->aux));
        return 0;
    }

    // the traceback jobs of `count` pairs from b0 on
    hipError_t traceJobs(int64_t b0, int count, hipStream_t on) {
        return launchTraceJobs(count, packRules(DpRules{1, 1, 0, kLastCell}), (const int32_t*)psq + b0, (const int32_t*)pst + b0,
                               (const int32_t*)pi + b0, (const int32_t*)pj + b0, db->d_offsets + start + b0, plan.slotDir,
                               windowStrips > 1 ? maxWindow : 0, (PairJob*)pjobs + b0, on);
    }

    // the job lists of a group's batches, each sorted: eight small kernels per batch, 0.15 ms per group of cfg3.
    // The first group's run where they always ran; the NEXT group's are built on the side stream beside the
    // direction kernel of the group at hand (they need the start cells only, and their own parts of the lists)
    int prepareGroup(int64_t firstBatch, hipStream_t on) {
        const int64_t g0 = firstBatch * batch, g1 = std::min<int64_t>(n, (firstBatch + plan.dirGroup) * batch);
        for (int64_t b0 = g0, b = firstBatch; b0 < g1; b0 += batch, ++b) {
            const int nb = (int)std::min<int64_t>(batch, n - b0);
            HIP_TRY(traceJobs(b0, nb, on));
            HIP_TRY(launchSortJobsByLength((PairJob*)pjobs + b0, nb, (int)maxWindow, (int*)pbins, (PairJob*)psorted + b0, on,
                                           maxHead > 0 ? (int*)phead + b : nullptr, (int)maxHead, sortRows));
        }
        return 0;
    }

    // the packed direction pass of the group of batches that starts at firstBatch, in one launch
    int launchGroup(int64_t firstBatch) {
        const int64_t g0 = firstBatch * batch, g1 = std::min<int64_t>(n, (firstBatch + plan.dirGroup) * batch);
        if (preparedGroup == firstBatch) HIP_TRY(hipStreamWaitEvent(stream, jobsReady.ev[0], 0));
        else RC_TRY(prepareGroup(firstBatch, stream));
        paAll = perPair;
        paAll.jobs = (const PairJob*)psorted + g0;
        paAll.nJobs = (int)(g1 - g0);
        paAll.dirs = (uint8_t*)pd;   // (the group's own buffer: the walks of the group before are done)
        paAll.score = (int32_t*)pts + g0;   // job.out is relative to the batch: outBatch
        paAll.outBatch = (int)batch;
        paAll.skipWaves = maxHead > 0 ? (const int*)phead + firstBatch : nullptr;
        paAll.dirWaveStride = plan.slotDirUsed * kLanes;
        paAll.dirStripColumns = dirStripColumns(true, maxWindow);
        if (windowStrips > 1) {
            void* pb;
            RC_TRY(ws->get(kPairB0, boundaryBytes(g1 - g0, maxWindow), &pb));
            paAll.boundary = (int2*)pb;
            paAll.boundaryStride = maxWindow;
        }
        paAll.profileStride = packedStride;
        paAll.packedBias = packedBias;
        paAll.reversed = 0;
        // (the big arrays leave beside THIS kernel - behind the job lists and their sorts, which crawl beside a
        // copy. The kernel is enqueued FIRST: the five copies took the host 90 us, with the device idle)
        const bool arrays = resultsPending || startsPending;
        const bool ahead = plan.overlapOps && g1 < n && !tuned(Tune::NO_JOBS_AHEAD);
        if (arrays || ahead) RC_TRY(ws->ensureAux());
        if (arrays) HIP_TRY(hipEventRecord(ws->evFork, stream));
        HIP_TRY(launchPerPairPackedTrace(paAll, packedLds, stream));
        if (arrays) RC_TRY(sendEarlyArrays(true));
        if (ahead) {
            // (BEHIND the direction kernel, beside the first walk: beside the direction kernel itself - which
            // holds every register of the chip - the lists took 0.5 ms, the kernel 0.84 instead of 0.79 ms, and
            // the copies behind them ran into the walk)
            if (jobsReady.ev.empty()) RC_TRY(jobsReady.create(2));
            HIP_TRY(hipEventRecord(jobsReady.ev[1], stream));
            HIP_TRY(hipStreamWaitEvent(ws->aux, jobsReady.ev[1], 0));
            RC_TRY(prepareGroup(firstBatch + plan.dirGroup, ws->aux));
            HIP_TRY(hipEventRecord(jobsReady.ev[0], ws->aux));
            preparedGroup = firstBatch + plan.dirGroup;
        }
        return 0;
    }

    // where the copy of the batch before may start, and the big arrays' departure beside the first direction kernel
    int markTraceStart(int64_t b, bool startMarked) {
        if (plan.overlapOps && !startMarked) HIP_TRY(hipEventRecord(traceStart.ev[(size_t)b], stream));
        RC_TRY(sendEarlyArrays());
        return 0;
    }

    // the outliers at the head of a batch's sorted list: one wavefront per pair
    int traceHead(int64_t b0, int nb, const PairJob* jobs, const int* headWaves, WalkArgs* wa) {
        const int nh = (int)std::min<int64_t>(nb, maxHead * kLanes);
        RC_TRY(s.runDeviceJobs(jobs, nh, (int32_t*)pts + b0, nullptr, nullptr, true, (uint8_t*)pheadDirs,
                               windowStrips > 1 ? maxWindow : 0, headWaves, plan.slotDir));
        wa->headWaves = headWaves;
        wa->headDirs = (const uint8_t*)pheadDirs;
        wa->headDirStride = plan.slotDir;
        return 0;
    }

    // batch b of a group launch: sorted and swept by launchGroup; what is left per batch: the outliers at the head of its list
    int traceBatchOfGroup(int64_t b, int64_t b0, int nb, bool startMarked, const PairJob** jobs, WalkArgs* wa) {
        *jobs = (PairJob*)psorted + b0;
        wa->slotByOut = 1;
        RC_TRY(markTraceStart(b, startMarked));
        if (maxHead > 0) RC_TRY(traceHead(b0, nb, *jobs, (const int*)phead + b, wa));
        wa->dirPlanes = 1;
        wa->dirColumnMajor = 1;
        wa->dirWaveStride = paAll.dirWaveStride;
        wa->dirStripColumns = paAll.dirStripColumns;
        return 0;
    }

    // batch b on one lane per pair, a launch of its own: the 32-bit kernel, its profile form or the packed one
    int traceBatchOnLanes(int64_t b, int64_t b0, int nb, const PairJob** jobs, WalkArgs* wa) {
        // neighbours of similar length share a wavefront; results stay addressed by job.out
        HIP_TRY(launchSortJobsByLength(*jobs, nb, (int)maxWindow, (int*)pbins, (PairJob*)psorted, stream, (int*)phead,
                                       (int)maxHead, sortRows));
        *jobs = (PairJob*)psorted;
        wa->slotByOut = 1;
        PerPairArgs pa = perPair;
        if (maxHead > 0) {
            RC_TRY(traceHead(b0, nb, *jobs, (const int*)phead, wa));
            pa.skipWaves = (const int*)phead;
        }
        pa.jobs = *jobs;
        pa.nJobs = nb;
        pa.dirs = (uint8_t*)pd;
        pa.score = (int32_t*)pts + b0;  // job.out is relative to the batch
        pa.dirWaveStride = plan.slotDirUsed * kLanes;
        pa.dirStripColumns = dirStripColumns(profileStride > 0, maxWindow);
        if (windowStrips > 1) {
            void* pb;
            RC_TRY(ws->get(kPairB0, boundaryBytes(nb, maxWindow), &pb));
            pa.boundary = (int2*)pb;
            pa.boundaryStride = maxWindow;
        }
        pa.profileStride = profileStride;
        pa.reversed = 0;
        RC_TRY(markTraceStart(b, false));
        if (plan.packedTrace) {
            pa.profileStride = packedStride;
            pa.packedBias = packedBias;
            HIP_TRY(launchPerPairPackedTrace(pa, packedLds, stream));
            wa->dirColumnMajor = 1;
        } else {
            HIP_TRY(launchPerPair(pa, kPerPairTrace, stream));
        }
        wa->dirPlanes = profileStride > 0;
        wa->dirWaveStride = pa.dirWaveStride;
        wa->dirStripColumns = pa.dirStripColumns;
        return 0;
    }

    // batch b: its jobs, its directions by one of three routes, its walk and gather, and the batch before on its way out
    int traceBatch(int64_t b) {
        const int64_t b0 = b * batch;
        const int nb = (int)std::min<int64_t>(batch, n - b0);
        const PairJob* jobs = (PairJob*)pjobs + b0;
        bool startMarked = false;
        if (oneLaunch && b % plan.dirGroup == 0) {
            // (the copy of the batch before starts beside this launch, not behind it)
            if (plan.overlapOps) HIP_TRY(hipEventRecord(traceStart.ev[(size_t)b], stream));
            startMarked = true;
            RC_TRY(launchGroup(b));
        }
        if (!oneLaunch) HIP_TRY(traceJobs(b0, nb, stream));
        // job.out is relative to the batch: offset the score pointer
        WalkArgs wa{};
        if (plan.traceLanePerPair && oneLaunch) {
            RC_TRY(traceBatchOfGroup(b, b0, nb, startMarked, &jobs, &wa));
        } else if (plan.traceLanePerPair) {
            RC_TRY(traceBatchOnLanes(b, b0, nb, &jobs, &wa));
        } else {
            RC_TRY(markTraceStart(b, startMarked));
            RC_TRY(s.runDeviceJobs(jobs, nb, (int32_t*)pts + b0, nullptr, nullptr, true, (uint8_t*)pd, windowStrips > 1 ? maxWindow : 0));
        }
        RC_TRY(walkAndGather(b, b0, nb, jobs, &wa));
        if (plan.overlapOps) {
            HIP_TRY(hipEventRecord(batchDone.ev[(size_t)b], stream));
            if (b > 0) RC_TRY(fetchOps(b - 1));   // batch b is queued behind it: the GPU stays busy
        }
        return 0;
    }

    // directions -> operations in the batch's slots -> compacted behind the batches before
    int walkAndGather(int64_t b, int64_t b0, int nb, const PairJob* jobs, WalkArgs* wa) {
        const uint8_t* dirs = (const uint8_t*)pd + (oneLaunch ? ((b % plan.dirGroup) * batch / kLanes) * (plan.slotDirUsed * kLanes) : 0);
        fillWalk(wa, jobs, nb, db, s, queryLength, dirs, pslots, plan.slotOps, (int32_t*)plen + b0);
        wa->opsOff = nullptr;
        HIP_TRY(launchWalk(*wa, stream));
        HIP_TRY(launchGatherOps(nb, (const uint8_t*)pslots, plan.slotOps, (const int32_t*)plen + b0, (int64_t*)pblock,
                                (const int64_t*)ptotals + b, (int64_t*)ptotals + b + 1, (uint8_t*)pcompact, stream));
        return 0;
    }

    // results back to the host: the small arrays (they carry the total size) are enqueued behind the last
    // batch's kernels before the host turns to the last batch's operations - the copies run side by side
    int finishOps() {
        RC_TRY(ws->stageDownload(&total, (const int64_t*)ptotals + nBatches, sizeof(int64_t)));
        if (!sideArrays) {
            RC_TRY(ws->stageDownload(lens, plen, (size_t)n * sizeof(int32_t)));
            RC_TRY(ws->stageDownload(startQuery, psq, (size_t)n * sizeof(int32_t)));
            RC_TRY(ws->stageDownload(startTarget, pst, (size_t)n * sizeof(int32_t)));
            RC_TRY(ws->stageDownload(tscore, pts, (size_t)n * sizeof(int32_t)));
        }
        // (the threads that will unpack the last share, started while the device is at work on the last batch)
        if (plan.overlapOps && copyOutEarly && !tuned(Tune::NO_UNPACK_CREW) &&
            (nBatches > 1 ? opsFetched / (nBatches - 1) : plan.opsCap / 4) >= (4 << 20)) {
            try {
                crew.reset(new unpack::Crew(7));
            } catch (const std::exception&) {
                crew.reset();
            }
        }
        if (plan.overlapOps) RC_TRY(fetchOps(nBatches - 1));
        pt.mark("traceback batches (enqueued)");
        RC_TRY(ws->finishDownloads());
        pt.mark("device pipeline + small D2H");
        sharer.drain();
        arrayer.drain();
        pt.mark("the helpers' shares");
        if (total < 0 || total > n * plan.slotOps) return fail(MIOPAL_ERR_INTERNAL, "bad operation count");
        if (!outOps->resize((size_t)total)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        if (plan.overlapOps) {
            // already in pinned memory (finishDownloads above waited for the side stream too): copied
            // out by helper threads while this one turns lengths into offsets and checks the scores
            if (opsFetched != total) return fail(MIOPAL_ERR_INTERNAL, "operation count changed");
            uint8_t* const out = outOps->data;
            const int64_t from = opsCopiedOut, to = total;
            // (the device has finished: this share is all that is left of the search - eight threads)
            const uint8_t* const staged = (const uint8_t*)ws->pinned + opsBase;
            unpack::Crew* const helpers = to > from ? crew.get() : nullptr;
            auto lastShare = [this, helpers, staged, out, from, to] {
                if (helpers) helpers->run(out, staged, from, to);
                else opsToCaller(out, from, to, 8);
            };
            try {
                copier.t = std::thread(lastShare);
            } catch (const std::exception&) {
                lastShare();
            }
        } else {
            RC_TRY(ws->stageDownload(outOps->data, pcompact, (size_t)total));
        }
        prefixUpTo(n);
        if (outOff[n] != total) return fail(MIOPAL_ERR_INTERNAL, "operation offsets disagree with the device");
        if (copier.t.joinable()) copier.t.join();
        crew.reset();   // (its threads end with the copy)
        RC_TRY(ws->finishDownloads());
        pt.mark("operations D2H");
        if (wrongAt >= 0)
            return fail(MIOPAL_ERR_INTERNAL, "traceback score %d differs from search score %d for target %lld",
                        tscore[(size_t)wrongAt], score[wrongAt], (long long)(start + wrongAt));
        return 0;
    }

    // miopalSearch's form of the result: one malloc'ed alignment per target (miopalSearchFlat's is outOps itself)
    int handOutAlignments() {
        if (!flat) {
            for (int64_t k = 0; k < n; ++k) {
                const int64_t len = outOff[k + 1] - outOff[k];
                alignment[k] = nullptr;
                alignmentLength[k] = (int)len;
                if (endQuery[k] < 0 || endTarget[k] < 0) continue;
                unsigned char* buf = (unsigned char*)malloc((size_t)std::max<int64_t>(len, 1));
                if (!buf) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
                memcpy(buf, outOps->data + outOff[k], (size_t)len);
                alignment[k] = buf;
            }
        }
        pt.mark("host copy-out");
        return 0;
    }

    // ================================================================================================================
    // the later passes with the host in the loop (round 1): under HOST_TRACEBACK, for an empty query or an empty
    // database, and when the operations' slots would not fit 16 GB
    // ================================================================================================================

    // start locations: reversed prefixes anchored on the end cell. `live`: the slots with a non-empty alignment
    int hostStartLocations(std::vector<int64_t>* livePairs) {
        std::vector<int64_t>& live = *livePairs;
        RC_TRY(sendResults());
        RC_TRY(ws->finishDownloads());   // (scores and end locations may still be staged: the host reads them from here on)
        for (int64_t k = 0; k < n; ++k) {
            startQuery[k] = startTarget[k] = -1;
            if (flat) {
                flatOff[k + 1] = 0;  // lengths first, prefix-summed at the end
            } else {
                alignment[k] = nullptr;
                alignmentLength[k] = 0;
            }
        }
        if (flat) {
            flatOff[0] = 0;
            if (!flatOps->reserve((size_t)n * (size_t)std::min<int64_t>(queryLength + 16, 4096)))
                return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        }
        for (int64_t k = 0; k < n; ++k)
            if (endQuery[k] >= 0 && endTarget[k] >= 0) live.push_back(k);
        if (mode == OPAL_MODE_NW) {
            for (int64_t k : live) startQuery[k] = startTarget[k] = 0;
            return 0;
        }
        if (live.empty()) return 0;
        const DpRules rr{1, 1, 0, fr.region};
        void *hrs, *hri, *hrj;
        const bool onDevice = queryLength <= kLanes;  // no strip workspace: jobs are built in HBM
        const size_t nOut = onDevice ? (size_t)n : live.size();
        RC_TRY(ws->get(kRScore, nOut * sizeof(int32_t), &hrs));
        RC_TRY(ws->get(kRI, nOut * sizeof(int32_t), &hri));
        RC_TRY(ws->get(kRJ, nOut * sizeof(int32_t), &hrj));
        if (onDevice) {
            void* jobsAt;
            RC_TRY(ws->get(kJobs, (size_t)n * sizeof(PairJob), &jobsAt));
            // pi / pj still hold the end locations of the forward pass (slice order)
            HIP_TRY(launchReverseJobs((int)n, (const int32_t*)ps, (const int32_t*)pi, (const int32_t*)pj,
                                      db->d_offsets + start, packRules(rr), 0, (PairJob*)jobsAt, stream));
            RC_TRY(s.runDeviceJobs((const PairJob*)jobsAt, (int)n, (int32_t*)hrs, (int32_t*)hri, (int32_t*)hrj));
        } else {
            std::vector<PairJob> jobs(live.size());
            for (size_t x = 0; x < live.size(); ++x) {
                const int64_t k = live[x];
                PairJob& j = jobs[x];
                j = PairJob{};
                j.tOff = db->offsets[(size_t)(start + k)] + endTarget[k];
                j.tLen = endTarget[k] + 1;
                j.tStep = -1;
                j.qOff = endQuery[k];
                j.qLen = endQuery[k] + 1;
                j.qStep = -1;
                j.rules = packRules(rr);
                j.out = (int32_t)x;
            }
            RC_TRY(s.runPairs(jobs, false, (int32_t*)hrs, (int32_t*)hri, (int32_t*)hrj, nullptr));
        }
        std::unique_ptr<int32_t[]> hs(new int32_t[nOut]), hi(new int32_t[nOut]), hj(new int32_t[nOut]);
        RC_TRY(ws->stageDownload(hs.get(), hrs, nOut * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(hi.get(), hri, nOut * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(hj.get(), hrj, nOut * sizeof(int32_t)));
        RC_TRY(ws->finishDownloads());
        for (size_t x = 0; x < live.size(); ++x) {
            const int64_t k = live[x];
            const size_t o = onDevice ? (size_t)k : x;
            int qi = hi[o], tj = hj[o];
            if (hs[o] != score[k] || qi < 0 || tj < 0) {
                // degenerate optimum (oracle/opal_oracle.c): one gap over one sequence only,
                // i.e. a border cell of the reversed problem; the other sequence's span is empty
                if (mode != OPAL_MODE_SW && score[k] == borderGap(endQuery[k], gapOpen, gapExt)) {
                    qi = endQuery[k];
                    tj = -1;
                } else if (mode == OPAL_MODE_OV && score[k] == borderGap(endTarget[k], gapOpen, gapExt)) {
                    qi = -1;
                    tj = endTarget[k];
                } else {
                    return fail(MIOPAL_ERR_INTERNAL, "reverse pass disagrees with the forward score for target %lld",
                                (long long)(start + k));
                }
            }
            startQuery[k] = endQuery[k] - qi;
            startTarget[k] = endTarget[k] - tj;
        }
        return 0;
    }

    // traceback on [start..end] rectangles, batched by direction workspace
    int hostTraceBatches(const std::vector<int64_t>& live) {
        size_t pos = 0;
        while (pos < live.size()) {
            std::vector<PairJob> jobs;
            std::vector<int64_t> opsOff(1, 0);
            int64_t dirBytes = 0;
            size_t first = pos;
            while (pos < live.size()) {
                const int64_t k = live[pos];
                const int qn = endQuery[k] - startQuery[k] + 1, tn = endTarget[k] - startTarget[k] + 1;
                const int64_t need = slotDir((qn + kLanes - 1) / kLanes, tn);
                if (!jobs.empty() && dirBytes + need > kDirBudget) break;
                PairJob j{};
                j.tOff = db->offsets[(size_t)(start + k)] + startTarget[k];
                j.tLen = tn;
                j.tStep = 1;
                j.qOff = startQuery[k];
                j.qLen = qn;
                j.qStep = 1;
                j.rules = packRules(DpRules{1, 1, 0, kLastCell});
                j.dirOff = dirBytes;
                j.out = (int32_t)jobs.size();
                jobs.push_back(j);
                dirBytes += need;
                opsOff.push_back(opsOff.back() + qn + tn);
                ++pos;
            }
            void *dirs, *po, *poff, *lensAt, *pscore;
            RC_TRY(ws->get(kDirs, (size_t)dirBytes, &dirs));
            RC_TRY(ws->get(kOps, (size_t)opsOff.back(), &po));
            RC_TRY(ws->get(kOpsOff, opsOff.size() * sizeof(int64_t), &poff));
            RC_TRY(ws->get(kOpsLen, jobs.size() * sizeof(int32_t), &lensAt));
            RC_TRY(ws->get(kRScore, jobs.size() * sizeof(int32_t), &pscore));
            RC_TRY(ws->stageUpload(poff, opsOff.data(), opsOff.size() * sizeof(int64_t), stream));
            RC_TRY(s.runPairs(jobs, true, (int32_t*)pscore, nullptr, nullptr, (uint8_t*)dirs));
            WalkArgs wa{};
            void* jobsAt;
            RC_TRY(ws->get(kJobs, jobs.size() * sizeof(PairJob), &jobsAt));
            fillWalk(&wa, (const PairJob*)jobsAt, (int)jobs.size(), db, s, queryLength, dirs, po, 0, lensAt);
            wa.opsOff = (const int64_t*)poff;
            HIP_TRY(launchWalk(wa, stream));
            if (pt.on) { HIP_TRY(hipStreamSynchronize(stream)); pt.mark("  trace + walk kernels"); }
            const size_t opsBytes = (size_t)opsOff.back();
            std::unique_ptr<uint8_t[]> ops(new uint8_t[std::max<size_t>(opsBytes, 1)]);
            std::unique_ptr<int32_t[]> hlens(new int32_t[jobs.size()]), hscore(new int32_t[jobs.size()]);
            RC_TRY(ws->stageDownload(ops.get(), po, opsBytes));
            RC_TRY(ws->stageDownload(hlens.get(), lensAt, jobs.size() * sizeof(int32_t)));
            RC_TRY(ws->stageDownload(hscore.get(), pscore, jobs.size() * sizeof(int32_t)));
            RC_TRY(ws->finishDownloads());
            pt.mark("  ops D2H");
            RC_TRY(hostCopyOut(live, first, jobs.size(), opsOff, ops.get(), hlens.get(), hscore.get()));
            pt.mark("  host copy-out");
        }
        if (flat)
            for (int64_t k = 0; k < n; ++k) flatOff[k + 1] += flatOff[k];
        return 0;
    }

    // a host-built batch's alignments into the caller's form, its traceback scores against the search's
    int hostCopyOut(const std::vector<int64_t>& live, size_t first, size_t count, const std::vector<int64_t>& opsOff,
                    const uint8_t* ops, const int32_t* hlens, const int32_t* hscore) {
        for (size_t x = 0; x < count; ++x) {
            const int64_t k = live[first + x];
            if (hscore[x] != score[k])
                return fail(MIOPAL_ERR_INTERNAL, "traceback score %d differs from search score %d for target %lld",
                            hscore[x], score[k], (long long)(start + k));
            const int len = hlens[x];
            const uint8_t* src = ops + opsOff[x + 1] - len;
            if (flat) {
                // jobs are visited in increasing target order, so appending keeps slice order
                if (!flatOps->append(src, (size_t)len)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
                flatOff[k + 1] = len;
            } else {
                unsigned char* buf = (unsigned char*)malloc((size_t)std::max(len, 1));
                if (!buf) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
                memcpy(buf, src, (size_t)len);
                alignment[k] = buf;
                alignmentLength[k] = len;
            }
        }
        return 0;
    }
};

}  // namespace

static int searchImpl(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                      const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                      int64_t end, int* score, int* endTarget, int* endQuery, int* startTarget,
                      int* startQuery, unsigned char** alignment, int* alignmentLength,
                      HostBytes* flatOps, int64_t* flatOff, const int* pssmRows = nullptr) {
    // (pssmRows, miopalSearchPssm: the score source is [queryLength][alphabetLength] rows, scoreMatrix is null, `query`
    // the consensus; its caller has made miopalSearch's checks on them)
    if (!pssmRows) RC_TRY(validate(db, query, queryLength, scoreMatrix, alphabetLength, searchType, mode, start, end));
    const int64_t n = end - start;
    if (n == 0) return 0;
    const FullCall call{db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType, mode, start, end,
                        score, endTarget, endQuery, startTarget, startQuery, alignment, alignmentLength, flatOps, flatOff,
                        pssmRows, n, flatOps != nullptr};
    RC_TRY(call.checkOutputs());
    HIP_TRY(hipSetDevice(db->device));
    PhaseTimer pt;
    WorkspaceLease lease(db);
    RC_TRY(lease.acquireInternal());
    Search s{db, lease.ws, lease.ws->stream, query, queryLength, gapOpen, gapExt, alphabetLength, searchType, mode,
             scoreMatrix, start, end, n};
    s.pssmRows = pssmRows;
    RC_TRY(s.prepare());
    pt.mark("workspace + query");

    // ---- the score / end pass, its results to the host ----
    FullSearch f(call, pt, lease, s);
    RC_TRY(f.bindHostOutputs());
    RC_TRY(s.scorePass((int32_t*)f.ps, (int32_t*)f.pi, (int32_t*)f.pj));
    RC_TRY(f.deliverScores());
    pt.mark("score/end pass + D2H");
    if (searchType != OPAL_SEARCH_ALIGNMENT) return 0;

    RC_TRY(s.rulesFor(mode, &f.fr));
    g_lastFullRouting = 0;
    // ---- the later passes on the device: start cells, directions, walk, gather, the operations' way out ----
    if (queryLength > 0 && db->maxLen > 0 && !tuned(Tune::HOST_TRACEBACK)) {
        RC_TRY(f.planLaterPasses());
        RC_TRY(f.scanStartCells());
        pt.mark("start cells (enqueued)");
        RC_TRY(f.readWindowChecks());
        f.planTrace();
        if (f.plan.fits) {   // else: host-built batches below
            RC_TRY(f.allocTrace());
            for (int64_t b = 0; b < f.nBatches; ++b) RC_TRY(f.traceBatch(b));
            RC_TRY(f.finishOps());
            return f.handOutAlignments();
        }
    }
    // ---- ... or with the host in the loop ----
    std::vector<int64_t> live;  // slots with a non-empty alignment
    RC_TRY(f.hostStartLocations(&live));
    pt.mark("start-location pass");
    return f.hostTraceBatches(live);
}
