// Part of host.hip (included there, not a translation unit of its own): searchImpl: score / end / full alignment search behind miopalSearch, miopalSearchFlat.
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
    if (!score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score output");
    if (searchType >= OPAL_SEARCH_SCORE_END && (!endTarget || !endQuery))
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
    const bool flat = flatOps != nullptr;
    if (searchType == OPAL_SEARCH_ALIGNMENT &&
        (!startTarget || !startQuery || (flat ? !flatOff : (!alignment || !alignmentLength))))
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "null alignment outputs");
    HIP_TRY(hipSetDevice(db->device));
    PhaseTimer pt;
    WorkspaceLease lease(db);
    RC_TRY(lease.acquireInternal());
    Workspace* ws = lease.ws;
    hipStream_t stream = ws->stream;
    Search s{db, ws, stream, query, queryLength, gapOpen, gapExt, alphabetLength, searchType, mode,
             scoreMatrix, start, end, n};
    s.pssmRows = pssmRows;
    RC_TRY(s.prepare());
    pt.mark("workspace + query");

    void *ps, *pi = nullptr, *pj = nullptr;
    RC_TRY(ws->get(kScore, (size_t)n * sizeof(int32_t), &ps));
    const bool wantEnd = searchType >= OPAL_SEARCH_SCORE_END;
    if (wantEnd) {
        RC_TRY(ws->get(kEndI, (size_t)n * sizeof(int32_t), &pi));
        RC_TRY(ws->get(kEndJ, (size_t)n * sizeof(int32_t), &pj));
    }
    // scores (and end locations) of a score / end search may leave the kernel straight for pinned host memory
    size_t hostOff = 0;
    const size_t hostBytes = ((size_t)n * sizeof(int32_t) + 255) & ~(size_t)255;
    const int hostArrays = searchType == OPAL_SEARCH_SCORE ? 1 : searchType == OPAL_SEARCH_SCORE_END ? 3 : 0;
    bool callerPinned = false;
    if (hostArrays > 0) {
        // A caller whose result arrays are themselves pinned, device-visible host memory (hipHostMalloc,
        // hipHostRegister, a pinned torch tensor) gets the results written into them by the kernel: no
        // bounce buffer, no copy on the host.
        // (the n entries must lie inside the pinned range: when the runtime can tell the range's extent and it
        // is too short, the bounce buffer is used instead)
        const size_t wantBytes = (size_t)n * sizeof(int32_t);
        auto devicePointerOf = [wantBytes](void* p) -> int32_t* {
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
        };
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
        } else {
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
        }
    }
    // A `full` search whose later passes stay on the device leaves the scores and end locations in the staging
    // buffer until its end: copying 12 MB into the caller's (fresh) pages here kept the device idle for 0.35 ms
    // between the end pass and the start-cell scan. (Whatever takes the host's paths below flushes first.)
    const bool deferResults = searchType == OPAL_SEARCH_ALIGNMENT;
    constexpr size_t kDeferFrom = 64u << 10;
    // scores and end locations of a `full` search that have not been sent on their way to the host yet, and the copies
    // themselves: on the side stream, behind whatever the main stream has been given so far
    bool resultsPending = false;
    // (forked: evFork has been recorded where the copies may start - the caller has enqueued more since)
    auto sendResults = [&](bool forked = false) -> int {
        if (!resultsPending) return 0;
        resultsPending = false;
        RC_TRY(ws->ensureAux());
        if (!forked) HIP_TRY(hipEventRecord(ws->evFork, stream));
        HIP_TRY(hipStreamWaitEvent(ws->aux, ws->evFork, 0));
        RC_TRY(ws->stageDownload(score, ps, (size_t)n * sizeof(int), true));
        RC_TRY(ws->stageDownload(endQuery, pi, (size_t)n * sizeof(int), true));
        RC_TRY(ws->stageDownload(endTarget, pj, (size_t)n * sizeof(int), true));
        return 0;
    };
    RC_TRY(s.scorePass((int32_t*)ps, (int32_t*)pi, (int32_t*)pj));
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
    pt.mark("score/end pass + D2H");
    if (searchType != OPAL_SEARCH_ALIGNMENT) return 0;

    DpRules fr;
    RC_TRY(s.rulesFor(mode, &fr));
    g_lastFullRouting = 0;
    // (test switch: one lane per pair whatever the cost estimates below say)
    const bool forceLanePerPair = tuned(Tune::FORCE_LANE_PER_PAIR) != nullptr;

    // ---- queries of one strip: the rest of the pipeline stays in HBM ---------------
    // (start cells, traceback jobs, direction bytes and operations are produced and
    // consumed on the device; the host only prefix-sums the alignment lengths)
    {
        const bool oneStrip = queryLength <= kLanes;
        bool deviceFull = queryLength > 0 && db->maxLen > 0 && !tuned(Tune::HOST_TRACEBACK);
        if (deviceFull) {
            HostBytes localOps;
            std::vector<int64_t> localOff;
            HostBytes* outOps = flatOps;
            int64_t* outOff = flatOff;
            if (!flat) {
                localOff.assign((size_t)n + 1, 0);
                outOps = &localOps;
                outOff = localOff.data();
            }
            void *rs = nullptr, *ri = nullptr, *rj = nullptr, *pjobs, *psq, *pst, *pmis, *plen, *pcompact, *pts;
            // one lane per pair (perpair.hip) instead of one wavefront per pair (intraseq.hip)
            // (it stages the query in LDS: up to 4096 residues; longer ones keep the wavefront-per-pair kernel)
            bool lanePerPair = queryLength <= 4096 && !tuned(Tune::NO_PERPAIR) &&
                               (n > kSmallSearch || !smallSearchAllowed(db));
            RC_TRY(s.ensurePairInputs());
            PerPairArgs perPair{};
            perPair.residues = db->d_residues;
            perPair.query = s.d_query;
            perPair.queryLength = queryLength;
            perPair.matrix = s.d_matrix;
            perPair.rows = s.d_rows;
            perPair.alphabet = alphabetLength;
            perPair.gapOpen = gapOpen;
            perPair.gapExt = gapExt;
            // the query-profile form of the kernel (signed bytes of score + open in LDS, columns on a sliding
            // scale of j x ext): queries whose profile fits 64 KB, matrices and gaps that fit the byte
            int profileStride = 0;
            const bool profiled = !tuned(Tune::NO_PERPAIR_PROFILE) &&
                                  perPairProfileBytes(queryLength, alphabetLength, &profileStride) > 0 &&
                                  s.maxScore + gapOpen <= 127 && s.minScore + gapOpen > -128 && gapOpen >= 0 &&
                                  gapExt >= 0 && (int64_t)db->maxLen * gapExt < (1 << 27) && db->total >= 4;
            perPair.residueCount = db->total;
            if (!profiled) profileStride = 0;
            // (position-specific scores outside the byte profile: perpair_kernel's row-indexed form stages all the rows
            // in LDS; more rows than fit keep the wavefront-per-pair kernel, as queries beyond 4096 residues do)
            if (!profiled && pssmRows && perPairPssmBytes(queryLength, alphabetLength) == 0) lanePerPair = false;
            RC_TRY(ws->get(kJobs, (size_t)n * sizeof(PairJob), &pjobs));
            RC_TRY(ws->get(kStartQ, (size_t)n * sizeof(int32_t), &psq));
            RC_TRY(ws->get(kStartT, (size_t)n * sizeof(int32_t), &pst));
            RC_TRY(ws->get(kMismatch, 4 * sizeof(int), &pmis));   // [3]: job counter of the persistent start-cell scan
            RC_TRY(ws->get(kOpsLen, (size_t)n * sizeof(int32_t), &plen));
            RC_TRY(ws->get(kRScore, (size_t)n * sizeof(int32_t), &rs));
            HIP_TRY(hipMemsetAsync(pmis, 0, 4 * sizeof(int), stream));
            bool startCellsDone = false;   // (written by the scan itself: perpair_packed.hip)
            if (mode != OPAL_MODE_NW) {
                RC_TRY(ws->get(kRI, (size_t)n * sizeof(int32_t), &ri));
                RC_TRY(ws->get(kRJ, (size_t)n * sizeof(int32_t), &rj));
                const DpRules rr{1, 1, 0, fr.region};
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
                    const double perLane = std::max((double)n * strips * meanLen * (14 * 4.5) / (1024 * 2.4e6),
                                                    strips * (double)db->maxLen * (64 * 14 * 4.5) / 2.4e6);
                    const double perWave = std::max((double)n * strips * (meanLen + 63) * 225.0 / (1024 * 2.4e6),
                                                    strips * (double)(db->maxLen + 63) * 250.0 / 2.4e6);
                    scanLanePerPair = perLane <= perWave || forceLanePerPair;
                }
                if (scanLanePerPair)
                    g_lastFullRouting |= 1 | (profileStride > 0 ? 2 : 0);
                // Smith-Waterman prefixes with two pairs per lane (perpair_packed.hip): every half of a lane on its own
                // schedule - pair, strip, column - so neither sorted wavefronts nor a boundary line per PAIR are needed
                int scanBias = 0, scanStride = 0, scanZero = 0;
                size_t scanLds = 0;
                bool packedScan = false;
                // (HW too: the same cells, the answer only in the query's last row. OV - last row or last column, the last row
                // another one in every pair: a select tree per column)
                const bool packedRegion = (mode == OPAL_MODE_SW && fr.region == kAllCells) ||
                                          (mode == OPAL_MODE_HW && fr.region == kLastRow && !tuned(Tune::NO_PACKED_HW_SCAN)) ||
                                          (mode == OPAL_MODE_OV && fr.region == kLastRowCol && !tuned(Tune::NO_PACKED_HW_SCAN));
                if (scanLanePerPair && profileStride > 0 && packedRegion && !tuned(Tune::NO_PACKED_SCAN)) {
                    // (no cell of a prefix scan beats the query's own best: every residue against its best partner)
                    const int64_t ownBest = queryBest(queryLength, alphabetLength, [&](int y, int t) { return s.at(y, t); });
                    const int64_t best = std::min<int64_t>(ownBest, std::min<int64_t>(queryLength, db->maxLen) * std::max(s.maxScore, 0));
                    packedScan = packedScanFits(queryLength, alphabetLength, gapOpen, gapExt, s.maxScore, s.minScore,
                                                db->maxLen, best, &scanBias, &scanZero, &scanStride, &scanLds) &&
                                 (oneStrip || ((n + 127) / 128) * kLanes * db->maxLen * (int64_t)sizeof(int2) <= (8ll << 30));
                }
                if (packedScan) {
                    g_lastFullRouting |= 128 | (oneStrip ? 32 : 0);
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
                        void *pbins, *porder;
                        RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
                        RC_TRY(ws->get(kScanOrder, (size_t)n * sizeof(int), &porder));
                        HIP_TRY(launchSortIndicesByKey((const int32_t*)pj, (int)n, (int)db->maxLen, (int*)pbins, (int*)porder, stream));
                        pa.order = (const int*)porder;
                    }
                    if (!oneStrip) {
                        HIP_TRY(launchReverseJobs((int)n, (const int32_t*)ps, (const int32_t*)pi, (const int32_t*)pj,
                                                  db->d_offsets + start, packRules(rr), 0, (PairJob*)pjobs, stream));
                        // longest prefixes first: the persistent wavefronts end together
                        void *pbins, *psorted;
                        RC_TRY(ws->get(kSortBins, (size_t)(std::min<int64_t>(db->maxLen, 8191) + 1) * sizeof(int), &pbins));
                        RC_TRY(ws->get(kSortedJobs, (size_t)n * sizeof(PairJob), &psorted));
                        HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, (int)n, (int)db->maxLen, (int*)pbins, (PairJob*)psorted, stream));
                        pa.jobs = (const PairJob*)psorted;
                        void* pb;
                        RC_TRY(ws->get(kPairB0, (size_t)((n + 127) / 128) * kLanes * db->maxLen * sizeof(int2), &pb));
                        pa.boundary = (int2*)pb;
                        pa.boundaryStride = db->maxLen;
                    }
                    pa.nJobs = (int)n;
                    pa.score = (int32_t*)rs;
                    pa.endI = (int32_t*)ri;
                    pa.endJ = (int32_t*)rj;
                    pa.profileStride = scanStride;
                    pa.packedBias = scanBias;
                    pa.packedZero = scanZero;
                    pa.reversed = 1;
                    pa.jobCounter = (int*)pmis + 3;
                    pa.computeUnits = db->computeUnits;
                    HIP_TRY(launchPerPairPackedScan(pa, scanLds, stream));
                } else if (scanLanePerPair) {
                    // chunks of whole wavefronts whose strip boundaries (8 B per column and pair) fit 4 GB
                    const int64_t chunk =
                        oneStrip ? n : std::max<int64_t>(kLanes, (4ll << 30) / (8 * db->maxLen) / kLanes * kLanes);
                    void *pb = nullptr, *pbins = nullptr, *psorted = nullptr;
                    if (!oneStrip) {
                        const int64_t most = std::min(chunk, n);
                        RC_TRY(ws->get(kPairB0, (size_t)((most + kLanes - 1) / kLanes * kLanes) * db->maxLen * sizeof(int2), &pb));
                        // prefixes of similar length share a wavefront (results stay addressed by job.out)
                        RC_TRY(ws->get(kSortBins, (size_t)(std::min<int64_t>(db->maxLen, 8191) + 1) * sizeof(int), &pbins));
                        RC_TRY(ws->get(kSortedJobs, (size_t)most * sizeof(PairJob), &psorted));
                    }
                    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
                        const int nc = (int)std::min<int64_t>(chunk, n - c0);
                        const PairJob* jobs = (PairJob*)pjobs + c0;
                        HIP_TRY(launchReverseJobs(nc, (const int32_t*)ps + c0, (const int32_t*)pi + c0,
                                                  (const int32_t*)pj + c0, db->d_offsets + start + c0,
                                                  packRules(rr), 0, (PairJob*)pjobs + c0, stream));
                        if (!oneStrip) {
                            HIP_TRY(launchSortJobsByLength(jobs, nc, (int)db->maxLen, (int*)pbins, (PairJob*)psorted, stream));
                            jobs = (const PairJob*)psorted;
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
                            g_lastFullRouting |= 32;
                        }
                        HIP_TRY(launchPerPair(pa, fr.region, stream));
                    }
                } else {
                    // chunks of targets whose strip boundaries (16 B per column and pair) fit 4 GB
                    const int64_t wsStride = oneStrip ? 0 : db->maxLen;
                    const int64_t chunk = oneStrip ? n : std::max<int64_t>(1, (4ll << 30) / (16 * wsStride));
                    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
                        const int nc = (int)std::min<int64_t>(chunk, n - c0);
                        PairJob* jobs = (PairJob*)pjobs + c0;
                        HIP_TRY(launchReverseJobs(nc, (const int32_t*)ps + c0, (const int32_t*)pi + c0,
                                                  (const int32_t*)pj + c0, db->d_offsets + start + c0,
                                                  packRules(rr), wsStride, jobs, stream));
                        RC_TRY(s.runDeviceJobs(jobs, nc, (int32_t*)rs + c0, (int32_t*)ri + c0, (int32_t*)rj + c0,
                                               false, nullptr, wsStride));
                    }
                }
            }
            if (!startCellsDone)
                HIP_TRY(launchStartCells((int)n, mode, gapOpen, gapExt, (const int32_t*)ps, (const int32_t*)pi,
                                         (const int32_t*)pj, (const int32_t*)rs, (const int32_t*)ri, (const int32_t*)rj,
                                         (int32_t*)psq, (int32_t*)pst, (int*)pmis, stream));
            pt.mark("start cells (enqueued)");
            // The slots of the traceback are sized by the longest target window of the slice
            // (local alignments are short whatever the targets' lengths): one small D2H + sync.
            int checks[3] = {0, 0, 0};
            RC_TRY(ws->stageDownload(checks, pmis, sizeof checks));
            RC_TRY(ws->finishDownloads(deferResults ? kDeferFrom : SIZE_MAX));
            if (checks[0])
                return fail(MIOPAL_ERR_INTERNAL, "reverse pass disagrees with the forward score for target %lld",
                            (long long)(start + checks[0] - 1));
            const int64_t maxWindow = std::max(checks[1], 1);
            const int64_t windowStrips = (std::max(checks[2], 1) + kLanes - 1) / kLanes;  // tallest query window
            // direction bytes of one pair (either layout: anti-diagonals of 64 lanes per strip, or
            // 64 rows per column)
            const int64_t slotDir = windowStrips * (maxWindow + kLanes - 1) * kLanes;
            const int64_t slotOps = (queryLength + maxWindow + 15) & ~(int64_t)15;  // operations of one pair (they leave 16 bytes at a time)
            const bool fits = n * slotOps <= (16ll << 30);  // else: host-built batches below
            if (fits) {
                // (whole units of 64 operations: copy_out_packed_kernel reads the unit a batch ends in to its end)
                RC_TRY(ws->get(kCompactOps, ((size_t)(n * slotOps) + 63) & ~(size_t)63, &pcompact));
                // traceback in batches of whole direction slots and whole wavefronts of 64 pairs: at most
                // 4 GB of directions per batch (the lane-per-pair layout packs two cells per byte)
                // two pairs per lane on 16-bit halves (perpair_packed.hip) when the scoring scheme and the windows fit
                int packedBias = 0, packedStride = 0;
                size_t packedLds = 0;
                bool packedOk = false;
                if (lanePerPair && profileStride > 0 && !tuned(Tune::NO_PACKED_TRACE)) {
                    const int64_t rows = windowStrips * kLanes, columns = (maxWindow + 3) & ~(int64_t)3;
                    const int64_t best = std::min(rows, columns) * std::max(s.maxScore, 0);
                    packedOk = packedTraceFits(queryLength, alphabetLength, gapOpen, gapExt, s.maxScore, s.minScore,
                                               rows, columns, best, &packedBias, &packedStride, &packedLds);
                }
                // (a round of the chip is twice the pairs with two in a lane, and the budget follows: Q = 300 on 1M x 300
                // asks for 58 KB of directions per pair - 15 GB per round)
                const int64_t dirBudget = packedOk ? kDirBudget * 8 : kDirBudget * 2;
                auto batchFor = [&](int64_t slotBytes) {
                    return std::max<int64_t>(kLanes, std::min<int64_t>(n + kLanes - 1, dirBudget / slotBytes) / kLanes * kLanes);
                };
                // lane per pair: whole rounds of the chip (two wavefronts of 64 pairs per SIMD; a batch of 1.1
                // rounds lasts as long as one of two), within 8 GB of directions: Q = 300 on 1M x 300 took
                // 14 batches of 1117 wavefronts, 5.2 ms each, where 8 of 2048 take 5.2 ms as well
                const int64_t chipRound = (int64_t)db->computeUnits * 4 * 2 * kLanes * (packedOk ? 2 : 1);
                int64_t batchLane = batchFor(std::max<int64_t>(slotDir / 4, 1));
                if (batchLane >= chipRound) batchLane = batchLane / chipRound * chipRound;
                else if (batchLane >= chipRound / 2 && n > batchLane) batchLane = chipRound / 2;
                const int64_t batchWave = batchFor(slotDir);
                int64_t batch = batchLane;
                const int64_t opsCap = n * slotOps;
                // (the pinned staging buffer holds the worst case, n x slotOps: Q = 300 on 1M x 300 asks for 664 MB)
                // (within it the operations leave batch by batch, two bits each; a larger result is downloaded whole, in bytes,
                // after the last batch)
                const bool overlapOps = opsCap <= (1024ll << 20);
                void *pd, *pslots, *pbins = nullptr, *psorted = nullptr;
                // Direction pass: one lane per pair needs ~64 x fewer instructions per cell but a
                // lane walks its whole window alone (strips x columns x 64 rows, ~0.4 us per strip
                // column); with few pairs per batch or huge windows (global alignments of long
                // targets) a wavefront per pair is done sooner. Rough cost of either, in ms:
                bool traceLanePerPair = lanePerPair;
                if (lanePerPair) {
                    const double cells = (double)windowStrips * (double)(maxWindow + kLanes - 1);
                    const double pairsL = (double)std::min<int64_t>(batchLane, n), pairsW = (double)std::min<int64_t>(batchWave, n);
                    const double perLane = std::ceil((double)n / (double)batchLane) * std::ceil(pairsL / kLanes / 2048.0) *
                                           cells * (64 * 21 * 4.5) / 2.4e6;
                    const double perWave = std::ceil((double)n / (double)batchWave) *
                                           std::max(pairsW * cells * 225.0 / (1024 * 2.4e6), cells * 250.0 / 2.4e6);
                    traceLanePerPair = perLane <= perWave || forceLanePerPair;
                }
                const bool packedTrace = traceLanePerPair && packedOk;
                if (traceLanePerPair) g_lastFullRouting |= 4 | (profileStride > 0 ? 8 : 0) | (packedTrace ? 64 : 0);
                if (overlapOps) g_lastFullRouting |= 16;
                batch = traceLanePerPair ? batchLane : batchWave;
                if (overlapOps && n >= 4 * 65536)
                    // (four batches, the last one half a batch: its operations are what the host unpacks with the device idle)
                {
                    int64_t target = std::max<int64_t>(65536, (n * 2 / 7 + kLanes - 1) / kLanes * kLanes);
                    // (a batch a little above a round of the chip lasts two: rather one round)
                    // (not when the direction pass runs over groups of batches anyway: host_full.inc, oneLaunch)
                    const bool grouped = traceLanePerPair && packedOk && !tuned(Tune::NO_ONE_LAUNCH) &&
                                         std::min<int64_t>(n + kLanes, 2 * target) * windowStrips * ((maxWindow + 3) & ~(int64_t)3) *
                                                 (kLanes / 2) <= kDirBudgetOneLaunch;
                    if (traceLanePerPair && !grouped && target > chipRound && target < chipRound * 3 / 2) target = chipRound;
                    batch = std::min(batch, target);
                }
                if (pt.on)
                    fprintf(stderr, "[miopal]   traceback: longest window %lld columns, %lld strip(s) of rows, %lld pairs per batch, %s per pair\n",
                            (long long)maxWindow, (long long)windowStrips, (long long)batch,
                            traceLanePerPair ? "lane" : "wavefront");
                const bool sortJobs = traceLanePerPair;
                // (the windows' rows as a minor sort key: common.h)
                const int sortRows = tuned(Tune::NO_SORT_BY_ROWS) ? 0 : queryLength;
                // hybrid: up to 2 GB of direction bytes for the outliers a wavefront-per-pair pass takes
                int64_t maxHead = 0;
                void *phead = nullptr, *pheadDirs = nullptr;
                if (sortJobs && !tuned(Tune::NO_HYBRID_TRACE)) {
                    maxHead = std::min<int64_t>((1ll << 30) / slotDir / kLanes, (batch + kLanes - 1) / kLanes);
                    if (maxHead > 0) {
                        RC_TRY(ws->get(kHeadWaves, sizeof(int), &phead));
                        if (!ws->tryGet(kHeadDirs, (size_t)(maxHead * kLanes * slotDir), &pheadDirs)) maxHead = 0;
                    }
                }
                // The packed direction pass of EVERY batch in one launch (round 5): a batch of cfg3 is one round of the
                // chip, so its kernel lasted as long as its longest wavefront - 0.5 ms where the work is 0.15 ms - and
                // four of them ran one after the other. The batches' job lists are sorted one by one (the walk, the
                // gather and the copies stay batch by batch), laid end to end, and swept by one launch whose late
                // wavefronts are the last batch's short ones; the directions of all n pairs stay in HBM meanwhile.
                const int64_t nBatchesPlanned = (n + batch - 1) / batch;
                const int64_t allSlots = (n + kLanes - 1) / kLanes * kLanes;
                // (batches per direction launch: the walks - whose operations the host unpacks - must not all come at
                // the end; two launches of two batches leave the host the second launch's time for the first's shares.
                // The direction bits of ONE group stay in HBM at a time)
                int64_t dirGroup = nBatchesPlanned >= 4 ? (nBatchesPlanned + 1) / 2 : nBatchesPlanned;
                if (const char* e = tuned(Tune::ONE_LAUNCH_GROUP)) dirGroup = std::max(1, atoi(e));
                // bytes of direction bits per pair: the lane-per-pair layouts pack two rows per byte (half of slotDir);
                // the packed kernel's lines need the window's columns rounded up to four, not the 63 columns of slack
                // of the anti-diagonal layout
                const int64_t slotDirUsed = packedTrace ? windowStrips * ((maxWindow + 3) & ~(int64_t)3) * (kLanes / 2)
                                            : traceLanePerPair ? slotDir / 2 : slotDir;
                const int64_t groupSlots = std::min(allSlots, dirGroup * batch);
                bool oneLaunch = packedTrace && sortJobs && nBatchesPlanned > 1 && !tuned(Tune::NO_ONE_LAUNCH) &&
                                 groupSlots * slotDirUsed <= kDirBudgetOneLaunch;
                void* pdAll = nullptr;
                if (oneLaunch && !ws->tryGet(kDirs, (size_t)(groupSlots * slotDirUsed), &pdAll)) oneLaunch = false;
                if (oneLaunch) g_lastFullRouting |= 256;
                if (maxHead > 0 && oneLaunch) RC_TRY(ws->get(kHeadWaves, (size_t)nBatchesPlanned * sizeof(int), &phead));
                if (sortJobs) {
                    RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
                    RC_TRY(ws->get(kSortedJobs, (size_t)(oneLaunch ? allSlots : batch) * sizeof(PairJob), &psorted));
                }
                // the direction workspace is the one allocation that can be refused on a GPU shared
                // with other work: halve the batch until it fits
                if (oneLaunch) pd = pdAll;
                while (!oneLaunch && !ws->tryGet(kDirs, (size_t)(batch * slotDirUsed), &pd)) {
                    if (batch <= kLanes) return fail(MIOPAL_ERR_HIP, "out of device memory for the traceback workspace");
                    batch = std::max<int64_t>(kLanes, batch / 2 / kLanes * kLanes);
                }
                RC_TRY(ws->get(kOps, (size_t)(batch * slotOps), &pslots));
                RC_TRY(ws->get(kTraceScore, (size_t)n * sizeof(int32_t), &pts));
                // Operations leave for the host batch by batch, on the side stream, while the next batch
                // is computed: at least four batches when there are enough pairs to fill the chip with
                // each (the copy of the last batch is all that is not hidden). They are staged in
                // pinned memory, contiguously, and copied out once the total is known.
                const int64_t nBatches = (n + batch - 1) / batch;
                struct Events {
                    std::vector<hipEvent_t> ev;
                    ~Events() {
                        for (hipEvent_t e : ev)
                            if (e) (void)hipEventDestroy(e);
                    }
                } batchDone, traceStart, copyDone;
                size_t opsBase = 0;
                // operations of the staged stream -> the caller's buffer (the unpacking of two-bit codes)
                auto opsToCaller = [&](uint8_t* out, int64_t from, int64_t to, int threads) {
                    if (to > from) unpack::ops(out, (const uint8_t*)ws->pinned + opsBase, from, to, threads);
                };
                int64_t opsFetched = 0;
                int64_t opsCopiedOut = 0;   // of the fetched operations: already in the caller's buffer
                bool copyOutEarly = false;
                int64_t* fetchedTotal = nullptr;   // pinned: running total read back per batch
                if (overlapOps) {
                    RC_TRY(ws->ensureAux());
                    batchDone.ev.assign((size_t)nBatches, nullptr);
                    for (auto& e : batchDone.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    traceStart.ev.assign((size_t)nBatches, nullptr);
                    for (auto& e : traceStart.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    copyDone.ev.assign((size_t)nBatches, nullptr);
                    for (auto& e : copyDone.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    // room for the operations, the running totals and the small per-target arrays that
                    // follow, reserved in one go (a later drain would reset the staging buffer)
                    // (the operations cross PCIe two bits each - copy_out_packed_kernel - a quarter of a byte per operation)
                    const size_t head = 256 + (((size_t)nBatches * 8 + 255) & ~(size_t)255);
                    const size_t stagedOps = ((size_t)opsCap + 63) / 64 * 16;
                    // (with the scores and end locations when they are still to be sent: sendResults)
                    RC_TRY(ws->reserveStaging(head + stagedOps + 256 + (size_t)n * (resultsPending ? 36 : 20) + 8192 + (size_t)nBatches * 1024));
                    fetchedTotal = (int64_t*)((char*)ws->pinned + ws->pinnedUsed);
                    opsBase = ws->pinnedUsed + head;   // (256-byte aligned: pinnedUsed and head are)
                    ws->pinnedUsed = opsBase + ((stagedOps + 255) & ~(size_t)255);
                    // The caller's buffer is filled batch by batch as the operations land (room for the worst
                    // case; pages that stay untouched are never committed): only the last batch's share is
                    // copied after the device has finished.
                    // (a host that refuses the worst case gets its operations in one piece at the end, as before)
                    copyOutEarly = outOps->resize((size_t)opsCap);
                }
                // (host scratch kept on the workspace: no malloc / free of megabytes per search)
                if (ws->hostScratchA.size() < (size_t)n) ws->hostScratchA.resize((size_t)n);
                if (ws->hostScratchB.size() < (size_t)n) ws->hostScratchB.resize((size_t)n);
                int32_t* const tscore = ws->hostScratchA.data();
                int32_t* const lens = ws->hostScratchB.data();
                // The small per-target arrays leave on the side stream as they become final - the start cells now,
                // lengths and traceback scores batch by batch - instead of four copies of 4 MB behind the last batch
                // (0.3 ms of a million targets' search with nothing else left to run beside them).
                const bool sideArrays = overlapOps && !tuned(Tune::NO_SIDE_COPIES);
                bool startsPending = sideArrays;
                // (beside the first direction kernel, with the scores and end locations)
                auto sendEarlyArrays = [&](bool forked = false) -> int {
                    RC_TRY(sendResults(forked));
                    if (startsPending) {
                        startsPending = false;
                        if (!forked) HIP_TRY(hipEventRecord(ws->evFork, stream));
                        HIP_TRY(hipStreamWaitEvent(ws->aux, ws->evFork, 0));
                        RC_TRY(ws->stageDownload(startQuery, psq, (size_t)n * sizeof(int32_t), true));
                        RC_TRY(ws->stageDownload(startTarget, pst, (size_t)n * sizeof(int32_t), true));
                    }
                    return 0;
                };
                // operation offsets from the lengths, and the traceback's scores against the search's, of the targets
                // whose arrays are on the host: [done, upTo)
                int64_t prefixDone = 0, wrongAt = -1;
                outOff[0] = 0;
                // (two loops: the running sum is one add per target and nothing else; the comparison has no chain and
                // vectorises - together, with the branch inside, they took 1.2 ns a target, 0.3-0.4 ms per batch of cfg3 on
                // the thread that was the last to finish)
                auto prefixUpTo = [&](int64_t upTo) {
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
                };
                void *pblock, *ptotals;
                RC_TRY(ws->get(kOpsOff, (size_t)((batch + 255) / 256) * sizeof(int64_t), &pblock));
                RC_TRY(ws->get(kOpsTotals, (size_t)(nBatches + 1) * sizeof(int64_t), &ptotals));
                HIP_TRY(hipMemsetAsync(ptotals, 0, sizeof(int64_t), stream));
                // batch b's compacted operations: wait for its gather on the side stream, read the
                // running total, start the copy of its share
                // The host's own share of a batch - its operations into the caller's buffer, its slices of the per-target
                // arrays into the caller's arrays, its offsets - is done as soon as the batch's copies have LANDED
                // (`copyDone`), while the device is at work on the next batch; it used to wait for the next batch's
                // gather first, so that behind the last gather the host still had two shares to unpack, one after
                // the other (0.4 + 0.5 ms of a cfg3 search with the device idle).
                const double shareClock0 = PhaseTimer::now();
                unpack::AsyncWork sharer, arrayer;   // (declared behind everything their tasks refer to: drained first on every way out)
                auto hostShare = [&](int64_t landed, int64_t upToBatch) -> int {
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
                    auto workOps = [&opsToCaller, out, from, to, timed, searchT0] {
                        const double t0 = timed ? PhaseTimer::now() : 0;
                        if (to > from) opsToCaller(out, from, to, 4);
                        if (timed)
                            fprintf(stderr, "[miopal]     share at %.3f ms: %lld operations %.3f ms\n", (t0 - searchT0) * 1e3,
                                    (long long)(to - from), (PhaseTimer::now() - t0) * 1e3);
                    };
                    auto workArrays = [&prefixUpTo, ws, upTo, timed, searchT0, entries = std::move(entries)] {
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
                };
                auto fetchOps = [&](int64_t b) -> int {
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
                    if (upTo < opsFetched || upTo > opsCap) return fail(MIOPAL_ERR_INTERNAL, "bad operation count");
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
                };
                PerPairArgs paAll{};
                // the job lists of a group's batches, each sorted: eight small kernels per batch, 0.15 ms per group of cfg3.
                // The first group's run where they always ran; the NEXT group's are built on the side stream beside the
                // direction kernel of the group at hand (they need the start cells only, and their own parts of the lists)
                auto prepareGroup = [&](int64_t firstBatch, hipStream_t on) -> int {
                    const int64_t g0 = firstBatch * batch, g1 = std::min<int64_t>(n, (firstBatch + dirGroup) * batch);
                    for (int64_t b0 = g0, b = firstBatch; b0 < g1; b0 += batch, ++b) {
                        const int nb = (int)std::min<int64_t>(batch, n - b0);
                        PairJob* jobs = (PairJob*)pjobs + b0;
                        HIP_TRY(launchTraceJobs(nb, packRules(DpRules{1, 1, 0, kLastCell}), (const int32_t*)psq + b0,
                                                (const int32_t*)pst + b0, (const int32_t*)pi + b0, (const int32_t*)pj + b0,
                                                db->d_offsets + start + b0, slotDir, windowStrips > 1 ? maxWindow : 0, jobs,
                                                on));
                        HIP_TRY(launchSortJobsByLength(jobs, nb, (int)maxWindow, (int*)pbins, (PairJob*)psorted + b0, on,
                                                       maxHead > 0 ? (int*)phead + b : nullptr, (int)maxHead, sortRows));
                    }
                    return 0;
                };
                int64_t preparedGroup = -1;   // first batch of the group whose lists the side stream has been given
                Events jobsReady;
                auto launchGroup = [&](int64_t firstBatch) -> int {
                    const int64_t g0 = firstBatch * batch, g1 = std::min<int64_t>(n, (firstBatch + dirGroup) * batch);
                    if (preparedGroup == firstBatch) HIP_TRY(hipStreamWaitEvent(stream, jobsReady.ev[0], 0));
                    else RC_TRY(prepareGroup(firstBatch, stream));
                    paAll = perPair;
                    paAll.jobs = (const PairJob*)psorted + g0;
                    paAll.nJobs = (int)(g1 - g0);
                    paAll.dirs = (uint8_t*)pd;   // (the group's own buffer: the walks of the group before are done)
                    paAll.score = (int32_t*)pts + g0;   // job.out is relative to the batch: outBatch
                    paAll.outBatch = (int)batch;
                    paAll.skipWaves = maxHead > 0 ? (const int*)phead + firstBatch : nullptr;
                    paAll.dirWaveStride = slotDirUsed * kLanes;
                    paAll.dirStripColumns = (maxWindow + 3) & ~(int64_t)3;
                    if (windowStrips > 1) {
                        void* pb;
                        RC_TRY(ws->get(kPairB0, (size_t)((g1 - g0 + kLanes - 1) / kLanes * kLanes) * maxWindow * sizeof(int2), &pb));
                        paAll.boundary = (int2*)pb;
                        paAll.boundaryStride = maxWindow;
                    }
                    paAll.profileStride = packedStride;
                    paAll.packedBias = packedBias;
                    paAll.reversed = 0;
                    // (the big arrays leave beside THIS kernel - behind the job lists and their sorts, which crawl beside a
                    // copy. The kernel is enqueued FIRST: the five copies took the host 90 us, with the device idle)
                    const bool arrays = resultsPending || startsPending;
                    const bool ahead = overlapOps && g1 < n && !tuned(Tune::NO_JOBS_AHEAD);
                    if (arrays || ahead) RC_TRY(ws->ensureAux());
                    if (arrays) {
                        HIP_TRY(hipEventRecord(ws->evFork, stream));
                    }
                    HIP_TRY(launchPerPairPackedTrace(paAll, packedLds, stream));
                    if (arrays) RC_TRY(sendEarlyArrays(true));
                    if (ahead) {
                        // (BEHIND the direction kernel, beside the first walk: beside the direction kernel itself - which
                        // holds every register of the chip - the lists took 0.5 ms, the kernel 0.84 instead of 0.79 ms, and
                        // the copies behind them ran into the walk)
                        if (jobsReady.ev.empty()) {
                            jobsReady.ev.assign(2, nullptr);
                            for (auto& e : jobsReady.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                        }
                        HIP_TRY(hipEventRecord(jobsReady.ev[1], stream));
                        HIP_TRY(hipStreamWaitEvent(ws->aux, jobsReady.ev[1], 0));
                        RC_TRY(prepareGroup(firstBatch + dirGroup, ws->aux));
                        HIP_TRY(hipEventRecord(jobsReady.ev[0], ws->aux));
                        preparedGroup = firstBatch + dirGroup;
                    }
                    return 0;
                };
                for (int64_t b0 = 0, b = 0; b0 < n; b0 += batch, ++b) {
                    const int nb = (int)std::min<int64_t>(batch, n - b0);
                    PairJob* jobs = (PairJob*)pjobs + b0;
                    bool startMarked = false;
                    if (oneLaunch && b % dirGroup == 0) {
                        // (the copy of the batch before starts beside this launch, not behind it)
                        if (overlapOps) HIP_TRY(hipEventRecord(traceStart.ev[(size_t)b], stream));
                        startMarked = true;
                        RC_TRY(launchGroup(b));
                    }
                    if (!oneLaunch)
                        HIP_TRY(launchTraceJobs(nb, packRules(DpRules{1, 1, 0, kLastCell}), (const int32_t*)psq + b0,
                                                (const int32_t*)pst + b0, (const int32_t*)pi + b0, (const int32_t*)pj + b0,
                                                db->d_offsets + start + b0, slotDir, windowStrips > 1 ? maxWindow : 0, jobs,
                                                stream));
                    // job.out is relative to the batch: offset the score pointer
                    WalkArgs wa{};
                    auto markTraceStart = [&]() -> int {
                        if (overlapOps && !startMarked) HIP_TRY(hipEventRecord(traceStart.ev[(size_t)b], stream));
                        RC_TRY(sendEarlyArrays());
                        return 0;
                    };
                    if (traceLanePerPair && oneLaunch) {
                        // (sorted and swept above; what is left per batch: the outliers at the head of its list)
                        jobs = (PairJob*)psorted + b0;
                        wa.slotByOut = 1;
                        RC_TRY(markTraceStart());
                        if (maxHead > 0) {
                            const int nh = (int)std::min<int64_t>(nb, maxHead * kLanes);
                            RC_TRY(s.runDeviceJobs(jobs, nh, (int32_t*)pts + b0, nullptr, nullptr, true,
                                                   (uint8_t*)pheadDirs, windowStrips > 1 ? maxWindow : 0,
                                                   (const int*)phead + b, slotDir));
                            wa.headWaves = (const int*)phead + b;
                            wa.headDirs = (const uint8_t*)pheadDirs;
                            wa.headDirStride = slotDir;
                        }
                        wa.dirPlanes = 1;
                        wa.dirColumnMajor = 1;
                        wa.dirWaveStride = paAll.dirWaveStride;
                        wa.dirStripColumns = paAll.dirStripColumns;
                    } else if (traceLanePerPair) {
                        // neighbours of similar length share a wavefront; results stay addressed by job.out
                        if (sortJobs) {
                            HIP_TRY(launchSortJobsByLength(jobs, nb, (int)maxWindow, (int*)pbins, (PairJob*)psorted,
                                                           stream, (int*)phead, (int)maxHead, sortRows));
                            jobs = (PairJob*)psorted;
                            wa.slotByOut = 1;
                        }
                        PerPairArgs pa = perPair;
                        if (maxHead > 0) {
                            // outliers at the head of the sorted list: one wavefront per pair
                            const int nh = (int)std::min<int64_t>(nb, maxHead * kLanes);
                            RC_TRY(s.runDeviceJobs(jobs, nh, (int32_t*)pts + b0, nullptr, nullptr, true,
                                                   (uint8_t*)pheadDirs, windowStrips > 1 ? maxWindow : 0,
                                                   (const int*)phead, slotDir));
                            pa.skipWaves = (const int*)phead;
                            wa.headWaves = (const int*)phead;
                            wa.headDirs = (const uint8_t*)pheadDirs;
                            wa.headDirStride = slotDir;
                        }
                        pa.jobs = jobs;
                        pa.nJobs = nb;
                        pa.dirs = (uint8_t*)pd;
                        pa.score = (int32_t*)pts + b0;  // job.out is relative to the batch
                        pa.dirWaveStride = slotDirUsed * kLanes;
                        // (the bit planes come in blocks of four columns: a multiple of 4, within the slot's maxWindow + 63)
                        pa.dirStripColumns = profileStride > 0 ? ((maxWindow + 3) & ~(int64_t)3) : maxWindow + kLanes - 1;
                        if (windowStrips > 1) {
                            void* pb;
                            RC_TRY(ws->get(kPairB0, (size_t)((nb + kLanes - 1) / kLanes * kLanes) * maxWindow *
                                                        sizeof(int2), &pb));
                            pa.boundary = (int2*)pb;
                            pa.boundaryStride = maxWindow;
                        }
                        pa.profileStride = profileStride;
                        pa.reversed = 0;
                        RC_TRY(markTraceStart());
                        if (packedTrace) {
                            pa.profileStride = packedStride;
                            pa.packedBias = packedBias;
                            HIP_TRY(launchPerPairPackedTrace(pa, packedLds, stream));
                            wa.dirColumnMajor = 1;
                        } else {
                            HIP_TRY(launchPerPair(pa, kPerPairTrace, stream));
                        }
                        wa.dirPlanes = profileStride > 0;
                        wa.dirWaveStride = pa.dirWaveStride;
                        wa.dirStripColumns = pa.dirStripColumns;
                    } else {
                        RC_TRY(markTraceStart());
                        RC_TRY(s.runDeviceJobs(jobs, nb, (int32_t*)pts + b0, nullptr, nullptr, true, (uint8_t*)pd,
                                               windowStrips > 1 ? maxWindow : 0));
                    }
                    wa.jobs = jobs;
                    wa.nJobs = nb;
                    wa.residues = db->d_residues;
                    wa.query = s.d_query;
                    wa.dirs = (const uint8_t*)pd + (oneLaunch ? ((b % dirGroup) * batch / kLanes) * (slotDirUsed * kLanes) : 0);
                    wa.ops = (uint8_t*)pslots;
                    wa.opsOff = nullptr;
                    wa.opsSlot = slotOps;
                    wa.queryLength = queryLength;
                    wa.opsLen = (int32_t*)plen + b0;
                    HIP_TRY(launchWalk(wa, stream));
                    HIP_TRY(launchGatherOps(nb, (const uint8_t*)pslots, slotOps, (const int32_t*)plen + b0,
                                            (int64_t*)pblock, (const int64_t*)ptotals + b, (int64_t*)ptotals + b + 1,
                                            (uint8_t*)pcompact, stream));
                    if (overlapOps) {
                        HIP_TRY(hipEventRecord(batchDone.ev[(size_t)b], stream));
                        if (b > 0) RC_TRY(fetchOps(b - 1));   // batch b is queued behind it: the GPU stays busy
                    }
                }
                // results back to the host: the small arrays (they carry the total size) are enqueued behind the last
                // batch's kernels before the host turns to the last batch's operations - the copies run side by side
                int64_t total = 0;
                RC_TRY(ws->stageDownload(&total, (const int64_t*)ptotals + nBatches, sizeof(int64_t)));
                if (!sideArrays) {
                    RC_TRY(ws->stageDownload(lens, plen, (size_t)n * sizeof(int32_t)));
                    RC_TRY(ws->stageDownload(startQuery, psq, (size_t)n * sizeof(int32_t)));
                    RC_TRY(ws->stageDownload(startTarget, pst, (size_t)n * sizeof(int32_t)));
                    RC_TRY(ws->stageDownload(tscore, pts, (size_t)n * sizeof(int32_t)));
                }
                // (the threads that will unpack the last share, started while the device is at work on the last batch)
                std::unique_ptr<unpack::Crew> crew;
                if (overlapOps && copyOutEarly && !tuned(Tune::NO_UNPACK_CREW) &&
                    (nBatches > 1 ? opsFetched / (nBatches - 1) : opsCap / 4) >= (4 << 20)) {
                    try {
                        crew.reset(new unpack::Crew(7));
                    } catch (const std::exception&) {
                        crew.reset();
                    }
                }
                if (overlapOps) RC_TRY(fetchOps(nBatches - 1));
                pt.mark("traceback batches (enqueued)");
                RC_TRY(ws->finishDownloads());
                pt.mark("device pipeline + small D2H");
                sharer.drain();
                arrayer.drain();
                pt.mark("the helpers' shares");
                if (total < 0 || total > n * slotOps) return fail(MIOPAL_ERR_INTERNAL, "bad operation count");
                if (!outOps->resize((size_t)total)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
                std::thread copier;
                if (overlapOps) {
                    // already in pinned memory (finishDownloads above waited for the side stream too): copied
                    // out by helper threads while this one turns lengths into offsets and checks the scores
                    if (opsFetched != total) return fail(MIOPAL_ERR_INTERNAL, "operation count changed");
                    uint8_t* const out = outOps->data;
                    const int64_t from = opsCopiedOut;
                    // (the device has finished: this share is all that is left of the search - eight threads)
                    const uint8_t* const staged = (const uint8_t*)ws->pinned + opsBase;
                    unpack::Crew* const helpers = total > from ? crew.get() : nullptr;
                    try {
                        copier = std::thread([&opsToCaller, helpers, staged, out, from, total] {
                            if (helpers) helpers->run(out, staged, from, total);
                            else opsToCaller(out, from, total, 8);
                        });
                    } catch (const std::exception&) {
                        if (helpers) helpers->run(out, staged, from, total);
                        else opsToCaller(out, from, total, 8);
                    }
                } else {
                    RC_TRY(ws->stageDownload(outOps->data, pcompact, (size_t)total));
                }
                struct Joiner {
                    std::thread& t;
                    ~Joiner() { if (t.joinable()) t.join(); }
                } joinCopier{copier};
                prefixUpTo(n);
                if (outOff[n] != total) return fail(MIOPAL_ERR_INTERNAL, "operation offsets disagree with the device");
                if (copier.joinable()) copier.join();
                RC_TRY(ws->finishDownloads());
                pt.mark("operations D2H");
                if (wrongAt >= 0)
                    return fail(MIOPAL_ERR_INTERNAL, "traceback score %d differs from search score %d for target %lld",
                                tscore[(size_t)wrongAt], score[wrongAt], (long long)(start + wrongAt));
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
        }
    }

    // ---- start locations: reversed prefixes anchored on the end cell ----------
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
    std::vector<int64_t> live;  // slots with a non-empty alignment
    for (int64_t k = 0; k < n; ++k)
        if (endQuery[k] >= 0 && endTarget[k] >= 0) live.push_back(k);
    if (mode == OPAL_MODE_NW) {
        for (int64_t k : live) startQuery[k] = startTarget[k] = 0;
    } else if (!live.empty()) {
        const DpRules rr{1, 1, 0, fr.region};
        void *rs, *ri, *rj;
        const bool onDevice = queryLength <= kLanes;  // no strip workspace: jobs are built in HBM
        const size_t nOut = onDevice ? (size_t)n : live.size();
        RC_TRY(ws->get(kRScore, nOut * sizeof(int32_t), &rs));
        RC_TRY(ws->get(kRI, nOut * sizeof(int32_t), &ri));
        RC_TRY(ws->get(kRJ, nOut * sizeof(int32_t), &rj));
        if (onDevice) {
            void* pjobs;
            RC_TRY(ws->get(kJobs, (size_t)n * sizeof(PairJob), &pjobs));
            // pi / pj still hold the end locations of the forward pass (slice order)
            HIP_TRY(launchReverseJobs((int)n, (const int32_t*)ps, (const int32_t*)pi, (const int32_t*)pj,
                                      db->d_offsets + start, packRules(rr), 0, (PairJob*)pjobs, stream));
            RC_TRY(s.runDeviceJobs((const PairJob*)pjobs, (int)n, (int32_t*)rs, (int32_t*)ri, (int32_t*)rj));
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
            RC_TRY(s.runPairs(jobs, false, (int32_t*)rs, (int32_t*)ri, (int32_t*)rj, nullptr));
        }
        std::unique_ptr<int32_t[]> hs(new int32_t[nOut]), hi(new int32_t[nOut]), hj(new int32_t[nOut]);
        RC_TRY(ws->stageDownload(hs.get(), rs, nOut * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(hi.get(), ri, nOut * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(hj.get(), rj, nOut * sizeof(int32_t)));
        RC_TRY(ws->finishDownloads());
        for (size_t x = 0; x < live.size(); ++x) {
            const int64_t k = live[x];
            const size_t o = onDevice ? (size_t)k : x;
            int ri = hi[o], rj = hj[o];
            if (hs[o] != score[k] || ri < 0 || rj < 0) {
                // degenerate optimum (oracle/opal_oracle.c): one gap over one sequence only,
                // i.e. a border cell of the reversed problem; the other sequence's span is empty
                if (mode != OPAL_MODE_SW && score[k] == borderGap(endQuery[k], gapOpen, gapExt)) {
                    ri = endQuery[k];
                    rj = -1;
                } else if (mode == OPAL_MODE_OV && score[k] == borderGap(endTarget[k], gapOpen, gapExt)) {
                    ri = -1;
                    rj = endTarget[k];
                } else {
                    return fail(MIOPAL_ERR_INTERNAL, "reverse pass disagrees with the forward score for target %lld",
                                (long long)(start + k));
                }
            }
            startQuery[k] = endQuery[k] - ri;
            startTarget[k] = endTarget[k] - rj;
        }
    }

    pt.mark("start-location pass");
    // ---- traceback on [start..end] rectangles, batched by direction workspace --
    size_t pos = 0;
    while (pos < live.size()) {
        std::vector<PairJob> jobs;
        std::vector<int64_t> opsOff(1, 0);
        int64_t dirBytes = 0;
        size_t first = pos;
        while (pos < live.size()) {
            const int64_t k = live[pos];
            const int qn = endQuery[k] - startQuery[k] + 1, tn = endTarget[k] - startTarget[k] + 1;
            const int64_t need = (int64_t)((qn + kLanes - 1) / kLanes) * (tn + kLanes - 1) * kLanes;
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
        void *pd, *po, *poff, *plen, *pscore;
        RC_TRY(ws->get(kDirs, (size_t)dirBytes, &pd));
        RC_TRY(ws->get(kOps, (size_t)opsOff.back(), &po));
        RC_TRY(ws->get(kOpsOff, opsOff.size() * sizeof(int64_t), &poff));
        RC_TRY(ws->get(kOpsLen, jobs.size() * sizeof(int32_t), &plen));
        RC_TRY(ws->get(kRScore, jobs.size() * sizeof(int32_t), &pscore));
        RC_TRY(ws->stageUpload(poff, opsOff.data(), opsOff.size() * sizeof(int64_t), stream));
        RC_TRY(s.runPairs(jobs, true, (int32_t*)pscore, nullptr, nullptr, (uint8_t*)pd));
        WalkArgs wa{};
        void* pjobs;
        RC_TRY(ws->get(kJobs, jobs.size() * sizeof(PairJob), &pjobs));
        wa.jobs = (const PairJob*)pjobs;
        wa.nJobs = (int)jobs.size();
        wa.residues = db->d_residues;
        wa.query = s.d_query;
        wa.dirs = (const uint8_t*)pd;
        wa.ops = (uint8_t*)po;
        wa.opsOff = (const int64_t*)poff;
        wa.opsLen = (int32_t*)plen;
        wa.queryLength = queryLength;
        HIP_TRY(launchWalk(wa, stream));
        if (pt.on) { HIP_TRY(hipStreamSynchronize(stream)); pt.mark("  trace + walk kernels"); }
        const size_t opsBytes = (size_t)opsOff.back();
        std::unique_ptr<uint8_t[]> ops(new uint8_t[std::max<size_t>(opsBytes, 1)]);
        std::unique_ptr<int32_t[]> lens(new int32_t[jobs.size()]), tscore(new int32_t[jobs.size()]);
        RC_TRY(ws->stageDownload(ops.get(), po, opsBytes));
        RC_TRY(ws->stageDownload(lens.get(), plen, jobs.size() * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(tscore.get(), pscore, jobs.size() * sizeof(int32_t)));
        RC_TRY(ws->finishDownloads());
        pt.mark("  ops D2H");
        for (size_t x = 0; x < jobs.size(); ++x) {
            const int64_t k = live[first + x];
            if (tscore[x] != score[k])
                return fail(MIOPAL_ERR_INTERNAL, "traceback score %d differs from search score %d for target %lld",
                            tscore[x], score[k], (long long)(start + k));
            const int len = lens[x];
            const uint8_t* src = ops.get() + opsOff[x + 1] - len;
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
        pt.mark("  host copy-out");
    }
    if (flat)
        for (int64_t k = 0; k < n; ++k) flatOff[k + 1] += flatOff[k];
    return 0;
}

