// Part of host.hip (included there, not a translation unit of its own): one search: the score pass (routing between the kernels, lane-width ladder, side stream).
// The two product knobs: a handle option (miopalDbSetOption) wins over the process-wide switch.
static inline int reservedCus(const MiopalDb* db) {   // -1: nobody asked
    const int opt = db->optReserveCus.load(std::memory_order_relaxed);
    if (opt >= 0) return opt;
    if (const char* r = tuned(Tune::RESERVE_CUS)) return std::max(0, atoi(r));
    return -1;
}
static inline bool smallSearchAllowed(const MiopalDb* db) {
    const int opt = db->optSmallSearch.load(std::memory_order_relaxed);
    if (opt >= 0) return opt != 0;
    return !tuned(Tune::NO_SMALL_SEARCH);
}

// the extreme entries of a score source (a matrix, the rows of a PSSM); no entries: no scores, 0 and 0
static inline void scoreExtremes(const int* entries, size_t count, int* maxScore, int* minScore) {
    *maxScore = count ? *std::max_element(entries, entries + count) : 0;
    *minScore = count ? *std::min_element(entries, entries + count) : 0;
}

// The column split's plan (interseq_impl.h): the launch's chunks - those of groupChunks[0 .. nGroups) in order, fewer
// than 2^31 - cut into `wavefronts` equal intervals. Entry w = where interval w begins and w - 1 ends: the group that
// holds that chunk (nGroups behind the last chunk), how many of the group's chunks lie in front of it, and its number.
static std::vector<int4> splitPlanOf(const int* groupChunks, int nGroups, int wavefronts) {
    int64_t total = 0;
    for (int g = 0; g < nGroups; ++g) total += groupChunks[g];
    const int64_t each = total / wavefronts, rest = total % wavefronts;
    std::vector<int4> plan((size_t)wavefronts + 1);
    int g = 0;
    int64_t before = 0;   // chunks of the groups in front of g
    for (int w = 0; w <= wavefronts; ++w) {
        const int64_t x = w * each + w * rest / wavefronts;
        while (g < nGroups && before + groupChunks[g] <= x) before += groupChunks[g++];
        plan[(size_t)w] = make_int4(g, (int)(x - before), (int)x, 0);
    }
    return plan;
}

// ---- one search ----------------------------------------------------------------
struct Search {
    MiopalDb* db;
    Workspace* ws;
    hipStream_t stream;
    const unsigned char* query;
    int Q, open, ext, A, searchType, mode;
    const int* matrix;
    int64_t start, end;
    int64_t n;
    // The score source. Plain searches: `matrix` ([A][A]) indexed by the query's residues. A position-specific
    // scoring matrix (miopalSearchPssm): pssmRows ([Q][A], row i = the scores of query position i), `matrix` is null
    // and `query` is the consensus (residues or 255), which only the traceback's match / mismatch test reads.
    // Everything on the host reads scores through at(); the kernels take d_rows where they index by row.
    const int* pssmRows = nullptr;
    int at(int i, int t) const { return pssmRows ? pssmRows[(size_t)i * A + t] : matrix[query[i] * A + t]; }
    int maxScore = 0, minScore = 0;
    int64_t balancedChunks = 0;
    bool globalPairRefused = false;   // the pair-table launch for NW / HW / OV failed on this device
    bool pairStripsRefused = false;   // the same for the multi-strip Smith-Waterman kernel
    bool globalStripsRefused = false; // ... and for the multi-strip NW / HW / OV kernel
    int* d_stripError = nullptr;      // units of intraseq_strips_kernel that gave up waiting (never seen)
    int stripErrorHost = 0;
    bool stripsEndsDeclined = false;  // ... with end locations: a probe of the longest groups left its range of 384
    // Smith-Waterman end locations of several strips whose scores are beyond the row keys' range: two sweeps of
    // the strips kernel - scores, then the first cell that holds each target's score (round 3)
    bool twoPassEnds = false;
    // miopalSearch: a pinned, device-visible buffer the scores may be written to directly (the one-strip
    // Smith-Waterman fast path scatters into it from the kernel); wroteHost says that it was used
    int32_t* hostScoreOut = nullptr;
    int32_t *hostEndIOut = nullptr, *hostEndJOut = nullptr;   // with end locations: query / target coordinates
    uint64_t hostScoreGeneration = 0;   // of the staging buffer when hostScoreOut was reserved in it
    bool hostScoreIsCallers = false;    // hostScoreOut is the caller's own pinned array
    bool wroteHost = false;
    bool besidePersistent = false;    // the side jobs of this pass run beside a strips kernel (persistent, one workgroup per CU)
    // a score pass that starts over (refused launch, declined probe) has already put its side jobs on
    // the side stream: they are not enqueued twice, and the join still waits for them
    // test hook (miopalTestInjectFault): kind 1 = a unit of the pair-table strips kernels, 2 = a unit of
    // intraseq_strips_kernel publishes nothing; the units below it wait at most faultSpinCap polls
    int faultKind = 0, faultUnit = 0, faultSpinCap = 0;
    std::vector<int32_t> sideDone;    // result slots computed on the side stream in this search, sorted
    bool sideForked = false;
    // the cut of the first pass through the routing (groups that leave for the side kernel): a pass that starts over
    // - a declined probe, two sweeps after all - keeps it, its side jobs are already on their way
    const View* cutView = nullptr;
    int cutFirstGroup = 0;

    uint8_t* d_query = nullptr;
    int32_t* d_matrix = nullptr;
    int32_t* d_rows = nullptr;         // pssmRows on the device ([Q][A]); null for a plain search

    // the border / answer rules of `mode`: set by scorePassImpl, read by its steps
    DpRules r{};
    int rules = 0;
    ScoreModel model() const { return {open, ext, maxScore, minScore}; }

    int rulesFor(int m, DpRules* out) const {
        if (rulesForMode(m, out)) return 0;
        return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", m);
    }

    int prepare() {
        if (g_fault[0] != 0) {   // one search only
            faultKind = g_fault[0];
            faultUnit = g_fault[1];
            faultSpinCap = g_fault[2];
            g_fault[0] = 0;
        }
        // (the extreme entries of the rows where the matrix's stand; no rows: no scores, as for an empty query)
        if (pssmRows) scoreExtremes(pssmRows, (size_t)std::max(Q, 0) * A, &maxScore, &minScore);
        else scoreExtremes(matrix, (size_t)A * A, &maxScore, &minScore);
        return 0;
    }

    // query + matrix are only needed by the intra-sequence / traceback kernels
    int ensurePairInputs() {
        if (d_query) return 0;
        void* p;
        RC_TRY(ws->get(kQuery, (size_t)std::max(Q, 1), &p));
        d_query = (uint8_t*)p;
        RC_TRY(ws->stageUpload(d_query, query, (size_t)Q, stream));
        if (pssmRows) {
            // (no [A][A] matrix: the kernels' row-indexed forms read the rows, the walk the consensus)
            RC_TRY(ws->get(kPssmRows, std::max<size_t>((size_t)Q * A, 1) * sizeof(int32_t), &p));
            d_rows = (int32_t*)p;
            RC_TRY(ws->stageUpload(d_rows, pssmRows, (size_t)Q * A * sizeof(int32_t), stream));
            return 0;
        }
        RC_TRY(ws->get(kMatrix, (size_t)A * A * sizeof(int32_t), &p));
        d_matrix = (int32_t*)p;
        RC_TRY(ws->stageUpload(d_matrix, matrix, (size_t)A * A * sizeof(int32_t), stream));
        return 0;
    }

    bool interseqUsable() const {
        if (Q <= 0) return false;
        if (open < 0 || ext < 0) return false;
        if (maxScore > 16383 || minScore < -16383) return false;
        return true;
    }

    // Runs the intra-sequence kernel over `jobs`; results land in the given device arrays.
    int runPairs(std::vector<PairJob>& jobs, bool trace, int32_t* d_score, int32_t* d_endI,
                 int32_t* d_endJ, uint8_t* d_dirs, hipStream_t on = nullptr, int slotBase = 0) {
        if (jobs.empty()) return 0;
        if (!on) on = stream;
        RC_TRY(ensurePairInputs());
        int64_t wsElems = 0;
        for (auto& j : jobs) {
            j.wsOff = wsElems;
            if (j.qLen > kLanes) wsElems += j.tLen;
        }
        void *pj, *b0, *b1;
        // the side stream has its own job / boundary buffers (slotBase = kAuxJobs - kJobs)
        RC_TRY(ws->get(kJobs + slotBase, jobs.size() * sizeof(PairJob), &pj));
        RC_TRY(ws->get(kPairB0 + slotBase, (size_t)wsElems * sizeof(int2), &b0));
        RC_TRY(ws->get(kPairB1 + slotBase, (size_t)wsElems * sizeof(int2), &b1));
        RC_TRY(ws->stageUpload(pj, jobs.data(), jobs.size() * sizeof(PairJob), on));
        IntraseqArgs a{};
        a.jobs = (const PairJob*)pj;
        a.nJobs = (int)jobs.size();
        a.residues = db->d_residues;
        a.query = d_query;
        a.matrix = d_matrix;
        a.rows = d_rows;
        a.alphabet = A;
        a.gapOpen = open;
        a.gapExt = ext;
        a.boundary[0] = (int2*)b0;
        a.boundary[1] = (int2*)b1;
        a.dirs = d_dirs;
        a.score = d_score;
        a.endI = d_endI;
        a.endJ = d_endJ;
        a.raisePriority = on != stream ? 1 : 0;
        // Pairs of several strips, scores / end locations: one wavefront per (pair, strip), the strips of
        // a pair side by side (intraseq.hip) - a pair is then a chain of L + 63 steps, not strips x that.
        // Worth it while the pairs are few against the chip (a chain is what is waited for); thousands of
        // pairs fill the chip either way.
        bool uniform = !trace && !jobs.empty() && jobs[0].qLen > kLanes && !tuned(Tune::NO_PAIR_STRIP_UNITS);
        for (const auto& j : jobs)
            if (j.qLen != jobs[0].qLen) uniform = false;
        const int jobStrips = uniform ? (jobs[0].qLen + kLanes - 1) / kLanes : 1;
        if (uniform && jobStrips >= 2 && (int64_t)jobs.size() * jobStrips <= (1 << 20) &&
            (int64_t)jobs.size() <= 16 * (int64_t)db->computeUnits) {
            void *st, *pt;
            const size_t ints = jobs.size() * (size_t)jobStrips + 1;
            RC_TRY(ws->get(kPairStripState + slotBase, ints * sizeof(int), &st));
            RC_TRY(ws->get(kPairStripPartial + slotBase, (ints - 1) * sizeof(int4), &pt));
            HIP_TRY(hipMemsetAsync(st, 0, ints * sizeof(int), on));
            if (!d_stripError) {
                // The counter only ever moves when a unit gives up, and a search that sees it moved
                // fails and zeroes it again (checkStripError): it is zeroed ONCE, when the workspace allocates
                // it, and the host waits for that - a memset left behind on whichever of the two streams asks
                // first is one that launches on the other stream would not be ordered after.
                // (On the asking stream and waited for there, not hipMemset: that one runs on the null stream,
                // which these non-blocking streams are not ordered with, and a search beside searches of other
                // threads read the counter of a fresh allocation before the zero had landed - -2 and 6439
                // "units gave up", tests/test_gpu_call_order.py, four threads with MIOPAL_PARKED_WORKSPACE_MB=0.)
                const bool fresh = ws->cap[kPairStripError] == 0;
                void* pe;
                RC_TRY(ws->get(kPairStripError, sizeof(int), &pe));
                if (fresh) {
                    HIP_TRY(hipMemsetAsync(pe, 0, sizeof(int), on));
                    HIP_TRY(hipStreamSynchronize(on));
                }
                d_stripError = (int*)pe;
            }
            a.nStrips = jobStrips;
            a.stripCounter = (int*)st;
            a.stripProgress = (int*)st + 1;
            a.stripPartial = (int4*)pt;
            a.error = d_stripError;
            a.stripWaitCap = faultSpinCap;
            a.faultUnit1 = faultKind == 2 ? faultUnit + 1 : 0;
            a.fatBlocks = besidePersistent ? 1 : 0;
            HIP_TRY(launchIntraseqStrips(a, on));
            return 0;
        }
        // pairs of one strip without the stop rule or direction bytes: two columns a step (intraseq_wide_kernel, round 4)
        bool wide = !trace;
        for (const auto& j : jobs)
            if (j.qLen > kLanes || (j.rules & kRuleStop)) wide = false;
        a.wide = wide ? 1 : 0;
        HIP_TRY(launchIntraseq(a, trace, on));
        return 0;
    }

    // Same with a job list that already sits in HBM. wsStride > 0: the jobs' query pieces may have
    // more than 64 rows, job k owns wsStride strip-boundary columns at wsOff = k * wsStride.
    // headWaves: only the first *headWaves x 64 jobs (hybrid direction pass), addressed by position.
    int runDeviceJobs(const PairJob* d_jobs, int nJobs, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ,
                      bool trace = false, uint8_t* d_dirs = nullptr, int64_t wsStride = 0,
                      const int* headWaves = nullptr, int64_t headDirStride = 0) {
        if (nJobs <= 0) return 0;
        RC_TRY(ensurePairInputs());
        IntraseqArgs a{};
        a.headWaves = headWaves;
        a.headDirStride = headDirStride;
        a.headWsStride = wsStride;
        if (wsStride > 0) {
            void *b0, *b1;
            RC_TRY(ws->get(kPairB0, (size_t)nJobs * wsStride * sizeof(int2), &b0));
            RC_TRY(ws->get(kPairB1, (size_t)nJobs * wsStride * sizeof(int2), &b1));
            a.boundary[0] = (int2*)b0;
            a.boundary[1] = (int2*)b1;
        }
        a.jobs = d_jobs;
        a.nJobs = nJobs;
        a.residues = db->d_residues;
        a.query = d_query;
        a.matrix = d_matrix;
        a.rows = d_rows;
        a.alphabet = A;
        a.gapOpen = open;
        a.gapExt = ext;
        a.score = d_score;
        a.endI = d_endI;
        a.endJ = d_endJ;
        a.dirs = d_dirs;
        HIP_TRY(launchIntraseq(a, trace, stream));
        return 0;
    }

    // After the streams have drained: did a (pair, strip) unit of intraseq_strips_kernel give up?
    // (both entry points that can route pairs there call it; never seen outside the fault-injection test)
    int checkStripError() {
        if (stripErrorHost == 0) return 0;
        const int seen = stripErrorHost;
        stripErrorHost = 0;
        HIP_TRY(hipMemsetAsync(d_stripError, 0, sizeof(int), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return fail(MIOPAL_ERR_INTERNAL, "%d (pair, strip) units of the wavefront-per-pair kernel gave up waiting for the strip above", seen);
    }

    PairJob forwardJob(int64_t id, int rules) const {
        PairJob j{};
        j.tOff = db->offsets[id];
        j.tLen = dbLen(db, id);
        j.tStep = 1;
        j.qOff = 0;
        j.qLen = Q;
        j.qStep = 1;
        j.rules = rules;
        j.out = (int32_t)(id - start);
        return j;
    }

    // ---- the score pass ------------------------------------------------------------------------------------------
    // scorePassImpl (at the end) is a sequence of steps: a plan (planWindows .. planLanes: no device call, no
    // workspace - they read this search's scalars, the handle's sizes, the tuning switches and the view's host
    // fields), then the profile, the side jobs, the kernel arguments, one of three launches, the scatter.
    // What one pass through the routing decided: rebuilt by every pass. What has to survive a pass that starts over
    // (refused launches, the declined probe, two sweeps, what is on the side stream, the cut) is on Search, above.
    struct ScorePlan {
        bool sw = false, locate = false;   // Smith-Waterman; end locations wanted
        // planWindows: long targets as overlapping windows
        int64_t queryBest = 0;
        int overlap = 0, stride = 0;
        int keyBias = 0;                   // HW in windows: scores above -2^22 in the merge keys
        bool keyed = false;                // windows with end locations: merged by key
        // planGeneralStrips / planSwPairStrips / planGlobalPairStrips
        int nStrips = 1, waves = 1;
        int stripRows = 0;                 // > 0: a multi-strip pair-table kernel, strips of that many rows
        bool globalStrips = false;         // ... the NW / HW / OV one
        // planSideCut: the leading groups that leave for the side kernel
        int firstGroup = 0, firstPos = 0;
        // planLanes: the lane arithmetic, its limits, and which targets the int32 kernel takes
        bool pairStrips = false;
        int rows = 0, qPad = 0, nSym = 0, pairRows = 0;
        int packedSkip = 0;                // first view position whose packed result is scattered
        int capGroups = 0, capChunks = 0;
        bool twoPass = false, rowKeys = false;
        bool usePair = false, biased = false, globalPair = false;
        bool swShifted = false, halfFloat = false;
        int biasedLimit = 0, swBias = 0, swLimit = 0, profileShift = 0;
        int64_t globalZero = 0;
        InterseqFlavour flavour = kSwInt16;
        bool mayOverflow = false;
        int64_t directLimit = 0;           // flagged lanes redone one by one before the view takes the next rung
        bool probeEnds = false;            // the strips kernel with row keys: probe the longest groups' scores first
    };
    // device buffers of a pass that several steps use
    struct PassBuffers {
        void* keys = nullptr;   // merge keys of a windowed search with end locations
        void* vo = nullptr;     // view-order overflow flags
        void* ct = nullptr;     // count of flagged lanes
    };
    // (a target whose windows are neighbours in the view is queued once)
    void queueWhole(std::vector<PairJob>& list, int32_t id) const {
        if (list.empty() || list.back().out != (int32_t)(id - start)) list.push_back(forwardJob(id, rules));
    }

    // step 1: the small-search route
    bool smallSearch() const {
        // Small searches: the wavefront-per-pair kernel has the shorter start-up (0.08-0.1 ms for a handful of targets
        // against 0.26-1.3 ms for the packed kernels' views, tables and persistent launch). Queries of one strip: up to
        // kSmallSearch targets. Longer ones: when an estimate of its time is below one of the packed kernels' - both
        // read off the small corner of the routing table (profiles/r03_small_searches_long_queries.txt): 7e9 strip
        // steps a second, a longest target whose strips follow each other 64 steps apart at 0.25 us a step, against
        // 0.26 ms + 0.6 us per query residue. (4 targets against a 300 / 2000-aa query 0.48 / 1.3 -> 0.18 / 0.72 ms,
        // 1000 x 300 against 300 aa 0.45 -> 0.34 ms; a thousand targets of which a tenth have 3000 residues stay packed.)
        bool small = Q <= kLanes && n <= kSmallSearch;
        if (Q > kLanes && n <= kSmallSearch) {
            const int64_t strips = ((int64_t)Q + kLanes - 1) / kLanes;
            const int64_t residues = db->offsets[(size_t)end] - db->offsets[(size_t)start];
            const int64_t steps = strips * (residues + (int64_t)(kLanes - 1) * n);
            const double perPair = 0.075 + std::max((double)steps / 7e6, (double)(db->maxLen + kLanes * strips) * 0.00025);
            // (round 4: ... and the packed kernels sweep the longest target column by column, about 0.3 us each with
            // the strips of a group pipelined over a workgroup: a thousand log-normal targets at Q = 65 .. 300 took
            // 0.6 - 1.1 ms packed and 0.43 - 0.53 ms one wavefront per pair, profiles/r04e_routing_table.txt)
            // (queries up to ~500 residues: beyond, the strips kernels run a group's strips side by side and the packed
            // side wins again - a thousand targets at Q = 1000: 1.4 ms packed, 1.75 one wavefront per pair)
            const double packed = 0.26 + 0.0006 * (double)Q + (Q <= 512 ? 0.0003 * (double)db->maxLen : 0.0);
            small = perPair < packed;
        }
        return small;
    }

    // step 2: the window plan
    void planWindows(ScorePlan& p) const {
        // Smith-Waterman: long targets can be searched as overlapping windows. A
        // local alignment with a positive score has at most Q aligned pairs and, each gap
        // column costing at least min(open, ext), at most Q * max(S) / min(open, ext) gap
        // columns, so it spans at most that many target columns (`reach`): with windows that
        // overlap by `reach` every alignment lies inside one of them, and the maximum over a
        // target's windows is its score. No window is longer than stride + overlap, so no
        // target has to leave the packed kernel for the 14x dearer wavefront-per-pair kernel.
        // (The aligned pairs are bounded by the query itself: every residue is aligned at most once, at best with
        // its most favourable partner - 280 for the 53-aa README query under BLOSUM62, where Q * max(S) says 583:
        // windows that overlap by 384 columns instead of 640.)
        p.queryBest = queryBest(Q, A, [this](int i, int t) { return at(i, t); });
        const int64_t pairsBest = std::min<int64_t>((int64_t)Q * std::max(maxScore, 0), p.queryBest);
        p.overlap = 0;
        if (mode == OPAL_MODE_SW && std::min(open, ext) > 0 && maxScore > 0 && (int64_t)Q * maxScore < (1 << 23) &&
            Q < 65536 && db->maxLen < (1 << 24) && !tuned(Tune::NO_SEGMENTS)) {
            const int64_t reach = Q + pairsBest / std::min(open, ext) + 1;
            // (steps of 128: queries of similar length share one cached view, and the window - the
            // critical path of a group of long targets - stays close to what the query needs)
            const int64_t rounded = (reach + 127) / 128 * 128;
            // WHETHER to cut is still decided on the bound of before (Q max(S)): cutting is not always the
            // cheaper way - few targets (the wavefront-per-pair kernel spreads the long ones over the idle
            // CUs: Q = 150 on 20k log-normal targets 0.86 ms, in windows 1.5 ms) or long targets that are the
            // bulk of the database (every window repeats `overlap` columns: a tenth of 500k targets thirty times
            // as long as the rest, Q = 150: 4.3 ms whole, 6.5 ms in windows) - and the old bound happened to
            // draw that line well (profiles/r03e_routing_table_windows_whenever_possible.txt has the table
            // with windows wherever the new bound allows them: 172 cells up, 42 down).
            const int64_t looseReach = Q + (int64_t)Q * maxScore / std::min(open, ext) + 1;
            const int64_t looseRounded = (looseReach + 127) / 128 * 128;
            const bool cut = looseRounded <= 2048 && db->maxLen > segmentStride((int)looseRounded) + looseRounded;
            if (cut && rounded <= 2048 && db->maxLen > segmentStride((int)rounded) + rounded) p.overlap = (int)rounded;
        }
        // HW (the whole query, free ends in the target) can be cut the same way. Its optimum is at least
        // -(open + (Q - 1) ext) (the query gapped against nothing) and at most Q max(S) minus what its
        // gap columns in the target cost, so it has at most (Q max(S) + open + (Q - 1) ext) / min(open, ext)
        // of them and spans Q + that many columns; a window's penalised left border stands for real
        // alignments (the query's head gapped from the free top border), so no window exceeds the whole
        // target and the one that holds the optimal alignment reaches it. NW spans the whole target by
        // definition; OV's last-column candidates only exist in a target's last window: both stay whole.
        p.keyBias = 0;
        if (mode == OPAL_MODE_HW && std::min(open, ext) > 0 && Q < 4096 && db->maxLen < (1 << 24) &&
            !tuned(Tune::NO_SEGMENTS)) {
            const int64_t gaps = (pairsBest + open + ((int64_t)Q - 1) * ext) / std::min(open, ext);
            const int64_t rounded = (Q + gaps + 1 + 127) / 128 * 128;
            const int64_t lowest = 2 * (int64_t)open + ((int64_t)Q + rounded + 8) * ext + (int64_t)Q * std::max(0, -minScore);
            const int64_t looseGaps = ((int64_t)Q * std::max(maxScore, 0) + open + ((int64_t)Q - 1) * ext) / std::min(open, ext);
            const int64_t looseRounded = (Q + looseGaps + 1 + 127) / 128 * 128;
            const bool cut = looseRounded <= 2048 && db->maxLen > segmentStride((int)looseRounded) + looseRounded;
            if (cut && rounded <= 2048 && db->maxLen > segmentStride((int)rounded) + rounded && lowest < (1 << 21)) {
                p.overlap = (int)rounded;
                p.keyBias = 1 << 22;   // scores above -2^22 in the key's 24-bit score field
            }
        }
        // Window stride. The overlap is what correctness needs; the stride only trades the length of a window
        // (a group of long targets is a chain of stride + overlap columns) against the work done twice (every
        // window repeats `overlap` columns: at the shortest stride, 0.6 overlap, a long target costs 2.7 times
        // its cells). When long targets are the bulk of the database rather than its tail - a tenth of 2M
        // targets thirty times as long as the rest: 5.3 TCUPS for Smith-Waterman at Q = 53 where NW, which
        // cannot cut them, ran at 9.6 - a window may be as long as 1.5 balanced shares of a wavefront slot.
        p.stride = p.overlap > 0 ? segmentStride(p.overlap) : 0;
        if (p.overlap > 0) {
            const double share = db->count > 0 ? (double)n / (double)db->count : 1.0;
            const double balancedColumns = (double)db->total * share / ((double)kGroupTargets * 12.0 * db->computeUnits);
            const int64_t want = (int64_t)(1.5 * balancedColumns) - p.overlap;
            if (want > p.stride) p.stride = (int)std::min<int64_t>((want + 255) / 256 * 256, 8192);
            // (MIOPAL_TEST_WINDOW_STRIDE: the stride of a search that is cut anyway, for the tests of the strides
            // that only databases of 1e8 .. 2e9 residues reach: a multiple of 256 between the shortest stride of
            // this overlap and 8192, anything else is ignored; it never turns windows on or off)
            if (const char* ts = tuned(Tune::TEST_WINDOW_STRIDE)) {
                char* rest = nullptr;
                const long v = strtol(ts, &rest, 10);
                if (rest != ts && *rest == 0 && v % 256 == 0 && v >= segmentStride(p.overlap) && v <= 8192) p.stride = (int)v;
            }
        }
    }

    // step 3: the strip plan - the general kernel's strips, then either pair-table strips kernel where it pays
    void planGeneralStrips(const View* view, ScorePlan& p) const {
        // Strips and wavefronts per workgroup for queries of more than 64 rows. A workgroup of W
        // wavefronts pipelines W strips of one group; a round with fewer strips than W leaves
        // wavefronts (and their registers and LDS) idle, so the number of strips is a multiple
        // of W, at the price of shorter strips (each strip pays ~6 rows' worth of per-column
        // overhead). Measured on 500k x 300 (tools history): Q=300 as 5 strips / 4 wavefronts
        // 10.1 ms, as 8 / 4 6.6 ms; Q=150 as 3 / 2 4.7 ms, as 4 / 4 3.3 ms. W = 4 is the cheapest
        // pipeline per cell, W = 8 pays off when there are too few groups to fill the chip
        // (Q=2000 vs 100k x 2000: 782 groups), W = 1 (strips in turn through HBM) only with
        // thousands of groups.
        p.nStrips = std::max(1, (Q + kMaxStripRows - 1) / kMaxStripRows);
        p.waves = p.nStrips >= 8 ? 8 : p.nStrips >= 4 ? 4 : p.nStrips >= 2 ? 2 : 1;
        if (Q > kMaxStripRows) {
            const double need = 24.0 * db->computeUnits;  // wavefronts that fill the chip
            const double groups = std::max(1, view->nGroups);
            double bestCost = 0;
            for (int w : {4, 8, 2, 1}) {
                const int strips = w * ((Q + kMaxStripRows * w - 1) / (kMaxStripRows * w));
                const int rows = ((Q + strips - 1) / strips + 7) / 8 * 8;
                // (strips are whole multiples of 8 rows; the last one must still hold row Q - 1)
                if ((strips - 1) * rows >= Q) continue;
                const double pipeline = w == 4 ? 1.0 : w == 8 ? 1.12 : w == 2 ? 1.06 : 1.08;
                double cost = (double)strips * (rows + 6) * pipeline;
                const double parallel = groups * w;
                if (parallel < need) cost *= need / parallel;
                if (bestCost == 0 || cost < bestCost) {
                    bestCost = cost;
                    p.nStrips = strips;
                    p.waves = w;
                }
            }
        }
        if (const char* o = tuned(Tune::STRIPS)) {  // experiments: "<strips>,<wavefronts>"
            int a = 0, b = 0;
            const int least = std::max(1, (Q + kMaxStripRows - 1) / kMaxStripRows);
            if (sscanf(o, "%d,%d", &a, &b) == 2 && a >= least && (b == 1 || b == 2 || b == 4 || b == 8) &&
                (a - 1) * (((Q + a - 1) / a + 7) / 8 * 8) < Q) {
                p.nStrips = a;
                p.waves = b;
            }
        }
    }

    // (sets twoPassEnds where MIOPAL_TWO_PASS_ENDS asks for two sweeps)
    void planSwPairStrips(const View* view, bool useHalf, ScorePlan& p) {
        // Smith-Waterman scores of more rows than one pair table holds: the pair-table kernel strip by
        // strip (interseq_pair_strips_kernel: units of (batch of 12 groups, strip), boundary rows
        // through HBM), when the scores and gap costs fit the biased halves' guard band. Strips of at
        // most 52 rows (the kernel's register budget), all of the same even height.
        p.stripRows = 0;
        {
            const char* noPair = tuned(Tune::NO_PAIR_TABLE);
            // (with end locations every value is scaled by 2^bits: the row inside a strip of 32 .. 48 rows)
            const bool wantEnds = searchType != OPAL_SEARCH_SCORE;
            // (two sweeps: unscaled values like a score search, strips of at most 40 rows; MIOPAL_TWO_PASS_ENDS=1
            // asks for them whatever the scores - tests)
            if (wantEnds && mode == OPAL_MODE_SW && tuned(Tune::TWO_PASS_ENDS)) twoPassEnds = true;
            const bool rowKeyEnds = wantEnds && !twoPassEnds;
            auto band = [&](int rowsP) { return biasedBandFits(model(), rowKeyBits(rowsP, rowKeyEnds), rowKeyEnds); };
            const bool oneStrip = oneStripFits(Q, A + 1, interseqPairFits);
            const int maxRows = tallestStrip(!wantEnds ? kPairStripsMaxRows : twoPassEnds ? kPairStripsMaxRowsKnown : kPairStripsMaxRowsLoc,
                                             A + 1, interseqPairFits);
            if (mode == OPAL_MODE_SW && Q < (1 << 20) && useHalf && !oneStrip && maxRows >= 32 &&
                !pairStripsRefused && !(wantEnds && stripsEndsDeclined && !twoPassEnds) && !(noPair && noPair[0] == '1') && !tuned(Tune::NO_BIASED) &&
                !tuned(Tune::NO_PAIR_STRIPS) && !tuned(Tune::STRIPS)) {
                const int ns = std::max(2, (Q + maxRows - 1) / maxRows);
                const int rowsP = ((Q + ns - 1) / ns + 1) / 2 * 2;
                // Worth it when there are units enough to keep every CU on one strip for a while, or strips
                // enough that the general kernel pays many rounds: measured on 2k .. 1M x 300, the strips
                // kernel wins from about 2.5 units per CU on (+9 .. +24 %) and from 20 strips on at any
                // size, and loses below (50k x 300 at Q = 300, 0.8 units per CU: 1.17 against 0.85 ms)
                const int64_t units = (int64_t)((view->nGroups + 11) / 12) * ns;
                // A wavefront sweeps a strip of ~50 rows at about a microsecond per column, whoever shares
                // its CU (a batch is twelve neighbours of the length-sorted view: all long, or all short),
                // where the general kernel pipelines a group's strips over the wavefronts of a workgroup
                // at a third of that. The longest group must therefore be short against the launch, or
                // it IS the launch: log-normal lengths, 500k targets at Q = 150, windows of 3072 columns:
                // 5.3 ms against the general kernel's 2.9 ms.
                const int64_t balanced = view->totalChunks * ns / ((int64_t)db->computeUnits * 12);
                // (Round 3, with the wavefronts of a SIMD paced: measured again over 20k .. 2M targets, uniform,
                // log-normal and bimodal lengths - tools/quick_routing_ab.py, profiles/r03_routing_ab.txt. The
                // strips kernel wins from 1.5 units per CU on; its longest group may be as long as 1.2 balanced
                // shares of a wavefront slot - the chain of that group is then about the whole launch - and with
                // 16 strips or more the general kernel's rounds cost more than any chain.)
                const bool hidden = view->nGroups > 0 && 5 * (int64_t)view->groupChunksHost[0] <= 6 * balanced;
                // (with 16 strips or more the strips kernel whatever the longest group: log-normal lengths, 20k
                // targets at Q = 2000: 3.2 against the general kernel's 1.1 TCUPS; the one shape that loses - 20k
                // targets, a tenth of them thirty times as long as the rest - loses 15 %: profiles/r03c_routing_table.txt)
                const bool enough = (ns >= 16 || (2 * units >= 3 * (int64_t)db->computeUnits && hidden)) || tuned(Tune::PAIR_STRIPS);
                if (enough && rowsP >= 32 && rowsP <= maxRows && band(rowsP) && (int64_t)(ns - 1) * rowsP < Q && ns <= 4096) {
                    p.stripRows = rowsP;
                    p.nStrips = ns;
                    p.waves = 1;   // (strips of a group in turn, each in its own unit)
                }
            }
        }
    }

    void planGlobalPairStrips(const View* view, bool useHalf, ScorePlan& p) const {
        // NW / HW / OV of more rows than one pair table holds: the same units with the one-strip global
        // kernel's cell (interseq_pair_global_strips_kernel, round 3: 3 integer adds + 3 max per cell pair
        // and no v_perm, against 5 + 1 v_perm and a barrier per chunk on the general kernel's cheapest
        // lanes). The true values around a pattern's zero are bounded by the QUERY (all of it: the strips
        // share one scale), not by the targets' lengths, so no target is redone at 32 bit; the bounds are
        // static:   below zero: 3 open + (Q + 4) ext + |min S|
        //           above: NW Q (max S + ext), HW / OV Q max S + the rebase shift.
        // A 2000-residue query under BLOSUM62 3 / 1 (BASELINE configs[3]) fits; from about 2200 (HW / OV)
        // and 2350 residues (NW) on the general kernel takes over.
        p.globalStrips = false;
        if (mode != OPAL_MODE_SW && useHalf && !globalStripsRefused && !tuned(Tune::NO_BIASED) &&
            !tuned(Tune::NO_GLOBAL_STRIPS) && !tuned(Tune::STRIPS)) {
            const char* noPair = tuned(Tune::NO_PAIR_TABLE);
            const bool oneStrip = oneStripFits(Q, A + 1, interseqPairFits);
            // (with end locations the row / column bookkeeping costs registers: shorter strips)
            const int maxRows = tallestStrip(searchType != OPAL_SEARCH_SCORE ? kPairStripsMaxRowsLoc : kPairStripsMaxRows, A + 1, interseqPairFits);
            const bool inRange = globalStripsFit(model(), Q, r.topGap != 0);
            if (!oneStrip && maxRows >= 32 && Q > 32 && inRange && !(noPair && noPair[0] == '1')) {
                // strip height: even, at most maxRows; every strip costs about four rows' worth of per-column
                // work on top of its cells (row above in, last row out, answers), and a last query row that
                // is the strip's last row is read without a select (Q = 2000: 40 strips of 50 rows)
                int bestRows = 0, bestNs = 0;
                int64_t bestCost = 0;
                for (int rowsP = maxRows; rowsP >= 32; rowsP -= 2) {
                    const int ns = (Q + rowsP - 1) / rowsP;
                    if (ns < 2 || (int64_t)(ns - 1) * rowsP >= Q) continue;
                    const int64_t cost = (int64_t)ns * (rowsP + 4) + ((int64_t)ns * rowsP - Q > 1 ? rowsP / 8 : 0);
                    if (bestRows == 0 || cost < bestCost) {
                        bestRows = rowsP;
                        bestNs = ns;
                        bestCost = cost;
                    }
                }
                if (bestRows > 0 && bestNs <= 4096) {
                    const int64_t units = (int64_t)((view->nGroups + 11) / 12) * bestNs;
                    const int64_t balanced = view->totalChunks * bestNs / ((int64_t)db->computeUnits * 12);
                    // (the general kernel's lanes are a third slower for these modes than this kernel's: a longest
                    // group of up to 1.5 balanced shares still pays, and so does one unit per CU)
                    const bool hidden = view->nGroups > 0 && 2 * (int64_t)view->groupChunksHost[0] <= 3 * balanced;
                    // (the same two limits as the Smith-Waterman strips kernel: units enough to keep every
                    // CU on one strip for a while, the longest group short against the launch)
                    const bool enough = (bestNs >= 16 || (units >= (int64_t)db->computeUnits && hidden)) || tuned(Tune::PAIR_STRIPS);
                    if (enough) {
                        p.stripRows = bestRows;
                        p.nStrips = bestNs;
                        p.waves = 1;
                        p.globalStrips = true;
                    }
                }
            }
        }
    }

    // step 4: the side cut - the ladder of cuts and its estimate; what leaves is queued in sideJobs
    // (keeps the cut for a pass that starts over - cutView, cutFirstGroup -, sets balancedChunks, reports in g_lastRouting)
    void planSideCut(const View* view, ScorePlan& p, std::vector<PairJob>& sideJobs) {
        // A group keeps its wavefronts busy for (columns of its longest target) x (rounds of strips).
        // Groups far above the balanced share of a workgroup slot would stretch the kernel to
        // their own length (one lane per target cannot split a target), so the leading
        // (longest) groups are skipped and their targets go to the intra-sequence kernel,
        // which spreads each pair over 64 lanes.
        p.firstGroup = 0;
        if (view->nGroups > 0) {
            const int64_t total = view->totalChunks;   // (= the sum of the groups' chunks)
            // (the strips kernel: 12 wavefronts per CU, a group's strips side by side in different ones)
            const int64_t slots = p.stripRows ? std::max<int64_t>(1, (int64_t)db->computeUnits * 12 / p.nStrips)
                                            : (int64_t)db->computeUnits * std::max(1, 12 / p.waves);
            // Which leading groups leave the packed launch for the wavefront-per-pair kernel on the side stream.
            // Round 3 cut at 2.5 balanced shares of a wavefront slot and compared that one cut with keeping
            // everything. Round 4: ONE estimate over a ladder of cuts (the multiples below, and "none"), the
            // cheapest wins: log-normal 500k at Q = 53, NW / OV, measured 1.56 ms at 2.5 shares (6528 targets on
            // the side), 1.37 at 3.5 (1408), 1.69 at 5 (256), 4.3 with everything packed
            // (profiles/r04_skewed_skip_shares.txt). The packed side of a cut: the balanced share of what stays,
            // or the chain of the longest group that stays - a wavefront sweeps a 4-column chunk of ~54 rows in
            // about 7 us beside two others on its SIMD and 2.5 times faster alone, which is how the long groups at
            // the head of the length-sorted hand-out end, the short ones long done. The side of a cut: the
            // int32 kernel fills about 1e12 cells a second with the chip to itself, and its longest pair is a chain
            // of (L + 128 per strip) anti-diagonal steps of 0.15 us. Both launches share the chip: their work adds
            // up, their chains run side by side.
            const int rowsNow = p.stripRows ? p.stripRows : std::min(Q, kMaxStripRows);
            const double rounds = p.stripRows ? 1.0 : (double)((p.nStrips + p.waves - 1) / p.waves);
            // (the general kernel of several strips: a workgroup pipelines a group's strips with a barrier
            // per chunk step, about 7.5 us per step and round whoever else is on the CU - no faster alone)
            const bool pipelined = !p.stripRows && p.nStrips > 1;
            const double tau = pipelined ? 7.5e-6 * rounds : 7e-6 * rowsNow / 54.0;
            // (... but the long groups at the head of the hand-out still end with the CU to themselves: log-normal
            // 500k at Q = 150 with nothing on the side, 5.2 ms for a longest group of 2000 chunks)
            // (not on the strips kernels: the twelve wavefronts of a unit are neighbours of the length-sorted view - all
            // long - and share their CU to the end; bimodal 20k at Q = 1000, `end`: 16 ms packed where the estimate
            // with the factor said 4)
            const double alone = p.stripRows ? 1.0 : 2.5;
            // (end locations in two sweeps of the strips kernel: the packed side twice)
            // (... known after the probe of the longest groups; before it, expected where the probe is made at all: scores of
            // long queries against long targets leave the row keys' 384, the cut is kept across the restart)
            const double sweeps = (p.stripRows && mode == OPAL_MODE_SW && searchType != OPAL_SEARCH_SCORE &&
                                   (twoPassEnds || std::min(Q, view->maxPackedLen) >= 512)) ? 2.0 : 1.0;
            // (a slot = the wavefronts that sweep one group: all its strips side by side on the strips kernels; round 3
            // multiplied the balanced share by the number of strips once more - the same factor on both sides of its one
            // comparison, but twenty times too much of a packed launch against the side kernel at Q = 1000)
            const double perSlot = 1.0 / (double)std::max<int64_t>(slots, 1);
            const int64_t balancedNow = total / std::max<int64_t>(slots, 1);
            const int64_t floorLimit = p.overlap > 0 ? (p.stride + p.overlap + 3) / 4 : 0;   // windows are as short as long targets get
            const int qStrips = (Q + kLanes - 1) / kLanes;
            auto cutAt = [&](double shares) {
                int64_t limit = std::max<int64_t>((int64_t)(shares * (double)balancedNow), 128);
                limit = std::max(limit, floorLimit);
                int g = 0;
                while (g < view->nGroups && view->groupChunksHost[g] > limit) ++g;
                return g;
            };
            auto estimate = [&](int fg) {
                int64_t skippedChunks = 0;
                for (int g = 0; g < fg; ++g) skippedChunks += view->groupChunksHost[g];
                const double nextLongest = fg < view->nGroups ? view->groupChunksHost[fg] : 0;
                const double packedWork = sweeps * (double)(total - skippedChunks) * perSlot * tau;
                const double packedChain = sweeps * nextLongest * tau / alone;
                if (fg == 0) return std::max(packedWork, packedChain);
                // (both kernels share the chip: their work adds up, their longest chains do not)
                double sideWork, sideChain;
                if (Q <= kLanes) {
                    // pairs of one strip: two columns a step (intraseq_wide_kernel), about 1.6e10 wavefront steps a
                    // second over the chip, 0.1 us a step of a pair's own chain (15 872 log-normal pairs at Q = 53:
                    // 0.55 ms - a side cell costs six times a packed one)
                    sideWork = ((double)skippedChunks * 2.0 * kGroupTargets + (double)fg * kGroupTargets * Q) / 1.6e10;
                    sideChain = ((double)view->groupChunksHost[0] * 2.0 + Q) * 0.1e-6;
                } else {
                    sideWork = (double)skippedChunks * 4.0 * kGroupTargets * (double)Q / 1.0e12;
                    sideChain = ((double)view->groupChunksHost[0] * 4.0 + 128.0 * qStrips) * 0.15e-6;   // (a long pair's strips run side by side)
                }
                return std::max({packedChain, sideChain, packedWork + sideWork});
            };
            if (cutView == view) {
                p.firstGroup = cutFirstGroup;
            } else {
                double bestCost = estimate(0);
                p.firstGroup = 0;
                int lastTried = 0;
                for (double shares : {8.0, 6.0, 5.0, 4.0, 3.5, 3.0, 2.5, 2.0, 1.5}) {
                    const int fg = cutAt(shares);
                    if (fg == lastTried) continue;
                    lastTried = fg;
                    const double cost = estimate(fg);
                    if (cost < 0.97 * bestCost) {   // (a cut has to pay for itself: fewer targets on the side at equal cost)
                        bestCost = cost;
                        p.firstGroup = fg;
                    }
                }
            }
            cutView = view;
            cutFirstGroup = p.firstGroup;
            const int skipped = std::min(p.firstGroup * kGroupTargets, view->nPacked);
            for (int k = 0; k < skipped; ++k) queueWhole(sideJobs, view->ids[k]);
            balancedChunks = total / std::max<int64_t>(slots, 1);
        }
        p.firstPos = std::min(p.firstGroup * kGroupTargets, view->nPacked);
        g_lastRouting[0] = (int64_t)sideJobs.size();
        g_lastRouting[2] = view->nGroups - p.firstGroup;
    }

    // step 5: the lane arithmetic - flavour, limits, caps, which targets go to the int32 kernel (jobs: after the
    // packed launch; sideJobs: beside it)
    void planLanes(const View* view, bool useHalf, ScorePlan& p, std::vector<PairJob>& jobs, std::vector<PairJob>& sideJobs) const {
        p.pairStrips = p.stripRows > 0;
        p.rows = p.pairStrips ? p.stripRows : (((Q + p.nStrips - 1) / p.nStrips) + 7) / 8 * 8;
        p.qPad = p.nStrips * p.rows;
        p.nSym = A + 1;
        // Lane arithmetic. Smith-Waterman: packed half floats are exact for integers
        // below 2048 and cost fewer instructions per cell (interseq_impl.h); saturating
        // int16 is the second rung, the int32 intra-sequence kernel the last. The other
        // modes use signed int16 lanes; whether a target fits is known from its length:
        //   every true H, E, F >= -(3*open + (Q + L)*ext)   and   H <= min(Q, L)*maxScore
        p.sw = mode == OPAL_MODE_SW;
        p.locate = searchType != OPAL_SEARCH_SCORE;  // end locations wanted
        p.packedSkip = p.firstPos;   // first view position whose packed result is scattered
        // Smith-Waterman with several strips and no windows (long queries): a few targets far longer
        // than the rest of the first group set that group's - on the strips kernel the launch's - length
        // (cfg4 with its tail: 4000 .. 8000 residues among 2000-residue targets, 56 instead of 47 ms).
        // With a pair's strips side by side the int32 kernel takes them in a few milliseconds beside the
        // packed launch: up to 64 leading targets more than a quarter longer than the longest of the next
        // group go there, and the first group stops at the longest target that stays.
        if ((p.sw || p.globalStrips) && p.overlap == 0 && Q > kLanes && view->nPacked - p.firstPos > 2 * kGroupTargets &&
            !tuned(Tune::NO_SIDE_STREAM)) {
            const int ref = dbLen(db, view->ids[p.firstPos + kGroupTargets]);
            int k = 0;
            while (k < 64 && (int64_t)dbLen(db, view->ids[p.firstPos + k]) * 4 > (int64_t)ref * 5 + 1024) ++k;
            if (k > 0) {
                for (int x = 0; x < k; ++x) sideJobs.push_back(forwardJob(view->ids[p.firstPos + x], rules));
                g_lastRouting[0] = (int64_t)sideJobs.size();
                p.packedSkip = p.firstPos + k;
                p.capGroups = 1;
                p.capChunks = std::max(1, (dbLen(db, view->ids[p.firstPos + k]) + 3) / 4);
            }
        }
        // one strip + Smith-Waterman scores: the pair-indexed LDS profile saves the v_perm per cell
        const char* noPair = tuned(Tune::NO_PAIR_TABLE);
        // first rung of the pair-table kernel: biased integer halves (exact below 25600,
        // interseq_impl.h) when the scores and gap costs leave its guard band alone (score_ranges.h).
        // With end locations every value is scaled by 2^bits (row keys in the low bits).
        // (Smith-Waterman: the query's own rows, the biased kernel exists for odd counts too; the NW / HW / OV
        // kernel sweeps rows in pairs)
        p.pairRows = p.sw ? std::max(1, Q) : pairTableRows(Q);
        // (row keys in the low bits of every value - unless the end locations come from a second sweep)
        p.twoPass = p.pairStrips && p.sw && p.locate && twoPassEnds;
        p.rowKeys = p.locate && !p.twoPass;
        const int bits = rowKeyBits(p.pairStrips ? p.stripRows : p.pairRows, p.rowKeys);
        const bool biasedFits = p.nStrips == 1 && useHalf && !tuned(Tune::NO_BIASED) && biasedBandFits(model(), bits, p.rowKeys);
        p.biasedLimit = biasedLimit(model(), bits, p.rowKeys);
        p.usePair = p.sw && p.nStrips == 1 && !(noPair && noPair[0] == '1') &&
                    interseqPairFits(biasedFits ? p.pairRows : p.rows, p.nSym) && (!p.locate || biasedFits);
        p.biased = p.usePair && biasedFits;
        // Smith-Waterman scores in the general kernel (several strips, or a pair table that does not
        // fit LDS): column-shifted unsigned patterns (ArithSwU16) when the longest packed target
        // leaves a range worth having.
        if (p.sw && !p.locate && !p.usePair && !p.pairStrips && useHalf && !tuned(Tune::NO_SW_SHIFT)) {
            const SwShiftPlan shift = swShiftPlan(model(), view->maxPackedLen);
            p.swBias = shift.bias;   // (the kernel arguments carry it whether the flavour is used or not)
            p.swShifted = shift.usable;
            p.swLimit = shift.limit;
        }
        // only matrices whose best possible score stays finite take the half-float rung
        p.halfFloat = p.sw && useHalf && !p.biased && !p.swShifted && !p.pairStrips && halfFloatFits(model(), Q, db->maxLen);
        p.flavour = p.sw ? (p.swShifted ? kSwShifted : p.halfFloat ? kSwHalf : kSwInt16) : kSignedInt16;
        p.profileShift = p.swShifted ? ext + p.swBias : 0;
        // One-strip NW / HW / OV: the pair-table kernel on biased integer halves (interseq_impl.h), its static
        // bounds in score_ranges.h; the multi-strip kernel shares its zero.
        p.globalZero = globalZeroPattern(model(), Q, false);
        p.globalPair = !p.sw && p.nStrips == 1 && !globalPairRefused && !(noPair && noPair[0] == '1') && !tuned(Tune::NO_BIASED) &&
                       interseqPairFits(p.pairRows, p.nSym) && globalOneStripFits(model(), Q, r.topGap != 0, false);
        if (p.globalPair || p.globalStrips) {
            // only empty targets (closed forms of the border) are left to the int32 kernel
            for (int e = view->nPacked - 1; e >= p.firstPos && dbLen(db, view->ids[e]) == 0; --e)
                jobs.push_back(forwardJob(view->ids[e], rules));
        } else if (!p.sw) {
            const ScoreModel m = model();
            auto plain = [&](int64_t L) { return fitsPlain(m, Q, L); };
            auto diag = [&](int64_t L) { return fitsDiag(m, Q, L); };
            auto unsignedDiag = [&](int64_t L) { return fitsUnsigned(m, Q, L); };
            // longest packed target that the plain flavour can take (view order: longest first)
            int firstFit = p.firstPos;
            while (firstFit < view->nPacked && !plain(dbLen(db, view->ids[firstFit]))) ++firstFit;
            // The shifted flavours need more head-room, i.e. shorter targets. A few targets too long
            // for them would put the WHOLE view on the plain int16 lanes (8 operations per cell pair
            // instead of 5: cfg4 with the reference's 1000 .. 35000 tail, NW: 78 ms instead of 48); the
            // int32 kernel takes a long pair in a few milliseconds now (one wavefront per strip), so up
            // to 1024 of the longest targets are handed to it when that buys the view a cheaper flavour.
            auto firstThat = [&](int from, auto&& fits) {
                int k = from;
                while (k < view->nPacked && k - from <= 1024 && !fits(dbLen(db, view->ids[k]))) ++k;
                return (k < view->nPacked && k - from <= 1024 && dbLen(db, view->ids[k]) > 0) ? k : -1;
            };
            const int firstPlain = firstFit;
            const int firstDiag = tuned(Tune::NO_DIAG_SHIFT) ? -1 : firstThat(firstFit, diag);
            if (firstDiag >= 0) {
                firstFit = firstDiag;
                p.flavour = kSignedInt16Diag;
                p.profileShift = 2 * ext;
                // The same shift on unsigned patterns compared as half floats (ArithU16Diag), where the model allows it
                if (unsignedDiagUsable(m)) {
                    const int firstU = firstThat(firstFit, unsignedDiag);
                    if (firstU >= 0) {
                        firstFit = firstU;
                        p.flavour = kUnsignedDiag;
                        p.profileShift = 2 * ext + (open - ext);
                    }
                }
                // Windows: every entry stays in the launch, and a lane sweeps its group's columns to the end. Beyond
                // the signed shifted flavour's range the shift (i + j) ext of a column no longer fits 16 bits, and HW's
                // last-row maximum, which that flavour takes over every swept column, would read it: plain lanes then
                // (the unsigned flavour masks the columns beyond its own target)
                if (p.flavour == kSignedInt16Diag && p.overlap > 0 && !diag(view->maxPackedLen)) {
                    firstFit = firstPlain;
                    p.flavour = kSignedInt16;
                    p.profileShift = 0;
                }
            }
            // The targets that do not fit form a prefix of the view: they go to the int32 kernel BESIDE
            // the packed launch, and the scatter starts behind them (their lanes of the packed kernel hold
            // nothing). Empty targets (closed forms of the border) form a suffix, redone after the scatter.
            // (windows of a segmented view are merged by key afterwards: there the whole targets are redone after)
            if (p.overlap > 0) {
                for (int k = p.firstPos; k < firstFit; ++k) queueWhole(jobs, view->ids[k]);
            } else {
                for (int k = p.firstPos; k < firstFit; ++k) sideJobs.push_back(forwardJob(view->ids[k], rules));
                p.packedSkip = firstFit;
                g_lastRouting[0] = (int64_t)sideJobs.size();
                // ... and the groups they sit in sweep no further than the longest target that stays (cfg4
                // with its tail: five targets of 4000 .. 8000 residues kept the first group, and with it
                // the launch, at 8000 columns: 57 instead of 48 ms)
                if (firstFit > p.firstPos && firstFit < view->nPacked) {
                    p.capGroups = (firstFit - p.firstPos + kGroupTargets - 1) / kGroupTargets;
                    p.capChunks = std::max(1, (dbLen(db, view->ids[firstFit]) + 3) / 4);
                }
            }
            for (int e = view->nPacked - 1; e >= firstFit && dbLen(db, view->ids[e]) == 0; --e)
                jobs.push_back(forwardJob(view->ids[e], rules));
        }
        // lanes can only leave the exact range when min(Q, L) * maxScore reaches the limit
        // (also bounded by the query itself: every residue is aligned at most once, at best with
        // its most favourable partner - 280 for the 53-aa README query under BLOSUM62, where
        // Q * max(S) says 583)
        const int64_t reach = std::min<int64_t>((int64_t)std::min(Q, view->maxPackedLen) * std::max(maxScore, 0), p.queryBest);
        const int64_t limit = (p.biased || p.pairStrips) ? p.biasedLimit : p.swShifted ? p.swLimit : p.halfFloat ? 2048 : 32767;
        // (the multi-strip NW / HW / OV kernel flags nothing for its range; the count brings back the
        // lanes of units that gave up on the strip above - never seen outside the fault-injection test)
        // (the strips kernels: always - the count also brings back the lanes of a unit that gave up on
        // the strip above it; searches of several strips take milliseconds, the 4-byte download is free)
        p.mayOverflow = p.sw ? (reach >= limit || p.pairStrips) : p.globalStrips;
        // How many flagged lanes are redone one by one before the whole view takes the next rung: the int32
        // kernel fills about 1e12 cells a second, the next rung 5e12 .. 8e12 over the WHOLE view - an eighth
        // of the view's targets costs the same either way (round 3; it was 2048 whatever the size: 0.3 % of
        // 1M x 300 beyond the row keys' 384 at Q = 1000 sent the other 99.7 % through a second launch)
        p.directLimit = std::max<int64_t>(kMaxDirectRecompute, (view->nPacked - p.packedSkip) / 8);
        // (random pairs only get there in the linear regime of the scoring system, and then score
        // about half a unit per aligned residue: nothing to probe for under ~500 residues)
        p.probeEnds = p.pairStrips && p.sw && p.rowKeys && p.mayOverflow && std::min(Q, view->maxPackedLen) >= 512 && !tuned(Tune::PAIR_STRIPS);
    }

    // step 6: the query profile of the packed kernels
    std::vector<int16_t> buildProfile(const ScorePlan& p) const {
        // query profile: profile[t][i] = S[q_i][t]; padding symbol and padding rows can
        // never win a max: -32768 (int16) or -inf (half)
        auto enc = [&](int v) -> int16_t {
            if (!p.halfFloat) return (int16_t)v;
            const _Float16 h = (_Float16)(float)v;
            int16_t bits;
            memcpy(&bits, &h, sizeof bits);
            return bits;
        };
        // (the unsigned shifted flavour: padding scores open - ext after the shift, see ArithU16Diag)
        const int16_t padValue = (p.biased || p.globalPair || p.pairStrips) ? (int16_t)kBiasedPad
                                 : p.swShifted ? (int16_t)0   // s + ext + K = 0: a true score of -(ext + K) <= 0
                                 : p.flavour == kUnsignedDiag ? (int16_t)(open - ext)
                                 : p.halfFloat ? (int16_t)0xFC00 : (int16_t)-32768;
        std::vector<int16_t> prof((size_t)p.nSym * p.qPad, padValue);
        for (int t = 0; t < A; ++t)
            for (int i = 0; i < Q; ++i) prof[(size_t)t * p.qPad + i] = enc(at(i, t) + p.profileShift);
        return prof;
    }

    // step 7: the side jobs go to the side stream (*forked: the pass has something to join)
    int forkSideJobs(const ScorePlan& p, std::vector<PairJob>& sideJobs, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ,
                     bool* forked, PhaseTimer& spt) {
        // targets kept out of the packed view (too long for one lane each) are computed by the
        // int32 kernel on a side stream BESIDE the packed kernel; packed targets that need
        // the int32 kernel are redone after it, because both write the same result slots
        if (!sideDone.empty()) {
            sideJobs.erase(std::remove_if(sideJobs.begin(), sideJobs.end(), [&](const PairJob& j) {
                               return std::binary_search(sideDone.begin(), sideDone.end(), j.out);
                           }), sideJobs.end());
        }
        // The side kernel is handed to its stream BEFORE the packed launch: its wavefronts are dispatched
        // first, over the whole chip, and the persistent packed workgroups (one per CU, every register of
        // it) start on a CU when its side wavefronts are done. (Handed over after the packed launch the
        // side kernel only finds the CUs the launch left out: cfg4 with its tail, 8 CUs: 54 against 44 ms.)
        // Beside a strips kernel the side units come in workgroups of 16 wavefronts,
        // so that they hold few CUs (launchIntraseqStrips), and the packed launch takes EVERY CU: the
        // workgroups that start late simply take fewer units.
        if (!sideJobs.empty() && !tuned(Tune::NO_SIDE_STREAM)) {
            RC_TRY(ws->ensureAux());
            RC_TRY(ensurePairInputs());
            HIP_TRY(hipEventRecord(ws->evFork, stream));
            HIP_TRY(hipStreamWaitEvent(ws->aux, ws->evFork, 0));
            *forked = true;
            besidePersistent = p.pairStrips;
            RC_TRY(runPairs(sideJobs, false, d_score, d_endI, d_endJ, nullptr, ws->aux, kAuxJobs - kJobs));
            HIP_TRY(hipEventRecord(ws->evJoin, ws->aux));
            for (const PairJob& j : sideJobs) sideDone.push_back(j.out);
            std::sort(sideDone.begin(), sideDone.end());
            sideJobs.clear();
            sideForked = true;   // (a score pass that starts over still joins what is on the side stream)
            spt.mark("    side jobs enqueued");
        }
        return 0;
    }

    static bool oneStripPair(const ScorePlan& p) { return !p.pairStrips && (p.usePair || p.globalPair); }

    // step 8: the packed kernels' arguments, and the unit / boundary buffers of the launch that was planned
    int prepareLaunch(const View* view, const ScorePlan& p, const std::vector<int16_t>& prof, PassBuffers& b, InterseqArgs& ia) {
        void *pp, *vs;
        RC_TRY(ws->get(kProfile, prof.size() * sizeof(int16_t), &pp));
        RC_TRY(ws->get(kViewScore, (size_t)view->nGroups * kGroupTargets * sizeof(int32_t), &vs));
        RC_TRY(ws->get(kViewOvf, (size_t)view->nGroups * kGroupTargets, &b.vo));
        RC_TRY(ws->get(kCounter, sizeof(int32_t), &b.ct));
        // (the one-strip pair-table launch sends the profile itself, or has its kernel read the staged copy: planOneStripPair)
        if (!oneStripPair(p)) RC_TRY(ws->stageUpload(pp, prof.data(), prof.size() * sizeof(prof[0]), stream));
        if (p.mayOverflow) HIP_TRY(hipMemsetAsync(b.ct, 0, sizeof(int32_t), stream));
        ia.pack = view->d_pack;
        ia.groupOff = view->d_groupOff;
        ia.groupChunks = view->d_groupChunks;
        ia.nGroups = view->nGroups - p.firstGroup;
        ia.groupBase = p.firstGroup;
        ia.profile = (const int16_t*)pp;
        ia.nSymbols = p.nSym;
        ia.qPad = p.qPad;
        ia.nStrips = p.nStrips;
        ia.qLen = Q;
        ia.gapOpen = std::min(open, 32767);
        ia.gapExt = std::min(ext, 32767);
        ia.topGap = r.topGap;
        ia.leftGap = r.leftGap;
        ia.region = r.region;
        ia.lens = view->d_lens;
        ia.score = (int32_t*)vs;
        if (p.locate) {
            void *vi, *vj;
            RC_TRY(ws->get(kViewEndI, (size_t)view->nGroups * kGroupTargets * sizeof(int32_t), &vi));
            RC_TRY(ws->get(kViewEndJ, (size_t)view->nGroups * kGroupTargets * sizeof(int32_t), &vj));
            ia.endI = (int32_t*)vi;
            ia.endJ = (int32_t*)vj;
        }
        ia.overflow = (p.sw || p.globalStrips) ? (uint8_t*)b.vo : nullptr;
        ia.stripSpinCap = faultSpinCap;
        ia.faultUnit1 = faultKind == 1 ? faultUnit + 1 : 0;
        ia.biasedLimit = p.swShifted ? p.swLimit : p.biasedLimit;
        ia.scoreBias = p.swBias;
        ia.biasedZero = (int)p.globalZero;
        ia.boundaryOff = view->d_boundaryOff;
        ia.capGroups = p.capGroups;
        ia.capChunks = p.capChunks;
        ia.priorityChunks = (int)std::min<int64_t>(std::max<int64_t>(balancedChunks, 16), INT32_MAX);
        if ((p.nStrips + p.waves - 1) / p.waves > 1) {
            void *b0, *b1;
            const size_t bytes = (size_t)view->totalChunks * 4 * kLanes * sizeof(uint2);
            RC_TRY(ws->get(kBoundary0, bytes, &b0));
            RC_TRY(ws->get(kBoundary1, bytes, &b1));
            ia.boundary[0] = (uint2*)b0;
            ia.boundary[1] = (uint2*)b1;
        }
        // several rounds of strips per group, scores only: (group, round) units instead of one
        // workgroup per group (interseq_impl.h, "unit mode")
        // Only when the groups are few for the chip (under six workgroup-lifetimes): the rounds of
        // a group are then far apart in time and its boundary rows come back from HBM, not from
        // the caches (500k x 300 at Q = 300, 7.6 lifetimes: 6.6 ms classic, 7.0 ms in units;
        // 100k x 2000 at Q = 2000, 3.05 lifetimes: 66 ms classic, 55 ms in units).
        const int64_t unitSlots = (int64_t)db->computeUnits * std::max(1, 8 / p.waves);
        const char* um = tuned(Tune::UNITS);
        const bool wantUnits = um ? um[0] == '1' : (int64_t)(view->nGroups - p.firstGroup) < 6 * unitSlots;
        if (p.pairStrips) {
            // unit counter + chunks published per (group, strip); scores and flags start from zero
            // (a group's answer is the maximum over its strips' units)
            void* us;
            const size_t ints = (size_t)ia.nGroups * p.nStrips + 2;
            RC_TRY(ws->get(kUnitState, ints * sizeof(int), &us));
            HIP_TRY(hipMemsetAsync(us, 0, ints * sizeof(int), stream));
            if (p.mayOverflow && p.sw) {
                // more flagged lanes than are redone one by one: the launch stops, the view takes the next rung
                ia.stripAbort = (int*)us + ints - 1;
                ia.stripAbortAt = (int)std::min<int64_t>(2 * p.directLimit, INT32_MAX / 2);
                ia.stripGaveUp = (int*)b.ct;
            }
            // (the scores-only form of the NW / HW / OV kernel folds OV's candidates into the view scores,
            // and what a unit that gave up leaves behind is "minus infinity" in every mode)
            if (p.globalStrips) HIP_TRY(launchFillInt32((int32_t*)vs, view->nGroups * kGroupTargets, INT32_MIN, stream));
            else HIP_TRY(hipMemsetAsync(vs, 0, (size_t)view->nGroups * kGroupTargets * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(b.vo, 0, (size_t)view->nGroups * kGroupTargets, stream));
            ia.unitCounter = (int*)us;
            ia.unitFlags = (int*)us + 1;
            if (p.locate) {
                void* sk;
                RC_TRY(ws->get(kStripKeys, (size_t)view->nGroups * kGroupTargets * sizeof(unsigned long long), &sk));
                HIP_TRY(hipMemsetAsync(sk, 0, (size_t)view->nGroups * kGroupTargets * sizeof(unsigned long long), stream));
                ia.stripKeys = (unsigned long long*)sk;
            }
        } else if ((p.nStrips + p.waves - 1) / p.waves > 1 && !p.locate && !p.usePair && !p.globalPair && wantUnits) {
            void *us, *up;
            const size_t ints = (size_t)ia.nGroups + 1;
            RC_TRY(ws->get(kUnitState, ints * sizeof(int), &us));
            RC_TRY(ws->get(kUnitPartial, (size_t)ia.nGroups * p.waves * kLanes * sizeof(uint2), &up));
            HIP_TRY(hipMemsetAsync(us, 0, ints * sizeof(int), stream));
            ia.unitCounter = (int*)us;
            ia.unitFlags = (int*)us + 1;
            ia.unitPartial = (uint2*)up;
        }
        return 0;
    }

    // step 9, the multi-strip pair-table kernels: the launch's size and flavour, ...
    struct StripsLaunch {
        int pairUnits = 0;
        PairFlavour flavour = kPairSwStrips;
        unsigned long long* timing = nullptr;
    };
    int prepareStripsLaunch(const ScorePlan& p, InterseqArgs& ia, StripsLaunch* sl) {
        int pairUnits = db->computeUnits;
        if (const int keep = reservedCus(db); keep >= 0)
            pairUnits = std::max(1, pairUnits - keep);
        // (no CUs are kept out of the launch for the side kernel, as round 2 did: the units are taken
        // dynamically, so a workgroup whose CU is busy with side wavefronts at first just starts later
        // and takes fewer)
        const PairFlavour stripsFlavour = p.globalStrips ? kPairGlobalStrips : kPairSwStrips;
        g_lastRouting[1] = 2 + (int)stripsFlavour;
        sl->pairUnits = pairUnits;
        sl->flavour = stripsFlavour;
        // few (group, strip) units: fewer groups per workgroup, so that every CU gets a unit and a
        // wavefront shares its SIMD with fewer others
        ia.batchGroups = (int)std::max<int64_t>(1, std::min<int64_t>(12, (int64_t)ia.nGroups * p.nStrips / std::max(1, pairUnits)));
        // (miopalLastLaunchShape: the width launchPairStripsR / launchPairGlobalStripsR give the launch)
        const int64_t stripUnits = (int64_t)((ia.nGroups + ia.batchGroups - 1) / ia.batchGroups) * p.nStrips;
        g_lastLaunchShape[1] = std::max<int64_t>(1, std::min<int64_t>(pairUnits, stripUnits));
        g_lastLaunchShape[2] = kPairWavesPerGroup;
        g_lastLaunchShape[3] = 0;
        // (diagnostic builds of the kernels, -DMIOPAL_STRIP_TIMING=1: their six counters, printed below)
        if (tuned(Tune::STRIP_TIMING)) {
            void* tb;
            RC_TRY(ws->get(kStripTiming, 8 * sizeof(unsigned long long), &tb));
            HIP_TRY(hipMemsetAsync(tb, 0, 8 * sizeof(unsigned long long), stream));
            ia.stripTiming = sl->timing = (unsigned long long*)tb;
        }
        return 0;
    }

    // ... the probe of the longest groups (p.probeEnds): how many of their scores are beyond the row keys' range, ...
    struct StripsProbe {
        hipError_t launch = hipSuccess;   // what the probe's launch said; nothing is counted when it was refused
        int beyond = 0, lanes = 0;        // scores at or beyond the row keys' limit, of that many
    };
    int probeStripsEnds(const ScorePlan& p, const InterseqArgs& ia, const StripsLaunch& sl, StripsProbe* seenOut) {
        // With end locations a lane is exact below 384 (768 for strips of 32 rows). Scores of
        // long queries against long targets under cheap gaps are in the thousands - every lane
        // would be redone, and a launch that gives up half-way has cost half its time. The
        // twelve longest groups (the highest scores) go through the scores-only kernel first:
        // 1536 targets, a unit's time; when half of them are beyond the range the general
        // kernel takes the search.
        InterseqArgs probe = ia;
        probe.nGroups = std::min(12, ia.nGroups);
        probe.batchGroups = 1;
        probe.overflow = nullptr;
        probe.stripKeys = nullptr;
        probe.stripAbort = nullptr;
        seenOut->launch = launchInterseqPair(probe, p.rows, kPairSwStrips, sl.pairUnits, stream, false);
        if (seenOut->launch == hipSuccess) {
            seenOut->lanes = probe.nGroups * kGroupTargets;
            std::vector<int32_t> seen((size_t)seenOut->lanes);
            RC_TRY(ws->stageDownload(seen.data(), ia.score + (size_t)p.firstGroup * kGroupTargets, seen.size() * sizeof(int32_t)));
            RC_TRY(ws->finishDownloads());
            for (int32_t v : seen) seenOut->beyond += v >= p.biasedLimit;
        }
        return 0;
    }

    // ... and the launch itself, with its second sweep where the end locations come from one (*pe: refused)
    int launchStripsSweeps(const View* view, const ScorePlan& p, const InterseqArgs& ia, const StripsLaunch& sl, hipError_t* refused) {
        hipError_t pe = hipSuccess;
        if (p.probeEnds) {
            // (the probe's units and scores are wiped: the real launch starts from zero)
            HIP_TRY(hipMemsetAsync(ia.unitCounter, 0, ((size_t)ia.nGroups * p.nStrips + 2) * sizeof(int), stream));
            HIP_TRY(hipMemsetAsync(ia.score, 0, (size_t)view->nGroups * kGroupTargets * sizeof(int32_t), stream));
        }
        pe = tuned(Tune::TEST_REFUSE_PAIR_LAUNCH) ? hipErrorInvalidValue
                                                  : launchInterseqPair(ia, p.rows, sl.flavour, sl.pairUnits, stream, p.rowKeys);
        if (pe == hipSuccess && sl.timing) {
            unsigned long long t[8] = {};
            HIP_TRY(hipMemcpyAsync(t, sl.timing, sizeof t, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            const double life = (double)std::max<unsigned long long>(t[4], 1);
            fprintf(stderr, "[miopal] strip timing (%llu wavefronts, s_memtime ticks): unit %.3f  poll %.3f  publish %.3f  sweeps %.3f "
                            "of the wavefronts' life (%.0f ticks each)\n",
                    t[5], t[0] / life, t[1] / life, t[2] / life, t[3] / life, life / (double)std::max<unsigned long long>(t[5], 1));
        }
        if (pe == hipSuccess && p.twoPass) {
            // second sweep: the first cell (column-major) that holds each target's score, as keys
            InterseqArgs second = ia;
            second.known = ia.score;
            second.overflow = nullptr;
            second.stripAbort = nullptr;
            second.faultUnit1 = 0;
            HIP_TRY(hipMemsetAsync(ia.unitCounter, 0, ((size_t)ia.nGroups * p.nStrips + 1) * sizeof(int), stream));
            pe = launchInterseqPair(second, p.rows, sl.flavour, sl.pairUnits, stream, false);
        }
        *refused = pe;
        return 0;
    }

    // step 9, the one-strip pair-table kernels, with the direct scatter and the column split
    struct OneStripLaunch {
        hipError_t launch = hipSuccess;   // what the launch said
        bool directScatter = false;       // the kernel writes database order itself
        int pairUnits = 0;                // CUs the launch may use
        PairFlavour flavour = kPairSwInt16;
    };
    // ... what the launch needs, decided and enqueued in front of the pass's first timing event: the CUs, the column split
    // with its flags and plan, where the results go, and the profile - so that the timed span is the kernel's, as it was
    // when prepareLaunch sent the profile
    int planOneStripPair(const View* view, const ScorePlan& p, const std::vector<int16_t>& prof, InterseqArgs& ia, int32_t* d_score,
                         int32_t* d_endI, int32_t* d_endJ, bool forked, bool nothingElseWrites, OneStripLaunch* done) {
        bool directScatter = false;
        // The persistent workgroups fill every CU (LDS and registers): a kernel of another
        // stream - the collective that gathers the previous search's scores - would wait for
        // them to leave. MIOPAL_RESERVE_CUS keeps a few CUs out of the launch for it.
        int pairUnits = db->computeUnits;
        if (const int keep = reservedCus(db); keep >= 0)
            pairUnits = std::max(1, pairUnits - keep);
        else if (forked)
            // The persistent workgroups hold their CU's registers for the whole launch: the
            // wavefront-per-pair kernel on the side stream only finds room as they leave, i.e. it
            // runs AFTER the packed kernel (log-normal lengths, NW at Q = 53, 6400 pairs on the side:
            // 2.07 ms; with CUs kept out of the persistent launch 1.66 ms). One CU per 256 pairs.
            pairUnits = std::max(1, pairUnits - (int)std::min<int64_t>(pairUnits / 4, std::max<int64_t>(8, (g_lastRouting[0] + 255) / 256)));
        // groups of similar length: every SIMD takes the same share of them (interseq_impl.h)
        const int longest = view->groupChunksHost[p.firstGroup];
        const bool uniform = (int64_t)view->groupChunksHost[view->nGroups - 1] * 5 >= (int64_t)longest * 4;
        {
            const int blocks = std::max(1, std::min(pairUnits, ia.nGroups));
            const char* tt = tuned(Tune::TAIL_THROTTLE);
            ia.tailThrottle = (tt ? tt[0] == '1' : uniform) ? (ia.nGroups + blocks * 4 - 1) / (blocks * 4) : 0;
        }
        const PairFlavour pf = p.globalPair ? kPairGlobalBiased : p.biased ? kPairSwBiased : p.halfFloat ? kPairSwHalf : kPairSwInt16;
        // Column split (interseq_impl.h): groups of similar length, Smith-Waterman scores of one strip on the
        // biased flavour, and at least a longest group's chunks for every resident wavefront - no group is cut
        // twice - or the launch keeps the dynamic hand-out. The plan follows the CUs the launch may use.
        // MIOPAL_COLUMN_SPLIT: 0 = off, n = forced on n workgroups, "recompute" = forced, nothing handed on.
        if (pf == kPairSwBiased && !p.locate) {
            const char* cs = tuned(Tune::COLUMN_SPLIT);
            const bool recompute = cs && !strcmp(cs, "recompute");
            const int forced = cs && !recompute ? std::max(0, atoi(cs)) : 0;
            int64_t chunks = view->totalChunks;
            for (int g = 0; g < p.firstGroup; ++g) chunks -= view->groupChunksHost[g];
            // (no empty interval, forced or not: the state of a cut is left for the NEXT wavefront)
            const int blocks = (int)std::min<int64_t>(forced > 0 ? std::min(forced, pairUnits) : std::max(1, std::min(pairUnits, ia.nGroups)),
                                                      chunks / kPairWavesPerGroup);
            const int64_t wavefronts = (int64_t)blocks * kPairWavesPerGroup;
            // (... and the launch's LDS - table, counters, the profile's copy - within the CU's: true of every table the host
            // accepts at all, miopalSelfTest(6); said here so that the launch's own refusal is never the one that decides)
            const bool ldsFits = pairSplitLdsBytes(p.pairRows, p.nSym, p.qPad) <= kCuLdsBytes;
            if (blocks >= 1 && ldsFits && (recompute || forced > 0 || (!cs && uniform && chunks / wavefronts >= longest))) {
                void *st, *fl, *pl;
                RC_TRY(ws->get(kSplitState, (size_t)(wavefronts + 1) * splitStateBytes(p.pairRows), &st));
                RC_TRY(ws->get(kSplitFlags, (size_t)(wavefronts + 1) * sizeof(int), &fl));
                RC_TRY(ws->get(kSplitPlan, (size_t)(wavefronts + 1) * sizeof(int4), &pl));
                // Nothing of this is done per launch. The flags carry the launch's epoch, counted per workspace: zeroed
                // when they are allocated (all of the allocation: a later, wider launch finds zeros too) and when the
                // counter would wrap, so that no flag left by an earlier launch - of any plan - equals a new epoch.
                // (MIOPAL_TEST_SPLIT_EPOCH: this launch's epoch, for the tests of the wrap)
                if (const char* te = tuned(Tune::TEST_SPLIT_EPOCH)) ws->splitEpoch = (uint32_t)strtoull(te, nullptr, 10) - 1u;
                if (ws->splitFlagsBorn != ws->born[kSplitFlags] || ws->splitEpoch == UINT32_MAX) {
                    HIP_TRY(hipMemsetAsync(fl, 0, ws->cap[kSplitFlags], stream));
                    ws->splitFlagsBorn = ws->born[kSplitFlags];
                    ws->splitEpoch = 0;
                }
                // ... and the plan of the intervals stays on the device for as long as view and width are the same
                if (ws->splitPlanBorn != ws->born[kSplitPlan] || ws->splitPlanView != view->serial ||
                    ws->splitPlanFirstGroup != p.firstGroup || ws->splitPlanBlocks != blocks) {
                    const std::vector<int4> plan = splitPlanOf(view->groupChunksHost.data() + p.firstGroup, ia.nGroups, (int)wavefronts);
                    RC_TRY(ws->stageUpload(pl, plan.data(), plan.size() * sizeof(int4), stream));
                    ws->splitPlanBorn = ws->born[kSplitPlan];
                    ws->splitPlanView = view->serial;
                    ws->splitPlanFirstGroup = p.firstGroup;
                    ws->splitPlanBlocks = blocks;
                }
                ia.splitMode = recompute ? 2 : 1;
                ia.splitBlocks = blocks;
                ia.splitState = (uint4*)st;
                ia.splitFlags = (int*)fl;
                ia.splitPlan = (const int4*)pl;
                ia.splitEpoch = ++ws->splitEpoch;
            }
        }
        // The profile goes into the staging buffer BEFORE the results' place is decided: should staging it (or the plan
        // above) ever drain the buffer, the generation check below sees that and the scores take the device array -
        // bindHostOutputs leaves 1 MB of room behind the host scores for these 50 KB, so it does not happen.
        const void* staged;
        RC_TRY(ws->stage(prof.data(), prof.size() * sizeof(prof[0]), &staged));
        // Headline fast path: one strip, Smith-Waterman scores, no lane can leave its range, nothing
        // else writes the results (no side jobs, no skipped groups, no windows): the kernel writes
        // database order itself - into the caller's device buffer, or for miopalSearch into the
        // pinned host buffer the results leave from (no scatter kernel, no device-to-host copy).
        // (round 3, later: with end locations too - three arrays instead of one)
        if ((p.biased || p.globalPair) && !p.mayOverflow && p.overlap == 0 && !forked && nothingElseWrites &&
            p.firstGroup == 0 && p.packedSkip == 0 && !tuned(Tune::NO_DIRECT_SCATTER)) {
            int32_t *target = d_score, *targetI = d_endI, *targetJ = d_endJ;
            if (hostScoreOut && (hostScoreIsCallers || hostScoreGeneration == ws->stagingGeneration) &&
                (!p.locate || (hostEndIOut && hostEndJOut)) && !tuned(Tune::NO_HOST_SCATTER)) {
                target = hostScoreOut;
                targetI = hostEndIOut;
                targetJ = hostEndJOut;
                wroteHost = true;
            }
            ia.directOut = target - start;
            if (p.locate) {
                ia.directEndI = targetI - start;
                ia.directEndJ = targetJ - start;
            }
            ia.directIds = view->d_ids;
            ia.directN = view->nPacked;
            ia.overflow = nullptr;
            directScatter = true;
        }
        // On the column split's fast path the kernel reads the staged copy itself, once per workgroup into LDS - no copy
        // in front of the launch. The staging buffer is not drained before the launch's stream has been waited for
        // (Workspace::stage), on the asynchronous entry points neither. Every other launch gets its copy on the device.
        if (ia.splitMode && directScatter) ia.profile = (const int16_t*)staged;
        else HIP_TRY(hipMemcpyAsync(const_cast<int16_t*>(ia.profile), staged, prof.size() * sizeof(prof[0]), hipMemcpyHostToDevice, stream));
        done->directScatter = directScatter;
        done->pairUnits = pairUnits;
        done->flavour = pf;
        return 0;
    }

    // ... and the launch itself
    int launchOneStripPair(const ScorePlan& p, InterseqArgs& ia, OneStripLaunch* done) {
        const int pairUnits = done->pairUnits;
        const PairFlavour pf = done->flavour;
        if (!ia.splitMode) {
            // (the dynamic hand-out's counter; the column split takes nothing from it)
            void* wc;
            RC_TRY(ws->get(kWorkCounter, sizeof(int), &wc));
            HIP_TRY(hipMemsetAsync(wc, 0, sizeof(int), stream));
            ia.workCounter = (int*)wc;
        }
        // (diagnostic builds of the Smith-Waterman kernel, -DMIOPAL_HEADLINE_TIMING=1: the SIMDs' finish times)
        unsigned long long* simdFinish = nullptr;
        // (behind the SIMDs of the launch's workgroups: when the pair table stood, latest and sum)
        const int blocks = ia.splitMode ? ia.splitBlocks : std::max(1, std::min(pairUnits, ia.nGroups));
        const int finishSlots = 1 + 4 * blocks + 2;
        if (pf == kPairSwBiased && tuned(Tune::STRIP_TIMING)) {
            void* tb;
            RC_TRY(ws->get(kStripTiming, finishSlots * sizeof(unsigned long long), &tb));
            HIP_TRY(hipMemsetAsync(tb, 0, finishSlots * sizeof(unsigned long long), stream));
            HIP_TRY(hipMemsetAsync(tb, 0xff, sizeof(unsigned long long), stream));
            ia.stripTiming = simdFinish = (unsigned long long*)tb;
        }
        g_lastRouting[1] = 2 + (int)pf + (ia.splitMode ? 64 : 0);   // (64: the column split)
        g_lastLaunchShape[1] = blocks;
        g_lastLaunchShape[2] = pf == kPairGlobalBiased ? (p.pairRows <= 54 ? 12 : 8) : kPairWavesPerGroup;   // (globalWaves)
        // (the int16 / half-float flavours and the column split hand out without shares, whatever ia.tailThrottle says)
        g_lastLaunchShape[3] = (pf == kPairSwBiased || pf == kPairGlobalBiased) && !ia.splitMode ? ia.tailThrottle : 0;
        // the biased kernels exist for every number of rows (NW / HW / OV: every even number): no padding rows to 8
        // (test switch: the launch behaves as if the runtime had refused it, e.g. its 150 KB of dynamic LDS)
        const hipError_t pe = tuned(Tune::TEST_REFUSE_PAIR_LAUNCH)
                                  ? hipErrorInvalidValue
                                  : launchInterseqPair(ia, (p.biased || p.globalPair) ? p.pairRows : p.rows, pf, pairUnits, stream, p.locate);
        if (pe == hipSuccess && simdFinish) {
            std::vector<unsigned long long> t((size_t)finishSlots);
            HIP_TRY(hipMemcpyAsync(t.data(), simdFinish, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            double sum = 0, last = 0, first = 1e30;
            int n = 0;
            for (int i = 1; i < finishSlots - 2; ++i) {
                if (t[i] == 0) continue;   // (a build without stamps, or a SIMD the launch left alone)
                const double us = (double)(t[i] - t[0]) / 100.0;   // 100 MHz ticks -> us
                sum += us;
                last = std::max(last, us);
                first = std::min(first, us);
                ++n;
            }
            if (n > 0)
                fprintf(stderr, "[miopal] headline timing (%d SIMDs, %d groups, %d rows): finish mean %.1f us  first %.1f  last %.1f  "
                                "last - mean %.1f us\n",
                        n, ia.nGroups, p.pairRows, sum / n, first, last, last - sum / n);
            if (t[finishSlots - 2] != 0)
                fprintf(stderr, "[miopal] headline prologue (%d workgroups): pair table ready %.2f us after the first wavefront's start "
                                "(mean), %.2f us (last)\n",
                        blocks, ((double)t[finishSlots - 1] / blocks - (double)t[0]) / 100.0, (double)(t[finishSlots - 2] - t[0]) / 100.0);
        }
        done->launch = pe;
        return 0;
    }

    // step 10: view order -> database order (windows: merged by key)
    int scatterResults(const View* view, const ScorePlan& p, const InterseqArgs& ia, const PassBuffers& b, bool sideEmpty, bool forked,
                       bool directScatter, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ) {
        const int nScatter = view->nPacked - p.packedSkip;
        if (p.keyed) {
            // nothing else writes the results of a segmented search before this point: no
            // target is kept out of the view, no group is skipped (limit >= one window)
            if (p.firstPos != 0 || !sideEmpty || forked)
                return fail(MIOPAL_ERR_INTERNAL, "segmented view with side jobs");
            HIP_TRY(launchScatterKeyed(ia.score, ia.endI, ia.endJ, (const uint8_t*)b.vo, view->d_ids,
                                       view->d_segStart, nScatter, start, (unsigned long long*)b.keys,
                                       p.mayOverflow ? (int32_t*)b.ct : nullptr, stream, p.keyBias));
            HIP_TRY(launchDecodeKeys((const unsigned long long*)b.keys, (int)n, d_score, d_endI, d_endJ, stream, p.keyBias));
        } else if (!directScatter) {
            HIP_TRY(launchScatter(ia.score + p.packedSkip, (const uint8_t*)b.vo + p.packedSkip, view->d_ids + p.packedSkip,
                                  nScatter, start, d_score, p.mayOverflow ? (int32_t*)b.ct : nullptr, p.overlap > 0,
                                  stream));
            if (p.locate)
                HIP_TRY(launchScatterEnds(ia.endI + p.packedSkip, ia.endJ + p.packedSkip, view->d_ids + p.packedSkip,
                                          nScatter, start, d_endI, d_endJ, stream));
        }
        return 0;
    }

    // Score pass (all search types). d_score/d_endI/d_endJ are in database order.
    int scorePass(int32_t* d_score, int32_t* d_endI, int32_t* d_endJ) {
        return scorePassImpl(d_score, d_endI, d_endJ, true);
    }

    // The steps in order. A pass that has to start over calls itself: every such condition is in this function.
    int scorePassImpl(int32_t* d_score, int32_t* d_endI, int32_t* d_endJ, bool useHalf) {
        RC_TRY(rulesFor(mode, &r));
        rules = packRules(r);
        std::vector<PairJob> jobs;
        RC_TRY(checkInt32Range(model(), Q, db->maxLen));
        // a pass that starts over (refused launch, declined probe, next rung) writes the device arrays:
        // whatever an earlier attempt put into the host-visible buffer is not the result
        wroteHost = false;

        g_lastRouting[0] = g_lastRouting[1] = g_lastRouting[2] = g_lastRouting[3] = 0;
        g_lastWindowPlan[0] = g_lastWindowPlan[1] = g_lastWindowPlan[2] = g_lastWindowPlan[3] = 0;
        g_lastLaunchShape[0] = db->computeUnits;   // miopalLastLaunchShape: [1 .. 3] are the persistent launch's, below
        g_lastLaunchShape[1] = g_lastLaunchShape[2] = g_lastLaunchShape[3] = 0;
        if (!interseqUsable() || (smallSearch() && smallSearchAllowed(db))) {
            g_lastRouting[0] = n;
            jobs.reserve((size_t)n);
            for (int64_t k = start; k < end; ++k) jobs.push_back(forwardJob(k, rules));
            return runPairs(jobs, false, d_score, d_endI, d_endJ, nullptr);
        }

        PhaseTimer spt;
        ScorePlan p;
        PassBuffers b;
        planWindows(p);
        std::shared_ptr<View> view;
        RC_TRY(getView(db, start, end, p.overlap, &view, p.stride));
        spt.mark("    view lookup");
        // not handled by the packed kernel: can be recomputed beside it
        std::vector<PairJob> sideJobs;
        for (int32_t id : view->longIds) sideJobs.push_back(forwardJob(id, rules));
        // windows of one target are merged with atomicMax: start from 0 (Smith-Waterman scores
        // are never negative); whole-target results of the int32 kernel are plain stores of the
        // final value, in either order the maximum is that value
        p.keyed = p.overlap > 0 && searchType != OPAL_SEARCH_SCORE;  // with end locations
        if (view->overlap > 0) {   // miopalLastWindowPlan: what the view holds, not what the plan wished for
            g_lastWindowPlan[0] = view->overlap;
            g_lastWindowPlan[1] = view->stride;
            g_lastWindowPlan[2] = view->nPacked;
            g_lastWindowPlan[3] = p.keyed ? 1 : 0;
        }
        if (p.keyed) {
            RC_TRY(ws->get(kKeys, (size_t)n * sizeof(unsigned long long), &b.keys));
            HIP_TRY(hipMemsetAsync(b.keys, 0, (size_t)n * sizeof(unsigned long long), stream));
        } else if (p.overlap > 0) {
            // (Smith-Waterman scores start from 0, HW scores from "minus infinity")
            if (p.keyBias) HIP_TRY(launchFillInt32(d_score, (int)n, INT32_MIN, stream));
            else HIP_TRY(hipMemsetAsync(d_score, 0, (size_t)n * sizeof(int32_t), stream));
        }
        planGeneralStrips(view.get(), p);
        planSwPairStrips(view.get(), useHalf, p);
        planGlobalPairStrips(view.get(), useHalf, p);
        planSideCut(view.get(), p, sideJobs);

        if (view->nGroups > p.firstGroup) {
            planLanes(view.get(), useHalf, p, jobs, sideJobs);
            const std::vector<int16_t> prof = buildProfile(p);
            // (a score pass that started over has its side jobs on the side stream already: they are still joined)
            bool forked = sideForked;
            bool directScatter = false;   // the packed kernel wrote database order itself
            RC_TRY(forkSideJobs(p, sideJobs, d_score, d_endI, d_endJ, &forked, spt));
            InterseqArgs ia{};
            RC_TRY(prepareLaunch(view.get(), p, prof, b, ia));
            const int16_t* const profileDevice = ia.profile;
            OneStripLaunch done;
            if (oneStripPair(p))
                RC_TRY(planOneStripPair(view.get(), p, prof, ia, d_score, d_endI, d_endJ, forked, sideJobs.empty() && jobs.empty(), &done));
            const bool timed = db->profiling.load() != 0;
            EventPair ev;
            if (timed) {
                HIP_TRY(hipEventCreate(&ev.e0));
                HIP_TRY(hipEventCreate(&ev.e1));
                HIP_TRY(hipEventRecord(ev.e0, stream));
            }
            g_lastRouting[1] = 1 + 32 * (int)p.flavour;  // general kernel and its lane arithmetic
            if (p.pairStrips) {
                StripsLaunch sl;
                RC_TRY(prepareStripsLaunch(p, ia, &sl));
                hipError_t pe = hipSuccess;
                if (p.probeEnds) {
                    StripsProbe probe;
                    RC_TRY(probeStripsEnds(p, ia, sl, &probe));
                    pe = probe.launch;
                    if (pe == hipSuccess && 2 * probe.beyond >= probe.lanes) {
                        // (round 3: two sweeps of this kernel instead of the general kernel's row scans;
                        // MIOPAL_NO_TWO_PASS_ENDS restores round 2)
                        stripsEndsDeclined = true;
                        twoPassEnds = !tuned(Tune::NO_TWO_PASS_ENDS);
                        return scorePassImpl(d_score, d_endI, d_endJ, useHalf);
                    }
                }
                if (pe == hipSuccess) RC_TRY(launchStripsSweeps(view.get(), p, ia, sl, &pe));
                if (pe != hipSuccess) {
                    // (e.g. the runtime refuses 150 KB of dynamic LDS: start over on the general kernel)
                    (void)hipGetLastError();
                    (p.globalStrips ? globalStripsRefused : pairStripsRefused) = true;
                    if (tuned(Tune::VERBOSE))
                        fprintf(stderr, "miopal: multi-strip pair-table kernel refused (%s), using the general kernel\n",
                                hipGetErrorString(pe));
                    return scorePassImpl(d_score, d_endI, d_endJ, useHalf);
                }
                // (score, column, row) keys merged over the strips -> view-order scores and end locations
                if (p.globalStrips && p.locate)
                    HIP_TRY(launchDecodeGlobalKeys(ia.stripKeys, view->d_lens, view->nGroups * kGroupTargets, Q, ia.score,
                                                   ia.endI, ia.endJ, stream));
                else if (p.locate)
                    HIP_TRY(launchDecodeStripKeys(ia.stripKeys, view->nGroups * kGroupTargets, ia.score, ia.endI, ia.endJ, stream));
            } else if (p.usePair || p.globalPair) {
                RC_TRY(launchOneStripPair(p, ia, &done));
                directScatter = done.directScatter;
                const hipError_t pe = done.launch;
                if (pe != hipSuccess) {
                    // e.g. the runtime refuses 150 KB of dynamic LDS: use the v_perm variant (the
                    // biased profile is a plain int16 profile whose padding score, -1024, cannot raise
                    // a Smith-Waterman maximum either)
                    (void)hipGetLastError();
                    if (p.globalPair) {
                        // (its profile and its routing of long targets do not suit the general kernel:
                        // start over without it)
                        globalPairRefused = true;
                        return scorePassImpl(d_score, d_endI, d_endJ, useHalf);
                    }
                    g_lastRouting[1] |= 16;
                    g_lastLaunchShape[1] = g_lastLaunchShape[2] = g_lastLaunchShape[3] = 0;   // (no persistent launch ran)
                    if (tuned(Tune::VERBOSE))
                        fprintf(stderr, "miopal: pair-table kernel refused (%s), using the general kernel\n",
                                hipGetErrorString(pe));
                    if (directScatter) {   // (the general kernel writes view order)
                        directScatter = wroteHost = false;
                        ia.directOut = nullptr;
                        ia.overflow = (uint8_t*)b.vo;
                    }
                    if (ia.profile != profileDevice) {   // (... and reads the profile from the device)
                        ia.profile = profileDevice;
                        RC_TRY(ws->stageUpload(const_cast<int16_t*>(profileDevice), prof.data(), prof.size() * sizeof(prof[0]), stream));
                    }
                    HIP_TRY(launchInterseq(ia, p.rows, p.waves, p.flavour, p.locate, stream));
                }
            } else {
                HIP_TRY(launchInterseq(ia, p.rows, p.waves, p.flavour, p.locate, stream));
            }
            if (timed) {
                HIP_TRY(hipEventRecord(ev.e1, stream));
                std::lock_guard<std::mutex> g(db->timingMutex);
                ws->timings.emplace_back(ev.release());
                db->lastTimed = ws;
            }
            RC_TRY(scatterResults(view.get(), p, ia, b, sideJobs.empty(), forked, directScatter, d_score, d_endI, d_endJ));
            if (forked) HIP_TRY(hipStreamWaitEvent(stream, ws->evJoin, 0));
            spt.mark("    packed kernel enqueued");
            if (spt.on) {
                HIP_TRY(hipStreamSynchronize(stream));
                spt.mark("    packed + side kernels done");
            }
            if (p.mayOverflow) {
                int32_t count = 0;
                RC_TRY(ws->stageDownload(&count, b.ct, sizeof(int32_t)));
                RC_TRY(ws->finishDownloads());
                if (p.pairStrips && p.sw && p.rowKeys && count > p.directLimit && !twoPassEnds && !tuned(Tune::NO_TWO_PASS_ENDS)) {
                    // many lanes left the row keys' range (384 .. 768): the scores' own range is 25600 -
                    // two sweeps of the strips kernel before the int16 rung
                    twoPassEnds = true;
                    return scorePassImpl(d_score, d_endI, d_endJ, useHalf);
                }
                if ((p.halfFloat || p.biased || p.swShifted || p.pairStrips) && count > p.directLimit) {
                    // many targets left the half-float range: second rung, int16 lanes,
                    // over the whole view (its results overwrite the first pass)
                    return scorePassImpl(d_score, d_endI, d_endJ, false);
                }
                if (count > 0) {
                    std::vector<uint8_t> flags((size_t)view->nPacked);
                    RC_TRY(ws->stageDownload(flags.data(), b.vo, flags.size()));
                    RC_TRY(ws->finishDownloads());
                    for (int k = p.packedSkip; k < view->nPacked; ++k)
                        if (flags[k]) queueWhole(jobs, view->ids[k]);
                    g_lastRouting[3] = count;
                }
            }
        }
        jobs.insert(jobs.end(), sideJobs.begin(), sideJobs.end());
        return runPairs(jobs, false, d_score, d_endI, d_endJ, nullptr);
    }
};

// miopalSearch's range check for its 32-bit kernels with the extreme entries of a PSSM's rows ([Q][A]) where the
// matrix's stand: made by the PSSM entry points themselves, in validate()'s place and before any device call. The
// plain forms have no such check in front of their score pass.
static int checkPssmRange(const MiopalDb* db, const int* rows, int Q, int A, int open, int ext) {
    ScoreModel m{open, ext, 0, 0};
    scoreExtremes(rows, (size_t)std::max(Q, 0) * A, &m.maxScore, &m.minScore);
    return checkInt32Range(m, Q, db->maxLen);
}

// The score-row pass of one query, for the entry points that select on the device: a workspace leased for the call,
// the search, and searchImpl's score / end pass with the results left in the workspace's device slots (d_endI and
// d_endJ: null without end locations). The selection is enqueued on ws->stream behind it - the score pass has joined
// its side-stream jobs and flagged lanes into that stream - downloads on `ws` and checks s.d_stripError, so this
// object outlives it. `matrix` or `pssmRows` is the score source (the other null; with rows, `query` is the consensus).
struct ScoreRows {
    WorkspaceLease lease;
    Workspace* ws = nullptr;
    Search s;
    int32_t *d_score = nullptr, *d_endI = nullptr, *d_endJ = nullptr;
    ScoreRows(MiopalDb* db, const unsigned char* query, int Q, int open, int ext, const int* matrix, const int* pssmRows,
              int A, int searchType, int mode, int64_t start, int64_t end)
        : lease(db), s{db, nullptr, nullptr, query, Q, open, ext, A, searchType, mode, matrix, start, end, end - start} {
        s.pssmRows = pssmRows;
    }
    int run() {
        HIP_TRY(hipSetDevice(s.db->device));
        RC_TRY(lease.acquireInternal());
        s.ws = ws = lease.ws;
        s.stream = ws->stream;
        RC_TRY(s.prepare());
        void *ps, *pi = nullptr, *pj = nullptr;
        RC_TRY(ws->get(kScore, (size_t)s.n * sizeof(int32_t), &ps));
        if (s.searchType == OPAL_SEARCH_SCORE_END) {
            RC_TRY(ws->get(kEndI, (size_t)s.n * sizeof(int32_t), &pi));
            RC_TRY(ws->get(kEndJ, (size_t)s.n * sizeof(int32_t), &pj));
        }
        d_score = (int32_t*)ps;
        d_endI = (int32_t*)pi;
        d_endJ = (int32_t*)pj;
        return s.scorePass(d_score, d_endI, d_endJ);
    }
};
