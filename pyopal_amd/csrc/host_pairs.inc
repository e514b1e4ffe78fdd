// Part of host.hip (included there, not a translation unit of its own): miopalAlignPairs, a list of (query, target)
// pairs against a resident handle in one call.
//
// Pair p is the one-target search of query pairQuery[p] against target pairTarget[p], and its answer is defined by
// miopalSearch on that slice. The list is cut into chunks whose workspaces fit the budgets of the `full` path
// (direction bytes: 2 x kDirBudget, strip boundaries: 4 GB, operation slots: 2 GB), sized from the tallest query and
// the longest target of the chunk; a list with a few long pairs among many short ones is taken in order of
// decreasing size so that the long pairs do not size everybody's workspace. Per chunk, on the device:
//   jobs (pairlist_jobs_kernel) -> forward pass -> [full: reversed-prefix scan -> start cells -> direction pass
//   -> walk -> gather] -> one download.
// Forward pass: one lane per pair (pairlist_forward_kernel; the jobs sorted by length, the outlier head of the sort
// on the wavefront-per-pair kernel) or one wavefront per pair (intraseq_kernel) for chunks too small to fill the
// chip, for queries of more than 4096 residues and under NO_PERPAIR - decided by the per-cell cost estimates of
// full_plan.h. Scan and direction pass: perpair_kernel / intraseq_kernel, as in a one-query `full` search, with the
// pair's query origin added to its jobs. Pairs with an empty query or target are answered here (closed forms of the
// border, oracle/opal_oracle.c).
//
// miopalAlignPairsPssm is the same function with another score source: a list of position-specific scoring matrices
// (pssmRows: their rows end to end, [total rows][A]; `queries` / `queryOffsets` then hold the consensus and the row
// offsets, `matrix` is null; the entry point has made the checks that need no handle). The jobs' query origin is the
// PSSM's first row, which the row-indexed kernels add to the row they look up. One lane per pair - the forward pass
// (pairlist_forward_kernel<., ., true>) as well as the scan and the direction pass of `full` (perpair_kernel<., false,
// true>) - needs the whole list's table in LDS (perPairPssmBytes of the total rows: 493 rows at 32 letters, 651 at
// 24); a list with more rows runs one wavefront per pair throughout.
//
// A `full` list may be given a consumer (PairChunkConsumer below; miopalProfileColumns, host_profile.inc): per chunk it
// is handed what the walk left on the device in the place of gather + download, and the operations never reach the
// host. Without one the function runs the statements it always ran.
//
// The passes behind the forward pass are runLaterPasses below, which the aligned occurrence search
// (host_occurrence_align.inc) shares: its end cells are the occurrences the write sweep left on the device.
namespace {

constexpr int64_t kPairChunkMax = int64_t(1) << 22;   // pairs per chunk at most (56-byte jobs, twice)
constexpr int kPairLaneMaxQuery = 4096;               // taller queries keep the wavefront-per-pair kernels
thread_local int64_t g_lastPairRouting[4] = {0, 0, 0, 0};   // miopalLastPairRouting

struct PairChunkPlan {
    int64_t first, count;   // positions in the processing order
    int maxQ, maxL;
    bool waveOnly;
};

inline int64_t pairStrips(int64_t q) { return std::max<int64_t>(1, (q + kLanes - 1) / kLanes); }

// pairs a chunk may hold when its tallest query has maxQ residues and its longest target maxL
int64_t pairChunkCapacity(int64_t maxQ, int64_t maxL, bool full) {
    int64_t cap = kPairChunkMax;
    const int64_t strips = pairStrips(maxQ);
    if (strips > 1) cap = std::min<int64_t>(cap, (4ll << 30) / (16 * std::max<int64_t>(maxL, 1)));
    if (full) {
        cap = std::min<int64_t>(cap, 2 * kDirBudget / slotDir(strips, maxL));
        cap = std::min<int64_t>(cap, (2ll << 30) / slotOpsMost(maxQ, maxL));
    }
    return std::max<int64_t>(cap, 1);
}

// What the walk of a chunk of a `full` list left on the device, for a consumer that takes the operations where they
// are (host_profile.inc): the operations of the chunk's pair k end with slot k of `slots` (slotOps bytes each;
// opsLen[k] of them), start at cell (startQ[k], startT[k]) of the pair, and its target begins at residue tOff[k];
// pairs[k] is its position in the caller's list. All device pointers but `pairs`; valid until the consumer returns.
struct PairChunk {
    Workspace* ws;
    int count;
    const int64_t* pairs;
    const uint8_t* slots;
    int64_t slotOps;
    const int32_t *opsLen, *startQ, *startT;
    const int64_t* tOff;
};
// The consumer of alignPairsImpl: with one, a chunk's operations are neither gathered nor downloaded - chunk() enqueues
// what it does with them on the chunk's stream, behind the walk, and they are final for it when the chunk's small
// arrays have come down. checks(): the consumer's own argument checks, after the list's and before any device call.
// noun: what the messages call an entry of the list.
struct PairChunkConsumer {
    const char* noun = "pair";
    std::function<int()> checks;
    std::function<int(const PairChunk&)> chunk;
};

// The later passes of a chunk of end cells that lie on the device - the `full` pair list's and the aligned occurrence
// search's (host_occurrence_align.inc): what they read, and what they leave on the host. Entry k of the chunk has the
// score / end cell score[k], endI[k] (query row), endJ[k] (target column); its target begins at residue tOff[k] and
// its query at qBase[k] of the query buffer (null: 0).
struct LaterPasses {
    MiopalDb* db;
    Search* s;
    int mode, open, ext, A, totalQuery;
    int nc, maxL;              // entries; the longest target (prefix) of the chunk
    bool oneStrip;             // no query (prefix) of the chunk has more than 64 rows
    int64_t fwdWsStride;       // strip-boundary columns per job of the wavefront-per-pair scan (0: one strip)
    bool lane, lanePossible, forceLane;   // the scan one lane per entry; the lane kernels may be used at all (then
                                          // `sorted`, `bins` and `head` are there)
    const int32_t *score, *endI, *endJ;
    const int64_t* tOff;
    const int32_t* qBase;
    PairJob *jobs, *sorted;
    int *bins, *head;
    bool startsOnly;           // stop after the start cells: no direction pass, no walk, no operations
    bool endsOnHost;           // hs / hi / hj hold the chunk's scores and end cells already: not downloaded again
    const PairChunkConsumer* consumer;
    const int64_t* pairs;      // the consumer's view of the entries' positions in the caller's list
    std::function<long long(int)> idOf;   // what the messages call entry k
    const char* noun;
    // host side: nc entries each
    int32_t *hs, *hi, *hj;
    std::vector<int32_t>*hsq, *hst, *hlen, *hts;
    HostBytes* outOps;         // the chunk's operations are appended
    // what the passes did: the longest target window; the direction pass one lane per entry, and the wavefronts at
    // the head of its sorted list that went one wavefront per entry (read back only when asked for)
    int64_t maxWindow = 0;
    bool traceLane = false;
    int* traceHeadWaves = nullptr;
};

}  // namespace

// From the start cells to the chunk's download: reversed-prefix scan with the stop rule -> start cells -> [direction
// pass -> walk -> gather (or the consumer)] -> one download.
static int runLaterPasses(LaterPasses& c) {
    MiopalDb* const db = c.db;
    Search& s = *c.s;
    Workspace* const ws = s.ws;
    hipStream_t const stream = s.stream;
    const int nc = c.nc, mode = c.mode, open = c.open, ext = c.ext, totalQuery = c.totalQuery;
    const int64_t nc64 = roundLanes(nc);
    const bool lane = c.lane, lanePossible = c.lanePossible, forceLane = c.forceLane, oneStrip = c.oneStrip;
    const int64_t fwdWsStride = c.fwdWsStride;
    const PairChunkConsumer* const consumer = c.consumer;
    const void *ps = c.score, *pi = c.endI, *pj = c.endJ, *ptoff = c.tOff, *pqbase = c.qBase;
    void *pjobs = c.jobs, *psorted = c.sorted, *pbins = c.bins, *phead = c.head;
    DpRules fr{};
    rulesForMode(mode, &fr);
    const PerPairArgs perPair = perPairCommon(db, s, totalQuery, c.A, open, ext);
    // ---- start cells: reversed prefixes anchored on the end cells -----------------------------------
    void *rs = nullptr, *ri = nullptr, *rj = nullptr, *psq, *pst, *pmis, *plen, *pts;
    RC_TRY(ws->get(kStartQ, (size_t)nc * sizeof(int32_t), &psq));
    RC_TRY(ws->get(kStartT, (size_t)nc * sizeof(int32_t), &pst));
    RC_TRY(ws->get(kMismatch, 4 * sizeof(int), &pmis));
    RC_TRY(ws->get(kOpsLen, (size_t)nc * sizeof(int32_t), &plen));
    RC_TRY(ws->get(kTraceScore, (size_t)nc * sizeof(int32_t), &pts));
    HIP_TRY(hipMemsetAsync(pmis, 0, 4 * sizeof(int), stream));
    if (mode != OPAL_MODE_NW) {
        RC_TRY(ws->get(kRScore, (size_t)nc * sizeof(int32_t), &rs));
        RC_TRY(ws->get(kRI, (size_t)nc * sizeof(int32_t), &ri));
        RC_TRY(ws->get(kRJ, (size_t)nc * sizeof(int32_t), &rj));
        const DpRules rr{1, 1, 0, fr.region};
        if (lane) {
            HIP_TRY(launchReverseJobs(nc, (const int32_t*)ps, (const int32_t*)pi, (const int32_t*)pj, (const int64_t*)ptoff,
                                      packRules(rr), 0, (PairJob*)pjobs, stream, (const int32_t*)pqbase));
            PerPairArgs pa = perPair;
            pa.jobs = (const PairJob*)pjobs;
            if (!oneStrip) {
                // prefixes of similar length share a wavefront
                HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, nc, c.maxL, (int*)pbins, (PairJob*)psorted, stream));
                pa.jobs = (const PairJob*)psorted;
                void* pb;
                RC_TRY(ws->get(kPairListBoundary, boundaryBytes(nc, c.maxL), &pb));
                pa.boundary = (int2*)pb;
                pa.boundaryStride = c.maxL;
            }
            pa.nJobs = nc;
            pa.score = (int32_t*)rs;
            pa.endI = (int32_t*)ri;
            pa.endJ = (int32_t*)rj;
            pa.reversed = 1;
            HIP_TRY(launchPerPair(pa, fr.region, stream));
        } else {
            HIP_TRY(launchReverseJobs(nc, (const int32_t*)ps, (const int32_t*)pi, (const int32_t*)pj, (const int64_t*)ptoff,
                                      packRules(rr), fwdWsStride, (PairJob*)pjobs, stream, (const int32_t*)pqbase));
            RC_TRY(s.runDeviceJobs((const PairJob*)pjobs, nc, (int32_t*)rs, (int32_t*)ri, (int32_t*)rj, false, nullptr, fwdWsStride));
        }
    }
    HIP_TRY(launchStartCells(nc, mode, open, ext, (const int32_t*)ps, (const int32_t*)pi, (const int32_t*)pj,
                             (const int32_t*)rs, (const int32_t*)ri, (const int32_t*)rj, (int32_t*)psq, (int32_t*)pst,
                             (int*)pmis, stream));
    // the traceback's slots are sized by the chunk's longest target window and tallest query window
    int checks[3] = {0, 0, 0};
    RC_TRY(ws->stageDownload(checks, pmis, sizeof checks));
    if (c.startsOnly) {
        // ... and nothing follows the start cells: they come down with the checks
        c.hsq->resize((size_t)nc); c.hst->resize((size_t)nc);
        RC_TRY(ws->stageDownload(c.hsq->data(), psq, (size_t)nc * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(c.hst->data(), pst, (size_t)nc * sizeof(int32_t)));
        if (!c.endsOnHost) {
            RC_TRY(ws->stageDownload(c.hs, ps, (size_t)nc * sizeof(int32_t)));
            RC_TRY(ws->stageDownload(c.hi, pi, (size_t)nc * sizeof(int32_t)));
            RC_TRY(ws->stageDownload(c.hj, pj, (size_t)nc * sizeof(int32_t)));
        }
    }
    RC_TRY(ws->finishDownloads());
    if (checks[0])
        return fail(MIOPAL_ERR_INTERNAL, "reverse pass disagrees with the forward score for %s %lld", c.noun, c.idOf(checks[0] - 1));
    const int64_t maxWindow = std::max(checks[1], 1), windowRows = std::max(checks[2], 1);
    c.maxWindow = maxWindow;
    if (c.startsOnly) return 0;
    const int64_t windowStrips = (windowRows + kLanes - 1) / kLanes;
    const int64_t slotDir = miopal::slotDir(windowStrips, maxWindow);
    const int64_t slotOps = miopal::slotOps(windowRows, maxWindow);
    const int64_t traceWsStride = windowStrips > 1 ? maxWindow : 0;
    // ---- directions: one lane or one wavefront per pair (full_plan.h; ms; the chunk is one batch) ------
    const double cells = traceCells(windowStrips, maxWindow);
    const bool traceLane = lanePossible && (forceLane || traceLaneMs(1, (double)nc, cells) <= traceWaveMs(1, (double)nc, cells));
    c.traceLane = traceLane;
    void *pd, *pslots, *pcompact = nullptr, *pblock, *ptotals;
    RC_TRY(ws->get(kOps, (size_t)(nc * slotOps), &pslots));
    if (!consumer) RC_TRY(ws->get(kCompactOps, (size_t)(nc * slotOps), &pcompact));
    RC_TRY(ws->get(kOpsOff, (size_t)((nc + 255) / 256) * sizeof(int64_t), &pblock));
    RC_TRY(ws->get(kOpsTotals, 2 * sizeof(int64_t), &ptotals));
    HIP_TRY(hipMemsetAsync(ptotals, 0, 2 * sizeof(int64_t), stream));
    HIP_TRY(launchTraceJobs(nc, packRules(DpRules{1, 1, 0, kLastCell}), (const int32_t*)psq, (const int32_t*)pst,
                            (const int32_t*)pi, (const int32_t*)pj, (const int64_t*)ptoff, slotDir, traceWsStride,
                            (PairJob*)pjobs, stream, (const int32_t*)pqbase));
    WalkArgs wa{};
    bool headUsed = false;
    if (traceLane) {
        const int64_t slotDirUsed = miopal::slotDirUsed(kDirLane, windowStrips, maxWindow);   // two rows per byte
        if (!ws->tryGet(kDirs, (size_t)(nc64 * slotDirUsed), &pd))
            return fail(MIOPAL_ERR_HIP, "out of device memory for the traceback workspace");
        int64_t maxHead = std::min<int64_t>((1ll << 30) / slotDir / kLanes, nc64 / kLanes);
        void* pheadDirs = nullptr;
        if (maxHead > 0 && !ws->tryGet(kHeadDirs, (size_t)(maxHead * kLanes * slotDir), &pheadDirs)) maxHead = 0;
        HIP_TRY(hipMemsetAsync(phead, 0, sizeof(int), stream));
        HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, nc, (int)maxWindow, (int*)pbins, (PairJob*)psorted, stream,
                                       maxHead > 0 ? (int*)phead : nullptr, (int)maxHead, (int)windowRows));
        PerPairArgs pa = perPair;
        if (maxHead > 0) {
            // outliers at the head of the sorted list: one wavefront per pair
            const int nh = (int)std::min<int64_t>(nc, maxHead * kLanes);
            RC_TRY(s.runDeviceJobs((const PairJob*)psorted, nh, (int32_t*)pts, nullptr, nullptr, true, (uint8_t*)pheadDirs,
                                   traceWsStride, (const int*)phead, slotDir));
            pa.skipWaves = (const int*)phead;
            wa.headWaves = (const int*)phead;
            wa.headDirs = (const uint8_t*)pheadDirs;
            wa.headDirStride = slotDir;
            headUsed = true;
        }
        pa.jobs = (const PairJob*)psorted;
        pa.nJobs = nc;
        pa.dirs = (uint8_t*)pd;
        pa.score = (int32_t*)pts;
        pa.dirWaveStride = slotDirUsed * kLanes;
        pa.dirStripColumns = dirStripColumns(false, maxWindow);
        if (windowStrips > 1) {
            void* pb;
            RC_TRY(ws->get(kPairListBoundary, boundaryBytes(nc, maxWindow), &pb));
            pa.boundary = (int2*)pb;
            pa.boundaryStride = maxWindow;
        }
        HIP_TRY(launchPerPair(pa, kPerPairTrace, stream));
        wa.slotByOut = 1;
        wa.dirWaveStride = pa.dirWaveStride;
        wa.dirStripColumns = pa.dirStripColumns;
    } else {
        if (!ws->tryGet(kDirs, (size_t)(nc * slotDir), &pd))
            return fail(MIOPAL_ERR_HIP, "out of device memory for the traceback workspace");
        RC_TRY(s.runDeviceJobs((const PairJob*)pjobs, nc, (int32_t*)pts, nullptr, nullptr, true, (uint8_t*)pd, traceWsStride));
    }
    fillWalk(&wa, (const PairJob*)(traceLane ? psorted : pjobs), nc, db, s, totalQuery, pd, pslots, slotOps, plen);
    HIP_TRY(launchWalk(wa, stream));
    if (consumer) {
        // (the operations stay where the walk left them: the consumer's kernels read the slots)
        RC_TRY(consumer->chunk(PairChunk{ws, nc, c.pairs, (const uint8_t*)pslots, slotOps,
                                         (const int32_t*)plen, (const int32_t*)psq, (const int32_t*)pst,
                                         (const int64_t*)ptoff}));
    } else {
        HIP_TRY(launchGatherOps(nc, (const uint8_t*)pslots, slotOps, (const int32_t*)plen, (int64_t*)pblock,
                                (const int64_t*)ptotals, (int64_t*)ptotals + 1, (uint8_t*)pcompact, stream));
    }
    // ---- one download: the small arrays (they carry the total), then the operations ---------------------
    std::vector<int32_t>&hsq = *c.hsq, &hst = *c.hst, &hlen = *c.hlen, &hts = *c.hts;
    hsq.resize((size_t)nc); hst.resize((size_t)nc); hlen.resize((size_t)nc); hts.resize((size_t)nc);
    int64_t total = 0;
    if (!consumer) RC_TRY(ws->stageDownload(&total, (const int64_t*)ptotals + 1, sizeof(int64_t)));
    if (!c.endsOnHost) {
        RC_TRY(ws->stageDownload(c.hs, ps, (size_t)nc * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(c.hi, pi, (size_t)nc * sizeof(int32_t)));
        RC_TRY(ws->stageDownload(c.hj, pj, (size_t)nc * sizeof(int32_t)));
    }
    RC_TRY(ws->stageDownload(hsq.data(), psq, (size_t)nc * sizeof(int32_t)));
    RC_TRY(ws->stageDownload(hst.data(), pst, (size_t)nc * sizeof(int32_t)));
    RC_TRY(ws->stageDownload(hlen.data(), plen, (size_t)nc * sizeof(int32_t)));
    RC_TRY(ws->stageDownload(hts.data(), pts, (size_t)nc * sizeof(int32_t)));
    if (c.traceHeadWaves) {
        *c.traceHeadWaves = 0;
        if (headUsed) RC_TRY(ws->stageDownload(c.traceHeadWaves, phead, sizeof(int)));
    }
    RC_TRY(ws->finishDownloads());
    if (!consumer) {
        if (total < 0 || total > nc * slotOps) return fail(MIOPAL_ERR_INTERNAL, "bad operation count");
        const size_t at = c.outOps->size;
        if (!c.outOps->resize(at + (size_t)total)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        RC_TRY(ws->stageDownload(c.outOps->data + at, pcompact, (size_t)total));
        RC_TRY(ws->finishDownloads());
    }
    int64_t sum = 0;
    for (int k = 0; k < nc; ++k) {
        if (c.hi[k] >= 0 && c.hj[k] >= 0 && hts[(size_t)k] != c.hs[k])
            return fail(MIOPAL_ERR_INTERNAL, "traceback score %d differs from search score %d for %s %lld",
                        hts[(size_t)k], c.hs[k], c.noun, c.idOf(k));
        sum += hlen[(size_t)k];
    }
    if (!consumer && sum != total) return fail(MIOPAL_ERR_INTERNAL, "operation offsets disagree with the device");
    return 0;
}

static int alignPairsImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                          const int32_t* pairQuery, const int64_t* pairTarget, int64_t nPairs, int open, int ext,
                          const int* matrix, int A, int searchType, int mode, int* score, int* endTarget,
                          int* endQuery, int* startTarget, int* startQuery, HostBytes* outOps, int64_t* opsOff,
                          const int* pssmRows = nullptr, const PairChunkConsumer* consumer = nullptr) {
    for (int k = 0; k < 4; ++k) g_lastPairRouting[k] = 0;
    const bool pssm = pssmRows != nullptr;
    const char* const noun = consumer ? consumer->noun : "pair";
    // what can be said without the handle first (a caller's mistake is reported whatever the handle's state): the search,
    // the queries and their residues, the pair list's query side, the outputs
    if (mode < OPAL_MODE_NW || mode > OPAL_MODE_SW) return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", mode);
    if (searchType < OPAL_SEARCH_SCORE || searchType > OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "invalid search type %d", searchType);
    if (nQueries < 0 || (nQueries > 0 && (!queryOffsets || !queries))) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad query list");
    if ((!pssm && !matrix) || A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad score matrix / alphabet length %d", A);
    for (int i = 0; i < nQueries && !pssm; ++i) {
        const int64_t len = queryOffsets[i + 1] - queryOffsets[i];
        if (queryOffsets[i] < 0 || len < 0 || len > INT32_MAX) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad query offsets at %d", i);
        for (int64_t x = 0; x < len; ++x)
            if (queries[queryOffsets[i] + x] >= A)
                return fail(MIOPAL_ERR_BAD_ARGUMENT, "query residue %d out of range at %lld of query %d", queries[queryOffsets[i] + x], (long long)x, i);
    }
    if (nPairs < 0 || (nPairs > 0 && (!pairQuery || !pairTarget))) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad pair list");
    for (int64_t p = 0; p < nPairs; ++p)
        if (pairQuery[p] < 0 || pairQuery[p] >= nQueries)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "%s %lld: %s index %d outside [0, %d)", noun, (long long)p, pssm ? "PSSM" : "query", pairQuery[p], nQueries);
    const bool locate = searchType >= OPAL_SEARCH_SCORE_END, full = searchType == OPAL_SEARCH_ALIGNMENT;
    if (full && (!outOps || !opsOff)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null alignment outputs");
    if (nPairs > 0) {
        if (!score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score output");
        if (locate && (!endTarget || !endQuery)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
        if (full && (!startTarget || !startQuery)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null alignment outputs");
    }
    // ... and with it: miopalSearch's own checks query by query, the pair list's target side
    if (pssm) {
        if (!db) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null database handle");
        if (A != db->alphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d differs from the database's %d", A, db->alphabet);
    } else {
        RC_TRY(validateBatch(db, queries, queryOffsets, nQueries, matrix, A, searchType, mode, 0, 0));
    }
    int64_t maxQ = 0, maxL = 0;
    for (int64_t p = 0; p < nPairs; ++p) {
        if (pairTarget[p] < 0 || pairTarget[p] >= db->count)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "%s %lld: target index %lld outside [0, %lld)", noun, (long long)p,
                        (long long)pairTarget[p], (long long)db->count);
        maxQ = std::max(maxQ, queryOffsets[pairQuery[p] + 1] - queryOffsets[pairQuery[p]]);
        maxL = std::max<int64_t>(maxL, dbLen(db, pairTarget[p]));
    }
    {
        // miopalSearch's range check for its 32-bit kernels, for the longest query and the longest target of the list
        // (position-specific scores: the extreme entries of the rows where the matrix's stand)
        const int* const entries = pssm ? pssmRows : matrix;
        const size_t nEntries = pssm ? (size_t)(nQueries > 0 ? queryOffsets[nQueries] - queryOffsets[0] : 0) * A : (size_t)A * A;
        const int maxScore = nEntries ? *std::max_element(entries, entries + nEntries) : 0;
        const int minScore = nEntries ? *std::min_element(entries, entries + nEntries) : 0;
        if (nPairs > 0) RC_TRY(checkInt32Range({open, ext, maxScore, minScore}, maxQ, maxL));
    }
    if (consumer) RC_TRY(consumer->checks());
    if (full) opsOff[0] = 0;
    if (nPairs == 0) return 0;

    // the queries end to end (the kernels' query buffer) and their origins in it
    std::vector<int32_t> qOff((size_t)nQueries + 1, 0);
    {
        int64_t total = 0;
        for (int i = 0; i < nQueries; ++i) total += queryOffsets[i + 1] - queryOffsets[i];
        if (total > INT32_MAX - 64) return fail(MIOPAL_ERR_BAD_ARGUMENT, "the queries of a pair list hold 2 GB at most");
    }
    std::vector<unsigned char> concat;
    for (int i = 0; i < nQueries; ++i) {
        qOff[(size_t)i] = (int32_t)concat.size();
        concat.insert(concat.end(), queries + queryOffsets[i], queries + queryOffsets[i + 1]);
    }
    qOff[(size_t)nQueries] = (int32_t)concat.size();
    auto qLenOf = [&](int64_t p) { return (int)(qOff[(size_t)pairQuery[p] + 1] - qOff[(size_t)pairQuery[p]]); };

    DpRules fr{};
    rulesForMode(mode, &fr);   // (the mode was checked above)
    // pairs without a DP: the closed forms of the border, no cell and no operations
    std::vector<int64_t> order;   // the other pairs, in the order they are processed
    order.reserve((size_t)nPairs);
    bool anyTall = false;
    for (int64_t p = 0; p < nPairs; ++p) {
        const int Q = qLenOf(p), L = dbLen(db, pairTarget[p]);
        if (Q > 0 && L > 0) {
            order.push_back(p);
            anyTall = anyTall || Q > kPairLaneMaxQuery;
            continue;
        }
        int v = 0;
        if (!fr.floor0) {
            if (Q > 0) v = fr.leftGap ? borderGap(Q - 1, open, ext) : 0;
            if (L > 0) v = fr.topGap ? borderGap(L - 1, open, ext) : 0;
        }
        score[p] = v;
        if (locate) endTarget[p] = endQuery[p] = -1;
        if (full) startTarget[p] = startQuery[p] = -1;
    }
    const int64_t nLive = (int64_t)order.size();
    g_lastPairRouting[2] = nPairs - nLive;
    std::vector<int32_t> lensByPair;   // operations per pair (full)
    if (full) lensByPair.assign((size_t)nPairs, 0);
    bool inPairOrder = true;           // the chunks' operations, end to end, are the caller's buffer
    if (nLive > 0) {
        // ---- chunks -----------------------------------------------------------------------------------------
        std::vector<PairChunkPlan> chunks;
        const int64_t capAll = pairChunkCapacity(maxQ, maxL, full);
        if (!anyTall && capAll >= std::min<int64_t>(nLive, 32768)) {
            for (int64_t c0 = 0; c0 < nLive; c0 += capAll)
                chunks.push_back({c0, std::min(capAll, nLive - c0), (int)maxQ, (int)maxL, capAll < kLanes});
        } else {
            // largest pairs first (stable counting sort by the size class of a pair's direction slot; queries the
            // lane kernels do not take in front), then chunks as large as their own tallest and longest allow
            inPairOrder = false;
            auto keyOf = [&](int64_t p) {
                const int64_t cells = pairStrips(qLenOf(p)) * ((int64_t)dbLen(db, pairTarget[p]) + kLanes);
                int lg = 0;
                while ((int64_t(1) << lg) < cells) ++lg;
                return (qLenOf(p) > kPairLaneMaxQuery ? 64 : 0) + std::min(lg, 63);
            };
            std::vector<int64_t> first(129, 0);
            std::vector<uint8_t> keys((size_t)nLive);
            for (int64_t x = 0; x < nLive; ++x) {
                keys[(size_t)x] = (uint8_t)keyOf(order[(size_t)x]);
                ++first[127 - keys[(size_t)x] + 1];
            }
            for (int k = 0; k < 128; ++k) first[(size_t)k + 1] += first[(size_t)k];
            std::vector<int64_t> sorted((size_t)nLive);
            for (int64_t x = 0; x < nLive; ++x) sorted[(size_t)first[127 - keys[(size_t)x]]++] = order[(size_t)x];
            order.swap(sorted);
            PairChunkPlan c{0, 0, 0, 0, false};
            for (int64_t x = 0; x < nLive; ++x) {
                const int64_t p = order[(size_t)x];
                const int Q = qLenOf(p), L = dbLen(db, pairTarget[p]);
                const bool tall = Q > kPairLaneMaxQuery;
                const int nq = std::max(c.maxQ, Q), nl = std::max(c.maxL, L);
                if (c.count > 0 && (tall != c.waveOnly || c.count + 1 > pairChunkCapacity(nq, nl, full))) {
                    chunks.push_back(c);
                    c = PairChunkPlan{x, 0, 0, 0, false};
                }
                if (c.count == 0) c.waveOnly = tall;
                c.maxQ = std::max(c.maxQ, Q);
                c.maxL = std::max(c.maxL, L);
                ++c.count;
            }
            chunks.push_back(c);
            for (auto& ch : chunks) ch.waveOnly = ch.waveOnly || pairChunkCapacity(ch.maxQ, ch.maxL, full) < kLanes;
        }
        if (nLive != nPairs) inPairOrder = false;

        HIP_TRY(hipSetDevice(db->device));
        WorkspaceLease lease(db);
        RC_TRY(lease.acquireInternal());
        Workspace* ws = lease.ws;
        hipStream_t stream = ws->stream;
        Search s{db, ws, stream, concat.data(), (int)concat.size(), open, ext, A, searchType, mode, matrix, 0, db->count, nLive};
        s.pssmRows = pssmRows;
        RC_TRY(s.prepare());
        RC_TRY(s.ensurePairInputs());
        void* pqoff;
        RC_TRY(ws->get(kPairListQOff, qOff.size() * sizeof(int32_t), &pqoff));
        RC_TRY(ws->stageUpload(pqoff, qOff.data(), qOff.size() * sizeof(int32_t), stream));
        const int totalQuery = (int)concat.size();
        const bool forceLane = tuned(Tune::FORCE_LANE_PER_PAIR) != nullptr;
        // (position-specific scores: the lane-per-pair kernels hold the rows of the whole list in LDS)
        const bool tableFits = !pssm || perPairPssmBytes(totalQuery, A) != 0;
        const int rules = packRules(fr);
        std::vector<int32_t> cq, hs, hi, hj, hsq, hst, hlen, hts;
        std::vector<int64_t> ct;
        if (full) outOps->size = 0;

        for (const PairChunkPlan& ch : chunks) {
            const int nc = (int)ch.count;
            const int64_t nc64 = roundLanes(nc);
            const bool oneStrip = ch.maxQ <= kLanes;
            cq.resize((size_t)nc);
            ct.resize((size_t)nc);
            // the chunk's cells, in 64-row column steps: what either kind of kernel sweeps (full_plan.h's estimates)
            double laneCols = 0, waveCols = 0, laneChain = 0, waveChain = 0;
            for (int k = 0; k < nc; ++k) {
                const int64_t p = order[(size_t)(ch.first + k)];
                cq[(size_t)k] = pairQuery[p];
                ct[(size_t)k] = pairTarget[p];
                const double strips = (double)pairStrips(qLenOf(p)), L = (double)dbLen(db, pairTarget[p]);
                laneCols += strips * L;
                waveCols += strips * (L + 63);
                laneChain = std::max(laneChain, strips * L);
                waveChain = std::max(waveChain, strips * (L + 63));
            }
            // one lane per pair, where a wavefront lasts as long as its longest lane, or one wavefront per pair, a chain
            // of L + 63 steps (full_plan.h; ms)
            const bool lanePossible = !ch.waveOnly && tableFits && !tuned(Tune::NO_PERPAIR) && (nc > kSmallSearch || !smallSearchAllowed(db));
            const bool lane = lanePossible && (forceLane || scanLaneMs(laneCols, laneChain) <= scanWaveMs(waveCols, waveChain));

            void *pcq, *pct, *ptoff, *pqbase, *pjobs, *ps, *pi = nullptr, *pj = nullptr;
            RC_TRY(ws->get(kPairListQ, (size_t)nc * sizeof(int32_t), &pcq));
            RC_TRY(ws->get(kPairListT, (size_t)nc * sizeof(int64_t), &pct));
            RC_TRY(ws->get(kPairListTOff, (size_t)nc * sizeof(int64_t), &ptoff));
            RC_TRY(ws->get(kPairListQBase, (size_t)nc * sizeof(int32_t), &pqbase));
            RC_TRY(ws->get(kJobs, (size_t)nc * sizeof(PairJob), &pjobs));
            RC_TRY(ws->get(kScore, (size_t)nc * sizeof(int32_t), &ps));
            if (locate) {
                RC_TRY(ws->get(kEndI, (size_t)nc * sizeof(int32_t), &pi));
                RC_TRY(ws->get(kEndJ, (size_t)nc * sizeof(int32_t), &pj));
            }
            RC_TRY(ws->stageUpload(pcq, cq.data(), (size_t)nc * sizeof(int32_t), stream));
            RC_TRY(ws->stageUpload(pct, ct.data(), (size_t)nc * sizeof(int64_t), stream));
            const int64_t fwdWsStride = oneStrip ? 0 : ch.maxL;
            HIP_TRY(launchPairListJobs(nc, (const int32_t*)pcq, (const int64_t*)pct, (const int32_t*)pqoff, db->d_offsets, rules,
                                       lane ? 0 : fwdWsStride, (PairJob*)pjobs, (int64_t*)ptoff, (int32_t*)pqbase, stream));
            const PerPairArgs perPair = perPairCommon(db, s, totalQuery, A, open, ext);
            void *pbins = nullptr, *psorted = nullptr, *phead = nullptr;
            int headWaves = 0;
            if (lanePossible) {
                RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
                RC_TRY(ws->get(kSortedJobs, (size_t)nc * sizeof(PairJob), &psorted));
                RC_TRY(ws->get(kHeadWaves, sizeof(int), &phead));
            }
            // ---- forward pass ---------------------------------------------------------------------------------
            if (lane) {
                // neighbours of similar length share a wavefront (results stay addressed by job.out); the outliers at
                // the head of the sorted list - a lane would hold its wavefront for their whole length - go to the
                // wavefront-per-pair kernel (strip boundaries of 16 bytes per column and job: within 1 GB)
                const int64_t maxHead = std::min<int64_t>(nc64 / kLanes, oneStrip ? nc64 / kLanes : (1ll << 30) / (16 * ch.maxL * kLanes));
                HIP_TRY(hipMemsetAsync(phead, 0, sizeof(int), stream));
                HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, nc, ch.maxL, (int*)pbins, (PairJob*)psorted, stream,
                                               maxHead > 0 ? (int*)phead : nullptr, (int)maxHead, ch.maxQ));
                PerPairArgs pa = perPair;
                pa.jobs = (const PairJob*)psorted;
                pa.nJobs = nc;
                pa.score = (int32_t*)ps;
                pa.endI = (int32_t*)pi;
                pa.endJ = (int32_t*)pj;
                pa.skipWaves = (const int*)phead;
                if (!oneStrip) {
                    void* pb;
                    RC_TRY(ws->get(kPairListBoundary, boundaryBytes(nc, ch.maxL), &pb));
                    pa.boundary = (int2*)pb;
                    pa.boundaryStride = ch.maxL;
                }
                HIP_TRY(launchPairListForward(pa, fr.region, locate, stream));
                if (maxHead > 0) {
                    const int nh = (int)std::min<int64_t>(nc, maxHead * kLanes);
                    RC_TRY(s.runDeviceJobs((const PairJob*)psorted, nh, (int32_t*)ps, (int32_t*)pi, (int32_t*)pj, false, nullptr,
                                           fwdWsStride, (const int*)phead, 0));
                    RC_TRY(ws->stageDownload(&headWaves, phead, sizeof(int)));
                }
            } else {
                RC_TRY(s.runDeviceJobs((const PairJob*)pjobs, nc, (int32_t*)ps, (int32_t*)pi, (int32_t*)pj, false, nullptr, fwdWsStride));
            }

            hs.resize((size_t)nc);
            if (locate) { hi.resize((size_t)nc); hj.resize((size_t)nc); }
            if (!full) {
                RC_TRY(ws->stageDownload(hs.data(), ps, (size_t)nc * sizeof(int32_t)));
                if (locate) {
                    RC_TRY(ws->stageDownload(hi.data(), pi, (size_t)nc * sizeof(int32_t)));
                    RC_TRY(ws->stageDownload(hj.data(), pj, (size_t)nc * sizeof(int32_t)));
                }
                RC_TRY(ws->finishDownloads());
            } else {
                // ---- the later passes, from the start cells to the chunk's download (runLaterPasses) -------------
                LaterPasses lp{};
                lp.db = db; lp.s = &s;
                lp.mode = mode; lp.open = open; lp.ext = ext; lp.A = A; lp.totalQuery = totalQuery;
                lp.nc = nc; lp.maxL = ch.maxL; lp.oneStrip = oneStrip; lp.fwdWsStride = fwdWsStride;
                lp.lane = lane; lp.lanePossible = lanePossible; lp.forceLane = forceLane;
                lp.score = (const int32_t*)ps; lp.endI = (const int32_t*)pi; lp.endJ = (const int32_t*)pj;
                lp.tOff = (const int64_t*)ptoff; lp.qBase = (const int32_t*)pqbase;
                lp.jobs = (PairJob*)pjobs; lp.sorted = (PairJob*)psorted; lp.bins = (int*)pbins; lp.head = (int*)phead;
                lp.consumer = consumer; lp.pairs = order.data() + ch.first; lp.noun = "pair";
                lp.idOf = [&](int k) { return (long long)order[(size_t)(ch.first + k)]; };
                lp.hs = hs.data(); lp.hi = hi.data(); lp.hj = hj.data();
                lp.hsq = &hsq; lp.hst = &hst; lp.hlen = &hlen; lp.hts = &hts; lp.outOps = outOps;
                RC_TRY(runLaterPasses(lp));
                for (int k = 0; k < nc; ++k) {
                    const int64_t p = order[(size_t)(ch.first + k)];
                    startQuery[p] = hsq[(size_t)k];
                    startTarget[p] = hst[(size_t)k];
                    lensByPair[(size_t)p] = hlen[(size_t)k];
                }
            }
            for (int k = 0; k < nc; ++k) {
                const int64_t p = order[(size_t)(ch.first + k)];
                score[p] = hs[(size_t)k];
                if (locate) {
                    endQuery[p] = hi[(size_t)k];
                    endTarget[p] = hj[(size_t)k];
                }
            }
            const int64_t toWave = lane ? std::min<int64_t>(nc, (int64_t)headWaves * kLanes) : nc;
            g_lastPairRouting[0] += nc - toWave;
            g_lastPairRouting[1] += toWave;
            g_lastPairRouting[3] += 1;
        }
    }
    if (full && !consumer) {
        for (int64_t p = 0; p < nPairs; ++p) opsOff[p + 1] = opsOff[p] + lensByPair[(size_t)p];
        if ((size_t)opsOff[nPairs] != outOps->size) return fail(MIOPAL_ERR_INTERNAL, "operation offsets disagree with the device");
        if (!inPairOrder && outOps->size > 0) {
            // the chunks' operations lie in processing order: into pair order
            HostBytes inOrder;
            if (!inOrder.resize(outOps->size)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
            int64_t from = 0;
            for (int64_t p : order) {
                const int32_t len = lensByPair[(size_t)p];
                memcpy(inOrder.data + opsOff[p], outOps->data + from, (size_t)len);
                from += len;
            }
            std::swap(outOps->data, inOrder.data);
            std::swap(outOps->size, inOrder.size);
            std::swap(outOps->cap, inOrder.cap);
        }
    }
    return 0;
}
