// Part of host.hip (included there, not a translation unit of its own): miopalSearchBatch, many queries against
// one slice of a resident handle.
//
// Queries of at most 64 residues whose gap and matrix model passes the static range checks of the batch kernels
// (interseq_batch_impl.h) share launches: one per row class and chunk of queries, units of (query, run of groups)
// over the handle's plain packed view of the slice (no Smith-Waterman windows: their overlap depends on the query).
// Every (query, target) pair the lanes do not settle - targets kept out of the packed view, empty targets of the
// modes without a floor, Smith-Waterman lanes flagged at the biased range's limit, or the whole chunk when the slice
// is a small search - goes into ONE launch of the wavefront-per-pair int32 kernel (PairJob::qOff into the chunk's
// concatenated queries). Every other query (longer than 64 residues, a model the batch kernels cannot hold, a query
// of length 0) runs through miopalSearch's own path inside the same call. Either way the answer is the one
// miopalSearch gives for that query alone.
namespace {

// pairs per chunk of queries: bounds the device buffers ([rows][slice] int32 per output array)
constexpr int64_t kBatchChunkPairs = int64_t(1) << 23;

struct BatchPlan {
    int rows = 0;              // row class (0: the query takes the single-query path)
    int biasedLimit = 0;       // Smith-Waterman: flag threshold
    int biasedZero = 0;        // NW / HW / OV: pattern of a true 0
    bool mayOverflow = false;  // Smith-Waterman: a lane can reach the limit
};

// whether (and how) the batch kernels take a query of Q residues under this model
void planBatchQuery(const unsigned char* query, int Q, int open, int ext, const int* matrix, int A, int maxScore,
                    int minScore, int searchType, int mode, int64_t maxLen, BatchPlan* out) {
    BatchPlan& p = *out;
    p = BatchPlan{};
    if (Q < 1 || Q > kMaxStripRows || open < 0 || ext < 0 || maxScore > 16383 || minScore < -16383) return;
    const ScoreModel m{open, ext, maxScore, minScore};
    // (miopalSearch's range check for its 32-bit kernels: a query that fails it fails there)
    if (!int32Fits(int32Bound(m, Q, maxLen))) return;
    const int R = batchRowClass(Q);
    if (R == 0 || !interseqPairFits(R, A + 1) || minScore <= kBiasedPad) return;
    const bool locate = searchType != OPAL_SEARCH_SCORE;
    if (mode == OPAL_MODE_SW) {
        // (the row keys of the class's R rows)
        const int bits = rowKeyBits(R, locate);
        if (!biasedBandFits(m, bits, locate)) return;
        p.biasedLimit = biasedLimit(m, bits, locate);
        // (every residue aligned at most once, at best with its most favourable partner)
        const int64_t best = queryBest(Q, A, [&](int i, int t) { return matrix[query[i] * A + t]; });
        p.mayOverflow = std::min<int64_t>((int64_t)Q * std::max(maxScore, 0), best) >= p.biasedLimit;
    } else {
        // the single-query kernel's static bounds with the class's R rows (padding rows included): the padding
        // rows score -2 ext, which the room below zero covers as well
        if (!globalOneStripFits(m, R, mode == OPAL_MODE_NW, true)) return;
        p.biasedZero = (int)globalZeroPattern(m, R, true);
    }
    p.rows = R;
}

// Which rows of a chunk hold nothing: batchImpl's plan once more, for the sinks that select on a chunk's device rows
// (a query that is no member of its chunk takes the single-query path; its row is never read). skip[r] is set for
// the queries i0 + r, r < rows, that do; true if any is. `model`: the gaps and the matrix's extremes, found once per call.
bool skippedRows(const unsigned char* queries, const int64_t* queryOffsets, int64_t i0, int rows, const ScoreModel& model,
                 const int* matrix, int A, int searchType, int mode, int64_t maxLen, std::vector<int>* skip) {
    skip->assign((size_t)rows, 0);
    bool any = false;
    for (int r = 0; r < rows; ++r) {
        const int64_t i = i0 + r;
        BatchPlan plan;
        planBatchQuery(queries + queryOffsets[i], (int)(queryOffsets[i + 1] - queryOffsets[i]), model.open, model.ext, matrix,
                       A, model.maxScore, model.minScore, searchType, mode, maxLen, &plan);
        (*skip)[(size_t)r] = plan.rows == 0;
        any = any || plan.rows == 0;
    }
    return any;
}

}  // namespace

// the checks of miopalSearch, query by query (and the model and slice once when the list is empty)
static int validateBatch(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                         const int* matrix, int A, int searchType, int mode, int64_t start, int64_t end) {
    if (nQueries < 0 || (nQueries > 0 && (!queryOffsets || !queries)))
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad query list");
    if (nQueries == 0) RC_TRY(validate(db, nullptr, 0, matrix, A, searchType, mode, start, end));
    for (int i = 0; i < nQueries; ++i) {
        const int64_t len = queryOffsets[i + 1] - queryOffsets[i];
        if (queryOffsets[i] < 0 || len < 0 || len > INT32_MAX) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad query offsets at %d", i);
        RC_TRY(validate(db, queries + queryOffsets[i], (int)len, matrix, A, searchType, mode, start, end));
    }
    return 0;
}

// What a batch does with its answers: miopalSearchBatch downloads every chunk's [rows][n] rows,
// miopalSearchBatchTop selects the k best of each row on the device first (host_top.inc).
struct BatchSink {
    // the caller's output arrays, checked after the arguments and before any work
    std::function<int(bool locate)> checkOutputs;
    // the device rows [rows][n] of queries i0 .. i0 + rows - 1 are final (rows of queries on the single-query
    // path among them hold nothing: single() answers those afterwards)
    std::function<int(Workspace* ws, int64_t i0, int rows, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ)> chunk;
    // query i takes miopalSearch's own path
    std::function<int(int i)> single;
};

static int batchImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries, int open,
                     int ext, const int* matrix, int A, int searchType, int mode, int64_t start, int64_t end,
                     const BatchSink& sink) {
    for (int k = 0; k < 4; ++k) g_lastBatchRouting[k] = g_lastLaunchShape[k] = 0;
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchBatch: alignments are not available in a batch");
    RC_TRY(validateBatch(db, queries, queryOffsets, nQueries, matrix, A, searchType, mode, start, end));
    const int64_t n = end - start;
    if (n == 0 || nQueries == 0) return 0;
    const bool locate = searchType >= OPAL_SEARCH_SCORE_END;
    RC_TRY(sink.checkOutputs(locate));
    HIP_TRY(hipSetDevice(db->device));

    const int maxScore = *std::max_element(matrix, matrix + A * A);
    const int minScore = *std::min_element(matrix, matrix + A * A);
    std::vector<BatchPlan> plan((size_t)nQueries);
    std::vector<int> single;
    for (int i = 0; i < nQueries; ++i) {
        const int Q = (int)(queryOffsets[i + 1] - queryOffsets[i]);
        planBatchQuery(queries + queryOffsets[i], Q, open, ext, matrix, A, maxScore, minScore, searchType, mode, db->maxLen,
                       &plan[(size_t)i]);
        if (plan[(size_t)i].rows == 0) single.push_back(i);
    }
    int64_t settled = 0, pairJobs = 0, launches = 0;
    if ((int)single.size() < nQueries) {
        WorkspaceLease lease(db);
        RC_TRY(lease.acquireInternal());
        Workspace* ws = lease.ws;
        hipStream_t stream = ws->stream;
        DpRules r{};
        rulesForMode(mode, &r);   // (validateBatch has seen the mode)
        const int rules = packRules(r);
        const bool sw = mode == OPAL_MODE_SW;
        // small searches: the wavefront-per-pair kernel for every pair (what miopalSearch does for one query)
        const bool small = n <= kSmallSearch && smallSearchAllowed(db);
        std::shared_ptr<View> view;
        if (!small) RC_TRY(getView(db, start, end, 0, &view));
        const int nSym = A + 1;
        // (a small search's chunk is a job list: 48 bytes a pair)
        const int64_t chunkPairs = small ? kBatchChunkPairs / 8 : kBatchChunkPairs;
        const int64_t rowsPerChunk = std::max<int64_t>(1, std::min<int64_t>(nQueries, chunkPairs / n));
        for (int64_t i0 = 0; i0 < nQueries; i0 += rowsPerChunk) {
            const int i1 = (int)std::min<int64_t>(nQueries, i0 + rowsPerChunk);
            const int rows = i1 - (int)i0;
            // the chunk's batch queries, by row class
            std::vector<int> members;
            for (int i = (int)i0; i < i1; ++i)
                if (plan[(size_t)i].rows) members.push_back(i);
            if (members.empty()) continue;
            std::stable_sort(members.begin(), members.end(), [&](int x, int y) { return plan[(size_t)x].rows < plan[(size_t)y].rows; });
            // concatenated residues (the int32 kernel's jobs point into them)
            std::vector<unsigned char> concat;
            std::vector<int32_t> qOff((size_t)rows, 0);
            for (int i : members) {
                qOff[(size_t)(i - i0)] = (int32_t)concat.size();
                concat.insert(concat.end(), queries + queryOffsets[i], queries + queryOffsets[i + 1]);
            }
            void *ps, *pi = nullptr, *pj = nullptr;
            RC_TRY(ws->get(kScore, (size_t)rows * n * sizeof(int32_t), &ps));
            if (locate) {
                RC_TRY(ws->get(kEndI, (size_t)rows * n * sizeof(int32_t), &pi));
                RC_TRY(ws->get(kEndJ, (size_t)rows * n * sizeof(int32_t), &pj));
            }
            int32_t* d_score = (int32_t*)ps;
            int32_t *d_endI = (int32_t*)pi, *d_endJ = (int32_t*)pj;
            Search s{db, ws, stream, concat.data(), (int)concat.size(), open, ext, A, searchType, mode, matrix, start, end, n};
            std::vector<PairJob> jobs;
            auto pairJob = [&](int i, int32_t id) {
                PairJob j{};
                j.tOff = db->offsets[id];
                j.tLen = dbLen(db, id);
                j.tStep = 1;
                j.qOff = qOff[(size_t)(i - i0)];
                j.qLen = (int32_t)(queryOffsets[i + 1] - queryOffsets[i]);
                j.qStep = 1;
                j.rules = rules;
                j.out = (int32_t)((i - i0) * n + (id - start));
                jobs.push_back(j);
            };
            if (small || view->nGroups == 0) {
                for (int i : members)
                    for (int64_t id = start; id < end; ++id) pairJob(i, (int32_t)id);
            } else {
                // one launch per row class; profiles [query][nSym][R] of the whole chunk in one upload, the small
                // per-query arrays, run boundaries and counters in another
                std::vector<int16_t> prof;
                std::vector<int32_t> meta;
                struct Launch { int rows, first, count, unitsPerQuery; size_t profOff, lenOff, rowOff, unitOff, counterOff; bool mayOverflow; int limit, zero; };
                std::vector<Launch> ls;
                const int G = view->nGroups;
                std::vector<int64_t> prefix((size_t)G + 1, 0);
                for (int g = 0; g < G; ++g) prefix[(size_t)g + 1] = prefix[(size_t)g] + view->groupChunksHost[(size_t)g];
                for (size_t k = 0; k < members.size();) {
                    const int R = plan[(size_t)members[k]].rows;
                    size_t e = k;
                    Launch L{};
                    L.rows = R;
                    L.first = (int)k;
                    while (e < members.size() && plan[(size_t)members[e]].rows == R) {
                        L.mayOverflow = L.mayOverflow || plan[(size_t)members[e]].mayOverflow;
                        ++e;
                    }
                    L.count = (int)(e - k);
                    L.limit = plan[(size_t)members[k]].biasedLimit;
                    L.zero = 0;
                    for (size_t x = k; x < e; ++x) L.zero = std::max(L.zero, plan[(size_t)members[x]].biasedZero);
                    // Runs of groups per query: enough units to give every workgroup two with few queries, one per query
                    // with many; a run keeps at least one group per wavefront
                    const int waves = sw ? (R <= 56 ? 12 : 8) : (R <= 54 ? 12 : 8);   // (batchSwWaves, globalWaves)
                    const int64_t want = (2 * (int64_t)db->computeUnits + L.count - 1) / L.count;
                    L.unitsPerQuery = (int)std::max<int64_t>(1, std::min<int64_t>(want, G / waves));
                    L.profOff = prof.size();
                    for (size_t x = k; x < e; ++x) {
                        const int i = members[x];
                        const int Q = (int)(queryOffsets[i + 1] - queryOffsets[i]);
                        const unsigned char* q = queries + queryOffsets[i];
                        const size_t base = prof.size();
                        prof.resize(base + (size_t)nSym * R, (int16_t)kBiasedPad);
                        for (int t = 0; t < A; ++t)
                            for (int y = 0; y < Q; ++y) prof[base + (size_t)t * R + y] = (int16_t)matrix[q[y] * A + t];
                    }
                    L.lenOff = meta.size();
                    for (size_t x = k; x < e; ++x) meta.push_back((int32_t)(queryOffsets[members[x] + 1] - queryOffsets[members[x]]));
                    L.rowOff = meta.size();
                    for (size_t x = k; x < e; ++x) meta.push_back(members[x] - (int32_t)i0);
                    // (runs of equal work: the view is sorted longest group first)
                    L.unitOff = meta.size();
                    const int64_t total = prefix[(size_t)G];
                    int g = 0;
                    meta.push_back(0);
                    for (int u = 1; u < L.unitsPerQuery; ++u) {
                        const int64_t goal = total * u / L.unitsPerQuery;
                        while (g < G && prefix[(size_t)g] < goal) ++g;
                        meta.push_back(std::max(g, meta.back()));
                    }
                    meta.push_back(G);
                    L.counterOff = meta.size();
                    meta.push_back(0);
                    ls.push_back(L);
                    k = e;
                }
                const size_t countOff = meta.size();   // per row: flagged lane halves
                meta.resize(meta.size() + (size_t)rows, 0);
                void *pp, *pm, *po = nullptr;
                RC_TRY(ws->get(kBatchProfiles, prof.size() * sizeof(int16_t), &pp));
                RC_TRY(ws->get(kBatchMeta, meta.size() * sizeof(int32_t), &pm));
                if (sw) RC_TRY(ws->get(kBatchOverflow, (size_t)rows * view->nPacked, &po));
                RC_TRY(ws->stageUpload(pp, prof.data(), prof.size() * sizeof(int16_t), stream));
                RC_TRY(ws->stageUpload(pm, meta.data(), meta.size() * sizeof(int32_t), stream));
                int32_t* dm = (int32_t*)pm;
                bool anyOverflow = false;
                for (const Launch& L : ls) {
                    BatchArgs ba{};
                    ba.pack = view->d_pack;
                    ba.groupOff = view->d_groupOff;
                    ba.groupChunks = view->d_groupChunks;
                    ba.lens = view->d_lens;
                    ba.ids = view->d_ids;
                    ba.nPacked = view->nPacked;
                    ba.sliceStart = start;
                    ba.profiles = (const int16_t*)pp + L.profOff;
                    ba.nSymbols = nSym;
                    ba.qLens = dm + L.lenOff;
                    ba.qRows = dm + L.rowOff;
                    ba.nQueries = L.count;
                    ba.unitsPerQuery = L.unitsPerQuery;
                    ba.unitFirst = dm + L.unitOff;
                    ba.unitCounter = dm + L.counterOff;
                    ba.gapOpen = open;
                    ba.gapExt = ext;
                    ba.topGap = r.topGap;
                    ba.leftGap = r.leftGap;
                    ba.region = r.region;
                    ba.biasedLimit = L.limit;
                    ba.biasedZero = L.zero;
                    ba.outStride = n;
                    ba.score = d_score;
                    ba.endI = d_endI;
                    ba.endJ = d_endJ;
                    ba.overflow = (uint8_t*)po;
                    ba.overflowCount = dm + countOff;
                    // (the persistent launch's width follows "reserve_cus" like the single-query launches'; the units -
                    // L.unitsPerQuery - are cut for the whole device either way, and handed out dynamically)
                    int width = db->computeUnits;
                    if (const int keep = reservedCus(db); keep >= 0) width = std::max(1, width - keep);
                    const hipError_t e = sw ? (locate ? launchInterseqBatchSwLoc(ba, L.rows, width, stream)
                                                      : launchInterseqBatchSw(ba, L.rows, width, stream))
                                            : (L.rows <= 32 ? launchInterseqBatchGlobalA(ba, L.rows, width, stream)
                                                            : launchInterseqBatchGlobalB(ba, L.rows, width, stream));
                    // miopalLastLaunchShape: the batch's last launch (launchBatchSwR / launchBatchGlobalR)
                    g_lastLaunchShape[0] = db->computeUnits;
                    g_lastLaunchShape[1] = std::max(1, std::min(width, L.count * L.unitsPerQuery));
                    g_lastLaunchShape[2] = sw ? (L.rows <= 56 ? 12 : 8) : (L.rows <= 54 ? 12 : 8);   // (batchSwWaves, globalWaves)
                    g_lastLaunchShape[3] = 0;
                    if (e != hipSuccess) {
                        (void)hipGetLastError();
                        return fail(MIOPAL_ERR_HIP, "batch kernel launch (%d rows): %s", L.rows, hipGetErrorString(e));
                    }
                    ++launches;
                    settled += (int64_t)L.count * view->nPacked;
                    anyOverflow = anyOverflow || (sw && L.mayOverflow);
                }
                // pairs the lanes do not settle: targets kept out of the view, empty targets of NW / HW / OV (closed
                // forms of the border), flagged Smith-Waterman lanes
                for (int i : members)
                    for (int32_t id : view->longIds) pairJob(i, id);
                if (!sw) {
                    for (int e = view->nPacked - 1; e >= 0 && dbLen(db, view->ids[(size_t)e]) == 0; --e) {
                        for (int i : members) pairJob(i, view->ids[(size_t)e]);
                        settled -= (int64_t)members.size();
                    }
                }
                if (anyOverflow) {
                    std::vector<int32_t> counts((size_t)rows);
                    HIP_TRY(hipMemcpyAsync(counts.data(), dm + countOff, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
                    HIP_TRY(hipStreamSynchronize(stream));
                    std::vector<uint8_t> flags((size_t)view->nPacked);
                    for (int i : members) {
                        const int row = i - (int)i0;
                        if (counts[(size_t)row] == 0) continue;
                        HIP_TRY(hipMemcpy(flags.data(), (uint8_t*)po + (size_t)row * view->nPacked, flags.size(), hipMemcpyDeviceToHost));
                        for (int k = 0; k < view->nPacked; ++k)
                            if (flags[(size_t)k]) pairJob(i, view->ids[(size_t)k]);
                        settled -= counts[(size_t)row];
                    }
                }
            }
            pairJobs += (int64_t)jobs.size();
            RC_TRY(s.runPairs(jobs, false, d_score, d_endI, d_endJ, nullptr));
            RC_TRY(sink.chunk(ws, i0, rows, d_score, d_endI, d_endJ));
        }
    }
    // the other queries: miopalSearch's own path, query by query
    for (int i : single) RC_TRY(sink.single(i));
    g_lastBatchRouting[0] = settled;
    g_lastBatchRouting[1] = pairJobs;
    g_lastBatchRouting[2] = (int64_t)single.size();
    g_lastBatchRouting[3] = launches;
    return 0;
}

// miopalSearchBatch: every row of every chunk to the caller
static int searchBatchImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                           int open, int ext, const int* matrix, int A, int searchType, int mode, int64_t start,
                           int64_t end, int* score, int* endTarget, int* endQuery) {
    const int64_t n = end - start;
    BatchSink sink;
    sink.checkOutputs = [&](bool locate) -> int {
        if (!score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score output");
        if (locate && (!endTarget || !endQuery)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
        return 0;
    };
    sink.chunk = [&](Workspace* ws, int64_t i0, int rows, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ) -> int {
        // rows of this chunk -> the caller (rows of queries on the single-query path are written again afterwards)
        const size_t bytes = (size_t)rows * n * sizeof(int32_t);
        RC_TRY(ws->stageDownload(score + i0 * n, d_score, bytes));
        if (d_endI) {
            RC_TRY(ws->stageDownload(endQuery + i0 * n, d_endI, bytes));
            RC_TRY(ws->stageDownload(endTarget + i0 * n, d_endJ, bytes));
        }
        return ws->finishDownloads();
    };
    sink.single = [&](int i) -> int {
        const int64_t at = (int64_t)i * n;
        const bool locate = searchType >= OPAL_SEARCH_SCORE_END;
        return searchImpl(db, queries + queryOffsets[i], (int)(queryOffsets[i + 1] - queryOffsets[i]), open, ext, matrix,
                          A, searchType, mode, start, end, score + at, locate ? endTarget + at : nullptr,
                          locate ? endQuery + at : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    return batchImpl(db, queries, queryOffsets, nQueries, open, ext, matrix, A, searchType, mode, start, end, sink);
}
