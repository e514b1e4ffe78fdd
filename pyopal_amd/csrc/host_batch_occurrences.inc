// Part of host.hip (included there, not a translation unit of its own): miopalSearchBatchOccurrences - every
// occurrence of every query of a panel in each target of a slice, one CSR for the whole panel.
//
// Queries of 1 .. 64 rows take the panel kernels (occurrences_batch.hip), chunk by chunk (occurrences_batch.h: a chunk
// of queries keeps queries x targets within a bound): the slice's jobs built and sorted by length once, ONE count
// sweep for all the chunk's queries, occurrences.hip's scan over the chunk's [queries][targets] counts, one small
// download - every query's offset and the totals - then one write sweep over the listed (query, target) pairs alone
// and the download of the chunk's occurrences. Two host round trips per chunk, whatever the number of its queries.
// A query of more than 64 rows runs through searchOccurrencesImpl inside the same call (what miopalSearchBatch does
// with its long queries); an empty query has no occurrences. The pieces are spliced into the CSR at the end: nothing
// is written to the outputs before the last step that can fail.
//
// miopalSearchBatchOccurrencesAligned is the same call with an alignment stage behind every write sweep
// (host_batch_occurrence_align.inc for the panel chunks, host_occurrence_align.inc's for a long query): every piece
// then carries its occurrences' starts and operations, and the splice puts those together as well.
//
// miopalSearchPssmBatchOccurrences and its aligned form are the same calls with a list of position-specific scoring
// matrices where the queries and the matrix stand (PanelSide): their own checks, in the single PSSM calls' order, then
// the same routing, chunks, groups and splice. A chunk's PSSM rows go up once, end to end ([rows][A] ints, kPssmRows),
// with one int per TABLE row that names its source row (-1: a pad row) where the plain form uploads the residue list;
// the sweeps are occurrences_batch_pssm.hip's, the stage host_batch_occurrence_align_pssm.inc's. No matrix goes up.
static int checkOccurrenceAlignOutputs(int** startTarget, int** startQuery, unsigned char** alignments,
                                       int64_t** alignmentOffsets);   // (host.hip, with the entry points)

namespace {

thread_local int64_t g_lastBatchOccurrenceRouting[4] = {0, 0, 0, 0};   // miopalLastBatchOccurrenceRouting
thread_local int64_t g_lastBatchOccurrenceGroups[3] = {0, 0, 0};       // miopalLastBatchOccurrenceGroups

// queries of a chunk at most (every group holds at least one: the count sweep's grid has one row of workgroups per group)
constexpr int64_t kBatchOccurrenceChunkQueries = 32768;

// entries of a chunk's count array at most: occurrences_batch.h's bound, or what the switch asks for
int64_t batchOccurrenceEntries() {
    if (const char* v = tuned(Tune::BATCH_OCCURRENCE_ENTRIES)) {
        const long long asked = atoll(v);
        if (asked >= 1) return std::min<long long>(asked, int64_t(1) << 30);
    }
    return kBatchOccurrenceEntries;
}

// workgroups of the count sweep per compute unit that the groups are formed for (occurrences_batch.h), or what the
// switch asks for; 0: a group is never smaller than the LDS makes it
int64_t batchOccurrenceWorkgroupsPerCu() {
    if (const char* v = tuned(Tune::BATCH_OCCURRENCE_WORKGROUPS_PER_CU)) {
        const long long asked = atoll(v);
        if (asked >= 0) return std::min<long long>(asked, 1024);
    }
    return kBatchOccurrenceWorkgroupsPerCu;
}

// The score source of a panel. Plain: `residues` / `offsets` are the queries, `matrix` [A][A], rowScores null. PSSM:
// rowScores holds A ints per row, `offsets` delimits the PSSMs in rows, `residues` is the consensus (never null here:
// a filler of 255s where the caller gave none) in the same row coordinates; matrix is null.
struct PanelSide {
    const unsigned char* residues;
    const int64_t* offsets;
    const int* matrix;
    const int* rowScores;
    bool pssm() const { return rowScores != nullptr; }
};

// where a query's occurrences lie until the CSR is put together; aligned (the aligned call): the starts of the piece
// `from`, entry for entry, and its operations - those of the stretch are opsOff[first] .. opsOff[first + count]
struct OccurrenceStretch {
    const HitArrays* from = nullptr;
    int64_t first = 0, count = 0;
    const OccurrenceAlignment* aligned = nullptr;
};

// the aligned call: whether operations are asked for, and where the pieces' alignments are kept until the splice
struct BatchOccurrenceAlign {
    bool operations;
    std::vector<std::unique_ptr<OccurrenceAlignment>> pieces;
};

}  // namespace

// The panel queries `panel` (indices into the call's list, ascending, 1 .. 64 rows each), chunk by chunk. counts[i]
// and stretch[i] are filled for every one of them; once *running passes maxHits (*over) the chunks are only counted.
// `align` (null: the plain call): the alignment stage runs behind every write sweep, and never once *over is set.
static int batchOccurrencePanel(MiopalDb* db, const PanelSide& side,
                                const std::vector<int>& panel, int open, int ext, int A, int mode,
                                int64_t start, int64_t end, const int* minScore, const int* window, int64_t maxHits,
                                int64_t* running, bool* over, std::vector<int64_t>* counts,
                                std::vector<OccurrenceStretch>* stretch, std::vector<std::unique_ptr<HitArrays>>* pieces,
                                BatchOccurrenceAlign* align) {
    const int64_t n = end - start;
    const int region = mode == OPAL_MODE_HW ? kLastRow : kAllCells;
    const int64_t maxL = db->maxLen;
    HIP_TRY(hipSetDevice(db->device));
    WorkspaceLease lease(db);
    RC_TRY(lease.acquireInternal());
    Workspace* ws = lease.ws;
    hipStream_t stream = ws->stream;
    const unsigned char* const queries = side.residues;
    const int64_t* const queryOffsets = side.offsets;
    const bool pssm = side.pssm();
    void* pmatrix = nullptr;
    if (!pssm) {
        RC_TRY(ws->get(kMatrix, (size_t)A * A * sizeof(int32_t), &pmatrix));
        RC_TRY(ws->stageUpload(pmatrix, side.matrix, (size_t)A * A * sizeof(int32_t), stream));
    }

    const int64_t perChunk = std::max<int64_t>(1, std::min<int64_t>(kBatchOccurrenceChunkQueries, batchOccurrenceEntries() / n));
    // A group is as many consecutive queries as fit the LDS - unless that leaves the count sweep fewer than
    // kBatchOccurrenceWorkgroupsPerCu workgroups per compute unit: then the queries are spread over more, smaller
    // groups, down to one query a group (occurrences_batch.h: what that rests on). Few targets: the panel fills the GPU
    // side by side. Many: the launch ends evenly.
    const int64_t targetBlocks = (std::min<int64_t>(n, kPairChunkMax) + 255) / 256;
    const int64_t perCu = batchOccurrenceWorkgroupsPerCu();
    const int64_t wantGroups = std::max<int64_t>(1, (perCu * (int64_t)std::max(db->computeUnits, 1) + targetBlocks - 1) / targetBlocks);
    int64_t jobsOf = -1;   // the chunk of targets whose sorted jobs kSortedJobs holds
    void* psorted = nullptr;
    for (size_t p0 = 0; p0 < panel.size(); p0 += (size_t)perChunk) {
        const int cq = (int)std::min<int64_t>(perChunk, (int64_t)(panel.size() - p0));
        const int64_t N = (int64_t)cq * n;
        // the chunk's row list, its queries and its groups
        // (PSSM panel: the chunk's rows end to end, unpadded, and per table row the row it holds)
        std::vector<uint8_t> rowResidue;
        std::vector<int32_t> rowSource;
        std::vector<int> chunkRows;
        std::vector<int4> meta;   // [cq] queries, then the groups
        meta.reserve((size_t)cq + 16);
        int tallest = 0;
        for (int q = 0; q < cq; ++q) {
            const int i = panel[p0 + (size_t)q];
            const int Q = (int)(queryOffsets[i + 1] - queryOffsets[i]);
            const size_t pad = (size_t)(batchOccurrenceRows(Q) - Q);
            if (pssm) {
                meta.push_back(make_int4((int)rowSource.size(), Q, minScore[i], window[i]));
                const int32_t origin = (int32_t)(chunkRows.size() / (size_t)A);
                for (int r = 0; r < Q; ++r) rowSource.push_back(origin + r);
                rowSource.resize(rowSource.size() + pad, -1);
                chunkRows.insert(chunkRows.end(), side.rowScores + (size_t)queryOffsets[i] * A,
                                 side.rowScores + (size_t)queryOffsets[i + 1] * A);
            } else {
                meta.push_back(make_int4((int)rowResidue.size(), Q, minScore[i], window[i]));
                rowResidue.insert(rowResidue.end(), queries + queryOffsets[i], queries + queryOffsets[i + 1]);
                rowResidue.resize(rowResidue.size() + pad, (uint8_t)kBatchOccurrencePadRow);
            }
            tallest = std::max(tallest, batchOccurrenceRows(Q));
        }
        const int64_t perGroup = std::max<int64_t>(1, (cq + wantGroups - 1) / wantGroups);
        int groups = 0;
        int64_t widest = 0;
        for (int q = 0; q < cq;) {
            int e = q;
            int64_t rows = 0;
            while (e < cq && e - q < perGroup &&
                   batchOccurrenceLdsBytes(rows + batchOccurrenceRows(meta[(size_t)e].y), A) <= kCuLdsBytes) {
                rows += batchOccurrenceRows(meta[(size_t)e].y);
                ++e;
            }
            meta.push_back(make_int4(q, e - q, meta[(size_t)q].x, (int)rows));
            g_lastBatchOccurrenceGroups[1] = std::max<int64_t>(g_lastBatchOccurrenceGroups[1], e - q);
            widest = std::max(widest, rows);
            ++groups;
            q = e;
        }
        g_lastBatchOccurrenceGroups[0] += groups;
        g_lastBatchOccurrenceGroups[2] = std::max<int64_t>(g_lastBatchOccurrenceGroups[2], (int64_t)batchOccurrenceLdsBytes(widest, A));
        void *prows, *pmeta, *pbounds, *pscratch, *pscores = nullptr;
        if (pssm) {
            RC_TRY(ws->get(kBatchOccurrenceRowSource, rowSource.size() * sizeof(int32_t), &prows));
            RC_TRY(ws->get(kPssmRows, chunkRows.size() * sizeof(int32_t), &pscores));
        } else {
            RC_TRY(ws->get(kQuery, rowResidue.size(), &prows));
        }
        RC_TRY(ws->get(kBatchOccurrenceMeta, meta.size() * sizeof(int4), &pmeta));
        RC_TRY(ws->get(kBatchOccurrenceBounds, ((size_t)cq + 3) * sizeof(int64_t) + ((size_t)cq + 1) * sizeof(int32_t), &pbounds));
        RC_TRY(ws->get(kOccurrenceScratch, occurrenceScratchBytes(N), &pscratch));
        if (pssm) {
            RC_TRY(ws->stageUpload(prows, rowSource.data(), rowSource.size() * sizeof(int32_t), stream));
            RC_TRY(ws->stageUpload(pscores, chunkRows.data(), chunkRows.size() * sizeof(int32_t), stream));
        } else {
            RC_TRY(ws->stageUpload(prows, rowResidue.data(), rowResidue.size(), stream));
        }
        RC_TRY(ws->stageUpload(pmeta, meta.data(), meta.size() * sizeof(int4), stream));
        const OccurrenceScratch sc = occurrenceScratchLayout(pscratch, N);
        int64_t* dHead = (int64_t*)pbounds;
        int32_t* dFirst = (int32_t*)(dHead + cq + 3);
        BatchOccurrenceArgs a{};
        a.residues = db->d_residues;
        if (pssm) a.rowSource = (const int32_t*)prows;
        else a.rowResidue = (const uint8_t*)prows;
        a.query = (const int4*)pmeta;
        a.group = a.query + cq;
        a.nQueries = cq;
        if (pssm) a.rows = (const int32_t*)pscores;
        else a.matrix = (const int32_t*)pmatrix;
        a.alphabet = A;
        a.gapOpen = open;
        a.gapExt = ext;
        a.n = n;
        a.count = sc.count;
        a.start = start;
        // the count sweep: every target of the slice, in chunks of jobs sorted by length
        for (int64_t c0 = 0; c0 < n; c0 += kPairChunkMax) {
            const int nc = (int)std::min<int64_t>(kPairChunkMax, n - c0);
            if (jobsOf != c0) {
                void *pjobs, *pbins;
                RC_TRY(ws->get(kJobs, (size_t)nc * sizeof(PairJob), &pjobs));
                RC_TRY(ws->get(kSortedJobs, (size_t)nc * sizeof(PairJob), &psorted));
                RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
                HIP_TRY(launchOccurrenceJobs(nullptr, c0, nc, start, db->d_offsets, 0, (PairJob*)pjobs, stream));
                HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, nc, (int)maxL, (int*)pbins, (PairJob*)psorted, stream));
                jobsOf = c0;
            }
            a.jobs = (const PairJob*)psorted;
            a.nJobs = nc;
            const hipError_t e = (pssm ? launchBatchOccurrencesCountPssm : launchBatchOccurrencesCount)(
                a, region, groups, batchOccurrenceLdsBytes(widest, A), stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(MIOPAL_ERR_HIP, "panel occurrence sweep launch (count): %s", hipGetErrorString(e));
            }
        }
        {
            hipError_t e = launchOccurrencesOffsets(sc, N, stream);
            if (e == hipSuccess) e = launchBatchOccurrencesBounds(sc, n, cq, dFirst, dHead, stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(MIOPAL_ERR_HIP, "panel occurrence offsets launch: %s", hipGetErrorString(e));
            }
        }
        std::vector<int64_t> head((size_t)cq + 3, 0);
        RC_TRY(ws->stageDownload(head.data(), dHead, sizeof(int64_t) * head.size()));
        RC_TRY(ws->finishDownloads());
        const int64_t total = head[(size_t)cq + 1], listed = head[(size_t)cq + 2];
        bool sane = head[0] == 0 && head[(size_t)cq] == total && total >= 0 && listed >= 0 && listed <= N && listed <= total;
        for (int q = 0; q < cq && sane; ++q) sane = head[(size_t)q + 1] >= head[(size_t)q];
        if (!sane) return fail(MIOPAL_ERR_INTERNAL, "panel occurrence counts: total %lld in %lld pairs", (long long)total, (long long)listed);
        g_lastBatchOccurrenceRouting[2] += 1;
        *running += total;
        if (maxHits >= 0 && *running > maxHits) *over = true;
        for (int q = 0; q < cq; ++q) (*counts)[(size_t)panel[p0 + (size_t)q]] = head[(size_t)q + 1] - head[(size_t)q];
        if (*over || total == 0) continue;
        // the write sweep over the listed pairs, and the chunk's occurrences
        pieces->emplace_back(new HitArrays());
        HitArrays& hits = *pieces->back();
        RC_TRY(hits.alloc(total, true));
        const HitsOutSlot slot(total, true);
        void* po;
        RC_TRY(ws->get(kOccurrenceOut, slot.bytes, &po));
        char* base = (char*)po;
        a.count = nullptr;
        a.offsets = sc.offsets;
        a.list = sc.list;
        a.first = dFirst;
        a.dbOffsets = db->d_offsets;
        a.outTarget = (int64_t*)base;
        a.outScore = (int32_t*)(base + slot.offScore);
        a.outRow = (int32_t*)(base + slot.offEndQ);
        a.outColumn = (int32_t*)(base + slot.offEndT);
        {
            const hipError_t e = (pssm ? launchBatchOccurrencesWritePssm : launchBatchOccurrencesWrite)(
                a, region, listed, batchOccurrenceLdsBytes(tallest, A), stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(MIOPAL_ERR_HIP, "panel occurrence sweep launch (write): %s", hipGetErrorString(e));
            }
        }
        g_lastBatchOccurrenceRouting[3] += listed;
        RC_TRY(ws->stageDownload(hits.target, a.outTarget, sizeof(int64_t) * (size_t)total));
        RC_TRY(ws->stageDownload(hits.score, a.outScore, sizeof(int) * (size_t)total));
        RC_TRY(ws->stageDownload(hits.endQ, a.outRow, sizeof(int) * (size_t)total));
        RC_TRY(ws->stageDownload(hits.endT, a.outColumn, sizeof(int) * (size_t)total));
        RC_TRY(ws->finishDownloads());
        const OccurrenceAlignment* aligned = nullptr;
        if (align) {
            // the stage, on the occurrences where they are (head[0 .. cq] still lies behind dHead). It takes kJobs,
            // kSortedJobs and kSortBins: the next chunk's count sweep builds the slice's sorted jobs again.
            align->pieces.emplace_back(new OccurrenceAlignment());
            // (PSSM panel: the chunk's rows stay where they are, kPssmRows, and the stage reads them there)
            const BatchOccurrencesOnDevice on{db, ws, queries, queryOffsets, panel.data() + p0, cq, open, ext, side.matrix, A,
                                              mode, total, a.outTarget, a.outScore, a.outRow, a.outColumn, dHead, &hits,
                                              side.rowScores, (const int32_t*)pscores, head.data()};
            RC_TRY((pssm ? alignPssmBatchOccurrencesStage : alignBatchOccurrencesStage)(on, align->operations,
                                                                                        align->pieces.back().get()));
            aligned = align->pieces.back().get();
            jobsOf = -1;
            psorted = nullptr;
        }
        for (int q = 0; q < cq; ++q)
            (*stretch)[(size_t)panel[p0 + (size_t)q]] =
                OccurrenceStretch{&hits, head[(size_t)q], head[(size_t)q + 1] - head[(size_t)q], aligned};
    }
    return 0;
}

static int batchOccurrencesCore(MiopalDb* db, const PanelSide& side, int nQueries, int open, int ext, int A, int mode,
                                int64_t start, int64_t end, const int* minScore, const int* window, int64_t maxHits,
                                int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget, int** endQuery,
                                bool wantAligned, int** startTarget, int** startQuery, unsigned char** alignments,
                                int64_t** alignmentOffsets);

// what the reporters of the panel occurrence searches say starts over with every call, plain or PSSM
static void resetBatchOccurrenceReports(bool wantAligned) {
    for (int k = 0; k < 4; ++k) g_lastBatchOccurrenceRouting[k] = 0;
    for (int k = 0; k < 3; ++k) g_lastBatchOccurrenceGroups[k] = 0;
    if (wantAligned)
        for (int k = 0; k < 4; ++k) g_lastBatchOccurrenceAlignRouting[k] = 0;
}

// Behind nothing: the checks of miopalSearchOccurrences over the whole list, in its order, come first.
// wantAligned: miopalSearchBatchOccurrencesAligned - the four outputs behind endQuery are checked and written too.
static int searchBatchOccurrencesImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                                      int open, int ext, const int* matrix, int A, int mode, int64_t start, int64_t end,
                                      const int* minScore, const int* window, int64_t maxHits, int64_t* hitOffsets,
                                      int64_t** targetIndex, int** score, int** endTarget, int** endQuery,
                                      bool wantAligned = false, int** startTarget = nullptr, int** startQuery = nullptr,
                                      unsigned char** alignments = nullptr, int64_t** alignmentOffsets = nullptr) {
    resetBatchOccurrenceReports(wantAligned);
    RC_TRY(validateBatch(db, queries, queryOffsets, nQueries, matrix, A, OPAL_SEARCH_SCORE_END, mode, start, end));
    if (mode != OPAL_MODE_HW && mode != OPAL_MODE_SW)
        return fail(OPAL_ERR_INVALID_MODE, "occurrences are defined for OPAL_MODE_HW and OPAL_MODE_SW, not for mode %d", mode);
    if (window)
        for (int i = 0; i < nQueries; ++i)
            if (window[i] < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative window %d at query %d", window[i], i);
    if (minScore && mode == OPAL_MODE_SW)
        for (int i = 0; i < nQueries; ++i)
            if (minScore[i] < 1)
                return fail(MIOPAL_ERR_BAD_ARGUMENT, "minScore = %d at query %d: OPAL_MODE_SW needs a cut of at least 1", minScore[i], i);
    if (nQueries > 0 && (!minScore || !window)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null minScore / window list");
    RC_TRY(checkHitsOutputs(OPAL_SEARCH_SCORE_END, hitOffsets, targetIndex, score, endTarget, endQuery));
    if (wantAligned) RC_TRY(checkOccurrenceAlignOutputs(startTarget, startQuery, alignments, alignmentOffsets));
    return batchOccurrencesCore(db, PanelSide{queries, queryOffsets, matrix, nullptr}, nQueries, open, ext, A, mode, start, end,
                                minScore, window, maxHits, hitOffsets, targetIndex, score, endTarget, endQuery, wantAligned,
                                startTarget, startQuery, alignments, alignmentOffsets);
}

// miopalSearchPssmBatchOccurrences(Aligned): what needs no handle first, in the single PSSM calls' order with the plain
// panel's per-query checks among it, then the handle and what depends on it; the range check of every PSSM, with the
// extreme entries of its own rows, is the core's.
static int searchPssmBatchOccurrencesImpl(MiopalDb* db, const int* rowScores, const unsigned char* consensus,
                                          const int64_t* rowOffsets, int nPssms, int open, int ext, int A, int mode,
                                          int64_t start, int64_t end, const int* minScore, const int* window, int64_t maxHits,
                                          int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget,
                                          int** endQuery, bool wantAligned, int** startTarget, int** startQuery,
                                          unsigned char** alignments, int64_t** alignmentOffsets) {
    resetBatchOccurrenceReports(wantAligned);
    if (mode < OPAL_MODE_NW || mode > OPAL_MODE_SW) return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", mode);
    if (mode != OPAL_MODE_HW && mode != OPAL_MODE_SW)
        return fail(OPAL_ERR_INVALID_MODE, "occurrences are defined for OPAL_MODE_HW and OPAL_MODE_SW, not for mode %d", mode);
    if (nPssms < 0 || (nPssms > 0 && !rowOffsets)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad PSSM list");
    for (int m = 0; m < nPssms; ++m)
        if (rowOffsets[m] < 0 || rowOffsets[m + 1] < rowOffsets[m]) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad row offsets at %d", m);
    const int64_t first = nPssms > 0 ? rowOffsets[0] : 0, totalRows = nPssms > 0 ? rowOffsets[nPssms] - first : 0;
    if (totalRows > INT32_MAX - 64) return fail(MIOPAL_ERR_BAD_ARGUMENT, "the PSSMs of a panel hold 2^31 - 65 rows at most");
    if (totalRows > 0 && !rowScores) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null row scores");
    if (A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad alphabet length %d", A);
    if (window)
        for (int i = 0; i < nPssms; ++i)
            if (window[i] < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative window %d at PSSM %d", window[i], i);
    if (minScore && mode == OPAL_MODE_SW)
        for (int i = 0; i < nPssms; ++i)
            if (minScore[i] < 1)
                return fail(MIOPAL_ERR_BAD_ARGUMENT, "minScore = %d at PSSM %d: OPAL_MODE_SW needs a cut of at least 1", minScore[i], i);
    if (nPssms > 0 && (!minScore || !window)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null minScore / window list");
    RC_TRY(checkHitsOutputs(OPAL_SEARCH_SCORE_END, hitOffsets, targetIndex, score, endTarget, endQuery));
    if (wantAligned) {
        RC_TRY(checkOccurrenceAlignOutputs(startTarget, startQuery, alignments, alignmentOffsets));
        if (alignments && totalRows > 0 && !consensus) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null consensus for an alignment search");
        if (consensus)
            for (int64_t i = first; i < first + totalRows; ++i)
                if (consensus[i] >= A && consensus[i] != 255)
                    return fail(MIOPAL_ERR_BAD_ARGUMENT, "consensus residue %d out of range at %lld", consensus[i], (long long)i);
    }
    // (a PSSM of more than 64 rows takes the single sweep, which keeps its rows in LDS)
    for (int i = 0; i < nPssms; ++i) {
        const int64_t Q = rowOffsets[i + 1] - rowOffsets[i];
        if (Q > kLanes && (Q > INT32_MAX || perPairPssmBytes((int)Q, A) == 0))
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "PSSM %d of the panel: a PSSM of %lld rows at %d letters does not fit the occurrence "
                        "sweep's LDS table: (rows + 1) x (letters + 1) x 4 bytes within 64 KB less 256, %d rows at most", i,
                        (long long)Q, A, (64 * 1024 - 256) / (4 * (A + 1)) - 1);
    }
    if (!db) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null database handle");
    if (A != db->alphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d differs from the database's %d", A, db->alphabet);
    if (start < 0 || end < start || end > db->count) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad slice [%lld, %lld)", (long long)start, (long long)end);
    // (without a consensus - the plain form, starts only - every position is "no residue": the kernels never read it)
    std::vector<unsigned char> none;
    if (!wantAligned || !consensus) {
        none.assign((size_t)(first + std::max<int64_t>(totalRows, 1)), 255);   // (indexed in the offsets' coordinates)
        consensus = none.data();
    }
    static const int64_t kNoPssms[1] = {0};
    static const int kNoPanelRows[1] = {0};   // (no rows: the score source still says "position-specific")
    return batchOccurrencesCore(db, PanelSide{consensus, nPssms > 0 ? rowOffsets : kNoPssms, nullptr, totalRows > 0 ? rowScores : kNoPanelRows},
                                nPssms, open, ext, A, mode, start, end, minScore, window, maxHits, hitOffsets, targetIndex, score,
                                endTarget, endQuery, wantAligned, startTarget, startQuery, alignments, alignmentOffsets);
}

// Behind the checks of either form: the range check of every query, the routing, the pieces and the splice.
static int batchOccurrencesCore(MiopalDb* db, const PanelSide& side, int nQueries, int open, int ext, int A, int mode,
                                int64_t start, int64_t end, const int* minScore, const int* window, int64_t maxHits,
                                int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget, int** endQuery,
                                bool wantAligned, int** startTarget, int** startQuery, unsigned char** alignments,
                                int64_t** alignmentOffsets) {
    const unsigned char* const queries = side.residues;
    const int64_t* const queryOffsets = side.offsets;
    const int* const matrix = side.matrix;
    const bool operations = wantAligned && alignments != nullptr;
    BatchOccurrenceAlign alignState{operations, {}};
    BatchOccurrenceAlign* const align = wantAligned ? &alignState : nullptr;
    const int64_t n = end - start;
    std::vector<int64_t> counts((size_t)nQueries, 0);
    std::vector<OccurrenceStretch> stretch((size_t)nQueries);
    std::vector<std::unique_ptr<HitArrays>> pieces;
    int64_t running = 0;
    bool over = false;
    if (n > 0 && nQueries > 0) {
        // miopalSearch's range check (32-bit arithmetic only), for every query before any device work (a PSSM: with
        // the extreme entries of its own rows)
        ScoreModel model{open, ext, 0, 0};
        if (!side.pssm()) scoreExtremes(matrix, (size_t)A * A, &model.maxScore, &model.minScore);
        std::vector<int> panel, single;
        for (int i = 0; i < nQueries; ++i) {
            const int Q = (int)(queryOffsets[i + 1] - queryOffsets[i]);
            if (side.pssm()) RC_TRY(checkPssmRange(db, side.rowScores + (size_t)queryOffsets[i] * A, Q, A, open, ext));
            else RC_TRY(checkInt32Range(model, Q, db->maxLen));
            if (Q > kLanes) single.push_back(i);
            else if (Q > 0) panel.push_back(i);
        }
        g_lastBatchOccurrenceRouting[0] = (int64_t)panel.size();
        g_lastBatchOccurrenceRouting[1] = (int64_t)single.size();
        // The long queries: the single-query search, its refusals (the strip workspace) what they are. What
        // miopalLastOccurrenceRouting reports belongs to the thread's last single-query CALL: it is put back behind them.
        // Once the bound is passed (`over`) the later ones still run their count sweeps, with no room: hitOffsets is
        // filled for every query also when there are too many hits, and nothing is written or downloaded for them.
        int64_t singleRouting[4];
        for (int k = 0; k < 4; ++k) singleRouting[k] = g_lastOccurrenceRouting[k];
        // (the same for what miopalLastOccurrenceAlignRouting reports, which a long query's stage counts in)
        int64_t singleAlignRouting[4];
        for (int k = 0; k < 4; ++k) singleAlignRouting[k] = g_lastOccurrenceAlignRouting[k];
        struct PutBack {
            const int64_t *saved, *savedAlign;
            ~PutBack() {
                for (int k = 0; k < 4; ++k) g_lastOccurrenceRouting[k] = saved[k];
                for (int k = 0; k < 4; ++k) g_lastOccurrenceAlignRouting[k] = savedAlign[k];
            }
        } putBack{singleRouting, singleAlignRouting};
        for (int i : single) {
            int64_t found = 0;
            const int64_t room = over ? 0 : maxHits < 0 ? -1 : maxHits - running;
            pieces.emplace_back(new HitArrays());
            HitArrays& hits = *pieces.back();
            // (aligned: the single-query stage behind its write sweep - it does not run when the bound is passed)
            OccurrenceAlignment* got = nullptr;
            if (align) {
                align->pieces.emplace_back(new OccurrenceAlignment());
                got = align->pieces.back().get();
                for (int k = 0; k < 4; ++k) g_lastOccurrenceAlignRouting[k] = 0;
            }
            const OccurrenceStage stage = [&](const OccurrencesOnDevice& o) { return alignOccurrencesStage(o, operations, got); };
            const int rc = searchOccurrencesImpl(db, queries + queryOffsets[i], (int)(queryOffsets[i + 1] - queryOffsets[i]), open,
                                                 ext, matrix, side.pssm() ? side.rowScores + (size_t)queryOffsets[i] * A : nullptr, A,
                                                 mode, start, end, minScore[i], window[i], room, &found,
                                                 &hits.target, &hits.score, &hits.endT, &hits.endQ, align ? &stage : nullptr);
            if (rc == MIOPAL_ERR_TOO_MANY_HITS) over = true;
            else if (rc) return rc;
            if (align) {
                for (int k = 0; k < 3; ++k) g_lastBatchOccurrenceAlignRouting[k] += g_lastOccurrenceAlignRouting[k];
                g_lastBatchOccurrenceAlignRouting[3] = std::max(g_lastBatchOccurrenceAlignRouting[3], g_lastOccurrenceAlignRouting[3]);
            }
            counts[(size_t)i] = found;
            running += found;
            if (!over) stretch[(size_t)i] = OccurrenceStretch{&hits, 0, found, found > 0 ? got : nullptr};
        }
        if (!panel.empty() && db->maxLen > 0)
            RC_TRY(batchOccurrencePanel(db, side, panel, open, ext, A, mode, start, end, minScore, window,
                                        maxHits, &running, &over, &counts, &stretch, &pieces, align));
    }
    HitArrays all;
    if (!over) RC_TRY(all.alloc(running, true));
    // (aligned: the starts, the rebased offsets - the single 0 without occurrences - and room for the operations)
    OccurrenceAlignment joined;
    if (align && !over) {
        if (running > 0) {
            joined.startT = (int*)malloc(sizeof(int) * (size_t)running);
            joined.startQ = (int*)malloc(sizeof(int) * (size_t)running);
            if (!joined.startT || !joined.startQ) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        }
        if (operations) {
            joined.opsOff = (int64_t*)malloc(sizeof(int64_t) * (size_t)(running + 1));
            if (!joined.opsOff) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
            joined.opsOff[0] = 0;
            int64_t at = 0, nOps = 0;
            for (int i = 0; i < nQueries; ++i) {
                const OccurrenceStretch& s = stretch[(size_t)i];
                for (int64_t k = 0; k < s.count; ++k, ++at) {
                    nOps += s.aligned->opsOff[s.first + k + 1] - s.aligned->opsOff[s.first + k];
                    joined.opsOff[at + 1] = nOps;
                }
            }
            if (at != running) return fail(MIOPAL_ERR_INTERNAL, "panel occurrence stretches hold %lld of %lld", (long long)at, (long long)running);
            if (running > 0 && !joined.ops.resize((size_t)nOps)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        }
    }
    // nothing failed: the outputs are written from here on
    hitOffsets[0] = 0;
    for (int i = 0; i < nQueries; ++i) hitOffsets[i + 1] = hitOffsets[i] + counts[(size_t)i];
    if (over) return fail(MIOPAL_ERR_TOO_MANY_HITS, "%lld occurrences, maxHits = %lld", (long long)running, (long long)maxHits);
    for (int i = 0; i < nQueries; ++i) {
        const OccurrenceStretch& s = stretch[(size_t)i];
        if (s.count == 0) continue;
        const size_t at = (size_t)hitOffsets[i], len = (size_t)s.count;
        memcpy(all.target + at, s.from->target + s.first, sizeof(int64_t) * len);
        memcpy(all.score + at, s.from->score + s.first, sizeof(int) * len);
        memcpy(all.endT + at, s.from->endT + s.first, sizeof(int) * len);
        memcpy(all.endQ + at, s.from->endQ + s.first, sizeof(int) * len);
        if (!align) continue;
        memcpy(joined.startT + at, s.aligned->startT + s.first, sizeof(int) * len);
        memcpy(joined.startQ + at, s.aligned->startQ + s.first, sizeof(int) * len);
        if (operations)
            memcpy(joined.ops.data + joined.opsOff[at], s.aligned->ops.data + s.aligned->opsOff[s.first],
                   (size_t)(joined.opsOff[at + len] - joined.opsOff[at]));
    }
    all.release(targetIndex, score, endTarget, endQuery);
    if (align) {
        *startTarget = joined.startT;
        *startQuery = joined.startQ;
        joined.startT = joined.startQ = nullptr;
        if (operations) {
            *alignments = joined.ops.release();
            *alignmentOffsets = joined.opsOff;
            joined.opsOff = nullptr;
        }
    }
    return 0;
}
