// Part of host.hip (included there, not a translation unit of its own): miopalSearchHits, miopalSearchPssmHits and
// miopalSearchBatchHits - every target of a query (of every query of a batch) that scores at least minScore,
// compacted on the device (select_hits.hip) from the score rows the search kernels leave in HBM. The size of the
// answer is decided on the device: the host reads the per-row offsets, sizes the outputs to the total and only then
// has the hits written. Two host round trips per selection; only the hits cross PCIe.

// The malloc'ed arrays of an answer (the caller of the C ABI frees them); null while there are no hits
struct HitArrays {
    int64_t* target = nullptr;
    int *score = nullptr, *endT = nullptr, *endQ = nullptr;
    HitArrays() = default;
    HitArrays(const HitArrays&) = delete;
    HitArrays& operator=(const HitArrays&) = delete;
    ~HitArrays() {
        free(target);
        free(score);
        free(endT);
        free(endQ);
    }
    int alloc(int64_t total, bool ends) {
        if (total <= 0) return 0;
        target = (int64_t*)malloc(sizeof(int64_t) * (size_t)total);
        score = (int*)malloc(sizeof(int) * (size_t)total);
        if (ends) {
            endT = (int*)malloc(sizeof(int) * (size_t)total);
            endQ = (int*)malloc(sizeof(int) * (size_t)total);
        }
        if (!target || !score || (ends && (!endT || !endQ))) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        return 0;
    }
    // the arrays change hands
    void release(int64_t** t, int** s, int** et, int** eq) {
        *t = target;
        *s = score;
        if (et) *et = endT;
        if (eq) *eq = endQ;
        target = nullptr;
        score = endT = endQ = nullptr;
    }
};

// What a selection leaves on the host: rowOffset[rows + 1] always; the hits themselves when they fit the room
struct HitRows {
    std::vector<int64_t> rowOffset{0};
    bool written = true;   // false: more hits than the room - counted, not written
    HitArrays hits;
    int64_t total() const { return rowOffset.back(); }
};

// The answer of a batch, collected piece by piece and put together as a CSR at the end (miopalSearchBatchHits,
// miopalSearchBatchSignificant). Chunks and single-path queries arrive out of query order: one piece per chunk (queries
// [first, first + rows)) or per single-path query (rows = 1), with one E-value per hit beside it in the significant form.
struct HitPieces {
    struct Piece {
        int64_t first;
        std::unique_ptr<HitRows> rows;
        std::vector<double> ev;
    };
    std::vector<Piece> pieces;
    std::vector<int64_t> counts;   // hits per query
    int64_t maxHits, running = 0;
    bool over = false;
    HitArrays all;
    double* allEv = nullptr;
    HitPieces(int nQueries, int64_t maxHits_) : counts((size_t)nQueries, 0), maxHits(maxHits_) {}
    HitPieces(const HitPieces&) = delete;
    HitPieces& operator=(const HitPieces&) = delete;
    ~HitPieces() { free(allEv); }
    // the room left for a piece; once the bound is passed the later pieces are only counted
    int64_t room() const { return over ? 0 : maxHits < 0 ? -1 : maxHits - running; }
    void take(int64_t first, std::unique_ptr<HitRows> got, std::vector<double> ev = {}) {
        const int nr = (int)got->rowOffset.size() - 1;
        for (int r = 0; r < nr; ++r) counts[(size_t)(first + r)] += got->rowOffset[(size_t)r + 1] - got->rowOffset[(size_t)r];
        running += got->total();
        if (!got->written) over = true;
        pieces.push_back(Piece{first, std::move(got), std::move(ev)});
    }
    // the arrays of the whole answer (none once the bound is passed): the one step of the end that can fail, made
    // before any output is touched
    int reserve(bool locate, bool withEvalues) {
        if (over) return 0;
        RC_TRY(all.alloc(running, locate));
        if (withEvalues && running > 0) {
            allEv = (double*)malloc(sizeof(double) * (size_t)running);
            if (!allEv) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        }
        return 0;
    }
    // hitOffsets - also when there are too many hits - then the arrays, which change hands (evalue: null in the hits form)
    int assemble(int nQueries, bool locate, int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget,
                 int** endQuery, double** evalue) {
        hitOffsets[0] = 0;
        for (int i = 0; i < nQueries; ++i) hitOffsets[i + 1] = hitOffsets[i] + counts[(size_t)i];
        if (over) return fail(MIOPAL_ERR_TOO_MANY_HITS, "%lld hits, maxHits = %lld", (long long)running, (long long)maxHits);
        for (const Piece& piece : pieces) {
            const HitRows& h = *piece.rows;
            if (h.total() == 0) continue;
            // (row by row: the hits of a single-path query lie between those of its neighbours in the chunk)
            for (size_t r = 0; r + 1 < h.rowOffset.size(); ++r) {
                const size_t from = (size_t)h.rowOffset[r], len = (size_t)(h.rowOffset[r + 1] - h.rowOffset[r]);
                if (len == 0) continue;
                const size_t at = (size_t)hitOffsets[piece.first + (int64_t)r];
                memcpy(all.target + at, h.hits.target + from, sizeof(int64_t) * len);
                memcpy(all.score + at, h.hits.score + from, sizeof(int) * len);
                if (evalue) memcpy(allEv + at, piece.ev.data() + from, sizeof(double) * len);
                if (locate) {
                    memcpy(all.endT + at, h.hits.endT + from, sizeof(int) * len);
                    memcpy(all.endQ + at, h.hits.endQ + from, sizeof(int) * len);
                }
            }
        }
        // (arrays the search type does not produce: NULL where the caller gave a place for them)
        if (!locate && endTarget) *endTarget = nullptr;
        if (!locate && endQuery) *endQuery = nullptr;
        all.release(targetIndex, score, locate ? endTarget : nullptr, locate ? endQuery : nullptr);
        if (evalue) {
            *evalue = allEv;
            allEv = nullptr;
        }
        return 0;
    }
};

// the device slot of the written hits: [target] [score] ([endQuery] [endTarget])
struct HitsOutSlot {
    size_t offScore, offEndQ, offEndT, bytes;
    HitsOutSlot(int64_t total, bool ends) {
        auto a256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
        offScore = a256(sizeof(int64_t) * (size_t)total);
        offEndQ = offScore + a256(sizeof(int) * (size_t)total);
        offEndT = offEndQ + (ends ? a256(sizeof(int) * (size_t)total) : 0);
        bytes = offEndT + (ends ? a256(sizeof(int) * (size_t)total) : 0);
    }
};

// The selection on `rows` device rows of n scores (and end locations), enqueued on the workspace's stream behind what
// produced them. Row r keeps its entries >= minScore[r]; rows with skip[r] != 0 (skip may be null) keep nothing and
// are not read. First trip: count and offsets, rowOffset comes back (with the strip error of `s`, the search that
// made the rows, or null). `room` < 0: no bound; a total above it is counted and not written. Second trip: the
// outputs are sized to the total, the write enqueued, exactly `total` entries per array downloaded.
// `binned` (host_stats.inc): entry i of row r is a hit iff score >= binned->threshold[r][binned->bin[i]] - the count and
// write passes of select_stats.hip in the place of select_hits.hip's; minScore is not read (null).
static int selectHitRows(Workspace* ws, Search* s, const int32_t* d_score, const int32_t* d_endI, const int32_t* d_endJ,
                         int rows, int64_t n, int64_t start, const int* minScore, const int* skip, int64_t room,
                         HitRows* out, const BinnedArgs* binned = nullptr) {
    const bool ends = d_endI != nullptr;
    void* p;
    RC_TRY(ws->get(kHitsScratch, hitsScratchBytes(rows, n), &p));
    const HitsScratch sc = hitsScratchLayout(p, rows, n);
    if (!binned) RC_TRY(ws->stageUpload(sc.minScore, minScore, sizeof(int) * (size_t)rows, ws->stream));
    if (skip) RC_TRY(ws->stageUpload(sc.skip, skip, sizeof(int) * (size_t)rows, ws->stream));
    else HIP_TRY(hipMemsetAsync(sc.skip, 0, sizeof(int) * (size_t)rows, ws->stream));
    HitsArgs a{};
    a.score = d_score;
    a.endI = d_endI;
    a.endJ = d_endJ;
    a.stride = n;
    a.rows = rows;
    a.start = start;
    a.scratch = p;
    hipError_t e = binned ? launchHitsBinnedCount(a, *binned, ws->stream) : launchHitsCount(a, ws->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIOPAL_ERR_HIP, "hit selection launch (count): %s", hipGetErrorString(e));
    }
    out->rowOffset.assign((size_t)rows + 1, 0);
    out->written = true;
    RC_TRY(ws->stageDownload(out->rowOffset.data(), sc.rowOffset, sizeof(int64_t) * ((size_t)rows + 1)));
    if (s && s->d_stripError) RC_TRY(ws->stageDownload(&s->stripErrorHost, s->d_stripError, sizeof(int)));
    RC_TRY(ws->finishDownloads());
    if (s) RC_TRY(s->checkStripError());
    const int64_t total = out->total();
    if (total < 0) return fail(MIOPAL_ERR_INTERNAL, "hit selection: negative total %lld", (long long)total);
    if (room >= 0 && total > room) {
        out->written = false;
        return 0;
    }
    if (total == 0) return 0;
    RC_TRY(out->hits.alloc(total, ends));
    const HitsOutSlot slot(total, ends);
    void* po;
    RC_TRY(ws->get(kHitsOut, slot.bytes, &po));
    char* base = (char*)po;
    a.capacity = total;
    a.target = (int64_t*)base;
    a.outScore = (int32_t*)(base + slot.offScore);
    a.outEndQ = ends ? (int32_t*)(base + slot.offEndQ) : nullptr;
    a.outEndT = ends ? (int32_t*)(base + slot.offEndT) : nullptr;
    e = binned ? launchHitsBinnedWrite(a, *binned, ws->stream) : launchHitsWrite(a, ws->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIOPAL_ERR_HIP, "hit selection launch (write): %s", hipGetErrorString(e));
    }
    RC_TRY(ws->stageDownload(out->hits.target, a.target, sizeof(int64_t) * (size_t)total));
    RC_TRY(ws->stageDownload(out->hits.score, a.outScore, sizeof(int) * (size_t)total));
    if (ends) {
        RC_TRY(ws->stageDownload(out->hits.endQ, a.outEndQ, sizeof(int) * (size_t)total));
        RC_TRY(ws->stageDownload(out->hits.endT, a.outEndT, sizeof(int) * (size_t)total));
    }
    return ws->finishDownloads();
}

static int checkHitsOutputs(int searchType, const void* counts, int64_t** targetIndex, int** score, int** endTarget,
                            int** endQuery) {
    if (!counts) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null count / hitOffsets output");
    if (!targetIndex || !score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null target / score outputs");
    if (searchType == OPAL_SEARCH_SCORE_END && (!endTarget || !endQuery))
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
    return 0;
}

// One query: the score-row pass (ScoreRows, host_search.inc), then the selection on the same stream. The caller has
// refused alignments and checked its outputs (after validate() for the plain form, before the handle for the PSSM
// form: searchTopImpl's and miopalSearchPssmTop's orders). pssmRows: the range check of the rows (validate()'s place;
// an empty slice has none) comes before `out` is touched.
static int searchHitsImpl(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                          const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                          int64_t end, int minScore, int64_t room, HitRows* out, const int* pssmRows = nullptr) {
    const int64_t n = end - start;
    if (pssmRows && n > 0) RC_TRY(checkPssmRange(db, pssmRows, queryLength, alphabetLength, gapOpen, gapExt));
    out->rowOffset.assign(2, 0);
    out->written = true;
    if (n == 0) return 0;
    ScoreRows rows(db, query, queryLength, gapOpen, gapExt, scoreMatrix, pssmRows, alphabetLength, searchType, mode, start, end);
    RC_TRY(rows.run());
    return selectHitRows(rows.ws, &rows.s, rows.d_score, rows.d_endI, rows.d_endJ, 1, n, start, &minScore, nullptr, room, out);
}

// the end of miopalSearchHits / miopalSearchPssmHits: the count, and the arrays unless there are too many
static int finishHits(HitRows& rows, int searchType, int64_t maxHits, int64_t* count, int64_t** targetIndex, int** score,
                      int** endTarget, int** endQuery) {
    *count = rows.total();
    if (!rows.written)
        return fail(MIOPAL_ERR_TOO_MANY_HITS, "%lld hits, maxHits = %lld", (long long)rows.total(), (long long)maxHits);
    const bool locate = searchType == OPAL_SEARCH_SCORE_END;
    // (arrays the search type does not produce: NULL where the caller gave a place for them)
    if (!locate && endTarget) *endTarget = nullptr;
    if (!locate && endQuery) *endQuery = nullptr;
    rows.hits.release(targetIndex, score, locate ? endTarget : nullptr, locate ? endQuery : nullptr);
    return 0;
}

// miopalSearchBatchHits: batchImpl's chunks, each chunk's final [rows][n] device rows compacted before they leave.
// Chunks and single-path queries arrive out of query order: the hits are kept per chunk / per query and assembled
// into the CSR at the end.
static int searchBatchHitsImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                               int open, int ext, const int* matrix, int A, int searchType, int mode, int64_t start,
                               int64_t end, const int* minScore, int64_t maxHits, int64_t* hitOffsets,
                               int64_t** targetIndex, int** score, int** endTarget, int** endQuery) {
    for (int c = 0; c < 4; ++c) g_lastBatchRouting[c] = 0;
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchBatchHits: alignments are not selected on the device");
    RC_TRY(validateBatch(db, queries, queryOffsets, nQueries, matrix, A, searchType, mode, start, end));
    RC_TRY(checkHitsOutputs(searchType, hitOffsets, targetIndex, score, endTarget, endQuery));
    if (nQueries > 0 && !minScore) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null minScore list");
    const bool locate = searchType == OPAL_SEARCH_SCORE_END;
    const int64_t n = end - start;
    HitPieces pieces(nQueries, maxHits);
    if (n > 0 && nQueries > 0) {
        ScoreModel model{open, ext, 0, 0};
        scoreExtremes(matrix, (size_t)A * A, &model.maxScore, &model.minScore);
        BatchSink sink;
        sink.checkOutputs = [](bool) { return 0; };
        sink.chunk = [&](Workspace* ws, int64_t i0, int rows, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ) -> int {
            // rows of queries on the single-query path hold nothing: neither counted nor downloaded
            std::vector<int> skip;
            skippedRows(queries, queryOffsets, i0, rows, model, matrix, A, searchType, mode, db->maxLen, &skip);
            std::unique_ptr<HitRows> got(new HitRows());
            RC_TRY(selectHitRows(ws, nullptr, d_score, d_endI, d_endJ, rows, n, start, minScore + i0, skip.data(),
                                 pieces.room(), got.get()));
            pieces.take(i0, std::move(got));
            return 0;
        };
        sink.single = [&](int i) -> int {
            std::unique_ptr<HitRows> got(new HitRows());
            RC_TRY(searchHitsImpl(db, queries + queryOffsets[i], (int)(queryOffsets[i + 1] - queryOffsets[i]), open, ext,
                                  matrix, A, searchType, mode, start, end, minScore[i], pieces.room(), got.get()));
            pieces.take(i, std::move(got));
            return 0;
        };
        RC_TRY(batchImpl(db, queries, queryOffsets, nQueries, open, ext, matrix, A, searchType, mode, start, end, sink));
    }
    // nothing failed: the outputs are written from here on
    RC_TRY(pieces.reserve(locate, false));
    return pieces.assemble(nQueries, locate, hitOffsets, targetIndex, score, endTarget, endQuery, nullptr);
}

// miopalTestSelectHits (test hook): the three kernels alone, on rows the caller supplies - launchHitsCount and
// launchHitsWrite as selectHitRows calls them (the same HitsArgs and scratch, one stream, the host between them), with
// no search and no handle in front of them. Device 0.
// miopalTestSelectHitsBinned: `binned` - the bins built on the device from length[stride] (length_bins_kernel), the
// table threshold[rows][kStatBins] in the place of minScore, and select_stats.hip's count and write passes.
static int testSelectHitsImpl(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride,
                              const int* minScore, int64_t start, int64_t* hitOffsets, int64_t** targetIndex,
                              int** outScore, int** outEndTarget, int** outEndQuery, bool binned = false,
                              const int32_t* length = nullptr, const int32_t* threshold = nullptr) {
    constexpr int64_t kMaxEntries = (int64_t)1 << 27;
    if (rows < 1 || stride < 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "rows = %d, stride = %lld: both at least 1", rows, (long long)stride);
    if (!score || (!binned && !minScore)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score rows / minScore list");
    if (binned && (!length || !threshold)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null lengths / threshold table");
    if ((endTarget == nullptr) != (endQuery == nullptr)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "one end array without the other");
    const bool ends = endTarget != nullptr;
    if (!hitOffsets || !targetIndex || !outScore) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null hitOffsets / target / score outputs");
    if (ends && (!outEndTarget || !outEndQuery)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
    if (stride > kMaxEntries || rows > kMaxEntries / stride)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "%d rows x %lld entries: more than 2^27", rows, (long long)stride);
    if (binned)
        for (int64_t i = 0; i < stride; ++i)
            if (length[i] < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative length at %lld", (long long)i);
    if (physicalDeviceCount() < 1) return fail(OPAL_ERR_NO_SIMD_SUPPORT, "no usable gfx950 device");
    HIP_TRY(hipSetDevice(usableDevices()[0]));

    const size_t inBytes = sizeof(int32_t) * (size_t)rows * (size_t)stride;
    DeviceBytes dScore, dEndI, dEndJ, dScratch, dOut, dLength, dBin, dTable;
    OwnedStream stream;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&dScore.p, inBytes));
    HIP_TRY(hipMalloc(&dScratch.p, hitsScratchBytes(rows, stride)));
    HIP_TRY(hipMemcpyAsync(dScore.p, score, inBytes, hipMemcpyHostToDevice, stream.s));
    if (ends) {
        HIP_TRY(hipMalloc(&dEndI.p, inBytes));
        HIP_TRY(hipMalloc(&dEndJ.p, inBytes));
        HIP_TRY(hipMemcpyAsync(dEndI.p, endQuery, inBytes, hipMemcpyHostToDevice, stream.s));
        HIP_TRY(hipMemcpyAsync(dEndJ.p, endTarget, inBytes, hipMemcpyHostToDevice, stream.s));
    }
    const HitsScratch sc = hitsScratchLayout(dScratch.p, rows, stride);
    if (!binned) HIP_TRY(hipMemcpyAsync(sc.minScore, minScore, sizeof(int) * (size_t)rows, hipMemcpyHostToDevice, stream.s));
    HIP_TRY(hipMemsetAsync(sc.skip, 0, sizeof(int) * (size_t)rows, stream.s));
    BinnedArgs table{};
    if (binned) {
        const size_t tableBytes = sizeof(int32_t) * (size_t)rows * kStatBins;
        HIP_TRY(hipMalloc(&dLength.p, sizeof(int32_t) * (size_t)stride));
        HIP_TRY(hipMalloc(&dBin.p, (size_t)stride));
        HIP_TRY(hipMalloc(&dTable.p, tableBytes));
        HIP_TRY(hipMemcpyAsync(dLength.p, length, sizeof(int32_t) * (size_t)stride, hipMemcpyHostToDevice, stream.s));
        HIP_TRY(hipMemcpyAsync(dTable.p, threshold, tableBytes, hipMemcpyHostToDevice, stream.s));
        HIP_TRY(launchLengthBins(nullptr, (const int32_t*)dLength.p, stride, (uint8_t*)dBin.p, stream.s));
        table.bin = (const uint8_t*)dBin.p;
        table.threshold = (const int32_t*)dTable.p;
    }
    HitsArgs a{};
    a.score = (const int32_t*)dScore.p;
    a.endI = (const int32_t*)dEndI.p;
    a.endJ = (const int32_t*)dEndJ.p;
    a.stride = stride;
    a.rows = rows;
    a.start = start;
    a.scratch = dScratch.p;
    hipError_t e = binned ? launchHitsBinnedCount(a, table, stream.s) : launchHitsCount(a, stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIOPAL_ERR_HIP, "hit selection launch (count): %s", hipGetErrorString(e));
    }
    std::vector<int64_t> rowOffset((size_t)rows + 1);
    HIP_TRY(hipMemcpyAsync(rowOffset.data(), sc.rowOffset, sizeof(int64_t) * rowOffset.size(), hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipStreamSynchronize(stream.s));
    const int64_t total = rowOffset.back();
    if (total < 0 || total > (int64_t)rows * stride) return fail(MIOPAL_ERR_INTERNAL, "hit selection: total %lld", (long long)total);
    HitArrays hits;
    RC_TRY(hits.alloc(total, ends));
    if (total > 0) {
        const HitsOutSlot slot(total, ends);
        HIP_TRY(hipMalloc(&dOut.p, slot.bytes));
        char* base = (char*)dOut.p;
        a.capacity = total;
        a.target = (int64_t*)base;
        a.outScore = (int32_t*)(base + slot.offScore);
        a.outEndQ = ends ? (int32_t*)(base + slot.offEndQ) : nullptr;
        a.outEndT = ends ? (int32_t*)(base + slot.offEndT) : nullptr;
        e = binned ? launchHitsBinnedWrite(a, table, stream.s) : launchHitsWrite(a, stream.s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "hit selection launch (write): %s", hipGetErrorString(e));
        }
        HIP_TRY(hipMemcpyAsync(hits.target, a.target, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, stream.s));
        HIP_TRY(hipMemcpyAsync(hits.score, a.outScore, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, stream.s));
        if (ends) {
            HIP_TRY(hipMemcpyAsync(hits.endQ, a.outEndQ, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, stream.s));
            HIP_TRY(hipMemcpyAsync(hits.endT, a.outEndT, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, stream.s));
        }
        HIP_TRY(hipStreamSynchronize(stream.s));
    }
    memcpy(hitOffsets, rowOffset.data(), sizeof(int64_t) * rowOffset.size());
    if (!ends && outEndTarget) *outEndTarget = nullptr;
    if (!ends && outEndQuery) *outEndQuery = nullptr;
    hits.release(targetIndex, outScore, ends ? outEndTarget : nullptr, ends ? outEndQuery : nullptr);
    return 0;
}
