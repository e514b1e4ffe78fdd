// Part of host.hip (included there, not a translation unit of its own): miopalSearchTop and miopalSearchBatchTop,
// the k best targets of a query (of every query of a batch), selected on the device (select_top.hip) from the score
// rows the search kernels leave in HBM. Only count + k entries per query cross PCIe.

static_assert(kTopMaxK == MIOPAL_MAX_TOP, "select_top.h mirrors miopal.h");

// checks shared by both entry points (after validate(), which has refused a bad search type already)
static int checkTopArgs(int searchType, int k, const int* count, const int64_t* targetIndex, const int* score,
                        const int* endTarget, const int* endQuery) {
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchTop: alignments are not selected on the device");
    if (k < 0 || k > MIOPAL_MAX_TOP) return fail(MIOPAL_ERR_BAD_ARGUMENT, "k = %d outside [0, %d]", k, MIOPAL_MAX_TOP);
    if (!count) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null count output");
    if (k > 0 && (!targetIndex || !score)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null target / score outputs");
    if (k > 0 && searchType == OPAL_SEARCH_SCORE_END && (!endTarget || !endQuery))
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
    return 0;
}

// rows [from, to) of the outputs: nothing chosen
static void emptyTopRows(int from, int to, int k, int* count, int64_t* targetIndex, int* score, int* endTarget,
                         int* endQuery) {
    for (int r = from; r < to; ++r) {
        count[r] = 0;
        const size_t at = (size_t)r * k;
        std::fill(targetIndex + at, targetIndex + at + k, (int64_t)-1);
        std::fill(score + at, score + at + k, -1);
        if (endTarget) std::fill(endTarget + at, endTarget + at + k, -1);
        if (endQuery) std::fill(endQuery + at, endQuery + at + k, -1);
    }
}

// One device slot of a selection: [error, count[rows]] [target] [score] ([endQuery] [endTarget]) | the selection's
// scratch. The outputs in front of the scratch come back in one download.
struct TopSlot {
    size_t offTarget, offScore, offEndQ, offEndT, outBytes, rk;
    int rows;
    bool ends;
    TopSlot(int rows_, int k, bool ends_) : rk((size_t)rows_ * k), rows(rows_), ends(ends_) {
        auto a256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
        offTarget = a256(sizeof(int) * ((size_t)rows + 1));
        offScore = offTarget + a256(sizeof(int64_t) * rk);
        offEndQ = offScore + a256(sizeof(int) * rk);
        offEndT = offEndQ + (ends ? a256(sizeof(int) * rk) : 0);
        outBytes = offEndT + (ends ? a256(sizeof(int) * rk) : 0);
    }
    size_t bytes(int64_t n, int k) const { return outBytes + topScratchBytes(rows, n, k); }
    // the selection's arguments for the slot at `base` (its error counter is zeroed by the caller)
    TopArgs args(char* base, const int32_t* d_score, const int32_t* d_endI, const int32_t* d_endJ, int64_t n, int k,
                 int minScore, int64_t start) const {
        TopArgs a{};
        a.score = d_score;
        a.endI = d_endI;
        a.endJ = d_endJ;
        a.stride = n;
        a.rows = rows;
        a.k = k;
        a.minScore = minScore;
        a.start = start;
        a.scratch = base + outBytes;
        a.error = (int*)base;
        a.count = (int32_t*)base + 1;
        a.target = (int64_t*)(base + offTarget);
        a.outScore = (int32_t*)(base + offScore);
        a.outEndQ = ends ? (int32_t*)(base + offEndQ) : nullptr;
        a.outEndT = ends ? (int32_t*)(base + offEndT) : nullptr;
        return a;
    }
    // the downloaded outputs -> the caller's arrays (row 0 of the selection at their row 0); returns the error counter
    int unpack(const char* host, int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery) const {
        int error;
        memcpy(&error, host, sizeof(int));
        memcpy(count, host + sizeof(int), sizeof(int) * (size_t)rows);
        memcpy(targetIndex, host + offTarget, sizeof(int64_t) * rk);
        memcpy(score, host + offScore, sizeof(int) * rk);
        if (ends) {
            memcpy(endQuery, host + offEndQ, sizeof(int) * rk);
            memcpy(endTarget, host + offEndT, sizeof(int) * rk);
        }
        return error;
    }
};

// The selection on `rows` device rows of n scores (and end locations), enqueued on the workspace's stream behind
// what produced them, and ONE download of the [rows] counts and [rows][k] entries into the caller's arrays, which
// hold row 0 of the selection at their row `outRow`. `s`: the search whose strip error is checked with it (or null).
static int selectTopRows(Workspace* ws, Search* s, const int32_t* d_score, const int32_t* d_endI,
                         const int32_t* d_endJ, int rows, int64_t n, int64_t start, int k, int minScore, int64_t outRow,
                         int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery) {
    const TopSlot slot(rows, k, d_endI != nullptr);
    void* p;
    RC_TRY(ws->get(kTopScratch, slot.bytes(n, k), &p));
    char* base = (char*)p;
    HIP_TRY(hipMemsetAsync(base, 0, sizeof(int), ws->stream));
    const hipError_t e = launchSelectTop(slot.args(base, d_score, d_endI, d_endJ, n, k, minScore, start), ws->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIOPAL_ERR_HIP, "top-k selection launch: %s", hipGetErrorString(e));
    }
    std::vector<char> host(slot.outBytes);
    RC_TRY(ws->stageDownload(host.data(), base, slot.outBytes));
    if (s && s->d_stripError) RC_TRY(ws->stageDownload(&s->stripErrorHost, s->d_stripError, sizeof(int)));
    RC_TRY(ws->finishDownloads());
    if (s) RC_TRY(s->checkStripError());
    int error;
    memcpy(&error, host.data(), sizeof(int));
    if (error) return fail(MIOPAL_ERR_INTERNAL, "top-k selection: %d blocks gave up waiting for the blocks before them", error);
    const size_t at = (size_t)outRow * k;
    slot.unpack(host.data(), count + outRow, targetIndex + at, score + at, slot.ends ? endTarget + at : nullptr,
                slot.ends ? endQuery + at : nullptr);
    return 0;
}

// miopalSearchTop: the score-row pass (ScoreRows, host_search.inc), then the selection on the same stream. Writes row
// `outRow` of the outputs.
// (pssmRows, miopalSearchPssmTop: the score source is [queryLength][alphabetLength] rows, as in searchImpl; scoreMatrix
// is null, `query` a consensus of 255s - no alignment reads it - and the caller has made miopalSearchPssm's checks;
// the range check of the rows comes before "nothing to select", as validate() does for the plain form's arguments)
static int searchTopImpl(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                         const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                         int64_t end, int k, int minScore, int64_t outRow, int* count, int64_t* targetIndex, int* score,
                         int* endTarget, int* endQuery, const int* pssmRows = nullptr) {
    if (!pssmRows) RC_TRY(validate(db, query, queryLength, scoreMatrix, alphabetLength, searchType, mode, start, end));
    RC_TRY(checkTopArgs(searchType, k, count, targetIndex, score, endTarget, endQuery));
    const bool locate = searchType == OPAL_SEARCH_SCORE_END;
    const int64_t n = end - start;
    if (pssmRows && n > 0) RC_TRY(checkPssmRange(db, pssmRows, queryLength, alphabetLength, gapOpen, gapExt));
    if (k == 0 || n == 0) {
        emptyTopRows((int)outRow, (int)outRow + 1, k, count, targetIndex, score, locate ? endTarget : nullptr,
                     locate ? endQuery : nullptr);
        return 0;
    }
    ScoreRows rows(db, query, queryLength, gapOpen, gapExt, scoreMatrix, pssmRows, alphabetLength, searchType, mode, start, end);
    RC_TRY(rows.run());
    return selectTopRows(rows.ws, &rows.s, rows.d_score, rows.d_endI, rows.d_endJ, 1, n, start, k, minScore, outRow, count,
                         targetIndex, score, endTarget, endQuery);
}

// miopalSearchBatchTop: batchImpl's chunks, each chunk's final [rows][n] device rows selected before they leave
static int searchBatchTopImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                              int open, int ext, const int* matrix, int A, int searchType, int mode, int64_t start,
                              int64_t end, int k, int minScore, int* count, int64_t* targetIndex, int* score,
                              int* endTarget, int* endQuery) {
    for (int c = 0; c < 4; ++c) g_lastBatchRouting[c] = 0;
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchBatchTop: alignments are not selected on the device");
    RC_TRY(validateBatch(db, queries, queryOffsets, nQueries, matrix, A, searchType, mode, start, end));
    if (nQueries == 0) return 0;
    RC_TRY(checkTopArgs(searchType, k, count, targetIndex, score, endTarget, endQuery));
    const bool locate = searchType == OPAL_SEARCH_SCORE_END;
    if (k == 0 || end == start) {
        emptyTopRows(0, nQueries, k, count, targetIndex, score, locate ? endTarget : nullptr, locate ? endQuery : nullptr);
        return 0;
    }
    const int64_t n = end - start;
    BatchSink sink;
    sink.checkOutputs = [](bool) { return 0; };
    sink.chunk = [&](Workspace* ws, int64_t i0, int rows, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ) -> int {
        return selectTopRows(ws, nullptr, d_score, d_endI, d_endJ, rows, n, start, k, minScore, i0, count, targetIndex,
                             score, endTarget, endQuery);
    };
    sink.single = [&](int i) -> int {
        return searchTopImpl(db, queries + queryOffsets[i], (int)(queryOffsets[i + 1] - queryOffsets[i]), open, ext,
                             matrix, A, searchType, mode, start, end, k, minScore, i, count, targetIndex, score,
                             endTarget, endQuery);
    };
    return batchImpl(db, queries, queryOffsets, nQueries, open, ext, matrix, A, searchType, mode, start, end, sink);
}

// miopalTestSelectTop (test hook): the selection alone, on rows the caller supplies - launchSelectTop as selectTopRows
// calls it (the same TopArgs, scratch from topScratchBytes, one stream), with no search and no handle in front of
// it, so that a test can build a row for every arm of the five kernels. Device 0.
static int testSelectTopImpl(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride, int k,
                             int minScore, int64_t start, int* count, int64_t* targetIndex, int* outScore,
                             int* outEndTarget, int* outEndQuery, int* gaveUp) {
    constexpr int64_t kMaxEntries = (int64_t)1 << 27;
    if (rows < 1 || stride < 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "rows = %d, stride = %lld: both at least 1", rows, (long long)stride);
    if (k < 1 || k > MIOPAL_MAX_TOP) return fail(MIOPAL_ERR_BAD_ARGUMENT, "k = %d outside [1, %d]", k, MIOPAL_MAX_TOP);
    if (!score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score rows");
    if ((endTarget == nullptr) != (endQuery == nullptr)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "one end array without the other");
    const bool ends = endTarget != nullptr;
    if (!count || !targetIndex || !outScore || !gaveUp) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null count / target / score / gaveUp outputs");
    if (ends && (!outEndTarget || !outEndQuery)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
    if (stride > kMaxEntries || rows > kMaxEntries / stride)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "%d rows x %lld entries: more than 2^27", rows, (long long)stride);
    if (physicalDeviceCount() < 1) return fail(OPAL_ERR_NO_SIMD_SUPPORT, "no usable gfx950 device");
    HIP_TRY(hipSetDevice(usableDevices()[0]));

    const size_t inBytes = sizeof(int32_t) * (size_t)rows * (size_t)stride;
    const TopSlot slot(rows, k, ends);
    DeviceBytes dScore, dEndI, dEndJ, dOut;
    OwnedStream stream;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&dScore.p, inBytes));
    HIP_TRY(hipMalloc(&dOut.p, slot.bytes(stride, k)));
    HIP_TRY(hipMemcpyAsync(dScore.p, score, inBytes, hipMemcpyHostToDevice, stream.s));
    if (ends) {
        HIP_TRY(hipMalloc(&dEndI.p, inBytes));
        HIP_TRY(hipMalloc(&dEndJ.p, inBytes));
        HIP_TRY(hipMemcpyAsync(dEndI.p, endQuery, inBytes, hipMemcpyHostToDevice, stream.s));
        HIP_TRY(hipMemcpyAsync(dEndJ.p, endTarget, inBytes, hipMemcpyHostToDevice, stream.s));
    }
    char* base = (char*)dOut.p;
    HIP_TRY(hipMemsetAsync(base, 0, sizeof(int), stream.s));
    const TopArgs a = slot.args(base, (const int32_t*)dScore.p, (const int32_t*)dEndI.p, (const int32_t*)dEndJ.p, stride, k,
                                minScore, start);
    const hipError_t e = launchSelectTop(a, stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIOPAL_ERR_HIP, "top-k selection launch: %s", hipGetErrorString(e));
    }
    std::vector<char> host(slot.outBytes);
    HIP_TRY(hipMemcpyAsync(host.data(), base, slot.outBytes, hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipStreamSynchronize(stream.s));
    *gaveUp = slot.unpack(host.data(), count, targetIndex, outScore, outEndTarget, outEndQuery);
    return 0;
}
