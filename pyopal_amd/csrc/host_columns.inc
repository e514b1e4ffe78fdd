// Part of host.hip (included there, not a translation unit of its own): miopalSearchBatchTargetTop, the m best
// queries of every target of a slice, folded on the device (select_columns.hip) from the [queries][targets] rows
// batchImpl's chunks and the single-query path leave in HBM. Only count + m entries per target cross PCIe.
//
// Where the state lives: in a workspace the call leases for itself and holds from its first device call to its last
// (slot kColumnsState; the answer in kColumnsOut of the same workspace). batchImpl leases ANOTHER workspace for its
// chunks and gives it back before the single-path queries run, each of which leases one of its own - possibly a third,
// on another stream: none of them owns the state, all of them fold into it.
// How the folds are ordered: a piece's fold is enqueued on the stream that produced the piece, behind its kernels, and
// the host waits for that stream before the piece's sink returns - one stream synchronisation per piece. The next
// fold, on whatever stream, starts after the one before it is complete; the zero fill of the state (the call's own
// stream) is waited for before the first piece, and the finish runs on the call's own stream after the last.

static_assert(kColumnsMaxM == MIOPAL_MAX_TARGET_TOP, "select_columns.h mirrors miopal.h");

// m and the outputs (after the query list: the header's order)
static int checkColumnsArgs(bool locate, int m, const int* count, const int32_t* queryIndex, const int* score,
                            const int* endTarget, const int* endQuery) {
    if (m < 1 || m > MIOPAL_MAX_TARGET_TOP)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "m = %d outside [1, %d]", m, MIOPAL_MAX_TARGET_TOP);
    if (!count || !queryIndex || !score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null count / query / score outputs");
    if (locate && (!endTarget || !endQuery)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
    return 0;
}

// The running state of one call, in slots of the workspace `own` (held by the caller for as long as this lives)
struct ColumnsFold {
    Workspace* own;
    int64_t n;
    int m, minScore;
    bool ends;
    ColumnsState st{};

    // the state allocated and zeroed: complete on return (the first fold may run on any stream)
    int begin() {
        void* p;
        const size_t bytes = columnsStateBytes(n, m, ends);
        RC_TRY(own->get(kColumnsState, bytes, &p));
        st = columnsStateLayout(p, n, m, ends);
        HIP_TRY(hipMemsetAsync(p, 0, bytes, own->stream));
        HIP_TRY(hipStreamSynchronize(own->stream));
        return 0;
    }
    // One piece - `rows` device rows of n entries, row r the query i0 + r - folded on `ws`'s stream behind what
    // produced it; complete on return. skip (host, may be null): rows that hold nothing. `s`: the search whose strip
    // error is checked with it (or null).
    int fold(Workspace* ws, Search* s, const int32_t* d_score, const int32_t* d_endI, const int32_t* d_endJ, int64_t i0,
             int rows, const int32_t* skip) {
        ColumnsPiece piece{};
        piece.score = d_score;
        piece.endI = ends ? d_endI : nullptr;
        piece.endJ = ends ? d_endJ : nullptr;
        piece.rows = rows;
        piece.firstRow = (int32_t)i0;
        if (skip) {
            void* p;
            RC_TRY(ws->get(kColumnsSkip, sizeof(int32_t) * (size_t)rows, &p));
            RC_TRY(ws->stageUpload(p, skip, sizeof(int32_t) * (size_t)rows, ws->stream));
            piece.skip = (const int32_t*)p;
        }
        const hipError_t e = launchColumnsFold(st, piece, n, m, minScore, ws->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "column selection launch (fold): %s", hipGetErrorString(e));
        }
        if (s && s->d_stripError) RC_TRY(ws->stageDownload(&s->stripErrorHost, s->d_stripError, sizeof(int)));
        // (the next piece may be folded on another stream: this one is complete first)
        HIP_TRY(hipStreamSynchronize(ws->stream));
        RC_TRY(ws->finishDownloads());
        if (s) RC_TRY(s->checkStripError());
        return 0;
    }
    // state -> the caller's count[n] and [n][m] arrays, on the call's own stream (every fold is complete)
    int finish(int* count, int32_t* queryIndex, int* score, int* endTarget, int* endQuery) {
        void* p;
        RC_TRY(own->get(kColumnsOut, columnsOutBytes(n, m, ends), &p));
        const ColumnsOut out = columnsOutLayout(p, n, m, ends);
        const hipError_t e = launchColumnsFinish(st, out, n, m, own->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "column selection launch (finish): %s", hipGetErrorString(e));
        }
        const size_t cells = sizeof(int32_t) * (size_t)n * (size_t)m;
        RC_TRY(own->stageDownload(count, out.count, sizeof(int32_t) * (size_t)n));
        RC_TRY(own->stageDownload(queryIndex, out.row, cells));
        RC_TRY(own->stageDownload(score, out.score, cells));
        if (ends) {
            RC_TRY(own->stageDownload(endQuery, out.endI, cells));
            RC_TRY(own->stageDownload(endTarget, out.endJ, cells));
        }
        return own->finishDownloads();
    }
};

static int searchBatchTargetTopImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                                    int open, int ext, const int* matrix, int A, int searchType, int mode, int64_t start,
                                    int64_t end, int m, int minScore, int* count, int32_t* queryIndex, int* score,
                                    int* endTarget, int* endQuery) {
    for (int c = 0; c < 4; ++c) g_lastBatchRouting[c] = 0;
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchBatchTargetTop: alignments are not selected on the device");
    RC_TRY(validateBatch(db, queries, queryOffsets, nQueries, matrix, A, searchType, mode, start, end));
    const bool locate = searchType == OPAL_SEARCH_SCORE_END;
    RC_TRY(checkColumnsArgs(locate, m, count, queryIndex, score, endTarget, endQuery));
    const int64_t n = end - start;
    if (n == 0) return 0;
    if (nQueries == 0) {
        std::fill(count, count + n, 0);
        std::fill(queryIndex, queryIndex + n * m, (int32_t)-1);
        std::fill(score, score + n * m, -1);
        if (locate) {
            std::fill(endTarget, endTarget + n * m, -1);
            std::fill(endQuery, endQuery + n * m, -1);
        }
        return 0;
    }
    HIP_TRY(hipSetDevice(db->device));
    WorkspaceLease mine(db);
    RC_TRY(mine.acquireInternal());
    ColumnsFold fold{mine.ws, n, m, minScore, locate};
    RC_TRY(fold.begin());
    ScoreModel model{open, ext, 0, 0};
    scoreExtremes(matrix, (size_t)A * A, &model.maxScore, &model.minScore);
    BatchSink sink;
    sink.checkOutputs = [](bool) { return 0; };
    sink.chunk = [&](Workspace* ws, int64_t i0, int rows, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ) -> int {
        // rows of queries on the single-query path hold nothing: never read
        std::vector<int> skip;
        const bool any = skippedRows(queries, queryOffsets, i0, rows, model, matrix, A, searchType, mode, db->maxLen, &skip);
        return fold.fold(ws, nullptr, d_score, d_endI, d_endJ, i0, rows, any ? skip.data() : nullptr);
    };
    sink.single = [&](int i) -> int {
        // the score-row pass in a workspace of its own (ScoreRows sets the call's device once more: harmless)
        ScoreRows rows(db, queries + queryOffsets[i], (int)(queryOffsets[i + 1] - queryOffsets[i]), open, ext, matrix, nullptr,
                       A, searchType, mode, start, end);
        RC_TRY(rows.run());
        return fold.fold(rows.ws, &rows.s, rows.d_score, rows.d_endI, rows.d_endJ, i, 1, nullptr);
    };
    RC_TRY(batchImpl(db, queries, queryOffsets, nQueries, open, ext, matrix, A, searchType, mode, start, end, sink));
    // nothing failed: the outputs are written from here on
    return fold.finish(count, queryIndex, score, endTarget, endQuery);
}

// miopalTestSelectColumns (test hook): the two kernels alone, on rows the caller supplies - launchColumnsFold once per
// piece, in the order of the list, and launchColumnsFinish, as ColumnsFold calls them (the same state and output
// layouts; one stream, so a fold is complete before the next starts), with no search and no handle in front of them.
// Device 0.
static int testSelectColumnsImpl(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride,
                                 const int32_t* pieceFirst, const int32_t* pieceCount, int pieces,
                                 const unsigned char* skip, int m, int minScore, int* count, int32_t* queryIndex,
                                 int* outScore, int* outEndTarget, int* outEndQuery) {
    constexpr int64_t kMaxEntries = (int64_t)1 << 27;
    if (rows < 1 || stride < 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "rows = %d, stride = %lld: both at least 1", rows, (long long)stride);
    if (m < 1 || m > MIOPAL_MAX_TARGET_TOP) return fail(MIOPAL_ERR_BAD_ARGUMENT, "m = %d outside [1, %d]", m, MIOPAL_MAX_TARGET_TOP);
    if (!score) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score rows");
    if (pieces < 0 || (pieces > 0 && (!pieceFirst || !pieceCount))) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad piece list");
    if ((endTarget == nullptr) != (endQuery == nullptr)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "one end array without the other");
    const bool ends = endTarget != nullptr;
    if (!count || !queryIndex || !outScore) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null count / query / score outputs");
    if (ends && (!outEndTarget || !outEndQuery)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null end-location outputs");
    for (int p = 0; p < pieces; ++p)
        if (pieceFirst[p] < 0 || pieceCount[p] < 1 || pieceCount[p] > rows - pieceFirst[p])
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "piece %d (rows %d + %d) outside [0, %d)", p, pieceFirst[p], pieceCount[p], rows);
    if (stride > kMaxEntries || rows > kMaxEntries / stride)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "%d rows x %lld entries: more than 2^27", rows, (long long)stride);
    if (physicalDeviceCount() < 1) return fail(OPAL_ERR_NO_SIMD_SUPPORT, "no usable gfx950 device");
    HIP_TRY(hipSetDevice(usableDevices()[0]));

    const int64_t n = stride;
    const size_t inBytes = sizeof(int32_t) * (size_t)rows * (size_t)stride;
    const size_t stateBytes = columnsStateBytes(n, m, ends);
    DeviceBytes dScore, dEndI, dEndJ, dSkip, dState, dOut;
    OwnedStream stream;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&dScore.p, inBytes));
    HIP_TRY(hipMalloc(&dState.p, stateBytes));
    HIP_TRY(hipMalloc(&dOut.p, columnsOutBytes(n, m, ends)));
    HIP_TRY(hipMemcpyAsync(dScore.p, score, inBytes, hipMemcpyHostToDevice, stream.s));
    if (ends) {
        HIP_TRY(hipMalloc(&dEndI.p, inBytes));
        HIP_TRY(hipMalloc(&dEndJ.p, inBytes));
        HIP_TRY(hipMemcpyAsync(dEndI.p, endQuery, inBytes, hipMemcpyHostToDevice, stream.s));
        HIP_TRY(hipMemcpyAsync(dEndJ.p, endTarget, inBytes, hipMemcpyHostToDevice, stream.s));
    }
    std::vector<int32_t> skipWords;   // (alive until the stream is drained)
    if (skip) {
        skipWords.assign(skip, skip + rows);
        HIP_TRY(hipMalloc(&dSkip.p, sizeof(int32_t) * (size_t)rows));
        HIP_TRY(hipMemcpyAsync(dSkip.p, skipWords.data(), sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, stream.s));
    }
    HIP_TRY(hipMemsetAsync(dState.p, 0, stateBytes, stream.s));
    const ColumnsState st = columnsStateLayout(dState.p, n, m, ends);
    for (int p = 0; p < pieces; ++p) {
        const size_t at = (size_t)pieceFirst[p] * (size_t)stride;
        ColumnsPiece piece{};
        piece.score = (const int32_t*)dScore.p + at;
        piece.endI = ends ? (const int32_t*)dEndI.p + at : nullptr;
        piece.endJ = ends ? (const int32_t*)dEndJ.p + at : nullptr;
        piece.rows = pieceCount[p];
        piece.firstRow = pieceFirst[p];
        piece.skip = skip ? (const int32_t*)dSkip.p + pieceFirst[p] : nullptr;
        const hipError_t e = launchColumnsFold(st, piece, n, m, minScore, stream.s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(stream.s);
            return fail(MIOPAL_ERR_HIP, "column selection launch (fold): %s", hipGetErrorString(e));
        }
    }
    const ColumnsOut out = columnsOutLayout(dOut.p, n, m, ends);
    const hipError_t e = launchColumnsFinish(st, out, n, m, stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream.s);
        return fail(MIOPAL_ERR_HIP, "column selection launch (finish): %s", hipGetErrorString(e));
    }
    // (into vectors of the call: on an error the caller's arrays are as they were)
    const size_t cells = (size_t)n * (size_t)m;
    std::vector<int32_t> hCount((size_t)n), hRow(cells), hScore(cells), hEndI(ends ? cells : 0), hEndJ(ends ? cells : 0);
    hipError_t c = hipMemcpyAsync(hCount.data(), out.count, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream.s);
    if (c == hipSuccess) c = hipMemcpyAsync(hRow.data(), out.row, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, stream.s);
    if (c == hipSuccess) c = hipMemcpyAsync(hScore.data(), out.score, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, stream.s);
    if (c == hipSuccess && ends) c = hipMemcpyAsync(hEndI.data(), out.endI, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, stream.s);
    if (c == hipSuccess && ends) c = hipMemcpyAsync(hEndJ.data(), out.endJ, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, stream.s);
    // (the stream is drained whatever happened: the vectors and skipWords go away with the call)
    const hipError_t d = hipStreamSynchronize(stream.s);
    if (c != hipSuccess || d != hipSuccess)
        return fail(MIOPAL_ERR_HIP, "column selection download: %s", hipGetErrorString(c != hipSuccess ? c : d));
    memcpy(count, hCount.data(), sizeof(int32_t) * (size_t)n);
    memcpy(queryIndex, hRow.data(), sizeof(int32_t) * cells);
    memcpy(outScore, hScore.data(), sizeof(int32_t) * cells);
    if (ends) {
        memcpy(outEndQuery, hEndI.data(), sizeof(int32_t) * cells);
        memcpy(outEndTarget, hEndJ.data(), sizeof(int32_t) * cells);
    }
    return 0;
}
