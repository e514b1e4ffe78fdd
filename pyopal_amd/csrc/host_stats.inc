// Part of host.hip (included there, not a translation unit of its own): miopalSearchSignificant, its PSSM and batch
// forms and the test hook of the statistics kernels. The search is its own calibration sample: per length bin the
// device sums n, score and score^2 of the rows the search kernels leave in HBM (select_stats.hip), the host fits
// mean score = intercept + slope ln(length) and one spread in doubles from those 128 x 3 integers, turns the E-value
// cut into one integer threshold per bin, and the device compacts with that table. A few KB cross PCIe per pass.

static const double kGumbelScale = M_PI / std::sqrt(6.0);   // of a Gumbel variable with mean 0 and variance 1
static const double kEulerGamma = 0.57721566490153286061;

static int clampToInt32(double v) {
    if (!(v > (double)INT32_MIN)) return INT32_MIN;
    if (!(v < (double)INT32_MAX)) return INT32_MAX;
    return (int)v;
}

// mean[b] of every bin that holds targets (1 .. 127; NaN elsewhere) under the fit's line
static void fitMeans(const MiopalScoreFit& f, double* mean) {
    for (int b = 0; b < MIOPAL_STAT_BINS; ++b) {
        mean[b] = std::nan("");
        if (b >= 1 && f.binTargets[b] > 0)
            mean[b] = f.intercept + f.slope * std::log((double)f.binLength[b] / (double)f.binTargets[b]);
    }
}

// The weighted least-squares line and the spread from f->kept (and binTargets / binLength): used, intercept, slope,
// sigma, degenerate
static void fitLine(MiopalScoreFit* f) {
    double Sn = 0, Snx = 0, Snxx = 0, Ss = 0, Sxs = 0;
    double x[MIOPAL_STAT_BINS];
    int bins = 0;
    int64_t used = 0;
    for (int b = 1; b < MIOPAL_STAT_BINS; ++b) {
        x[b] = 0;
        if (f->binTargets[b] <= 0 || f->kept[b][0] <= 0) continue;
        x[b] = std::log((double)f->binLength[b] / (double)f->binTargets[b]);
        const double n = (double)f->kept[b][0], s = (double)f->kept[b][1];
        ++bins;
        used += f->kept[b][0];
        Sn += n;
        Snx += n * x[b];
        Snxx += n * x[b] * x[b];
        Ss += s;
        Sxs += x[b] * s;
    }
    f->used = used;
    f->intercept = f->slope = f->sigma = 0;
    f->degenerate = 1;
    if (used < 3) return;
    const double denom = Sn * Snxx - Snx * Snx;
    double slope = 0, intercept = Ss / Sn;   // (every target in one bin: the mean)
    if (bins > 1 && denom > 0) {
        slope = (Sn * Sxs - Snx * Ss) / denom;
        intercept = (Ss - slope * Snx) / Sn;
    }
    double resid = 0;
    for (int b = 1; b < MIOPAL_STAT_BINS; ++b) {
        if (f->binTargets[b] <= 0 || f->kept[b][0] <= 0) continue;
        const double m = intercept + slope * x[b];
        resid += (double)f->kept[b][2] - 2 * m * (double)f->kept[b][1] + (double)f->kept[b][0] * m * m;
    }
    const double sigma = std::sqrt(resid / (double)(used - 2));
    if (!(resid > 0) || !std::isfinite(intercept) || !std::isfinite(slope) || !std::isfinite(sigma) || !(sigma > 0)) return;
    f->intercept = intercept;
    f->slope = slope;
    f->sigma = sigma;
    f->degenerate = 0;
}

// the ceilings of a refit: floor(mean_b + excludeZ sigma) for the bins that hold targets, none elsewhere
static void fitCeilings(const MiopalScoreFit& f, double excludeZ, int32_t* ceiling) {
    double mean[MIOPAL_STAT_BINS];
    fitMeans(f, mean);
    for (int b = 0; b < MIOPAL_STAT_BINS; ++b)
        ceiling[b] = std::isnan(mean[b]) ? INT32_MAX : clampToInt32(std::floor(mean[b] + excludeZ * f.sigma));
}

// zCut and the table: a target of bin b is a hit iff score >= threshold[b]
static void fitThresholds(MiopalScoreFit* f, double maxEvalue) {
    for (int b = 0; b < MIOPAL_STAT_BINS; ++b) f->threshold[b] = INT32_MAX;
    f->zCut = 0;
    if (f->degenerate || f->targets <= 0) return;
    double mean[MIOPAL_STAT_BINS];
    fitMeans(*f, mean);
    const double p = maxEvalue / (double)f->targets;
    if (p >= 1) {
        f->zCut = -INFINITY;
        for (int b = 1; b < MIOPAL_STAT_BINS; ++b)
            if (!std::isnan(mean[b])) f->threshold[b] = INT32_MIN;
        return;
    }
    f->zCut = -(std::log(-std::log1p(-p)) + kEulerGamma) / kGumbelScale;
    for (int b = 1; b < MIOPAL_STAT_BINS; ++b)
        if (!std::isnan(mean[b])) f->threshold[b] = clampToInt32(std::ceil(mean[b] + f->zCut * f->sigma));
}

static double fitEvalue(const MiopalScoreFit& f, const double* mean, int score, int bin) {
    const double z = ((double)score - mean[bin]) / f.sigma;
    return (double)f.targets * -std::expm1(-std::exp(-kGumbelScale * z - kEulerGamma));
}

static void emptyFit(MiopalScoreFit* f) {
    memset(f, 0, sizeof(*f));
    f->degenerate = 1;
    for (int b = 0; b < MIOPAL_STAT_BINS; ++b) f->ceiling[b] = f->threshold[b] = INT32_MAX;
}

// The handle's bin per target, built on the device from d_offsets at the first call and published - under the lock -
// only once the array is complete
static int ensureBins(MiopalDb* db, hipStream_t stream, const uint8_t** out) {
    std::lock_guard<std::mutex> g(db->binsMutex);
    if (!db->d_bins) {
        DeviceBytes fresh;
        HIP_TRY(hipMalloc(&fresh.p, (size_t)std::max<int64_t>(db->count, 16)));
        HIP_TRY(launchLengthBins(db->d_offsets, nullptr, db->count, (uint8_t*)fresh.p, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        db->d_bins = (uint8_t*)fresh.p;
        fresh.p = nullptr;
    }
    *out = db->d_bins;
    return 0;
}

static size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// the device scratch of the statistics of `rows` rows (kStatsScratch)
struct StatsScratch {
    int64_t* stats;        // [rows][bins][3]
    int32_t* ceiling;      // [rows][bins]
    int32_t* threshold;    // [rows][bins]
    int32_t* skip;         // [rows]: rows a pass leaves out
    int64_t* lengths;      // [bins][2]: targets and the sum of their lengths, of the slice
    static size_t bytes(int rows) {
        return pad256(sizeof(int64_t) * 3 * MIOPAL_STAT_BINS * (size_t)rows) +
               2 * pad256(sizeof(int32_t) * MIOPAL_STAT_BINS * (size_t)rows) + pad256(sizeof(int32_t) * (size_t)rows) +
               pad256(sizeof(int64_t) * 2 * MIOPAL_STAT_BINS);
    }
    StatsScratch(void* base, int rows) {
        char* p = (char*)base;
        stats = (int64_t*)p;
        p += pad256(sizeof(int64_t) * 3 * MIOPAL_STAT_BINS * (size_t)rows);
        ceiling = (int32_t*)p;
        p += pad256(sizeof(int32_t) * MIOPAL_STAT_BINS * (size_t)rows);
        threshold = (int32_t*)p;
        p += pad256(sizeof(int32_t) * MIOPAL_STAT_BINS * (size_t)rows);
        skip = (int32_t*)p;
        p += pad256(sizeof(int32_t) * (size_t)rows);
        lengths = (int64_t*)p;
    }
};

// What a call knows of its slice's lengths, gathered on the device once per call
struct SliceLengths {
    bool known = false;
    int64_t sums[MIOPAL_STAT_BINS][2];
};

// The significant hits of `rows` device rows of n scores (and end locations), enqueued on the workspace's stream behind
// what produced them: selectHitRows with the fit in front of it. Per row: one statistics pass, up to
// MIOPAL_FIT_MAX_REFITS passes under ceilings (all rows that still refit in one launch), the fit, the table; then the
// binned compaction. fits[r] and - when the hits were written - evalue (one per hit, in the order of the hits) are
// filled; rows with skip[r] != 0 keep nothing, are not read and leave fits[r] untouched.
static int significantRows(MiopalDb* db, Workspace* ws, Search* s, const int32_t* d_score, const int32_t* d_endI,
                           const int32_t* d_endJ, int rows, int64_t n, int64_t start, SliceLengths* lengths,
                           const double* maxEvalue, double excludeZ, const int* skip, int64_t room, MiopalScoreFit* fits,
                           HitRows* out, std::vector<double>* evalue) {
    constexpr size_t kRowStats = (size_t)3 * MIOPAL_STAT_BINS, kRowTable = MIOPAL_STAT_BINS;
    const uint8_t* bins;
    RC_TRY(ensureBins(db, ws->stream, &bins));
    void* p;
    RC_TRY(ws->get(kStatsScratch, StatsScratch::bytes(rows), &p));
    const StatsScratch sc(p, rows);
    std::vector<int64_t> host(kRowStats * (size_t)rows);
    std::vector<int> leftOut((size_t)rows, 0);
    for (int r = 0; r < rows; ++r) leftOut[(size_t)r] = skip && skip[r];
    StatsArgs a{};
    a.score = d_score;
    a.stride = n;
    a.rows = rows;
    a.bin = bins + start;
    a.skip = sc.skip;
    a.stats = sc.stats;
    auto pass = [&](bool withCeilings, bool first) -> int {
        RC_TRY(ws->stageUpload(sc.skip, leftOut.data(), sizeof(int) * (size_t)rows, ws->stream));
        HIP_TRY(hipMemsetAsync(sc.stats, 0, sizeof(int64_t) * kRowStats * (size_t)rows, ws->stream));
        a.ceiling = withCeilings ? sc.ceiling : nullptr;
        hipError_t e = launchRowsStats(a, ws->stream);
        if (e == hipSuccess && first && !lengths->known) {
            e = hipMemsetAsync(sc.lengths, 0, sizeof(lengths->sums), ws->stream);
            if (e == hipSuccess) e = launchLengthSums(db->d_offsets + start, n, sc.lengths, ws->stream);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "score statistics launch: %s", hipGetErrorString(e));
        }
        RC_TRY(ws->stageDownload(host.data(), sc.stats, sizeof(int64_t) * host.size()));
        if (first && !lengths->known) RC_TRY(ws->stageDownload(lengths->sums, sc.lengths, sizeof(lengths->sums)));
        if (first && s && s->d_stripError) RC_TRY(ws->stageDownload(&s->stripErrorHost, s->d_stripError, sizeof(int)));
        RC_TRY(ws->finishDownloads());
        if (first) lengths->known = true;
        if (first && s) RC_TRY(s->checkStripError());
        return 0;
    };
    // every target
    RC_TRY(pass(false, true));
    std::vector<int> refitting((size_t)rows, 0);
    for (int r = 0; r < rows; ++r) {
        if (leftOut[(size_t)r]) continue;
        MiopalScoreFit* f = &fits[r];
        emptyFit(f);
        for (int b = 0; b < MIOPAL_STAT_BINS; ++b) {
            f->binTargets[b] = lengths->sums[b][0];
            f->binLength[b] = lengths->sums[b][1];
            if (b >= 1) f->targets += f->binTargets[b];
        }
        memcpy(f->all, host.data() + kRowStats * (size_t)r, sizeof(f->all));
        memcpy(f->kept, f->all, sizeof(f->kept));
        f->passes = 1;
        fitLine(f);
        refitting[(size_t)r] = excludeZ > 0 && !f->degenerate;
    }
    // the upper tail left out: related sequences inflate the spread
    std::vector<int32_t> ceilings(kRowTable * (size_t)rows, INT32_MAX);
    for (int refit = 1; refit <= MIOPAL_FIT_MAX_REFITS; ++refit) {
        bool any = false;
        for (int r = 0; r < rows; ++r) {
            if (!refitting[(size_t)r]) continue;
            int32_t* next = ceilings.data() + kRowTable * (size_t)r;
            fitCeilings(fits[r], excludeZ, next);
            if (memcmp(next, fits[r].ceiling, sizeof(fits[r].ceiling)) == 0) refitting[(size_t)r] = 0;   // (they repeat)
            any = any || refitting[(size_t)r];
        }
        if (!any) break;
        for (int r = 0; r < rows; ++r) leftOut[(size_t)r] = !refitting[(size_t)r];
        RC_TRY(ws->stageUpload(sc.ceiling, ceilings.data(), sizeof(int32_t) * ceilings.size(), ws->stream));
        RC_TRY(pass(true, false));
        for (int r = 0; r < rows; ++r) {
            if (!refitting[(size_t)r]) continue;
            MiopalScoreFit* f = &fits[r];
            memcpy(f->kept, host.data() + kRowStats * (size_t)r, sizeof(f->kept));
            memcpy(f->ceiling, ceilings.data() + kRowTable * (size_t)r, sizeof(f->ceiling));
            ++f->passes;
            fitLine(f);
            if (f->degenerate) refitting[(size_t)r] = 0;
        }
    }
    // the tables and the compaction
    std::vector<int32_t> table(kRowTable * (size_t)rows, INT32_MAX);
    for (int r = 0; r < rows; ++r) {
        if (skip && skip[r]) continue;
        fitThresholds(&fits[r], maxEvalue[r]);
        memcpy(table.data() + kRowTable * (size_t)r, fits[r].threshold, sizeof(fits[r].threshold));
    }
    RC_TRY(ws->stageUpload(sc.threshold, table.data(), sizeof(int32_t) * table.size(), ws->stream));
    BinnedArgs binned{bins + start, sc.threshold};
    RC_TRY(selectHitRows(ws, nullptr, d_score, d_endI, d_endJ, rows, n, start, nullptr, skip, room, out, &binned));
    evalue->clear();
    if (!out->written || out->total() == 0) return 0;
    evalue->resize((size_t)out->total());
    for (int r = 0; r < rows; ++r) {
        double mean[MIOPAL_STAT_BINS];
        if (out->rowOffset[(size_t)r + 1] > out->rowOffset[(size_t)r]) fitMeans(fits[r], mean);
        for (int64_t h = out->rowOffset[(size_t)r]; h < out->rowOffset[(size_t)r + 1]; ++h) {
            const int64_t t = out->hits.target[h];
            const int bin = lengthBin(db->offsets[(size_t)t + 1] - db->offsets[(size_t)t]);
            (*evalue)[(size_t)h] = fitEvalue(fits[r], mean, out->hits.score[h], bin);
        }
    }
    return 0;
}

// what the three forms check beside their Hits counterparts' checks
static int checkSignificantArgs(const void* fit, double** evalue) {
    if (!fit) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null fit output");
    if (!evalue) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null evalue output");
    return 0;
}
static int checkEvalueCut(double maxEvalue, double excludeZ) {
    if (!std::isfinite(maxEvalue) || !(maxEvalue > 0)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "maxEvalue must be finite and positive");
    if (std::isnan(excludeZ)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "excludeZ is not a number");
    return 0;
}

// One query: searchHitsImpl with the fit and the table in the place of minScore
static int searchSignificantImpl(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                                 const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                                 int64_t end, double maxEvalue, double excludeZ, int64_t room, SliceLengths* lengths,
                                 MiopalScoreFit* fit, HitRows* out, std::vector<double>* evalue,
                                 const int* pssmRows = nullptr) {
    const int64_t n = end - start;
    if (pssmRows && n > 0) RC_TRY(checkPssmRange(db, pssmRows, queryLength, alphabetLength, gapOpen, gapExt));
    out->rowOffset.assign(2, 0);
    out->written = true;
    evalue->clear();
    if (n == 0) {
        emptyFit(fit);
        return 0;
    }
    ScoreRows rows(db, query, queryLength, gapOpen, gapExt, scoreMatrix, pssmRows, alphabetLength, searchType, mode, start, end);
    RC_TRY(rows.run());
    MiopalScoreFit got;
    RC_TRY(significantRows(db, rows.ws, &rows.s, rows.d_score, rows.d_endI, rows.d_endJ, 1, n, start, lengths, &maxEvalue,
                           excludeZ, nullptr, room, &got, out, evalue));
    *fit = got;
    return 0;
}

// the malloc'ed E-values of an answer (null without hits)
static int mallocEvalues(const std::vector<double>& ev, double** out) {
    *out = nullptr;
    if (ev.empty()) return 0;
    *out = (double*)malloc(sizeof(double) * ev.size());
    if (!*out) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
    memcpy(*out, ev.data(), sizeof(double) * ev.size());
    return 0;
}

// the end of miopalSearchSignificant / miopalSearchPssmSignificant: finishHits with the E-values beside the arrays
static int finishSignificant(HitRows& rows, const std::vector<double>& ev, int searchType, int64_t maxHits, int64_t* count,
                             int64_t** targetIndex, int** score, int** endTarget, int** endQuery, double** evalue) {
    double* e = nullptr;
    if (rows.written) RC_TRY(mallocEvalues(ev, &e));
    const int rc = finishHits(rows, searchType, maxHits, count, targetIndex, score, endTarget, endQuery);
    if (rc == 0) *evalue = e;
    else free(e);
    return rc;
}

// miopalSearchBatchSignificant: searchBatchHitsImpl with a fit per query
static int searchBatchSignificantImpl(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                                      int open, int ext, const int* matrix, int A, int searchType, int mode, int64_t start,
                                      int64_t end, const double* maxEvalue, double excludeZ, int64_t maxHits,
                                      MiopalScoreFit* fits, int64_t* hitOffsets, int64_t** targetIndex, int** score,
                                      int** endTarget, int** endQuery, double** evalue) {
    for (int c = 0; c < 4; ++c) g_lastBatchRouting[c] = 0;
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchBatchSignificant: alignments are not selected on the device");
    RC_TRY(validateBatch(db, queries, queryOffsets, nQueries, matrix, A, searchType, mode, start, end));
    RC_TRY(checkHitsOutputs(searchType, hitOffsets, targetIndex, score, endTarget, endQuery));
    if (!evalue) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null evalue output");
    if (nQueries > 0 && !maxEvalue) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null maxEvalue list");
    if (nQueries > 0 && !fits) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null fits output");
    for (int i = 0; i < nQueries; ++i) RC_TRY(checkEvalueCut(maxEvalue[i], excludeZ));
    if (std::isnan(excludeZ)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "excludeZ is not a number");
    const bool locate = searchType == OPAL_SEARCH_SCORE_END;
    const int64_t n = end - start;
    HitPieces pieces(nQueries, maxHits);
    std::vector<MiopalScoreFit> got((size_t)nQueries);
    for (auto& f : got) emptyFit(&f);
    SliceLengths lengths;
    if (n > 0 && nQueries > 0) {
        ScoreModel model{open, ext, 0, 0};
        scoreExtremes(matrix, (size_t)A * A, &model.maxScore, &model.minScore);
        BatchSink sink;
        sink.checkOutputs = [](bool) { return 0; };
        sink.chunk = [&](Workspace* ws, int64_t i0, int rows, int32_t* d_score, int32_t* d_endI, int32_t* d_endJ) -> int {
            std::vector<int> skip;
            skippedRows(queries, queryOffsets, i0, rows, model, matrix, A, searchType, mode, db->maxLen, &skip);
            std::unique_ptr<HitRows> rowsGot(new HitRows());
            std::vector<double> ev;
            RC_TRY(significantRows(db, ws, nullptr, d_score, d_endI, d_endJ, rows, n, start, &lengths, maxEvalue + i0, excludeZ,
                                   skip.data(), pieces.room(), got.data() + i0, rowsGot.get(), &ev));
            pieces.take(i0, std::move(rowsGot), std::move(ev));
            return 0;
        };
        sink.single = [&](int i) -> int {
            std::unique_ptr<HitRows> rowsGot(new HitRows());
            std::vector<double> ev;
            RC_TRY(searchSignificantImpl(db, queries + queryOffsets[i], (int)(queryOffsets[i + 1] - queryOffsets[i]), open, ext,
                                         matrix, A, searchType, mode, start, end, maxEvalue[i], excludeZ, pieces.room(),
                                         &lengths, &got[(size_t)i], rowsGot.get(), &ev));
            pieces.take(i, std::move(rowsGot), std::move(ev));
            return 0;
        };
        RC_TRY(batchImpl(db, queries, queryOffsets, nQueries, open, ext, matrix, A, searchType, mode, start, end, sink));
    }
    // nothing failed: the outputs are written from here on (the fits also when there are too many hits)
    RC_TRY(pieces.reserve(locate, true));
    for (int i = 0; i < nQueries; ++i) fits[i] = got[(size_t)i];
    return pieces.assemble(nQueries, locate, hitOffsets, targetIndex, score, endTarget, endQuery, evalue);
}

// miopalTestRowStats (test hook): length_bins_kernel and rows_stats_kernel alone, on rows the caller supplies -
// launchRowsStats as significantRows calls it, with no search and no handle in front of it. Device 0.
static int testRowStatsImpl(const int* score, int rows, int64_t stride, const int32_t* length, const int32_t* ceiling,
                            const int* skip, int64_t* stats, unsigned char* bin) {
    constexpr int64_t kMaxEntries = (int64_t)1 << 27;
    if (rows < 1 || stride < 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "rows = %d, stride = %lld: both at least 1", rows, (long long)stride);
    if (!score || !length) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null score rows / lengths");
    if (!stats || !bin) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null stats / bin outputs");
    if (stride > kMaxEntries || rows > kMaxEntries / stride)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "%d rows x %lld entries: more than 2^27", rows, (long long)stride);
    for (int64_t i = 0; i < stride; ++i)
        if (length[i] < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative length at %lld", (long long)i);
    if (physicalDeviceCount() < 1) return fail(OPAL_ERR_NO_SIMD_SUPPORT, "no usable gfx950 device");
    HIP_TRY(hipSetDevice(usableDevices()[0]));

    const size_t inBytes = sizeof(int32_t) * (size_t)rows * (size_t)stride;
    const size_t statBytes = sizeof(int64_t) * 3 * MIOPAL_STAT_BINS * (size_t)rows;
    const size_t tableBytes = sizeof(int32_t) * MIOPAL_STAT_BINS * (size_t)rows;
    DeviceBytes dScore, dLength, dBin, dCeiling, dSkip, dStats;
    OwnedStream stream;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&dScore.p, inBytes));
    HIP_TRY(hipMalloc(&dLength.p, sizeof(int32_t) * (size_t)stride));
    HIP_TRY(hipMalloc(&dBin.p, (size_t)stride));
    HIP_TRY(hipMalloc(&dStats.p, statBytes));
    HIP_TRY(hipMemcpyAsync(dScore.p, score, inBytes, hipMemcpyHostToDevice, stream.s));
    HIP_TRY(hipMemcpyAsync(dLength.p, length, sizeof(int32_t) * (size_t)stride, hipMemcpyHostToDevice, stream.s));
    HIP_TRY(hipMemsetAsync(dStats.p, 0, statBytes, stream.s));
    if (ceiling) {
        HIP_TRY(hipMalloc(&dCeiling.p, tableBytes));
        HIP_TRY(hipMemcpyAsync(dCeiling.p, ceiling, tableBytes, hipMemcpyHostToDevice, stream.s));
    }
    if (skip) {
        HIP_TRY(hipMalloc(&dSkip.p, sizeof(int) * (size_t)rows));
        HIP_TRY(hipMemcpyAsync(dSkip.p, skip, sizeof(int) * (size_t)rows, hipMemcpyHostToDevice, stream.s));
    }
    HIP_TRY(launchLengthBins(nullptr, (const int32_t*)dLength.p, stride, (uint8_t*)dBin.p, stream.s));
    StatsArgs a{};
    a.score = (const int32_t*)dScore.p;
    a.stride = stride;
    a.rows = rows;
    a.bin = (const uint8_t*)dBin.p;
    a.skip = (const int32_t*)dSkip.p;
    a.ceiling = (const int32_t*)dCeiling.p;
    a.stats = (int64_t*)dStats.p;
    const hipError_t e = launchRowsStats(a, stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIOPAL_ERR_HIP, "score statistics launch: %s", hipGetErrorString(e));
    }
    std::vector<int64_t> hostStats((size_t)3 * MIOPAL_STAT_BINS * (size_t)rows);
    std::vector<unsigned char> hostBin((size_t)stride);
    HIP_TRY(hipMemcpyAsync(hostStats.data(), dStats.p, statBytes, hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipMemcpyAsync(hostBin.data(), dBin.p, (size_t)stride, hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipStreamSynchronize(stream.s));
    memcpy(stats, hostStats.data(), statBytes);
    memcpy(bin, hostBin.data(), (size_t)stride);
    return 0;
}
