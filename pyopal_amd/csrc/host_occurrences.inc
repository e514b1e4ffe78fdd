// Part of host.hip (included there, not a translation unit of its own): miopalSearchOccurrences,
// miopalSearchPssmOccurrences - every occurrence of one query (one PSSM) in each target of a slice, picked on the device
// (occurrences.hip) - and the hook miopalTestPickOccurrences.
//
// Two sweeps of the lane-per-target kernel with the host between them (host_hits.inc's pattern): the count sweep over
// the slice's targets, the scan of the counts (which also lists the targets that have occurrences, in database
// order), one download of {total, listed targets}; the outputs are sized to the total and the write sweep runs over
// the listed targets alone. Both sweeps take their targets in chunks (what the strip boundaries of a query of more
// than 64 rows allow), each chunk's jobs built from the handle's d_offsets and sorted by length as the pair list sorts
// them, so that a wavefront's lanes end together; job.out keeps the position in the slice. Only the occurrences cross
// PCIe. Targets longer than a lane should own (the pair list hands those to the wavefront-per-pair kernel) are swept
// like the others.
namespace {

thread_local int64_t g_lastOccurrenceRouting[4] = {0, 0, 0, 0};   // miopalLastOccurrenceRouting

// The strip workspace of a query of more than 64 rows: per column and lane the boundary row (8 bytes) and, under SW,
// the column's running maximum beside it (8 more), for whole wavefronts of 64 targets, within 2 GB.
constexpr int64_t kOccurrenceStripBytes = 2ll << 30;
inline int64_t occurrenceColumnBytes(int region) { return region == kAllCells ? 16 : 8; }
// the longest target such a query may meet: one wavefront's columns must fit (2M columns under SW, 4M under HW)
inline int64_t occurrenceLongestTarget(int region) { return kOccurrenceStripBytes / (occurrenceColumnBytes(region) * kLanes); }
// targets a chunk may hold (a multiple of 64, at least 64: searchOccurrencesImpl has refused longer targets)
int64_t occurrenceChunkCapacity(int Q, int region, int64_t maxL) {
    int64_t cap = kPairChunkMax;
    if (Q > kLanes)
        cap = std::min<int64_t>(cap, kOccurrenceStripBytes / (occurrenceColumnBytes(region) * std::max<int64_t>(maxL, 1)) / kLanes * kLanes);
    return std::max<int64_t>(cap, kLanes);
}

// a launcher's answer: 0, or its failure under the launch's name (the error is taken off the runtime)
int launched(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    return fail(MIOPAL_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// The checks the family shares; the entry points and the panel forms make them in their own orders.
// The consensus beside a PSSM's rows first .. first + rows, in every entry point that takes one (the pair list's and the
// profile's included): `required` (operations are asked for) there must be one; every residue is a letter or 255, "none".
int checkConsensus(const unsigned char* consensus, int64_t first, int64_t rows, int A, bool required) {
    if (required && rows > 0 && !consensus) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null consensus for an alignment search");
    if (consensus)
        for (int64_t i = first; i < first + rows; ++i)
            if (consensus[i] >= A && consensus[i] != 255)
                return fail(MIOPAL_ERR_BAD_ARGUMENT, "consensus residue %d out of range at %lld", consensus[i], (long long)i);
    return 0;
}

// A PSSM of Q rows fits the LDS table of the single sweep, which keeps its rows there as the lane-per-pair kernels of a
// PSSM pair list do. panelIndex >= 0: PSSM number panelIndex of a panel, which takes that sweep with more than 64 rows only.
int checkOccurrenceTableFits(int64_t Q, int A, int panelIndex = -1) {
    if (panelIndex >= 0 && Q <= kLanes) return 0;
    if (Q <= INT32_MAX && perPairPssmBytes((int)Q, A) != 0) return 0;
    char which[48] = "";
    if (panelIndex >= 0) snprintf(which, sizeof which, "PSSM %d of the panel: ", panelIndex);
    return fail(MIOPAL_ERR_BAD_ARGUMENT, "%sa PSSM of %lld rows at %d letters does not fit the occurrence sweep's LDS table: "
                "(rows + 1) x (letters + 1) x 4 bytes within 64 KB less 256, %d rows at most", which, (long long)Q, A,
                (64 * 1024 - 256) / (4 * (A + 1)) - 1);
}

// The mode, the windows and the cuts of n queries: the refusals of an occurrence search that need no handle. `noun`
// ("query", "PSSM"): a panel's lists, whose texts say where; null: the one cut and window of the single form. (n = 0:
// the mode alone, which the PSSM panel checks ahead of its lists.)
int checkOccurrenceRule(int mode, int n, const int* minScore, const int* window, const char* noun) {
    if (mode != OPAL_MODE_HW && mode != OPAL_MODE_SW)
        return fail(OPAL_ERR_INVALID_MODE, "occurrences are defined for OPAL_MODE_HW and OPAL_MODE_SW, not for mode %d", mode);
    char at[40] = "";
    auto where = [&](int i) {
        if (noun) snprintf(at, sizeof at, " at %s %d", noun, i);
        return at;
    };
    for (int i = 0; window && i < n; ++i)
        if (window[i] < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative window %d%s", window[i], where(i));
    for (int i = 0; minScore && mode == OPAL_MODE_SW && i < n; ++i)
        if (minScore[i] < 1)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "minScore = %d%s: OPAL_MODE_SW needs a cut of at least 1", minScore[i], where(i));
    if (n > 0 && (!minScore || !window)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null minScore / window list");
    return 0;
}

// What every call of the family is given,
struct OccurrenceRequest {
    MiopalDb* db;
    int open, ext, A, mode;
    int64_t start, end, maxHits;
};

// one query with its cut and window: `matrix` or `pssmRows` is the score source (with rows, `residues` is the consensus),
struct OccurrenceQuery {
    const unsigned char* residues;
    int Q;
    const int *matrix, *pssmRows;
    int minScore, window;
};

// and the caller's outputs. counts: a single form's count, a panel form's hitOffsets. aligned: an Aligned form, with the
// four outputs behind endQuery - the starts always, the operations and their offsets together or not at all.
struct OccurrenceOutputs {
    int64_t* counts;
    int64_t** targetIndex;
    int **score, **endTarget, **endQuery;
    bool aligned = false;
    int **startTarget = nullptr, **startQuery = nullptr;
    unsigned char** alignments = nullptr;
    int64_t** alignmentOffsets = nullptr;
    bool operations() const { return aligned && alignments != nullptr; }
    int check() const {
        RC_TRY(checkHitsOutputs(OPAL_SEARCH_SCORE_END, counts, targetIndex, score, endTarget, endQuery));
        if (!aligned) return 0;
        if (!startTarget || !startQuery) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null start-location outputs");
        if ((alignments == nullptr) != (alignmentOffsets == nullptr))
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "alignments and alignmentOffsets: both, or neither (starts only)");
        return 0;
    }
};

// The device slot the write sweep fills (kOccurrenceOut), sized to the occurrences, and its way down into `hits`
struct OccurrenceOutSlot {
    int64_t* target = nullptr;
    int32_t *score = nullptr, *row = nullptr, *column = nullptr;
    int get(Workspace* ws, int64_t total) {
        const HitsOutSlot slot(total, true);
        void* po;
        RC_TRY(ws->get(kOccurrenceOut, slot.bytes, &po));
        char* base = (char*)po;
        target = (int64_t*)base;
        score = (int32_t*)(base + slot.offScore);
        row = (int32_t*)(base + slot.offEndQ);
        column = (int32_t*)(base + slot.offEndT);
        return 0;
    }
    int download(Workspace* ws, int64_t total, HitArrays* hits) const {
        RC_TRY(ws->stageDownload(hits->target, target, sizeof(int64_t) * (size_t)total));
        RC_TRY(ws->stageDownload(hits->score, score, sizeof(int) * (size_t)total));
        RC_TRY(ws->stageDownload(hits->endQ, row, sizeof(int) * (size_t)total));
        RC_TRY(ws->stageDownload(hits->endT, column, sizeof(int) * (size_t)total));
        return ws->finishDownloads();
    }
};

// The occurrences where the write sweep left them, for a stage that goes on with them on the device
// (host_occurrence_align.inc): `total` entries each in the workspace of `s`; `hits` holds the same arrays on the host.
struct OccurrencesOnDevice {
    Search* s;
    int64_t total;
    OccurrenceOutSlot slot;
    const HitArrays* hits;
};
using OccurrenceStage = std::function<int(const OccurrencesOnDevice&)>;

}  // namespace

// One sweep (count: list == null, every target of the slice; write: the `listed` targets of `list`), chunk by chunk
// (`routing`: the figures of miopalLastOccurrenceRouting, counted where the caller says)
static int occurrenceSweep(Search& s, OccurrenceArgs a, int region, bool write, const int32_t* list, int64_t targets,
                           int64_t* routing) {
    Workspace* ws = s.ws;
    const int64_t maxL = s.db->maxLen;
    const int64_t cap = occurrenceChunkCapacity(s.Q, region, maxL);
    for (int64_t c0 = 0; c0 < targets; c0 += cap) {
        const int nc = (int)std::min(cap, targets - c0);
        void *pjobs, *psorted, *pbins;
        RC_TRY(ws->get(kJobs, (size_t)nc * sizeof(PairJob), &pjobs));
        RC_TRY(ws->get(kSortedJobs, (size_t)nc * sizeof(PairJob), &psorted));
        RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
        HIP_TRY(launchOccurrenceJobs(list, c0, nc, s.start, s.db->d_offsets, s.Q, (PairJob*)pjobs, s.stream));
        HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, nc, (int)maxL, (int*)pbins, (PairJob*)psorted, s.stream));
        a.jobs = (const PairJob*)psorted;
        a.nJobs = nc;
        if (s.Q > kLanes) {
            // the boundary rows, and under SW the running maxima behind them
            const size_t each = boundaryBytes(nc, maxL);
            const bool carry = region == kAllCells;
            void* pb;
            RC_TRY(ws->get(kPairListBoundary, carry ? 2 * each : each, &pb));
            a.boundary = (int2*)pb;
            a.carry = carry ? (int2*)((char*)pb + each) : nullptr;
            a.boundaryStride = maxL;
        }
        RC_TRY(write ? launched(launchOccurrencesWrite(a, region, s.stream), "occurrence sweep launch (write)")
                     : launched(launchOccurrencesCount(a, region, s.stream), "occurrence sweep launch (count)"));
        routing[2] += 1;
    }
    routing[write ? 1 : 0] += targets;
    return 0;
}

// Behind the entry points' checks. Nothing is handed out before the last step that can fail: *found and `hits` (empty
// without occurrences) are the answer; with more than the request's maxHits, *found is their number all the same.
// `stage`: what the aligned forms run behind the download of the occurrences (null: none). `routing`: where the figures
// of miopalLastOccurrenceRouting are counted - the entry points pass the thread's, a panel's long query a scratch array.
static int searchOccurrencesImpl(const OccurrenceRequest& rq, const OccurrenceQuery& q, int64_t* found, HitArrays* hits,
                                 const OccurrenceStage* stage, int64_t* routing) {
    MiopalDb* const db = rq.db;
    const int Q = q.Q, A = rq.A;
    const int64_t start = rq.start, n = rq.end - rq.start, maxHits = rq.maxHits;
    for (int k = 0; k < 4; ++k) routing[k] = 0;
    *found = 0;
    if (n == 0) return 0;   // (an empty slice: checked and answered, nothing launched)
    Search s{db, nullptr, nullptr, q.residues, Q, rq.open, rq.ext, A, OPAL_SEARCH_SCORE_END, rq.mode, q.matrix, start, rq.end, n};
    s.pssmRows = q.pssmRows;
    RC_TRY(s.prepare());
    RC_TRY(checkInt32Range(s.model(), Q, db->maxLen));   // miopalSearch's range check: 32-bit arithmetic only
    routing[3] = (Q + kLanes - 1) / kLanes;
    if (Q == 0 || db->maxLen == 0) return 0;      // an empty query, or nothing but empty targets
    const int region = rq.mode == OPAL_MODE_HW ? kLastRow : kAllCells;
    if (Q > kLanes && db->maxLen > occurrenceLongestTarget(region))
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "a query of more than 64 rows against a database whose longest target has %lld "
                    "residues: the strip workspace of the occurrence sweep holds targets of %lld residues at most",
                    (long long)db->maxLen, (long long)occurrenceLongestTarget(region));

    HIP_TRY(hipSetDevice(db->device));
    WorkspaceLease lease(db);
    RC_TRY(lease.acquireInternal());
    Workspace* ws = s.ws = lease.ws;
    s.stream = ws->stream;
    RC_TRY(s.ensurePairInputs());
    void* pscratch;
    RC_TRY(ws->get(kOccurrenceScratch, occurrenceScratchBytes(n), &pscratch));
    const OccurrenceScratch sc = occurrenceScratchLayout(pscratch, n);
    OccurrenceArgs a{};
    a.residues = db->d_residues;
    a.query = s.d_query;
    a.matrix = s.d_matrix;
    a.rows = s.d_rows;
    a.queryLength = Q;
    a.alphabet = A;
    a.gapOpen = rq.open;
    a.gapExt = rq.ext;
    a.minScore = q.minScore;
    a.window = q.window;
    a.start = start;
    a.count = sc.count;
    RC_TRY(occurrenceSweep(s, a, region, false, nullptr, n, routing));
    RC_TRY(launched(launchOccurrencesOffsets(sc, n, s.stream), "occurrence offsets launch"));
    int64_t totals[2] = {0, 0};
    RC_TRY(ws->stageDownload(totals, sc.totals, sizeof totals));
    RC_TRY(ws->finishDownloads());
    const int64_t total = totals[0], listed = totals[1];
    if (total < 0 || listed < 0 || listed > n || listed > total)
        return fail(MIOPAL_ERR_INTERNAL, "occurrence counts: total %lld in %lld targets", (long long)total, (long long)listed);
    if (maxHits >= 0 && total > maxHits) {
        *found = total;
        return fail(MIOPAL_ERR_TOO_MANY_HITS, "%lld occurrences, maxHits = %lld", (long long)total, (long long)maxHits);
    }
    if (total == 0) return 0;
    RC_TRY(hits->alloc(total, true));
    OccurrenceOutSlot slot;
    RC_TRY(slot.get(ws, total));
    a.count = nullptr;
    a.offsets = sc.offsets;
    a.outTarget = slot.target;
    a.outScore = slot.score;
    a.outRow = slot.row;
    a.outColumn = slot.column;
    RC_TRY(occurrenceSweep(s, a, region, true, sc.list, listed, routing));
    RC_TRY(slot.download(ws, total, hits));
    // (a stage behind the sweeps takes the occurrences where they are, in the workspace this call holds)
    if (stage) RC_TRY((*stage)(OccurrencesOnDevice{&s, total, slot, hits}));
    *found = total;
    return 0;
}

// miopalTestPickOccurrences: the picker alone on rows the caller supplies, through the launchers of the search - count,
// offsets (and the list of the rows that have occurrences), write over the listed rows - one lane per row. Device 0.
static int testPickOccurrencesImpl(const int* value, const int* valueRow, int rows, int64_t stride, const int32_t* length,
                                   int minScore, int window, int64_t* hitOffsets, int32_t** column, int** score, int** row) {
    constexpr int64_t kMaxEntries = (int64_t)1 << 27;
    if (rows < 1 || stride < 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "rows = %d, stride = %lld: both at least 1", rows, (long long)stride);
    if (!value || !length) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null value rows / lengths");
    if (!hitOffsets || !column || !score || !row) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null hitOffsets / column / score / row outputs");
    if (stride > kMaxEntries || rows > kMaxEntries / stride)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "%d rows x %lld entries: more than 2^27", rows, (long long)stride);
    for (int r = 0; r < rows; ++r)
        if (length[r] < 0 || length[r] > stride)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "length %d of row %d outside [0, %lld]", length[r], r, (long long)stride);
    if (window < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative window %d", window);
    if (physicalDeviceCount() < 1) return fail(OPAL_ERR_NO_SIMD_SUPPORT, "no usable gfx950 device");
    HIP_TRY(hipSetDevice(usableDevices()[0]));

    const size_t inBytes = sizeof(int32_t) * (size_t)rows * (size_t)stride;
    DeviceBytes dValue, dValueRow, dLength, dScratch, dOut;
    OwnedStream stream;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&dValue.p, inBytes));
    HIP_TRY(hipMalloc(&dLength.p, sizeof(int32_t) * (size_t)rows));
    HIP_TRY(hipMalloc(&dScratch.p, occurrenceScratchBytes(rows)));
    HIP_TRY(hipMemcpyAsync(dValue.p, value, inBytes, hipMemcpyHostToDevice, stream.s));
    HIP_TRY(hipMemcpyAsync(dLength.p, length, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, stream.s));
    if (valueRow) {
        HIP_TRY(hipMalloc(&dValueRow.p, inBytes));
        HIP_TRY(hipMemcpyAsync(dValueRow.p, valueRow, inBytes, hipMemcpyHostToDevice, stream.s));
    }
    const OccurrenceScratch sc = occurrenceScratchLayout(dScratch.p, rows);
    OccurrenceArgs a{};
    a.value = (const int32_t*)dValue.p;
    a.valueRow = (const int32_t*)dValueRow.p;
    a.length = (const int32_t*)dLength.p;
    a.stride = stride;
    a.nJobs = rows;
    a.minScore = minScore;
    a.window = window;
    a.count = sc.count;
    hipError_t e = launchOccurrencesCount(a, kLastRow, stream.s);
    if (e == hipSuccess) e = launchOccurrencesOffsets(sc, rows, stream.s);
    RC_TRY(launched(e, "occurrence picker launch (count)"));
    std::vector<int64_t> rowOffset((size_t)rows + 1);
    int64_t totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(rowOffset.data(), sc.offsets, sizeof(int64_t) * rowOffset.size(), hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipMemcpyAsync(totals, sc.totals, sizeof totals, hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipStreamSynchronize(stream.s));
    const int64_t total = totals[0], listed = totals[1];
    if (total < 0 || total > (int64_t)rows * stride || total != rowOffset.back() || listed < 0 || listed > rows)
        return fail(MIOPAL_ERR_INTERNAL, "occurrence picker: total %lld in %lld rows", (long long)total, (long long)listed);
    int32_t *hc = nullptr, *hs = nullptr, *hr = nullptr;
    if (total > 0) {
        hc = (int32_t*)malloc(sizeof(int32_t) * (size_t)total);
        hs = (int32_t*)malloc(sizeof(int32_t) * (size_t)total);
        hr = (int32_t*)malloc(sizeof(int32_t) * (size_t)total);
        struct Free {
            int32_t *&a, *&b, *&c;
            bool keep = false;
            ~Free() {
                if (!keep) { free(a); free(b); free(c); }
            }
        } guard{hc, hs, hr};
        if (!hc || !hs || !hr) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        HIP_TRY(hipMalloc(&dOut.p, 3 * sizeof(int32_t) * (size_t)total));
        a.count = nullptr;
        a.nJobs = (int)listed;
        a.list = sc.list;
        a.offsets = sc.offsets;
        a.outColumn = (int32_t*)dOut.p;
        a.outScore = a.outColumn + total;
        a.outRow = a.outScore + total;
        RC_TRY(launched(launchOccurrencesWrite(a, kLastRow, stream.s), "occurrence picker launch (write)"));
        HIP_TRY(hipMemcpyAsync(hc, a.outColumn, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, stream.s));
        HIP_TRY(hipMemcpyAsync(hs, a.outScore, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, stream.s));
        HIP_TRY(hipMemcpyAsync(hr, a.outRow, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, stream.s));
        HIP_TRY(hipStreamSynchronize(stream.s));
        guard.keep = true;
    }
    memcpy(hitOffsets, rowOffset.data(), sizeof(int64_t) * rowOffset.size());
    *column = hc;
    *score = hs;
    *row = hr;
    return 0;
}
