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

// the mode, the window and the cut: the refusals of an occurrence search that need no handle
int checkOccurrenceRule(int mode, int minScore, int window) {
    if (mode != OPAL_MODE_HW && mode != OPAL_MODE_SW)
        return fail(OPAL_ERR_INVALID_MODE, "occurrences are defined for OPAL_MODE_HW and OPAL_MODE_SW, not for mode %d", mode);
    if (window < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative window %d", window);
    if (mode == OPAL_MODE_SW && minScore < 1)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "minScore = %d: OPAL_MODE_SW needs a cut of at least 1", minScore);
    return 0;
}

// The occurrences where the write sweep left them, for a stage that goes on with them on the device
// (host_occurrence_align.inc): entry k is (target[k], score[k], row[k], column[k]), `total` entries each in the
// workspace of `s`; `hits` holds the same arrays on the host, already down.
struct OccurrencesOnDevice {
    Search* s;
    int64_t total;
    const int64_t* target;
    const int32_t *score, *row, *column;
    const HitArrays* hits;
    int region;
};
using OccurrenceStage = std::function<int(const OccurrencesOnDevice&)>;

}  // namespace

// One sweep (count: list == null, every target of the slice; write: the `listed` targets of `list`), chunk by chunk
static int occurrenceSweep(Search& s, OccurrenceArgs a, int region, bool write, const int32_t* list, int64_t targets) {
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
        const hipError_t e = write ? launchOccurrencesWrite(a, region, s.stream) : launchOccurrencesCount(a, region, s.stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "occurrence sweep launch (%s): %s", write ? "write" : "count", hipGetErrorString(e));
        }
        g_lastOccurrenceRouting[2] += 1;
    }
    g_lastOccurrenceRouting[write ? 1 : 0] += targets;
    return 0;
}

// Behind the entry points' checks. `matrix` or `pssmRows` is the score source (the other null; with rows, `query` is
// the filler consensus). Nothing is written to the outputs before the last step that can fail. `stage`: what
// miopalSearchOccurrencesAligned runs behind the download of the occurrences; the two entry points of this file pass none.
static int searchOccurrencesImpl(MiopalDb* db, const unsigned char* query, int Q, int open, int ext, const int* matrix,
                                 const int* pssmRows, int A, int mode, int64_t start, int64_t end, int minScore,
                                 int window, int64_t maxHits, int64_t* count, int64_t** targetIndex, int** score,
                                 int** endTarget, int** endQuery, const OccurrenceStage* stage = nullptr) {
    for (int k = 0; k < 4; ++k) g_lastOccurrenceRouting[k] = 0;
    const int64_t n = end - start;
    auto nothing = [&] {
        *count = 0;
        *targetIndex = nullptr;
        *score = *endTarget = *endQuery = nullptr;
        return 0;
    };
    if (n == 0) return nothing();   // (an empty slice: checked and answered, nothing launched)
    Search s{db, nullptr, nullptr, query, Q, open, ext, A, OPAL_SEARCH_SCORE_END, mode, matrix, start, end, n};
    s.pssmRows = pssmRows;
    RC_TRY(s.prepare());
    RC_TRY(checkInt32Range(s.model(), Q, db->maxLen));   // miopalSearch's range check: 32-bit arithmetic only
    g_lastOccurrenceRouting[3] = (Q + kLanes - 1) / kLanes;
    if (Q == 0 || db->maxLen == 0) return nothing();      // an empty query, or nothing but empty targets
    const int region = mode == OPAL_MODE_HW ? kLastRow : kAllCells;
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
    a.gapOpen = open;
    a.gapExt = ext;
    a.minScore = minScore;
    a.window = window;
    a.start = start;
    a.count = sc.count;
    RC_TRY(occurrenceSweep(s, a, region, false, nullptr, n));
    {
        const hipError_t e = launchOccurrencesOffsets(sc, n, s.stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "occurrence offsets launch: %s", hipGetErrorString(e));
        }
    }
    int64_t totals[2] = {0, 0};
    RC_TRY(ws->stageDownload(totals, sc.totals, sizeof totals));
    RC_TRY(ws->finishDownloads());
    const int64_t total = totals[0], listed = totals[1];
    if (total < 0 || listed < 0 || listed > n || listed > total)
        return fail(MIOPAL_ERR_INTERNAL, "occurrence counts: total %lld in %lld targets", (long long)total, (long long)listed);
    if (maxHits >= 0 && total > maxHits) {
        *count = total;
        return fail(MIOPAL_ERR_TOO_MANY_HITS, "%lld occurrences, maxHits = %lld", (long long)total, (long long)maxHits);
    }
    if (total == 0) return nothing();
    HitArrays hits;
    RC_TRY(hits.alloc(total, true));
    const HitsOutSlot slot(total, true);
    void* po;
    RC_TRY(ws->get(kOccurrenceOut, slot.bytes, &po));
    char* base = (char*)po;
    a.count = nullptr;
    a.offsets = sc.offsets;
    a.outTarget = (int64_t*)base;
    a.outScore = (int32_t*)(base + slot.offScore);
    a.outRow = (int32_t*)(base + slot.offEndQ);
    a.outColumn = (int32_t*)(base + slot.offEndT);
    RC_TRY(occurrenceSweep(s, a, region, true, sc.list, listed));
    RC_TRY(ws->stageDownload(hits.target, a.outTarget, sizeof(int64_t) * (size_t)total));
    RC_TRY(ws->stageDownload(hits.score, a.outScore, sizeof(int) * (size_t)total));
    RC_TRY(ws->stageDownload(hits.endQ, a.outRow, sizeof(int) * (size_t)total));
    RC_TRY(ws->stageDownload(hits.endT, a.outColumn, sizeof(int) * (size_t)total));
    RC_TRY(ws->finishDownloads());
    // (a stage behind the sweeps takes the occurrences where they are, in the workspace this call holds)
    if (stage) RC_TRY((*stage)(OccurrencesOnDevice{&s, total, a.outTarget, a.outScore, a.outRow, a.outColumn, &hits, region}));
    *count = total;
    hits.release(targetIndex, score, endTarget, endQuery);
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
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIOPAL_ERR_HIP, "occurrence picker launch (count): %s", hipGetErrorString(e));
    }
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
        e = launchOccurrencesWrite(a, kLastRow, stream.s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "occurrence picker launch (write): %s", hipGetErrorString(e));
        }
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
