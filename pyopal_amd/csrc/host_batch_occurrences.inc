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
// (A chunk goes through named steps, DESIGN 8p: plan, upload, count, bounds, write, stage.)
namespace {

thread_local int64_t g_lastBatchOccurrenceRouting[4] = {0, 0, 0, 0};   // miopalLastBatchOccurrenceRouting
thread_local int64_t g_lastBatchOccurrenceGroups[3] = {0, 0, 0};       // miopalLastBatchOccurrenceGroups

static_assert(sizeof(OccurrenceMeta) == sizeof(int4) && alignof(OccurrenceMeta) <= alignof(int4), "the kernels read the meta array as int4");

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

// The panel: its score source and its lists. Plain: `residues` / `offsets` are the queries, `matrix` [A][A], rowScores
// null. PSSM: rowScores holds A ints per row, `offsets` delimits the PSSMs in rows, `residues` is the consensus (never
// null here: a filler of 255s where the caller gave none) in the same row coordinates; matrix is null.
struct PanelSide {
    const unsigned char* residues;
    const int64_t* offsets;
    int nQueries;
    const int* matrix;
    const int* rowScores;
    const int *minScore, *window;
    bool pssm() const { return rowScores != nullptr; }
    int rows(int i) const { return (int)(offsets[i + 1] - offsets[i]); }
    const int* rowsOf(int i, int A) const { return pssm() ? rowScores + (size_t)offsets[i] * A : nullptr; }
};

// One chunk of panel queries on its way through the steps: panel[0 .. cq) of the call's list. A stage gets it behind
// the write sweep and reads rq, side, ws, panel, cq, total, head / dHead, dScores, slot and hits; the rest is the sweeps'.
struct PanelChunk {
    const OccurrenceRequest& rq;
    const PanelSide& side;
    Workspace* ws;
    const void* dMatrix;
    const int* panel;
    int cq;
    const OccurrenceChunkPlan& plan;
    int region = 0;
    int64_t n = 0, N = 0;              // targets of the slice, entries of the count array
    BatchOccurrenceArgs a{};
    OccurrenceScratch sc{};
    int64_t* dHead = nullptr;          // head[0 .. cq], total, listed (occurrences_batch.h)
    int32_t* dFirst = nullptr;
    const int32_t* dScores = nullptr;  // PSSM: the chunk's rows end to end
    std::vector<int64_t> head;
    int64_t total = 0, listed = 0;
    OccurrenceOutSlot slot;            // the occurrences where the write sweep left them, `total` entries each,
    const HitArrays* hits = nullptr;   // and on the host
};

}  // namespace

// (the stages of the aligned calls, which take a chunk as it is)
#include "host_batch_occurrence_align.inc"
#include "host_batch_occurrence_align_pssm.inc"

namespace {

// where a query's occurrences lie until the CSR is put together; aligned (the aligned call): the starts of the piece
// `from`, entry for entry, and its operations - those of the stretch are opsOff[first] .. opsOff[first + count]
struct OccurrenceStretch {
    const HitArrays* from = nullptr;
    int64_t first = 0, count = 0;
    const OccurrenceAlignment* aligned = nullptr;
};

// What a panel call collects until the splice: per query of the list its count and its stretch; the pieces the stretches
// point into (one per panel chunk or long query, with its alignment in the aligned call); the occurrences so far, and
// whether they have passed maxHits - from then on everything is only counted.
struct PanelPieces {
    bool aligned, operations;
    std::vector<int64_t> counts;
    std::vector<OccurrenceStretch> stretch;
    std::deque<HitArrays> hits;   // (deques: a new piece leaves the stretches' pointers to the others valid)
    std::deque<OccurrenceAlignment> alignments;
    int64_t running = 0;
    bool over = false;
    PanelPieces(int nQueries, const OccurrenceOutputs& out)
        : aligned(out.aligned), operations(out.operations()), counts((size_t)nQueries, 0), stretch((size_t)nQueries) {}
};

// the sorted jobs of a chunk of the slice's targets (kSortedJobs), kept from one chunk of queries to the next
struct SliceJobs {
    int64_t of = -1;
    void* sorted = nullptr;
};

}  // namespace

// Upload: the plan's row list (plain) or row-source map and the chunk's PSSM rows end to end (PSSM), the entries of the
// queries and groups; and the arguments both sweeps share.
static int uploadPanelChunk(PanelChunk& c) {
    Workspace* const ws = c.ws;
    hipStream_t stream = ws->stream;
    const int A = c.rq.A, cq = c.cq;
    const OccurrenceChunkPlan& plan = c.plan;
    c.n = c.rq.end - c.rq.start;
    c.N = (int64_t)cq * c.n;
    c.region = c.rq.mode == OPAL_MODE_HW ? kLastRow : kAllCells;
    void *prows, *pmeta, *pbounds, *pscratch;
    BatchOccurrenceArgs& a = c.a;
    if (c.side.pssm()) {
        std::vector<int> chunkRows;
        for (int q = 0; q < cq; ++q)
            chunkRows.insert(chunkRows.end(), c.side.rowsOf(c.panel[q], A), c.side.rowsOf(c.panel[q] + 1, A));
        void* pscores;
        RC_TRY(ws->get(kBatchOccurrenceRowSource, plan.rowSource.size() * sizeof(int32_t), &prows));
        RC_TRY(ws->get(kPssmRows, chunkRows.size() * sizeof(int32_t), &pscores));
        RC_TRY(ws->stageUpload(prows, plan.rowSource.data(), plan.rowSource.size() * sizeof(int32_t), stream));
        RC_TRY(ws->stageUpload(pscores, chunkRows.data(), chunkRows.size() * sizeof(int32_t), stream));
        a.rowSource = (const int32_t*)prows;
        a.rows = c.dScores = (const int32_t*)pscores;
    } else {
        RC_TRY(ws->get(kQuery, plan.rowResidue.size(), &prows));
        RC_TRY(ws->stageUpload(prows, plan.rowResidue.data(), plan.rowResidue.size(), stream));
        a.rowResidue = (const uint8_t*)prows;
        a.matrix = (const int32_t*)c.dMatrix;
    }
    RC_TRY(ws->get(kBatchOccurrenceMeta, plan.meta.size() * sizeof(OccurrenceMeta), &pmeta));
    RC_TRY(ws->get(kBatchOccurrenceBounds, ((size_t)cq + 3) * sizeof(int64_t) + ((size_t)cq + 1) * sizeof(int32_t), &pbounds));
    RC_TRY(ws->get(kOccurrenceScratch, occurrenceScratchBytes(c.N), &pscratch));
    RC_TRY(ws->stageUpload(pmeta, plan.meta.data(), plan.meta.size() * sizeof(OccurrenceMeta), stream));
    c.sc = occurrenceScratchLayout(pscratch, c.N);
    c.dHead = (int64_t*)pbounds;
    c.dFirst = (int32_t*)(c.dHead + cq + 3);
    a.residues = c.rq.db->d_residues;
    a.query = (const int4*)pmeta;
    a.group = a.query + cq;
    a.nQueries = cq;
    a.alphabet = A;
    a.gapOpen = c.rq.open;
    a.gapExt = c.rq.ext;
    a.n = c.n;
    a.count = c.sc.count;
    a.start = c.rq.start;
    return 0;
}

// The count sweep: every target of the slice, in chunks of jobs sorted by length
static int countPanelChunk(PanelChunk& c, SliceJobs& jobs) {
    Workspace* const ws = c.ws;
    MiopalDb* const db = c.rq.db;
    const bool pssm = c.side.pssm();
    for (int64_t c0 = 0; c0 < c.n; c0 += kPairChunkMax) {
        const int nc = (int)std::min<int64_t>(kPairChunkMax, c.n - c0);
        if (jobs.of != c0) {
            void *pjobs, *pbins;
            RC_TRY(ws->get(kJobs, (size_t)nc * sizeof(PairJob), &pjobs));
            RC_TRY(ws->get(kSortedJobs, (size_t)nc * sizeof(PairJob), &jobs.sorted));
            RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
            HIP_TRY(launchOccurrenceJobs(nullptr, c0, nc, c.rq.start, db->d_offsets, 0, (PairJob*)pjobs, ws->stream));
            HIP_TRY(launchSortJobsByLength((const PairJob*)pjobs, nc, (int)db->maxLen, (int*)pbins, (PairJob*)jobs.sorted, ws->stream));
            jobs.of = c0;
        }
        c.a.jobs = (const PairJob*)jobs.sorted;
        c.a.nJobs = nc;
        RC_TRY(launched((pssm ? launchBatchOccurrencesCountPssm : launchBatchOccurrencesCount)(
                            c.a, c.region, c.plan.groups, batchOccurrenceLdsBytes(c.plan.widest, c.rq.A), ws->stream),
                        "panel occurrence sweep launch (count)"));
    }
    return 0;
}

// The scan of the counts and the bounds, one small download - every query's offset and the totals - and its sanity check
static int boundsOfPanelChunk(PanelChunk& c) {
    Workspace* const ws = c.ws;
    const int cq = c.cq;
    hipError_t e = launchOccurrencesOffsets(c.sc, c.N, ws->stream);
    if (e == hipSuccess) e = launchBatchOccurrencesBounds(c.sc, c.n, cq, c.dFirst, c.dHead, ws->stream);
    RC_TRY(launched(e, "panel occurrence offsets launch"));
    std::vector<int64_t>& head = c.head;
    head.assign((size_t)cq + 3, 0);
    RC_TRY(ws->stageDownload(head.data(), c.dHead, sizeof(int64_t) * head.size()));
    RC_TRY(ws->finishDownloads());
    const int64_t total = c.total = head[(size_t)cq + 1], listed = c.listed = head[(size_t)cq + 2];
    bool sane = head[0] == 0 && head[(size_t)cq] == total && total >= 0 && listed >= 0 && listed <= c.N && listed <= total;
    for (int q = 0; q < cq && sane; ++q) sane = head[(size_t)q + 1] >= head[(size_t)q];
    if (!sane) return fail(MIOPAL_ERR_INTERNAL, "panel occurrence counts: total %lld in %lld pairs", (long long)total, (long long)listed);
    return 0;
}

// The write sweep over the listed pairs, and the chunk's occurrences down into `hits`
static int writePanelChunk(PanelChunk& c, HitArrays* hits) {
    Workspace* const ws = c.ws;
    RC_TRY(hits->alloc(c.total, true));
    RC_TRY(c.slot.get(ws, c.total));
    BatchOccurrenceArgs& a = c.a;
    a.count = nullptr;
    a.offsets = c.sc.offsets;
    a.list = c.sc.list;
    a.first = c.dFirst;
    a.dbOffsets = c.rq.db->d_offsets;
    a.outTarget = c.slot.target;
    a.outScore = c.slot.score;
    a.outRow = c.slot.row;
    a.outColumn = c.slot.column;
    RC_TRY(launched((c.side.pssm() ? launchBatchOccurrencesWritePssm : launchBatchOccurrencesWrite)(
                        a, c.region, c.listed, batchOccurrenceLdsBytes(c.plan.tallest, c.rq.A), ws->stream),
                    "panel occurrence sweep launch (write)"));
    c.hits = hits;
    return c.slot.download(ws, c.total, hits);
}

// The panel queries `panel` (indices into the call's list, ascending, 1 .. 64 rows each), chunk by chunk. counts[i]
// and stretch[i] of `got` are filled for every one of them; once got->running passes maxHits (got->over) the chunks are
// only counted. The aligned call: the alignment stage runs behind every write sweep, and never once `over` is set.
static int batchOccurrencePanel(const OccurrenceRequest& rq, const PanelSide& side, const std::vector<int>& panel, PanelPieces* got) {
    MiopalDb* const db = rq.db;
    const int64_t n = rq.end - rq.start;
    HIP_TRY(hipSetDevice(db->device));
    WorkspaceLease lease(db);
    RC_TRY(lease.acquireInternal());
    Workspace* ws = lease.ws;
    void* pmatrix = nullptr;
    if (!side.pssm()) {
        RC_TRY(ws->get(kMatrix, (size_t)rq.A * rq.A * sizeof(int32_t), &pmatrix));
        RC_TRY(ws->stageUpload(pmatrix, side.matrix, (size_t)rq.A * rq.A * sizeof(int32_t), ws->stream));
    }
    const int64_t perChunk = occurrenceChunkQueries(batchOccurrenceEntries(), n);
    const int64_t wantGroups = occurrenceWantGroups(n, kPairChunkMax, batchOccurrenceWorkgroupsPerCu(), db->computeUnits);
    OccurrenceChunkPlan plan;
    SliceJobs jobs;
    size_t p0 = 0;
    for (const int cq : occurrenceChunkSizes(perChunk, panel.size())) {
        planOccurrenceChunk(side.pssm() ? nullptr : side.residues, side.offsets, side.minScore, side.window, panel.data() + p0, cq,
                            rq.A, wantGroups, (int64_t)kCuLdsBytes, &plan);
        g_lastBatchOccurrenceGroups[0] += plan.groups;
        g_lastBatchOccurrenceGroups[1] = std::max(g_lastBatchOccurrenceGroups[1], plan.mostQueries);
        g_lastBatchOccurrenceGroups[2] = std::max<int64_t>(g_lastBatchOccurrenceGroups[2], (int64_t)batchOccurrenceLdsBytes(plan.widest, rq.A));
        PanelChunk c{rq, side, ws, pmatrix, panel.data() + p0, cq, plan};
        p0 += (size_t)cq;
        RC_TRY(uploadPanelChunk(c));
        RC_TRY(countPanelChunk(c, jobs));
        RC_TRY(boundsOfPanelChunk(c));
        g_lastBatchOccurrenceRouting[2] += 1;
        got->running += c.total;
        if (rq.maxHits >= 0 && got->running > rq.maxHits) got->over = true;
        for (int q = 0; q < cq; ++q) got->counts[(size_t)c.panel[q]] = c.head[(size_t)q + 1] - c.head[(size_t)q];
        if (got->over || c.total == 0) continue;
        HitArrays& hits = got->hits.emplace_back();
        RC_TRY(writePanelChunk(c, &hits));
        g_lastBatchOccurrenceRouting[3] += c.listed;
        OccurrenceAlignment* aligned = nullptr;
        if (got->aligned) {
            // the stage, on the occurrences where they are (head[0 .. cq] still lies behind dHead; a PSSM panel's rows stay
            // in kPssmRows). It takes kJobs, kSortedJobs and kSortBins: the next count sweep sorts the slice's jobs again.
            aligned = &got->alignments.emplace_back();
            jobs = SliceJobs{};
            RC_TRY((side.pssm() ? alignPssmBatchOccurrencesStage : alignBatchOccurrencesStage)(c, got->operations, aligned));
        }
        for (int q = 0; q < cq; ++q)
            got->stretch[(size_t)c.panel[q]] = OccurrenceStretch{&hits, c.head[(size_t)q], c.head[(size_t)q + 1] - c.head[(size_t)q], aligned};
    }
    return 0;
}

// The long queries: the single-query search, its refusals (the strip workspace) what they are. Its sweeps count into a
// scratch array (miopalLastOccurrenceRouting belongs to the thread's last single-query CALL), its stage into the panel's
// reporter. Once the bound is passed (`over`) the later ones still run their count sweeps, with no room: hitOffsets is
// filled for every query also when there are too many hits, and nothing is written or downloaded for them.
static int batchOccurrenceLongQueries(const OccurrenceRequest& rq, const PanelSide& side, const std::vector<int>& single, PanelPieces* got) {
    int64_t routing[4];
    for (int i : single) {
        int64_t found = 0;
        OccurrenceRequest one = rq;
        one.maxHits = got->over ? 0 : rq.maxHits < 0 ? -1 : rq.maxHits - got->running;
        HitArrays& hits = got->hits.emplace_back();
        // (aligned: the single-query stage behind its write sweep - it does not run when the bound is passed)
        OccurrenceAlignment* const aligned = got->aligned ? &got->alignments.emplace_back() : nullptr;
        const OccurrenceStage stage = [&](const OccurrencesOnDevice& o) {
            return alignOccurrencesStage(o, got->operations, g_lastBatchOccurrenceAlignRouting, aligned);
        };
        const OccurrenceQuery q{side.residues + side.offsets[i], side.rows(i), side.matrix, side.rowsOf(i, rq.A), side.minScore[i], side.window[i]};
        const int rc = searchOccurrencesImpl(one, q, &found, &hits, got->aligned ? &stage : nullptr, routing);
        if (rc == MIOPAL_ERR_TOO_MANY_HITS) got->over = true;
        else if (rc) return rc;
        got->counts[(size_t)i] = found;
        got->running += found;
        if (!got->over) got->stretch[(size_t)i] = OccurrenceStretch{&hits, 0, found, found > 0 ? aligned : nullptr};
    }
    return 0;
}

// Behind the checks of either form: the range check of every query, the routing, the pieces and the splice.
static int batchOccurrencesCore(const OccurrenceRequest& rq, const PanelSide& side, const OccurrenceOutputs& out) {
    MiopalDb* const db = rq.db;
    const int nQueries = side.nQueries, A = rq.A;
    PanelPieces got(nQueries, out);
    if (rq.end > rq.start && nQueries > 0) {
        // miopalSearch's range check (32-bit arithmetic only), for every query before any device work (a PSSM: with
        // the extreme entries of its own rows)
        ScoreModel model{rq.open, rq.ext, 0, 0};
        if (!side.pssm()) scoreExtremes(side.matrix, (size_t)A * A, &model.maxScore, &model.minScore);
        std::vector<int> panel, single;
        for (int i = 0; i < nQueries; ++i) {
            const int Q = side.rows(i);
            if (side.pssm()) RC_TRY(checkPssmRange(db, side.rowsOf(i, A), Q, A, rq.open, rq.ext));
            else RC_TRY(checkInt32Range(model, Q, db->maxLen));
            if (Q > kLanes) single.push_back(i);
            else if (Q > 0) panel.push_back(i);
        }
        g_lastBatchOccurrenceRouting[0] = (int64_t)panel.size();
        g_lastBatchOccurrenceRouting[1] = (int64_t)single.size();
        RC_TRY(batchOccurrenceLongQueries(rq, side, single, &got));
        if (!panel.empty() && db->maxLen > 0) RC_TRY(batchOccurrencePanel(rq, side, panel, &got));
    }
    const int64_t running = got.running;
    HitArrays all;
    if (!got.over) RC_TRY(all.alloc(running, true));
    // (aligned: the starts, the rebased offsets and room for the operations)
    OccurrenceAlignment joined;
    if (got.aligned && !got.over) {
        RC_TRY(joined.reserve(running, got.operations));
        if (got.operations) {
            int64_t at = 0, nOps = 0;
            for (int i = 0; i < nQueries; ++i) {
                const OccurrenceStretch& s = got.stretch[(size_t)i];
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
    int64_t* const hitOffsets = out.counts;
    hitOffsets[0] = 0;
    for (int i = 0; i < nQueries; ++i) hitOffsets[i + 1] = hitOffsets[i] + got.counts[(size_t)i];
    if (got.over) return fail(MIOPAL_ERR_TOO_MANY_HITS, "%lld occurrences, maxHits = %lld", (long long)running, (long long)rq.maxHits);
    for (int i = 0; i < nQueries; ++i) {
        const OccurrenceStretch& s = got.stretch[(size_t)i];
        if (s.count == 0) continue;
        const size_t at = (size_t)hitOffsets[i], len = (size_t)s.count;
        memcpy(all.target + at, s.from->target + s.first, sizeof(int64_t) * len);
        memcpy(all.score + at, s.from->score + s.first, sizeof(int) * len);
        memcpy(all.endT + at, s.from->endT + s.first, sizeof(int) * len);
        memcpy(all.endQ + at, s.from->endQ + s.first, sizeof(int) * len);
        if (!got.aligned) continue;
        memcpy(joined.startT + at, s.aligned->startT + s.first, sizeof(int) * len);
        memcpy(joined.startQ + at, s.aligned->startQ + s.first, sizeof(int) * len);
        if (got.operations)
            memcpy(joined.ops.data + joined.opsOff[at], s.aligned->ops.data + s.aligned->opsOff[s.first],
                   (size_t)(joined.opsOff[at + len] - joined.opsOff[at]));
    }
    all.release(out.targetIndex, out.score, out.endTarget, out.endQuery);
    if (got.aligned) joined.release(out);
    return 0;
}

// what the reporters of the panel occurrence searches say starts over with every call, plain or PSSM
static void resetBatchOccurrenceReports(bool wantAligned) {
    for (int k = 0; k < 4; ++k) g_lastBatchOccurrenceRouting[k] = 0;
    for (int k = 0; k < 3; ++k) g_lastBatchOccurrenceGroups[k] = 0;
    if (wantAligned)
        for (int k = 0; k < 4; ++k) g_lastBatchOccurrenceAlignRouting[k] = 0;
}

// miopalSearchBatchOccurrences(Aligned). Behind nothing: the checks of miopalSearchOccurrences over the whole list, in
// its order, come first; the aligned form's four outputs behind endQuery are checked with the others.
static int searchBatchOccurrencesImpl(const OccurrenceRequest& rq, const PanelSide& side, const OccurrenceOutputs& out) {
    resetBatchOccurrenceReports(out.aligned);
    RC_TRY(validateBatch(rq.db, side.residues, side.offsets, side.nQueries, side.matrix, rq.A, OPAL_SEARCH_SCORE_END, rq.mode, rq.start, rq.end));
    RC_TRY(checkOccurrenceRule(rq.mode, side.nQueries, side.minScore, side.window, "query"));
    RC_TRY(out.check());
    return batchOccurrencesCore(rq, side, out);
}

// miopalSearchPssmBatchOccurrences(Aligned): what needs no handle first, in the single PSSM calls' order with the plain
// panel's per-query checks among it, then the handle and what depends on it; the range check of every PSSM, with the
// extreme entries of its own rows, is the core's. `side` as the caller gave it: the consensus may be null.
static int searchPssmBatchOccurrencesImpl(const OccurrenceRequest& rq, PanelSide side, const OccurrenceOutputs& out) {
    MiopalDb* const db = rq.db;
    const int nPssms = side.nQueries, A = rq.A, mode = rq.mode;
    const int64_t* const rowOffsets = side.offsets;
    resetBatchOccurrenceReports(out.aligned);
    if (mode < OPAL_MODE_NW || mode > OPAL_MODE_SW) return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", mode);
    RC_TRY(checkOccurrenceRule(mode, 0, nullptr, nullptr, nullptr));
    if (nPssms < 0 || (nPssms > 0 && !rowOffsets)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad PSSM list");
    for (int m = 0; m < nPssms; ++m)
        if (rowOffsets[m] < 0 || rowOffsets[m + 1] < rowOffsets[m]) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad row offsets at %d", m);
    const int64_t first = nPssms > 0 ? rowOffsets[0] : 0, totalRows = nPssms > 0 ? rowOffsets[nPssms] - first : 0;
    if (totalRows > INT32_MAX - 64) return fail(MIOPAL_ERR_BAD_ARGUMENT, "the PSSMs of a panel hold 2^31 - 65 rows at most");
    if (totalRows > 0 && !side.rowScores) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null row scores");
    if (A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad alphabet length %d", A);
    RC_TRY(checkOccurrenceRule(mode, nPssms, side.minScore, side.window, "PSSM"));
    RC_TRY(out.check());
    if (out.aligned) RC_TRY(checkConsensus(side.residues, first, totalRows, A, out.alignments != nullptr));
    // (a PSSM of more than 64 rows takes the single sweep, which keeps its rows in LDS)
    for (int i = 0; i < nPssms; ++i) RC_TRY(checkOccurrenceTableFits(rowOffsets[i + 1] - rowOffsets[i], A, i));
    if (!db) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null database handle");
    if (A != db->alphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d differs from the database's %d", A, db->alphabet);
    if (rq.start < 0 || rq.end < rq.start || rq.end > db->count)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad slice [%lld, %lld)", (long long)rq.start, (long long)rq.end);
    // (without a consensus - the plain form, starts only - every position is "no residue": the kernels never read it)
    std::vector<unsigned char> none;
    if (!out.aligned || !side.residues) {
        none.assign((size_t)(first + std::max<int64_t>(totalRows, 1)), 255);   // (indexed in the offsets' coordinates)
        side.residues = none.data();
    }
    static const int64_t kNoPssms[1] = {0};
    static const int kNoPanelRows[1] = {0};   // (no rows: the score source still says "position-specific")
    if (nPssms == 0) side.offsets = kNoPssms;
    if (totalRows == 0) side.rowScores = kNoPanelRows;
    return batchOccurrencesCore(rq, side, out);
}
