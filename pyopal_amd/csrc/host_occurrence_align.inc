// Part of host.hip (included there, not a translation unit of its own): miopalSearchOccurrencesAligned,
// miopalSearchPssmOccurrencesAligned - the occurrence search (host_occurrences.inc) with the other end of every
// occurrence: where it starts and, when asked for, its operations.
//
// The stage runs behind the write sweep, in the workspace the search holds. The occurrences stay where the sweep left
// them: `score`, `row` and `column` of the output slot are the score / endI / endJ arrays of the later passes of a
// `full` pair list (runLaterPasses, host_pairs.inc), taken chunk by chunk as sub-arrays, and
// occurrence_pair_inputs_kernel (occurrence_align.hip) gathers each occurrence's target origin from the handle's
// d_offsets. The query is the call's one query (one PSSM: one table), at origin 0. Nothing of the list goes up over
// PCIe; the five arrays have come down once (searchOccurrencesImpl), starts - and lengths and operations - follow per
// chunk. Chunks are taken in occurrence order and sized as the pair list sizes them, from the query and the longest
// target that has an occurrence, so the operations concatenate in output order. One lane or one wavefront per
// occurrence: the estimates of full_plan.h, over the reversed prefixes (row + 1) x (column + 1) the scan sweeps.
// Starts only: the scan and the start cells, and chunks as large as a pair list without alignments takes.
namespace {

thread_local int64_t g_lastOccurrenceAlignRouting[4] = {0, 0, 0, 0};   // miopalLastOccurrenceAlignRouting

// What the stage leaves for the entry point (and a panel call splices into), malloc'ed like the occurrences' own arrays
struct OccurrenceAlignment {
    int *startT = nullptr, *startQ = nullptr;
    int64_t* opsOff = nullptr;
    HostBytes ops;
    OccurrenceAlignment() = default;
    OccurrenceAlignment(const OccurrenceAlignment&) = delete;
    OccurrenceAlignment& operator=(const OccurrenceAlignment&) = delete;
    ~OccurrenceAlignment() {
        free(startT);
        free(startQ);
        free(opsOff);
    }
    // the arrays for `total` occurrences; without any the starts stay null and the offsets hold their single 0
    int reserve(int64_t total, bool operations) {
        if (total > 0) {
            startT = (int*)malloc(sizeof(int) * (size_t)total);
            startQ = (int*)malloc(sizeof(int) * (size_t)total);
            if (!startT || !startQ) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        }
        if (operations) {
            opsOff = (int64_t*)malloc(sizeof(int64_t) * (size_t)(total + 1));
            if (!opsOff) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
            opsOff[0] = 0;
        }
        return 0;
    }
    // the arrays change hands (nothing here can fail: the last step of an aligned call)
    void release(const OccurrenceOutputs& to) {
        *to.startTarget = startT;
        *to.startQuery = startQ;
        startT = startQ = nullptr;
        if (!to.operations()) return;
        *to.alignments = ops.release();
        *to.alignmentOffsets = opsOff;
        opsOff = nullptr;
    }
};

}  // namespace

// The stage itself, shared with the panel form (host_batch_occurrence_align.inc): the occurrences whose arrays
// score / row / column lie in the workspace of `s` and whose host copies are `hits`, chunk by chunk in output order.
// `s` holds the query buffer (ensurePairInputs has run or runs here): the call's one query, or a panel chunk's queries
// end to end; Q = its tallest query, which sizes the chunks. gather(c0, nc, targetOff, &qBase) enqueues what fills
// targetOff[0 .. nc) for the occurrences c0 .. c0 + nc and names their query origins (null: all at 0). What the
// chunks did is added to `routing` (the figures of miopalLastOccurrenceAlignRouting, or of the panel's reporter).
using OccurrenceGather = std::function<int(int64_t c0, int nc, int64_t* targetOff, const int32_t** qBase)>;
struct OccurrenceAlignJob {
    const HitArrays* hits;
    OccurrenceOutSlot slot;
    int Q;
    bool operations;
    const OccurrenceGather* gather;
    int64_t* routing;
    OccurrenceAlignment* out;
};

// ... in three steps, so that the PSSM panel can run the chunks over one stretch of the occurrences after another, each
// with a query buffer of its own (host_batch_occurrence_align_pssm.inc): OccurrenceAlignment::reserve for all of them,
// the chunks of the occurrences first .. last (stretches are taken in ascending order, none left out: the operations
// are appended and opsOff[first] is the stretch before's last entry),
static int alignOccurrenceRange(Search& s, int64_t first, int64_t last, const OccurrenceAlignJob& job) {
    const HitArrays& hits = *job.hits;
    MiopalDb* const db = s.db;
    Workspace* const ws = s.ws;
    int64_t maxL = 1;
    for (int64_t k = first; k < last; ++k) maxL = std::max<int64_t>(maxL, dbLen(db, hits.target[k]));
    const int64_t cap = pairChunkCapacity(job.Q, maxL, job.operations);
    const bool waveOnly = job.Q > kPairLaneMaxQuery || cap < kLanes;
    const bool forceLane = tuned(Tune::FORCE_LANE_PER_PAIR) != nullptr;
    const bool tableFits = !s.pssmRows || perPairPssmBytes(s.Q, s.A) != 0;   // (the whole buffer's rows are the table)
    const bool oneStrip = job.Q <= kLanes;
    std::vector<int32_t> hsq, hst, hlen, hts;
    for (int64_t c0 = first; c0 < last; c0 += cap) {
        const int nc = (int)std::min(cap, last - c0);
        // the reversed prefixes of the chunk, in 64-row column steps (full_plan.h's estimates)
        double laneCols = 0, waveCols = 0, laneChain = 0, waveChain = 0;
        int chunkL = 1;
        for (int k = 0; k < nc; ++k) {
            const double strips = (double)pairStrips((int64_t)hits.endQ[c0 + k] + 1), L = (double)hits.endT[c0 + k] + 1;
            chunkL = std::max(chunkL, hits.endT[c0 + k] + 1);
            laneCols += strips * L;
            waveCols += strips * (L + 63);
            laneChain = std::max(laneChain, strips * L);
            waveChain = std::max(waveChain, strips * (L + 63));
        }
        const bool lanePossible = !waveOnly && tableFits && !tuned(Tune::NO_PERPAIR) && (nc > kSmallSearch || !smallSearchAllowed(db));
        const bool lane = lanePossible && (forceLane || scanLaneMs(laneCols, laneChain) <= scanWaveMs(waveCols, waveChain));
        void *ptoff, *pjobs, *pbins = nullptr, *psorted = nullptr, *phead = nullptr;
        RC_TRY(ws->get(kPairListTOff, (size_t)nc * sizeof(int64_t), &ptoff));
        RC_TRY(ws->get(kJobs, (size_t)nc * sizeof(PairJob), &pjobs));
        if (lanePossible) {
            RC_TRY(ws->get(kSortBins, (size_t)8192 * sizeof(int), &pbins));
            RC_TRY(ws->get(kSortedJobs, (size_t)nc * sizeof(PairJob), &psorted));
            RC_TRY(ws->get(kHeadWaves, sizeof(int), &phead));
        }
        const int32_t* pqbase = nullptr;
        RC_TRY((*job.gather)(c0, nc, (int64_t*)ptoff, &pqbase));
        int headWaves = 0;
        LaterPasses lp{};
        lp.db = db; lp.s = &s;
        lp.mode = s.mode; lp.open = s.open; lp.ext = s.ext; lp.A = s.A; lp.totalQuery = s.Q;
        lp.nc = nc; lp.maxL = chunkL; lp.oneStrip = oneStrip; lp.fwdWsStride = oneStrip ? 0 : chunkL;
        lp.lane = lane; lp.lanePossible = lanePossible; lp.forceLane = forceLane;
        lp.score = job.slot.score + c0; lp.endI = job.slot.row + c0; lp.endJ = job.slot.column + c0;
        lp.tOff = (const int64_t*)ptoff; lp.qBase = pqbase;
        lp.jobs = (PairJob*)pjobs; lp.sorted = (PairJob*)psorted; lp.bins = (int*)pbins; lp.head = (int*)phead;
        lp.startsOnly = !job.operations; lp.endsOnHost = true;
        lp.consumer = nullptr; lp.pairs = nullptr; lp.noun = "occurrence";
        lp.idOf = [c0](int k) { return (long long)(c0 + k); };
        lp.hs = hits.score + c0; lp.hi = hits.endQ + c0; lp.hj = hits.endT + c0;
        lp.hsq = &hsq; lp.hst = &hst; lp.hlen = &hlen; lp.hts = &hts; lp.outOps = &job.out->ops;
        lp.traceHeadWaves = &headWaves;
        RC_TRY(runLaterPasses(lp));
        for (int k = 0; k < nc; ++k) {
            job.out->startQ[c0 + k] = hsq[(size_t)k];
            job.out->startT[c0 + k] = hst[(size_t)k];
            if (job.operations) job.out->opsOff[c0 + k + 1] = job.out->opsOff[c0 + k] + hlen[(size_t)k];
        }
        if (job.operations) {
            const int64_t toWave = lp.traceLane ? std::min<int64_t>(nc, (int64_t)headWaves * kLanes) : nc;
            job.routing[0] += nc - toWave;
            job.routing[1] += toWave;
        }
        job.routing[2] += 1;
        job.routing[3] = std::max(job.routing[3], lp.maxWindow);
    }
    return 0;
}

// and what is checked behind the last stretch.
static int finishOccurrenceAlignment(int64_t total, bool operations, OccurrenceAlignment* out) {
    if (operations && (size_t)out->opsOff[total] != out->ops.size)
        return fail(MIOPAL_ERR_INTERNAL, "operation offsets disagree with the device");
    if (operations && !out->ops.data && !out->ops.resize(0)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
    return 0;
}

static int alignOccurrenceChunks(Search& s, int64_t total, const OccurrenceAlignJob& job) {
    RC_TRY(job.out->reserve(total, job.operations));
    RC_TRY(alignOccurrenceRange(s, 0, total, job));
    return finishOccurrenceAlignment(total, job.operations, job.out);
}

static int alignOccurrencesStage(const OccurrencesOnDevice& o, bool operations, int64_t* routing, OccurrenceAlignment* out) {
    Search& s = *o.s;
    const OccurrenceGather gather = [&](int64_t c0, int nc, int64_t* targetOff, const int32_t**) {
        HIP_TRY(launchOccurrencePairInputs(nc, o.slot.target + c0, s.db->d_offsets, s.db->count, targetOff, s.stream));
        return 0;
    };
    return alignOccurrenceChunks(s, o.total, OccurrenceAlignJob{o.hits, o.slot, s.Q, operations, &gather, routing, out});
}

// The single forms' last step: the count and the four arrays change hands - with too many occurrences their number alone
static int finishOccurrences(int rc, int64_t found, HitArrays& hits, const OccurrenceOutputs& out) {
    if (rc == MIOPAL_ERR_TOO_MANY_HITS) *out.counts = found;
    if (rc) return rc;
    *out.counts = found;
    hits.release(out.targetIndex, out.score, out.endTarget, out.endQuery);
    return 0;
}

// Behind the checks of the four single entry points: the sweeps, then the outputs - all of them, or none. An aligned
// call runs the stage behind the sweeps and hands its arrays over too; a plain call builds nothing for it.
static int searchOccurrencesCall(const OccurrenceRequest& rq, const OccurrenceQuery& q, const OccurrenceOutputs& out) {
    HitArrays hits;
    int64_t found = 0;
    if (!out.aligned)
        return finishOccurrences(searchOccurrencesImpl(rq, q, &found, &hits, nullptr, g_lastOccurrenceRouting), found, hits, out);
    for (int k = 0; k < 4; ++k) g_lastOccurrenceAlignRouting[k] = 0;
    const bool operations = out.operations();
    OccurrenceAlignment got;
    const OccurrenceStage stage = [&](const OccurrencesOnDevice& o) {
        return alignOccurrencesStage(o, operations, g_lastOccurrenceAlignRouting, &got);
    };
    int rc = searchOccurrencesImpl(rq, q, &found, &hits, &stage, g_lastOccurrenceRouting);
    // (the stage has run, or there was nothing to run it on: nothing behind the reserve can fail)
    if (rc == 0 && found == 0) rc = got.reserve(0, operations);
    RC_TRY(finishOccurrences(rc, found, hits, out));
    got.release(out);
    return 0;
}
