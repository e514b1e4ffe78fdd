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

// what the stage leaves for the entry point: malloc'ed like the occurrences' own arrays
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
};

}  // namespace

// The stage itself, shared with the panel form (host_batch_occurrence_align.inc): the `total` occurrences whose arrays
// dScore / dRow / dColumn lie in the workspace of `s` and whose host copies are `hits`, chunk by chunk in output order.
// `s` holds the query buffer (ensurePairInputs has run or runs here): the call's one query, or a panel chunk's queries
// end to end; Q = its tallest query, which sizes the chunks. gather(c0, nc, targetOff, &qBase) enqueues what fills
// targetOff[0 .. nc) for the occurrences c0 .. c0 + nc and names their query origins (null: all at 0). What the
// chunks did is added to `routing` (the figures of miopalLastOccurrenceAlignRouting).
using OccurrenceGather = std::function<int(int64_t c0, int nc, int64_t* targetOff, const int32_t** qBase)>;

// ... in three steps, so that the PSSM panel can run the chunks over one stretch of the occurrences after another, each
// with a query buffer of its own (host_batch_occurrence_align_pssm.inc): the arrays for all `total` occurrences,
static int allocOccurrenceAlignment(int64_t total, bool operations, OccurrenceAlignment* out) {
    out->startT = (int*)malloc(sizeof(int) * (size_t)total);
    out->startQ = (int*)malloc(sizeof(int) * (size_t)total);
    if (operations) out->opsOff = (int64_t*)malloc(sizeof(int64_t) * (size_t)(total + 1));
    if (!out->startT || !out->startQ || (operations && !out->opsOff)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
    if (operations) out->opsOff[0] = 0;
    return 0;
}

// the chunks of the occurrences first .. last (stretches are taken in ascending order, none left out: the operations
// are appended and opsOff[first] is the stretch before's last entry),
static int alignOccurrenceRange(Search& s, int64_t first, int64_t last, const HitArrays& hits, const int32_t* dScore,
                                const int32_t* dRow, const int32_t* dColumn, int Q, bool operations,
                                const OccurrenceGather& gather, int64_t* routing, OccurrenceAlignment* out) {
    MiopalDb* const db = s.db;
    Workspace* const ws = s.ws;
    int64_t maxL = 1;
    for (int64_t k = first; k < last; ++k) maxL = std::max<int64_t>(maxL, dbLen(db, hits.target[k]));
    const int64_t cap = pairChunkCapacity(Q, maxL, operations);
    const bool waveOnly = Q > kPairLaneMaxQuery || cap < kLanes;
    const bool forceLane = tuned(Tune::FORCE_LANE_PER_PAIR) != nullptr;
    const bool tableFits = !s.pssmRows || perPairPssmBytes(s.Q, s.A) != 0;   // (the whole buffer's rows are the table)
    const bool oneStrip = Q <= kLanes;
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
        RC_TRY(gather(c0, nc, (int64_t*)ptoff, &pqbase));
        int headWaves = 0;
        LaterPasses lp{};
        lp.db = db; lp.s = &s;
        lp.mode = s.mode; lp.open = s.open; lp.ext = s.ext; lp.A = s.A; lp.totalQuery = s.Q;
        lp.nc = nc; lp.maxL = chunkL; lp.oneStrip = oneStrip; lp.fwdWsStride = oneStrip ? 0 : chunkL;
        lp.lane = lane; lp.lanePossible = lanePossible; lp.forceLane = forceLane;
        lp.score = dScore + c0; lp.endI = dRow + c0; lp.endJ = dColumn + c0;
        lp.tOff = (const int64_t*)ptoff; lp.qBase = pqbase;
        lp.jobs = (PairJob*)pjobs; lp.sorted = (PairJob*)psorted; lp.bins = (int*)pbins; lp.head = (int*)phead;
        lp.startsOnly = !operations; lp.endsOnHost = true;
        lp.consumer = nullptr; lp.pairs = nullptr; lp.noun = "occurrence";
        lp.idOf = [c0](int k) { return (long long)(c0 + k); };
        lp.hs = hits.score + c0; lp.hi = hits.endQ + c0; lp.hj = hits.endT + c0;
        lp.hsq = &hsq; lp.hst = &hst; lp.hlen = &hlen; lp.hts = &hts; lp.outOps = &out->ops;
        lp.traceHeadWaves = &headWaves;
        RC_TRY(runLaterPasses(lp));
        for (int k = 0; k < nc; ++k) {
            out->startQ[c0 + k] = hsq[(size_t)k];
            out->startT[c0 + k] = hst[(size_t)k];
            if (operations) out->opsOff[c0 + k + 1] = out->opsOff[c0 + k] + hlen[(size_t)k];
        }
        if (operations) {
            const int64_t toWave = lp.traceLane ? std::min<int64_t>(nc, (int64_t)headWaves * kLanes) : nc;
            routing[0] += nc - toWave;
            routing[1] += toWave;
        }
        routing[2] += 1;
        routing[3] = std::max(routing[3], lp.maxWindow);
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

static int alignOccurrenceChunks(Search& s, int64_t total, const HitArrays& hits, const int32_t* dScore, const int32_t* dRow,
                                 const int32_t* dColumn, int Q, bool operations, const OccurrenceGather& gather,
                                 int64_t* routing, OccurrenceAlignment* out) {
    RC_TRY(allocOccurrenceAlignment(total, operations, out));
    RC_TRY(alignOccurrenceRange(s, 0, total, hits, dScore, dRow, dColumn, Q, operations, gather, routing, out));
    return finishOccurrenceAlignment(total, operations, out);
}

static int alignOccurrencesStage(const OccurrencesOnDevice& o, bool operations, OccurrenceAlignment* out) {
    Search& s = *o.s;
    const OccurrenceGather gather = [&](int64_t c0, int nc, int64_t* targetOff, const int32_t**) {
        HIP_TRY(launchOccurrencePairInputs(nc, o.target + c0, s.db->d_offsets, s.db->count, targetOff, s.stream));
        return 0;
    };
    return alignOccurrenceChunks(s, o.total, *o.hits, o.score, o.row, o.column, s.Q, operations, gather,
                                 g_lastOccurrenceAlignRouting, out);
}

// Behind the entry points' checks: the sweeps with the stage behind them, then the outputs - all of them, or none.
static int searchOccurrencesAlignedImpl(MiopalDb* db, const unsigned char* query, int Q, int open, int ext, const int* matrix,
                                        const int* pssmRows, int A, int mode, int64_t start, int64_t end, int minScore,
                                        int window, int64_t maxHits, int64_t* count, int64_t** targetIndex, int** score,
                                        int** endTarget, int** endQuery, int** startTarget, int** startQuery,
                                        unsigned char** alignments, int64_t** alignmentOffsets) {
    for (int k = 0; k < 4; ++k) g_lastOccurrenceAlignRouting[k] = 0;
    const bool operations = alignments != nullptr;
    OccurrenceAlignment got;
    // (without occurrences the offsets still hold their single 0: reserved before anything is written)
    int64_t* none = nullptr;
    struct FreeNone {
        int64_t*& p;
        ~FreeNone() { free(p); }
    } guard{none};
    if (operations) {
        none = (int64_t*)malloc(sizeof(int64_t));
        if (!none) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        none[0] = 0;
    }
    const OccurrenceStage stage = [&](const OccurrencesOnDevice& o) { return alignOccurrencesStage(o, operations, &got); };
    // (the stage has run, or there was nothing to run it on, when this returns 0: nothing below can fail)
    RC_TRY(searchOccurrencesImpl(db, query, Q, open, ext, matrix, pssmRows, A, mode, start, end, minScore, window, maxHits,
                                 count, targetIndex, score, endTarget, endQuery, &stage));
    if (*count == 0) {
        *startTarget = *startQuery = nullptr;
        if (operations) {
            *alignments = nullptr;
            *alignmentOffsets = none;
            none = nullptr;
        }
        return 0;
    }
    *startTarget = got.startT;
    *startQuery = got.startQ;
    got.startT = got.startQ = nullptr;
    if (operations) {
        *alignments = got.ops.release();
        *alignmentOffsets = got.opsOff;
        got.opsOff = nullptr;
    }
    return 0;
}
