// Part of host.hip (included there, not a translation unit of its own): the alignment stage of the panel occurrence
// search, miopalSearchBatchOccurrencesAligned - where every occurrence of a panel starts and, when asked for, its
// operations. The call itself is host_batch_occurrences.inc's with this stage behind every write sweep.
//
// Per panel chunk that has occurrences, in the workspace the chunk holds: the chunk's queries go up once more, end to
// end WITHOUT the pad rows of the sweep's row list (the later passes of a `full` pair list index a query buffer by
// origin + row), with their cq + 1 origins beside them. The occurrences stay where the write sweep left them, in
// output order - query after query, target ascending, column ascending - and are taken in sub-chunks sized as the
// pair list sizes its chunks, from the tallest query of the chunk and the longest target that has an occurrence
// (alignOccurrenceChunks, host_occurrence_align.inc). Per sub-chunk batch_occurrence_origins_kernel
// (occurrence_align_batch.hip) gathers each occurrence's target origin from the handle's offsets and its query's
// origin from its position: the chunk's head[0 .. cq] - occurrences in front of each query - still lies in the
// kBatchOccurrenceBounds slot behind launchBatchOccurrencesBounds. Then runLaterPasses with that qBase, one strip
// (every panel query has at most 64 rows). Up over PCIe: the concatenated queries and cq + 1 origins per chunk; nothing
// of the occurrence list. Down: starts - and lengths and operations - per sub-chunk, appended in output order.
namespace {

thread_local int64_t g_lastBatchOccurrenceAlignRouting[4] = {0, 0, 0, 0};   // miopalLastBatchOccurrenceAlignRouting

}  // namespace

// What either panel stage gathers per sub-chunk: each occurrence's target origin and, from its position among
// head[0 .. nq] (the occurrences in front of each of nq queries, on the device), its query's origin dQOff[query].
static OccurrenceGather panelOccurrenceGather(const PanelChunk& o, const int64_t* head, int nq, const int32_t* dQOff) {
    return [&o, head, nq, dQOff](int64_t c0, int nc, int64_t* targetOff, const int32_t** qBase) {
        void* pqbase;
        RC_TRY(o.ws->get(kPairListQBase, (size_t)nc * sizeof(int32_t), &pqbase));
        HIP_TRY(launchBatchOccurrenceOrigins(nc, c0, o.slot.target + c0, o.rq.db->d_offsets, o.rq.db->count, head, nq, dQOff, targetOff,
                                             (int32_t*)pqbase, o.ws->stream));
        *qBase = (const int32_t*)pqbase;
        return 0;
    };
}

// Takes kQuery (where the chunk's row list lay: the write sweep that read it is in front of this upload in stream
// order, and the next chunk uploads its own list), kMatrix (the same matrix again) and, through the shared stage,
// kJobs / kSortedJobs / kSortBins: the caller's sorted jobs of the slice are gone afterwards.
static int alignBatchOccurrencesStage(const PanelChunk& o, bool operations, OccurrenceAlignment* out) {
    Workspace* const ws = o.ws;
    std::vector<unsigned char> concat;
    std::vector<int32_t> qOff((size_t)o.cq + 1, 0);
    int tallest = 0;
    for (int q = 0; q < o.cq; ++q) {
        const int i = o.panel[q];
        qOff[(size_t)q] = (int32_t)concat.size();
        concat.insert(concat.end(), o.side.residues + o.side.offsets[i], o.side.residues + o.side.offsets[i + 1]);
        tallest = std::max(tallest, (int)(o.side.offsets[i + 1] - o.side.offsets[i]));
    }
    qOff[(size_t)o.cq] = (int32_t)concat.size();
    Search s{o.rq.db, ws, ws->stream, concat.data(), (int)concat.size(), o.rq.open, o.rq.ext, o.rq.A, OPAL_SEARCH_ALIGNMENT, o.rq.mode,
             o.side.matrix, 0, o.rq.db->count, o.total};
    RC_TRY(s.prepare());
    RC_TRY(s.ensurePairInputs());
    void* pqoff;
    RC_TRY(ws->get(kPairListQOff, qOff.size() * sizeof(int32_t), &pqoff));
    RC_TRY(ws->stageUpload(pqoff, qOff.data(), qOff.size() * sizeof(int32_t), s.stream));
    const OccurrenceGather gather = panelOccurrenceGather(o, o.dHead, o.cq, (const int32_t*)pqoff);
    return alignOccurrenceChunks(s, o.total, OccurrenceAlignJob{o.hits, o.slot, tallest, operations, &gather,
                                                                g_lastBatchOccurrenceAlignRouting, out});
}
