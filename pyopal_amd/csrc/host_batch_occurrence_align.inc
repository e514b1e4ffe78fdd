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

// A panel chunk's occurrences where the write sweep left them: entry k is (target[k], score[k], row[k], column[k]),
// `total` entries each in `ws`; head[0 .. cq] on the device (see above); `hits` holds the four arrays on the host.
// The chunk's queries are panel[0 .. cq) of the call's list. A PSSM panel (rowScores: the call's rows, else null;
// host_batch_occurrence_align_pssm.inc): `queries` is the consensus in the offsets' row coordinates, dRows the chunk's
// rows end to end where the sweeps read them, hostHead the host's copy of head[0 .. cq].
struct BatchOccurrencesOnDevice {
    MiopalDb* db;
    Workspace* ws;
    const unsigned char* queries;
    const int64_t* queryOffsets;
    const int* panel;
    int cq;
    int open, ext;
    const int* matrix;
    int A, mode;
    int64_t total;
    const int64_t* target;
    const int32_t *score, *row, *column;
    const int64_t* head;
    const HitArrays* hits;
    const int* rowScores = nullptr;
    const int32_t* dRows = nullptr;
    const int64_t* hostHead = nullptr;
};

}  // namespace

// Takes kQuery (where the chunk's row list lay: the write sweep that read it is in front of this upload in stream
// order, and the next chunk uploads its own list), kMatrix (the same matrix again) and, through the shared stage,
// kJobs / kSortedJobs / kSortBins: the caller's sorted jobs of the slice are gone afterwards.
static int alignBatchOccurrencesStage(const BatchOccurrencesOnDevice& o, bool operations, OccurrenceAlignment* out) {
    Workspace* const ws = o.ws;
    std::vector<unsigned char> concat;
    std::vector<int32_t> qOff((size_t)o.cq + 1, 0);
    int tallest = 0;
    for (int q = 0; q < o.cq; ++q) {
        const int i = o.panel[q];
        qOff[(size_t)q] = (int32_t)concat.size();
        concat.insert(concat.end(), o.queries + o.queryOffsets[i], o.queries + o.queryOffsets[i + 1]);
        tallest = std::max(tallest, (int)(o.queryOffsets[i + 1] - o.queryOffsets[i]));
    }
    qOff[(size_t)o.cq] = (int32_t)concat.size();
    Search s{o.db, ws, ws->stream, concat.data(), (int)concat.size(), o.open, o.ext, o.A, OPAL_SEARCH_ALIGNMENT, o.mode,
             o.matrix, 0, o.db->count, o.total};
    RC_TRY(s.prepare());
    RC_TRY(s.ensurePairInputs());
    void* pqoff;
    RC_TRY(ws->get(kPairListQOff, qOff.size() * sizeof(int32_t), &pqoff));
    RC_TRY(ws->stageUpload(pqoff, qOff.data(), qOff.size() * sizeof(int32_t), s.stream));
    const OccurrenceGather gather = [&](int64_t c0, int nc, int64_t* targetOff, const int32_t** qBase) {
        void* pqbase;
        RC_TRY(ws->get(kPairListQBase, (size_t)nc * sizeof(int32_t), &pqbase));
        HIP_TRY(launchBatchOccurrenceOrigins(nc, c0, o.target + c0, o.db->d_offsets, o.db->count, o.head, o.cq,
                                             (const int32_t*)pqoff, targetOff, (int32_t*)pqbase, s.stream));
        *qBase = (const int32_t*)pqbase;
        return 0;
    };
    return alignOccurrenceChunks(s, o.total, *o.hits, o.score, o.row, o.column, tallest, operations, gather,
                                 g_lastBatchOccurrenceAlignRouting, out);
}
