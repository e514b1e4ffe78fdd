// Part of host.hip (included there, not a translation unit of its own): the alignment stage of the PSSM panel occurrence
// search, miopalSearchPssmBatchOccurrencesAligned. host_batch_occurrence_align.inc's stage with the row-indexed later
// passes (what miopalAlignPairsPssm and miopalSearchPssmOccurrencesAligned reach through runLaterPasses): an
// occurrence's origin is a ROW origin into a table of PSSM rows and into the consensus beside it.
//
// What is new: the lane-per-pair later passes keep the whole table in LDS (perPairPssmBytes: 493 rows at 32 letters), and
// a chunk of motifs has more rows than that. A chunk's occurrences are PSSM-major, so a RUN of consecutive PSSMs owns
// the contiguous stretch head[first PSSM] .. head[behind the last]: the chunk's PSSMs are split into runs whose rows
// fit the table and the stage runs once per run, with that run's rows as the table - no occurrence leaves the
// lane-per-pair kernels because the chunk is large (one PSSM of at most 64 rows always fits). PSSMs without occurrences
// in front of a run are left out of it; a run without occurrences is not run at all. The rows are not uploaded again:
// the chunk's rows lie end to end, unpadded, where the sweeps read them (kPssmRows), and a run's table is a window of
// them. Up per run: its consensus (one byte a row) and its PSSMs' row origins. Sub-chunks inside a run are sized as
// the plain stage sizes them, from the run's tallest PSSM.
static int alignPssmBatchOccurrencesStage(const PanelChunk& o, bool operations, OccurrenceAlignment* out) {
    Workspace* const ws = o.ws;
    const int A = o.rq.A;
    auto rowsOf = [&](int q) { return (int)(o.side.offsets[o.panel[q] + 1] - o.side.offsets[o.panel[q]]); };
    // the chunk's row origins (what the sweeps' upload used: the PSSMs end to end)
    std::vector<int64_t> origin((size_t)o.cq + 1, 0);
    for (int q = 0; q < o.cq; ++q) origin[(size_t)q + 1] = origin[(size_t)q] + rowsOf(q);
    RC_TRY(out->reserve(o.total, operations));
    std::vector<unsigned char> consensus;
    std::vector<int> rows;
    std::vector<int32_t> qOff;
    for (int q0 = 0; q0 < o.cq;) {
        if (o.head[q0 + 1] == o.head[q0]) {   // (no occurrences: not the start of a run)
            ++q0;
            continue;
        }
        int q1 = q0, tallest = 0;
        int64_t runRows = 0;
        while (q1 < o.cq && (q1 == q0 || perPairPssmBytes((int)(runRows + rowsOf(q1)), A) != 0)) {
            runRows += rowsOf(q1);
            tallest = std::max(tallest, rowsOf(q1));
            ++q1;
        }
        const int64_t first = o.head[q0], last = o.head[q1];
        // the run's consensus, rows (the host's copy: what the stage reads of the scores there) and origins
        consensus.clear();
        rows.clear();
        qOff.assign((size_t)(q1 - q0) + 1, 0);
        for (int q = q0; q < q1; ++q) {
            const int64_t r0 = o.side.offsets[o.panel[q]], r1 = o.side.offsets[o.panel[q] + 1];
            qOff[(size_t)(q - q0)] = (int32_t)consensus.size();
            consensus.insert(consensus.end(), o.side.residues + r0, o.side.residues + r1);
            rows.insert(rows.end(), o.side.rowScores + (size_t)r0 * A, o.side.rowScores + (size_t)r1 * A);
        }
        qOff[(size_t)(q1 - q0)] = (int32_t)consensus.size();
        Search s{o.rq.db, ws, ws->stream, consensus.data(), (int)runRows, o.rq.open, o.rq.ext, A, OPAL_SEARCH_ALIGNMENT, o.rq.mode,
                 nullptr, 0, o.rq.db->count, last - first};
        s.pssmRows = rows.data();
        RC_TRY(s.prepare());
        void *pcons, *pqoff;
        RC_TRY(ws->get(kQuery, (size_t)runRows, &pcons));
        RC_TRY(ws->stageUpload(pcons, consensus.data(), (size_t)runRows, s.stream));
        s.d_query = (uint8_t*)pcons;   // (ensurePairInputs has nothing left to do)
        s.d_rows = const_cast<int32_t*>(o.dScores) + (size_t)origin[(size_t)q0] * A;
        RC_TRY(ws->get(kPairListQOff, qOff.size() * sizeof(int32_t), &pqoff));
        RC_TRY(ws->stageUpload(pqoff, qOff.data(), qOff.size() * sizeof(int32_t), s.stream));
        // (head[q0 ..] holds the chunk's positions: a sub-chunk's first is one of them, at or behind head[q0])
        const OccurrenceGather gather = panelOccurrenceGather(o, o.dHead + q0, q1 - q0, (const int32_t*)pqoff);
        RC_TRY(alignOccurrenceRange(s, first, last, OccurrenceAlignJob{o.hits, o.slot, tallest, operations, &gather,
                                                                       g_lastBatchOccurrenceAlignRouting, out}));
        q0 = q1;
    }
    return finishOccurrenceAlignment(o.total, operations, out);
}
