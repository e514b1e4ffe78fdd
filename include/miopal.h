/*
 * miopal.h -- resident-database extension of the Opal C ABI for MI355X.
 *
 * `opalSearchDatabase` (opal.h; src/pyopal/opal.pxd:38-52) receives N host
 * pointers on every call (the layout of pyopal's Database,
 * src/pyopal/lib.pxd:95-98), which forces a pack + PCIe upload per query. The
 * entry points below are what a GPU-aware binding would call instead: the
 * database is packed and uploaded once, searches run against the device
 * mirror. They replace, one for one:
 *
 *   miopalDbCreate          <- the (sequences, lengths, size) triple that
 *                              BaseDatabase.get_sequences/get_lengths/get_size
 *                              hand to the plugin (src/pyopal/lib.pxd:90-92,
 *                              src/pyopal/platform/pyx.in:54-59)
 *   miopalSearch            <- opalSearchDatabase(...) at
 *                              src/pyopal/platform/pyx.in:77-91, including the
 *                              [start, end) slicing done there by pointer
 *                              offset (pyx.in:80-82)
 *   miopalSearchDeviceScores<- same call for searchType = OPAL_SEARCH_SCORE
 *                              with results left in HBM (multi-GPU shard
 *                              driver, src/pyopal/_align.py:150-170)
 *
 * All functions return 0 or an OPAL_ERR_* / MIOPAL_ERR_* code (opal.h), never
 * throw, never take the Python GIL, and may be called concurrently from many
 * threads on one handle (the reference's callers do exactly that while
 * holding the database read lock: src/pyopal/lib.pyx:1364,
 * src/pyopal/_align.py:150-170). No torch types cross this boundary.
 */
#ifndef MIOPAL_H
#define MIOPAL_H

#include <stdint.h>

#include "opal.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct MiopalDb MiopalDb;

/* Number of usable gfx950 devices (0 when there is none or HIP fails). */
int miopalDeviceCount(void);

/* Human-readable description of the last error raised on this thread. */
const char* miopalLastError(void);

/*
 * Build a device-resident database from N host sequences of ordinals
 * (< alphabetLength <= 32). `device` is the HIP device ordinal. The host
 * buffers are not referenced after the call returns.
 */
int miopalDbCreate(MiopalDb** out, const unsigned char* const* sequences, const int* lengths,
                   int64_t count, int alphabetLength, int device);

/* Same, from one concatenated residue buffer and offsets[count + 1]. */
int miopalDbCreateFlat(MiopalDb** out, const unsigned char* residues, const int64_t* offsets,
                       int64_t count, int alphabetLength, int device);

/*
 * A new handle holding the targets `indices[0 .. count)` of `parent` (any order, repeats allowed), on
 * the parent's device: the residues are gathered from the parent's resident copy on the device, nothing
 * is uploaded. What Database.mask / Database.extract need (src/pyopal/lib.pyx:694-778: subsets that
 * share the parent's sequence buffers) - here the subset owns a device-side copy of its residues, so
 * either handle may be destroyed first. The parent must not be destroyed during the call.
 */
int miopalDbCreateSubset(MiopalDb** out, const MiopalDb* parent, const int64_t* indices, int64_t count);

void miopalDbDestroy(MiopalDb* db);

/* opalSearchDatabase (include/opal.h) receives the whole database on every call; the library keeps
 * the handles such calls built (device memory, pinned bounce buffers, streams: at most 4 handles of at
 * most MIOPAL_SPARE_HANDLE_MB, default 4096, MiB of device memory each) and refills them on the next
 * call. This releases everything kept that way. No reference counterpart.
 */
void miopalReleaseCaches(void);

/*
 * Searches keep their device workspaces (strip boundaries, direction bits and operations of `full`, staging)
 * parked on the handle for the next search of whatever thread comes first - up to 64 GB per handle, beyond which a
 * returning workspace is freed. A process that has run a burst of large `full` searches from many threads and
 * wants the memory back calls this: every idle workspace of the handle is released (running searches keep
 * theirs). Returns the device bytes released. No reference counterpart.
 */
int64_t miopalDbReleaseWorkspaces(MiopalDb* db);

int64_t miopalDbCount(const MiopalDb* db);
int64_t miopalDbTotalLength(const MiopalDb* db);
/* Bytes of HBM held by the mirror (linear copy + packed views). */
int64_t miopalDbDeviceBytes(const MiopalDb* db);

/*
 * One query against targets [start, end) of the database.
 * Host output arrays have end - start entries and may be NULL when the
 * search type does not produce them:
 *   score                                  all search types
 *   endTarget, endQuery                    SCORE_END and ALIGNMENT
 *   startTarget, startQuery                ALIGNMENT
 *   alignment[k] (malloc'ed, caller frees), alignmentLength[k]   ALIGNMENT
 */
int miopalSearch(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen,
                 int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                 int mode, int64_t start, int64_t end, int* score, int* endTarget,
                 int* endQuery, int* startTarget, int* startQuery, unsigned char** alignment,
                 int* alignmentLength);

/*
 * Same search with the alignments returned as ONE malloc'ed buffer
 * (*operations, caller frees) and operationOffsets[end - start + 1]: target k's
 * operations are (*operations)[operationOffsets[k] .. operationOffsets[k+1]).
 * This is the bulk form of the per-result `alignment` pointers of
 * OpalSearchResult (src/pyopal/opal.pxd:24-32): one allocation instead of N.
 */
int miopalSearchFlat(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen,
                     int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                     int mode, int64_t start, int64_t end, int* score, int* endTarget,
                     int* endQuery, int* startTarget, int* startQuery,
                     unsigned char** operations, int64_t* operationOffsets);

/*
 * miopalSearchFlat with a position-specific scoring matrix (PSSM) in the place of (query, scoreMatrix):
 * rowScores[i * alphabetLength + t] is the score of aligning query position i with target residue t
 * (queryLength rows, row-major). gapOpen / gapExt, searchType, mode, the slice and every output as in
 * miopalSearchFlat. For rowScores[i][t] = scoreMatrix[query[i]][t] and consensus = query every output
 * equals miopalSearchFlat's, and the search takes the same kernels (miopalLastRouting /
 * miopalLastFullRouting report it like any other) - with one exception, in OPAL_SEARCH_ALIGNMENT only: when the
 * scores miss the byte profile of the lane-per-pair kernels (an entry + gapOpen outside [-127, 127]) AND
 * (queryLength + 1) * (alphabetLength + 1) * 4 bytes exceed 64 KB less 256 (more than 493 rows at 32 letters, 651
 * at 24), the start-cell scan and the direction pass run one wavefront per pair where the plain search keeps one
 * lane per pair up to 4096 residues: the row-indexed lane-per-pair kernel holds all rows in LDS. Results are the
 * same; those two passes are slower.
 * consensus: queryLength residues (< alphabetLength, or 255 = "no residue, never a match"). Only used
 * by OPAL_SEARCH_ALIGNMENT to tell OPAL_ALIGN_MATCH from OPAL_ALIGN_MISMATCH (position i matches target
 * residue t iff consensus[i] == t); required there, may be NULL for the other search types.
 * Checked before any device call, with miopalSearch's codes - first what needs no handle (mode and
 * search type, queryLength < 0, NULL rowScores with queryLength > 0, the alphabet length's range, NULL
 * consensus for an alignment search, a consensus entry that is neither a residue nor 255), then the
 * handle, the alphabet length against it, the slice, and miopalSearch's 32-bit range check with the
 * extreme entries of the rows where the matrix's stand (OPAL_ERR_OVERFLOW). An empty slice returns 0
 * with nothing launched. Thread safety as miopalSearch.
 * Where the scores leave the ranges of the profile-driven kernels, the 32-bit kernels stage the rows of
 * the strip at hand in LDS instead of the matrix ("Position-specific scoring matrices").
 * The k best hits and pair lists take a PSSM too: miopalSearchPssmTop and miopalAlignPairsPssm, below.
 * Out of scope: PSSM forms of miopalSearchBatch and miopalSearchBatchTop (their kernels take queries of at
 * most 64 rows, which few PSSMs are - motifs are: miopalSearchPssmBatchOccurrences takes a panel of them), of
 * opalSearchDatabase and of the multi-GPU shard driver. The columns a PSSM
 * is built from come from miopalProfileColumns, below; the pseudocounts and log-odds on top of them are the
 * caller's (Pssm.from_columns in the Python layer). Still out of scope there: per-column reduced alignments as
 * PSI-BLAST weights them, composition-based statistics, insertion-aware profiles.
 */
int miopalSearchPssm(MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength,
                     int gapOpen, int gapExt, int alphabetLength, int searchType, int mode,
                     int64_t start, int64_t end, int* score, int* endTarget, int* endQuery,
                     int* startTarget, int* startQuery, unsigned char** operations, int64_t* operationOffsets);

/*
 * miopalSearchFlat with the operations written into a buffer the caller lends.
 * In: *operations is NULL, or a malloc'ed buffer of *operationsCapacity bytes
 * (the one an earlier call returned, its contents no longer needed). Out:
 * *operations holds the operations and *operationsCapacity its size in bytes.
 * "Large enough" is judged against the search's WORST case - targets x (query
 * length + longest alignment window, rounded up to 16), not against the
 * operations it ends up producing; a buffer this library returned carries a
 * quarter of headroom for that reason.
 * When the lent buffer is large enough the SAME pointer comes back, written in
 * place: its pages are resident already, where a fresh buffer of a million
 * alignments is 67-360 MB of first-touch page faults per search (and as much to
 * unmap when it is freed). When it is too small the call returns a buffer of its
 * own and leaves the lent one untouched - still the caller's, to free or to keep.
 * On error both values are as they were. Same per-result `alignment` semantics
 * as above (src/pyopal/opal.pxd:24-32).
 */
int miopalSearchFlatInto(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen,
                         int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                         int mode, int64_t start, int64_t end, int* score, int* endTarget,
                         int* endQuery, int* startTarget, int* startQuery,
                         unsigned char** operations, int64_t* operationsCapacity,
                         int64_t* operationOffsets);

/*
 * Score-only search whose int32 results stay in HBM: `deviceScores` is a
 * device pointer with end - start entries (database order), `stream` a
 * hipStream_t (NULL = the null stream). The call only enqueues work; the
 * scores are valid once `stream` has drained. Targets whose 16-bit lanes
 * saturate are recomputed at 32 bit inside the same stream. (Two kinds of
 * search synchronise before they return: one whose lanes may leave the
 * exact range - a 4-byte count comes back - and one that sent long pairs of
 * a multi-strip query to the wavefront-per-pair kernel's strip units, whose
 * give-up counter is read so that a partial answer cannot pass for a score.)
 */
int miopalSearchDeviceScores(MiopalDb* db, const unsigned char* query, int queryLength,
                             int gapOpen, int gapExt, const int* scoreMatrix,
                             int alphabetLength, int mode, int64_t start, int64_t end,
                             int* deviceScores, void* stream);

/*
 * Timing of the dominant kernel of the most recent search on this handle,
 * measured with HIP events on the stream the kernel ran on. Returns the
 * number of launches timed; *ms receives their total duration.
 * Enabled with miopalSetProfiling(db, 1) (adds two event records per launch).
 */
void miopalSetProfiling(MiopalDb* db, int enabled);
int miopalLastKernelTime(MiopalDb* db, float* ms);

/*
 * How the score pass of the calling thread's most recent search was scheduled
 * (diagnostics for tests and benchmarks; no reference counterpart):
 *   counts[0] targets computed by the wavefront-per-pair (int32) kernel
 *   counts[1] kernel of the lane-per-target pass, low four bits: 0 none, 1 general (v_perm profile), 2 / 3 / 4
 *             pair table with int16 / half-float / biased-integer lanes (Smith-Waterman), 5 pair table for
 *             NW / HW / OV, 6 pair table strip by strip (Smith-Waterman scores of several strips), 7 the same for
 *             NW / HW / OV; + 16 when the
 *             pair-table launch was refused and the general kernel ran instead;
 *             + 32 x the general kernel's lane arithmetic (0 half floats, 1 int16, 2 signed int16, 4 / 5
 *             anti-diagonally shifted signed / unsigned, 6 column-shifted unsigned Smith-Waterman)
 *   counts[2] groups given to the main lane-per-target kernel
 *   counts[3] targets recomputed because a 16-bit lane left its exact range
 */
void miopalLastRouting(int64_t counts[4]);

/*
 * The windows of the calling thread's most recent score pass (diagnostics for tests; no reference counterpart).
 * Smith-Waterman and HW searches may cut long targets into overlapping windows [k stride, k stride + stride +
 * overlap) that are merged on the device; all four fields are reset when a score pass starts:
 *   out[0] the overlap of the windows in columns; 0: no windows (the small-search route included)
 *   out[1] the stride of the view the pass ran on - read from the view itself, not from what the plan asked for.
 *          The two agree: views are cached by (slice, overlap, stride), and a view whose lists were built ahead of
 *          the upload is only taken for a request of its own overlap AND stride (such views are whole-target views,
 *          overlap 0 and stride 0, today).
 *   out[2] the entries of that view: windows, plus one for every target that is not cut
 *   out[3] 1 when the windows were merged by (score, column, row) keys - end locations were wanted -, 0 when the
 *          scores alone were merged
 */
void miopalLastWindowPlan(int64_t out[4]);

/*
 * The shape of the persistent launch of the calling thread's most recent score pass (diagnostics for tests; no
 * reference counterpart): what "reserve_cus" (miopalDbSetOption) made of the launch, as opposed to what was asked.
 * All zeros before the thread's first search; out[1 .. 3] are reset when a score pass starts, all four when a batch
 * starts (miopalSearchBatch and the entry points built on it):
 *   out[0] the compute units the handle sees
 *   out[1] the workgroups of the pass's main persistent launch - the one-strip or strips pair-table kernel, for the
 *          column split the workgroups of its plan; a batch: of its last batch-kernel launch -, 0 if there was none
 *          (small searches, the general kernel, a refused launch)
 *   out[2] the wavefronts per workgroup of that launch
 *   out[3] the per-SIMD share of groups the launch's hand-out stops a SIMD at, 0 = off (always 0 for the int16 and
 *          half-float flavours, the column split, the strips and the batch kernels: they have no shares)
 */
void miopalLastLaunchShape(int64_t out[4]);

/*
 * Many queries against one slice [start, end) of a resident handle in one call (no reference counterpart:
 * the batch form of pyopal's thread-pool loop of searches). Query k is
 * queries[queryOffsets[k] .. queryOffsets[k + 1]) (nQueries + 1 offsets); outputs are row-major
 * [nQueries][end - start]: score, and for OPAL_SEARCH_SCORE_END endTarget / endQuery. Every result equals
 * what miopalSearch returns for that query alone, and the checks are miopalSearch's, query by query (bad
 * residues, a bad slice, a matrix of another alphabet). OPAL_SEARCH_ALIGNMENT is refused with
 * OPAL_ERR_INVALID_MODE. nQueries = 0 or an empty slice: nothing to do, 0.
 * Queries of 1..64 residues share persistent launches of the batch kernels (interseq_batch_impl.h); longer
 * queries, queries of length 0, and gap / matrix models beyond the batch kernels' static range checks run
 * through miopalSearch's own path inside the same call. Thread-safe like miopalSearch.
 */
int miopalSearchBatch(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                      int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                      int mode, int64_t start, int64_t end, int* score, int* endTarget, int* endQuery);

/*
 * The k best targets of a query in the slice [start, end), selected on the device (no reference counterpart:
 * what pyopal's worked example does on the host with sorted(results, key=score)[:k]).
 *   Order: score descending; equal scores by target index ascending - exactly Python's stable
 *     sorted(aligner.align(...), key=lambda r: r.score, reverse=True).
 *   Hits: targets whose score is >= minScore (INT_MIN: no bound).
 *   Outputs: count = min(k, hits); targetIndex (absolute), score and, for OPAL_SEARCH_SCORE_END, endTarget /
 *     endQuery of the first `count` hits in that order, each equal to what miopalSearch returns for that target.
 *     Slots count .. k - 1 hold -1 in every output.
 *   0 <= k <= MIOPAL_MAX_TOP; k > end - start is allowed. k = 0 or an empty slice: count 0, nothing launched,
 *     the arguments are checked all the same.
 * The checks, error codes and thread safety are miopalSearch's (OPAL_ERR_OVERFLOW included); OPAL_SEARCH_ALIGNMENT
 * is refused with OPAL_ERR_INVALID_MODE. Only count + k entries cross PCIe: the scores stay in HBM.
 */
#define MIOPAL_MAX_TOP 4096
int miopalSearchTop(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                    const int* scoreMatrix, int alphabetLength, int searchType, int mode,
                    int64_t start, int64_t end, int k, int minScore,
                    int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery);

/*
 * miopalSearchTop with a position-specific scoring matrix in the place of (query, scoreMatrix): rowScores
 * ([queryLength][alphabetLength], as in miopalSearchPssm) and no consensus - the call produces no alignments.
 * miopalSearchTop's contract holds to the letter: the order (score descending, then target index ascending),
 * minScore, count = min(k, hits), -1 in the slots past count, k in [0, MIOPAL_MAX_TOP], k = 0 or an empty slice
 * checked and answered with nothing launched. Entry i equals what miopalSearchPssm returns for targetIndex[i], the
 * score pass takes the kernels miopalSearchPssm takes (miopalLastRouting reports the same), and the selection is
 * miopalSearchTop's.
 * Checked before any device call, with miopalSearchPssm's codes and in its order - first what needs no handle (mode
 * and search type, queryLength < 0, NULL rowScores with queryLength > 0, the alphabet length's range,
 * OPAL_SEARCH_ALIGNMENT: OPAL_ERR_INVALID_MODE, k outside its range), then the handle, the alphabet length against
 * it, the slice, the outputs (miopalSearchTop's), and the 32-bit range check with the extreme entries of the rows
 * (OPAL_ERR_OVERFLOW). Thread safety as miopalSearch.
 */
int miopalSearchPssmTop(MiopalDb* db, const int* rowScores, int queryLength,
                        int gapOpen, int gapExt, int alphabetLength, int searchType, int mode,
                        int64_t start, int64_t end, int k, int minScore,
                        int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery);

/*
 * miopalSearchTop of every query of a batch (queries and queryOffsets as in miopalSearchBatch), in one call through
 * miopalSearchBatch's chunks: each chunk's [queries][targets] rows are selected on the device before they leave.
 * count has nQueries entries; the other outputs are [nQueries][k], row-major. Row i equals miopalSearchTop of query i
 * alone, and miopalLastBatchRouting reports what miopalSearchBatch reports for the same inputs. nQueries = 0:
 * nothing to do, 0.
 */
int miopalSearchBatchTop(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                         int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                         int mode, int64_t start, int64_t end, int k, int minScore,
                         int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery);

/*
 * Every target of the slice that scores at least minScore, compacted on the device: the hits of a query are the
 * targets of [start, end) with score >= minScore, in index order (database order), and each carries what miopalSearch
 * returns for it - *targetIndex (absolute indices), *score and, for OPAL_SEARCH_SCORE_END, *endTarget / *endQuery,
 * *count entries each. minScore = INT_MIN: every target. No bound on the number of hits (miopalSearchTop stops at
 * MIOPAL_MAX_TOP); only the hits cross PCIe, in two host round trips - the counts, then arrays sized to them.
 * Every output array is malloc'ed by the library and freed by the caller (like *operations of miopalSearchFlat); a
 * pointer is NULL when there are no hits or when the search type does not produce that array (endTarget / endQuery
 * may themselves be NULL for OPAL_SEARCH_SCORE).
 * maxHits < 0: no bound. With more than maxHits hits the call returns MIOPAL_ERR_TOO_MANY_HITS: *count is filled - the
 * caller knows what it would take - nothing is allocated, the array pointers are as they were and the handle stays
 * usable. On any other error every output is as it was.
 * Checks, codes, their order and thread safety: miopalSearchTop's - miopalSearch's checks (the handle first), then
 * OPAL_SEARCH_ALIGNMENT refused with OPAL_ERR_INVALID_MODE, then null outputs; OPAL_ERR_OVERFLOW as miopalSearch. An
 * empty slice is checked and answered with *count = 0 and NULL arrays, nothing launched. The score pass takes the
 * kernels miopalSearch takes (miopalLastRouting reports the same).
 */
int miopalSearchHits(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                     const int* scoreMatrix, int alphabetLength, int searchType, int mode,
                     int64_t start, int64_t end, int minScore, int64_t maxHits,
                     int64_t* count, int64_t** targetIndex, int** score, int** endTarget, int** endQuery);

/*
 * miopalSearchHits with a position-specific scoring matrix in the place of (query, scoreMatrix): rowScores as in
 * miopalSearchPssm, no consensus. miopalSearchHits' contract holds to the letter, and hit i equals what
 * miopalSearchPssm returns for (*targetIndex)[i]. Checked before any device call, with miopalSearchPssmTop's codes and
 * in its order - first what needs no handle (mode and search type, queryLength < 0, NULL rowScores with
 * queryLength > 0, the alphabet length's range, OPAL_SEARCH_ALIGNMENT: OPAL_ERR_INVALID_MODE, null outputs), then the
 * handle, the alphabet length against it, the slice, and the 32-bit range check with the extreme entries of the rows
 * (OPAL_ERR_OVERFLOW).
 */
int miopalSearchPssmHits(MiopalDb* db, const int* rowScores, int queryLength,
                         int gapOpen, int gapExt, int alphabetLength, int searchType, int mode,
                         int64_t start, int64_t end, int minScore, int64_t maxHits,
                         int64_t* count, int64_t** targetIndex, int** score, int** endTarget, int** endQuery);

/*
 * miopalSearchHits of every query of a batch (queries and queryOffsets as in miopalSearchBatch) with one threshold per
 * query (minScore[nQueries]), in one call through miopalSearchBatch's chunks: each chunk's [queries][targets] rows are
 * compacted on the device before they leave. The answer is a CSR: hitOffsets (nQueries + 1 entries, the CALLER's
 * array; hitOffsets[0] = 0) and the malloc'ed arrays of hitOffsets[nQueries] entries; entries hitOffsets[i] ..
 * hitOffsets[i + 1] equal miopalSearchHits of query i alone. maxHits bounds the total over all queries; with more,
 * MIOPAL_ERR_TOO_MANY_HITS with hitOffsets filled and nothing allocated. miopalLastBatchRouting reports what
 * miopalSearchBatch reports for the same inputs. Checks and their order: miopalSearchBatchTop's (OPAL_SEARCH_ALIGNMENT
 * refused first, then the query list, then every query with miopalSearch's checks), then null outputs and a NULL
 * minScore with nQueries > 0. nQueries = 0 or an empty slice: checked, hitOffsets all 0, NULL arrays, 0.
 */
int miopalSearchBatchHits(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                          int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                          int mode, int64_t start, int64_t end, const int* minScore, int64_t maxHits,
                          int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget, int** endQuery);

/*
 * Every occurrence of a query in each target of the slice, picked on the device: where miopalSearch keeps one best
 * score per target, this call returns every place the query matches - an adapter a read carries twice, the binding
 * sites of a primer, the copies of a repeated domain.
 *
 * One query against the targets [start, end). Gap model and score source are miopalSearch's. The arithmetic is 32-bit
 * only (no 16-bit ladder); miopalSearch's range check decides OPAL_ERR_OVERFLOW. mode is OPAL_MODE_HW or OPAL_MODE_SW;
 * OPAL_MODE_NW and OPAL_MODE_OV are refused with OPAL_ERR_INVALID_MODE.
 *
 * Column values of a target of length L for a query of Q rows:
 *   HW  v[j] = H[Q - 1][j] of the recurrence of oracle/opal_oracle.c under HW's borders (the top row free, the left
 *       column penalised with borderGap); r[j] = Q - 1.
 *   SW  v[j] = max over i of H[i][j], with the floor at 0; r[j] = the smallest i that reaches it. minScore >= 1 is
 *       required (MIOPAL_ERR_BAD_ARGUMENT otherwise).
 * The occurrences of a target are what this rule emits, left to right - greedy peak picking with a suppression window:
 *
 *   cand = none
 *   for j in 0 .. L - 1:
 *       if cand and j - cand.j > window:  emit(cand); cand = none
 *       if v[j] >= minScore and (cand is none or v[j] > cand.v):  cand = (j, v[j], r[j])
 *   if cand: emit(cand)
 *
 * window >= 0; a negative window is MIOPAL_ERR_BAD_ARGUMENT. Consequences:
 *   - two occurrences of one target are more than `window` columns apart;
 *   - window = 0 returns every column with v[j] >= minScore;
 *   - the first column that reaches the target's maximum is an occurrence when that maximum is >= minScore: for every
 *     target whose miopalSearch(..., OPAL_SEARCH_SCORE_END) score is >= minScore, that search's (score, endTarget,
 *     endQuery) is one of the target's occurrences, and the highest-scoring;
 *   - a target scoring below minScore has no occurrences.
 * An empty query or an empty target has no occurrences.
 *
 * Output: miopalSearchHits' contract to the letter - *count and the malloc'ed *targetIndex (absolute indices), *score,
 * *endTarget (the column j), *endQuery (the row r), *count entries each, freed by the caller, NULL without
 * occurrences; several entries may name one target. maxHits < 0: no bound; with more than maxHits occurrences
 * MIOPAL_ERR_TOO_MANY_HITS with *count filled and nothing allocated. On any other error every output is as it was. An
 * empty slice is checked and answered with nothing launched. Order: target index ascending, then column ascending; two
 * calls return the same bytes.
 * Checks and their order: miopalSearchHits' (miopalSearch's, the handle first); where that function refuses
 * alignments - the mode, then the window, then the SW rule for minScore; then null outputs.
 * On the device: a count sweep over the slice (one lane per target), a scan of the counts, and a write sweep over the
 * targets that have occurrences only; only the occurrences cross PCIe, in two host round trips.
 * A query of more than 64 rows keeps 8 (HW) or 16 (SW) bytes per column for every target of a wavefront between its
 * strips, within 2 GB: against a handle whose longest target has more than 4 194 304 (HW) or 2 097 152 (SW) residues such
 * a query is refused with MIOPAL_ERR_BAD_ARGUMENT and a message that states the limit, after the range check and before
 * any device call. Queries of at most 64 rows have no such limit.
 * Not part of this call: opalSearchDatabase and the multi-GPU driver (the start locations and operations of an
 * occurrence: miopalSearchOccurrencesAligned below; a panel of queries: miopalSearchBatchOccurrences). Thread safety as
 * miopalSearch.
 */
int miopalSearchOccurrences(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                            const int* scoreMatrix, int alphabetLength, int mode,
                            int64_t start, int64_t end, int minScore, int window, int64_t maxHits,
                            int64_t* count, int64_t** targetIndex, int** score, int** endTarget, int** endQuery);

/*
 * miopalSearchOccurrences with a position-specific scoring matrix in the place of (query, scoreMatrix): rowScores as
 * in miopalSearchPssm, no consensus; row i of the recurrence scores with rowScores[i]. The contract above holds to the
 * letter. The sweep keeps the rows in LDS: a PSSM of more rows than (64 KB - 256) / (4 (alphabetLength + 1)) - 1 (493
 * at 32 letters, 651 at 24) is refused with MIOPAL_ERR_BAD_ARGUMENT and a message that states the limit; taller PSSMs
 * are not supported.
 * Checked before any device call in miopalSearchPssmHits' order: what needs no handle first (mode, queryLength < 0,
 * NULL rowScores with queryLength > 0, the alphabet length's range; then the mode, the window and the SW rule for
 * minScore; null outputs; the PSSM's height), then the handle, the alphabet length against it, the slice, and the
 * 32-bit range check with the extreme entries of the rows (OPAL_ERR_OVERFLOW).
 */
int miopalSearchPssmOccurrences(MiopalDb* db, const int* rowScores, int queryLength,
                                int gapOpen, int gapExt, int alphabetLength, int mode,
                                int64_t start, int64_t end, int minScore, int window, int64_t maxHits,
                                int64_t* count, int64_t** targetIndex, int** score, int** endTarget, int** endQuery);

/*
 * What the last occurrence search of the calling thread did: counts[0] = targets swept by the count pass, counts[1] =
 * targets swept by the write pass (those that have occurrences), counts[2] = chunks over both passes, counts[3] =
 * strips per sweep, ceil(queryLength / 64). All 0 for an empty slice.
 */
void miopalLastOccurrenceRouting(int64_t counts[4]);

/*
 * miopalSearchOccurrences for a whole panel of queries in one call - 96 barcodes, a primer panel, a kit's adapters
 * with their reverse complements - against the targets [start, end). queries / queryOffsets / nQueries are
 * miopalSearchBatch's; minScore[nQueries] and window[nQueries] hold one cut and one suppression window per query. Gap
 * model, matrix, modes (OPAL_MODE_HW and OPAL_MODE_SW only) and the picking rule are miopalSearchOccurrences' to the
 * letter.
 *
 * Output: a CSR as miopalSearchBatchHits returns it. hitOffsets is the caller's array of nQueries + 1 entries,
 * hitOffsets[0] = 0; *targetIndex, *score, *endTarget and *endQuery are malloc'ed, hitOffsets[nQueries] entries each,
 * freed by the caller, NULL without occurrences. Entries hitOffsets[i] .. hitOffsets[i + 1] are byte for byte what
 * miopalSearchOccurrences returns for query i alone with minScore[i] and window[i]: targets absolute and ascending,
 * columns ascending inside a target; two calls return the same bytes. maxHits bounds the TOTAL over all queries
 * (< 0: no bound): with more, MIOPAL_ERR_TOO_MANY_HITS with hitOffsets filled and nothing allocated. On any other
 * error every output is as it was. nQueries = 0 or an empty slice: checked, hitOffsets all 0, NULL arrays, nothing
 * launched.
 * Checks and their order, all before any device work: the query list, then every query with miopalSearch's checks
 * (one failing query refuses the call); the mode; every window[i] >= 0; under OPAL_MODE_SW every minScore[i] >= 1; NULL
 * minScore / window with nQueries > 0; null outputs; miopalSearch's 32-bit range check for every query
 * (OPAL_ERR_OVERFLOW).
 * On the device: queries of 1 .. 64 rows share launches. A chunk of them (queries x targets of the slice within 2^25
 * entries, 32 768 queries at most) costs one count sweep - the slice's jobs built and sorted once, the rows of a group
 * of queries side by side in a compute unit's LDS, a lane walking its target once per query of the group - one scan,
 * one small download, one write sweep over the (query, target) pairs that have occurrences only, and the download of
 * the occurrences: two host round trips per chunk, not per query. A group is as many consecutive queries as fit the
 * 160 KB of LDS, except where that would leave the count sweep fewer than 32 workgroups per compute unit (targets / 256
 * x groups): then the queries are spread over more, smaller groups, down to one query a group. The figure 32 rests on
 * one measured panel and is the switch BATCH_OCCURRENCE_WORKGROUPS_PER_CU (0: groups only as the LDS
 * makes them); the answer does not depend on it. An empty query has no occurrences. A query of more than 64 rows
 * runs through miopalSearchOccurrences' own path inside the call (its strip-workspace refusal included) and its
 * stretch is spliced into the CSR at its place; what miopalLastOccurrenceRouting reports is left as it was. Once the
 * total has passed maxHits the remaining queries are still counted - hitOffsets is complete - but nothing is written.
 * Not part of this call: opalSearchDatabase and the multi-GPU driver (the start locations and operations of a
 * panel's occurrences: miopalSearchBatchOccurrencesAligned below; a panel of PSSMs: miopalSearchPssmBatchOccurrences
 * below). Thread safety as miopalSearch.
 */
int miopalSearchBatchOccurrences(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                                 int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int mode,
                                 int64_t start, int64_t end, const int* minScore, const int* window, int64_t maxHits,
                                 int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget, int** endQuery);

/*
 * What the last panel occurrence search of the calling thread, plain or PSSM, did: counts[0] = queries on the panel kernels,
 * counts[1] = queries on the single-query path, counts[2] = chunks (one count sweep + scan + download + write sweep
 * each), counts[3] = (query, target) pairs the write sweeps took - those that have occurrences. All 0 for an empty
 * slice or an empty list.
 */
void miopalLastBatchOccurrenceRouting(int64_t counts[4]);

/*
 * How the last panel occurrence search of the calling thread, plain or PSSM, grouped its panel queries: counts[0] = groups over
 * all chunks (the rows of a group share a workgroup's LDS in the count sweep), counts[1] = the most queries in one
 * group, counts[2] = the bytes of LDS of the largest group's rows. All 0 when no panel kernel ran.
 */
void miopalLastBatchOccurrenceGroups(int64_t counts[3]);

/*
 * miopalSearchOccurrences with the other end of every occurrence: where it starts and, when asked for, its operations
 * - an adapter is trimmed at the column where it begins, a repeated domain is cut out from start to end, occurrences
 * are filtered by identity.
 *
 * The first five outputs (*count, *targetIndex, *score, *endTarget, *endQuery) are miopalSearchOccurrences' outputs to
 * the letter: same rule, same order, same bytes. maxHits is honoured before any alignment work
 * (MIOPAL_ERR_TOO_MANY_HITS with *count filled and nothing allocated).
 *
 * Start of the occurrence (v, r, j) of target t: the start rule at the head of oracle/opal_oracle.c, applied to the
 * occurrence's end cell (r, j) in the place of the target's best. The scan runs over the reversed prefixes q[0..r],
 * t[0..j] under NW borders; the region is the last row for OPAL_MODE_HW and all cells for OPAL_MODE_SW; candidates are
 * scanned column by column, row by row inside a column, and a candidate replaces the best only when strictly greater.
 * The cell (a, b) found gives (*startQuery)[k] = r - a and (*startTarget)[k] = j - b. The degenerate HW optimum is the
 * checker's: when v equals the border gap over q[0..r] and no real alignment reaches it, the target span is empty,
 * startTarget = j + 1, startQuery = 0, and the alignment is all query-consuming gaps (OPAL_ALIGN_DEL).
 * For the target's best occurrence (miopalSearchOccurrences' anchor property) start and operations are those of
 * miopalSearch(..., OPAL_SEARCH_ALIGNMENT) on that target.
 *
 * Operations: the checker's traceback of the global alignment of q[startQuery..r] with t[startTarget..j], one byte
 * per operation as miopalAlignPairs encodes them; the operations of occurrence k lie in
 * (*alignments)[(*alignmentOffsets)[k] .. (*alignmentOffsets)[k + 1]); *alignmentOffsets has *count + 1 entries.
 * alignments == NULL and alignmentOffsets == NULL together: starts only - the reversed scan and the start cells run,
 * and no direction pass, no walk and no operation traffic follow. Exactly one of the two NULL is
 * MIOPAL_ERR_BAD_ARGUMENT.
 *
 * Outputs: all malloc'ed by the library, sized on the device, freed by the caller; NULL with *count = 0, except
 * *alignmentOffsets, which then holds the single 0. On any error every output is as it was (MIOPAL_ERR_TOO_MANY_HITS
 * fills *count). Two calls return the same bytes.
 * Checks and their order: miopalSearchOccurrences', then null startTarget / startQuery, then the pair alignments /
 * alignmentOffsets.
 * On the device: the occurrences stay where the write sweep left them; their target origins are gathered from the
 * handle's offsets (occurrence_pair_inputs_kernel), and the later passes of a miopalAlignPairs `full` list - the
 * reversed-prefix scan with the stop rule, the start cells, the direction pass, the walk, the gather - run on them
 * chunk by chunk in occurrence order, chunks sized as that call sizes them. Nothing of the occurrence list goes up
 * over PCIe; starts, lengths and operations come down per chunk.
 * Not part of this call: opalSearchDatabase and the multi-GPU driver (a panel of queries in one call:
 * miopalSearchBatchOccurrencesAligned below). Thread safety as miopalSearch.
 */
int miopalSearchOccurrencesAligned(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                                   const int* scoreMatrix, int alphabetLength, int mode,
                                   int64_t start, int64_t end, int minScore, int window, int64_t maxHits,
                                   int64_t* count, int64_t** targetIndex, int** score, int** endTarget, int** endQuery,
                                   int** startTarget, int** startQuery,
                                   unsigned char** alignments, int64_t** alignmentOffsets);

/*
 * miopalSearchOccurrencesAligned with a position-specific scoring matrix in the place of (query, scoreMatrix):
 * rowScores and consensus as in miopalSearchPssm. The consensus tells OPAL_ALIGN_MATCH from OPAL_ALIGN_MISMATCH; it is
 * required when operations are asked for (queryLength > 0), as miopalAlignPairsPssm requires it, and may be NULL for
 * starts only. The first five outputs are miopalSearchPssmOccurrences'; the later passes are the row-indexed ones of
 * miopalAlignPairsPssm with this one PSSM in the table. The height limit of the sweep stays.
 * Checked before any device call in miopalSearchPssmOccurrences' order, with the new null outputs behind its own and
 * the consensus (missing; a residue out of range) behind them, before the PSSM's height.
 */
int miopalSearchPssmOccurrencesAligned(MiopalDb* db, const int* rowScores, const unsigned char* consensus,
                                       int queryLength, int gapOpen, int gapExt, int alphabetLength, int mode,
                                       int64_t start, int64_t end, int minScore, int window, int64_t maxHits,
                                       int64_t* count, int64_t** targetIndex, int** score, int** endTarget,
                                       int** endQuery, int** startTarget, int** startQuery,
                                       unsigned char** alignments, int64_t** alignmentOffsets);

/*
 * What the alignment stage of the calling thread's last miopalSearchOccurrencesAligned / ...PssmOccurrencesAligned
 * did: counts[0] = occurrences whose direction pass ran one lane each, counts[1] = one wavefront each (both 0 for
 * starts only: no direction work), counts[2] = chunks of the stage, counts[3] = the longest target window
 * (endTarget - startTarget + 1) of the call. All 0 without occurrences. miopalLastOccurrenceRouting keeps reporting
 * the sweeps.
 */
void miopalLastOccurrenceAlignRouting(int64_t counts[4]);

/*
 * miopalSearchBatchOccurrences with the other end of every occurrence - miopalSearchOccurrencesAligned for a whole
 * panel of queries in one call: the user who demultiplexes on 96 barcodes is the one who trims at their starts.
 *
 * The first outputs (hitOffsets, *targetIndex, *score, *endTarget, *endQuery) are miopalSearchBatchOccurrences' to the
 * letter: same rule, same order, same bytes. *startTarget, *startQuery, *alignments and *alignmentOffsets are one CSR
 * with them: entries hitOffsets[i] .. hitOffsets[i + 1] of the starts, and the operations
 * (*alignments)[(*alignmentOffsets)[k] .. (*alignmentOffsets)[k + 1]) of those occurrences k, are byte for byte what
 * miopalSearchOccurrencesAligned returns for query i alone with minScore[i] and window[i], the alignment offsets
 * rebased: *alignmentOffsets has hitOffsets[nQueries] + 1 entries, entry 0 is 0 and the operations concatenate in CSR
 * order. alignments == NULL and alignmentOffsets == NULL together: starts only, no direction pass, no walk and no
 * operation traffic. Exactly one of the two NULL is MIOPAL_ERR_BAD_ARGUMENT.
 *
 * Outputs: all malloc'ed by the library, freed by the caller; with no occurrences the pointers are NULL, except
 * *alignmentOffsets, which then holds the single 0 (nQueries = 0 and an empty slice included). On any error every
 * output is as it was, hitOffsets under MIOPAL_ERR_TOO_MANY_HITS excepted. Two calls return the same bytes.
 * maxHits bounds the TOTAL over all queries (< 0: no bound). Unlike miopalSearchOccurrencesAligned, which honours it
 * before any alignment work, the panel learns its total chunk by chunk: once the running total passes maxHits no
 * further alignment stage runs and the remaining queries are only counted, what earlier chunks aligned is discarded,
 * hitOffsets is filled for every query, nothing else is allocated or written, and the call returns
 * MIOPAL_ERR_TOO_MANY_HITS.
 * Checks and their order, all before any device work: miopalSearchBatchOccurrences' up to its null outputs, then null
 * startTarget / startQuery, then the pair alignments / alignmentOffsets, then its 32-bit range check for every query
 * (one failing query refuses the call).
 * On the device: miopalSearchBatchOccurrences' sweeps, and behind the write sweep of every panel chunk that has
 * occurrences the alignment stage, in the workspace the chunk holds. The chunk's queries go up once more, end to end,
 * with their origins; the occurrences stay where the write sweep left them and are taken in output order, in
 * sub-chunks sized as miopalAlignPairs sizes its chunks (from the tallest query of the chunk and the longest target
 * that has an occurrence). Per sub-chunk one gather (batch_occurrence_origins_kernel) finds each occurrence's
 * target origin in the handle's offsets and its query's origin from the occurrence's position - a binary search in the
 * chunk's per-query offsets, which the scan left on the device - and the later passes of a miopalAlignPairs `full`
 * list run on them. Nothing of the occurrence list goes up over PCIe; starts, lengths and operations come down per
 * sub-chunk. A query of more than 64 rows runs through miopalSearchOccurrencesAligned's own path inside the call and
 * its stretch is spliced into the CSR at its place; an empty query has no occurrences. What
 * miopalLastOccurrenceRouting and miopalLastOccurrenceAlignRouting report is left as it was.
 * Not part of this call: opalSearchDatabase and the multi-GPU driver (a panel of PSSMs:
 * miopalSearchPssmBatchOccurrencesAligned below). Thread safety as miopalSearch.
 */
int miopalSearchBatchOccurrencesAligned(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets,
                                        int nQueries, int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength,
                                        int mode, int64_t start, int64_t end, const int* minScore, const int* window,
                                        int64_t maxHits, int64_t* hitOffsets, int64_t** targetIndex, int** score,
                                        int** endTarget, int** endQuery, int** startTarget, int** startQuery,
                                        unsigned char** alignments, int64_t** alignmentOffsets);

/*
 * What the alignment stages of the last panel occurrence search of the calling thread, plain or PSSM, did
 * (miopalSearchBatchOccurrencesAligned, miopalSearchPssmBatchOccurrencesAligned): counts[0] =
 * occurrences whose direction pass ran one lane each, counts[1] = one wavefront each (both 0 for starts only),
 * counts[2] = sub-chunks of the stage, counts[3] = the longest target window (endTarget - startTarget + 1) of the
 * call; the first three summed, the last the maximum, over panel chunks and long queries. All 0 without occurrences.
 * miopalLastBatchOccurrenceRouting and miopalLastBatchOccurrenceGroups keep reporting the sweeps.
 */
void miopalLastBatchOccurrenceAlignRouting(int64_t counts[4]);

/*
 * miopalSearchBatchOccurrences with a panel of position-specific scoring matrices in the place of (queries,
 * scoreMatrix) - a library of transcription-factor weight matrices over promoters, degenerate primers written as
 * weights, barcodes with per-position quality weights - each with its reverse complement where both strands count.
 * The list is passed as miopalAlignPairsPssm passes it: rowScores holds alphabetLength ints per row, row r at
 * rowScores[r * alphabetLength]; rowOffsets[nPssms + 1] delimits the PSSMs in rows; minScore[nPssms] and
 * window[nPssms] hold one cut and one window per PSSM.
 *
 * Output: miopalSearchBatchOccurrences' CSR. Entries hitOffsets[i] .. hitOffsets[i + 1] of every output are byte for
 * byte what miopalSearchPssmOccurrences returns for PSSM i alone with minScore[i] and window[i]. The CSR layout,
 * maxHits bounding the TOTAL and the behaviour under MIOPAL_ERR_TOO_MANY_HITS (hitOffsets filled, nothing allocated),
 * the result with no occurrences, with nPssms = 0, with an empty PSSM and with an empty slice, every output left as it
 * was on any other error, two calls returning the same bytes, OPAL_MODE_HW and OPAL_MODE_SW only: all as
 * miopalSearchBatchOccurrences states them.
 * Checks and their order, all before any device work. First what needs no handle: the mode; the list (nPssms < 0, NULL
 * rowOffsets, an offset that is negative or decreases, more than 2^31 - 65 rows in all - miopalAlignPairsPssm's bound);
 * NULL rowScores with rows present; alphabetLength outside 1 .. 32; every window[i] >= 0; under OPAL_MODE_SW every
 * minScore[i] >= 1; NULL minScore / window with nPssms > 0; null outputs; then the height of every PSSM of more than
 * 64 rows against the single sweep's LDS table (miopalSearchPssmOccurrences' limit: 493 rows at 32 letters, 651 at
 * 24) - one PSSM that is too tall refuses the whole call with that call's message, naming the PSSM. Then the null
 * handle, alphabetLength against the handle's, the slice, and miopalSearch's 32-bit range check of every PSSM with the
 * extreme entries of its own rows: one failing PSSM refuses the call with OPAL_ERR_OVERFLOW.
 * On the device: PSSMs of 1 .. 64 rows take the panel kernels, chunked and grouped exactly as
 * miopalSearchBatchOccurrences chunks and groups queries of those heights (the same bounds and switches). The sweep is
 * that call's cell for cell; what differs is where a group's LDS table comes from: a chunk's rows go up once, end to
 * end (4 x alphabetLength bytes a row), with one int per table row that names the row it holds, and a workgroup fills
 * its table with rows[r][t] + gapOpen, the pad score in the pad column and in the pad rows behind each PSSM. No
 * matrix and no residue list are involved. An empty PSSM has no occurrences. A PSSM of more than 64 rows runs through
 * miopalSearchPssmOccurrences' own path inside the call and its stretch is spliced into the CSR at its place; what
 * miopalLastOccurrenceRouting reports is left as it was. miopalLastBatchOccurrenceRouting and
 * miopalLastBatchOccurrenceGroups report this call as they report the plain one.
 * Not part of this call: PSSM forms of miopalSearchBatch and miopalSearchBatchTop, PSSMs taller than the single
 * sweep's table, opalSearchDatabase and the multi-GPU driver, statistics for motif scores. Thread safety as miopalSearch.
 */
int miopalSearchPssmBatchOccurrences(MiopalDb* db, const int* rowScores, const int64_t* rowOffsets, int nPssms,
                                     int gapOpen, int gapExt, int alphabetLength, int mode, int64_t start, int64_t end,
                                     const int* minScore, const int* window, int64_t maxHits,
                                     int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget,
                                     int** endQuery);

/*
 * miopalSearchPssmBatchOccurrences with the other end of every occurrence - miopalSearchPssmOccurrencesAligned for a
 * whole panel of PSSMs in one call. consensus holds one residue (or 255) per row, in rowOffsets' row coordinates; it
 * tells OPAL_ALIGN_MATCH from OPAL_ALIGN_MISMATCH, is required when operations are asked for and rows are present,
 * and may be NULL for starts only - miopalSearchPssmOccurrencesAligned's rule.
 *
 * Output: miopalSearchBatchOccurrencesAligned's. Entries hitOffsets[i] .. hitOffsets[i + 1] of every output, and the
 * operations of those occurrences, are byte for byte what miopalSearchPssmOccurrencesAligned returns for PSSM i alone
 * with minScore[i] and window[i], the alignment offsets rebased as miopalSearchBatchOccurrencesAligned rebases them.
 * Starts only, the outputs without occurrences and on error, and maxHits - once the running total passes it no further
 * stage runs, what was aligned is discarded, hitOffsets is filled - are that call's.
 * Checks and their order: miopalSearchPssmBatchOccurrences' up to its null outputs, then null startTarget /
 * startQuery, the pair alignments / alignmentOffsets, the consensus (missing; a residue out of range), then the
 * heights, the handle and the range checks as there.
 * On the device: miopalSearchPssmBatchOccurrences' sweeps, and behind the write sweep of every panel chunk that has
 * occurrences the alignment stage with the row-indexed later passes of miopalAlignPairsPssm. Their lane-per-pair
 * kernels keep the whole row table in LDS (64 KB less 256 bytes: 493 rows at 32 letters), and a chunk of motifs has
 * more rows than that. A chunk's occurrences lie PSSM after PSSM, so a run of consecutive PSSMs owns a contiguous
 * stretch of them: the chunk's PSSMs are split into runs whose rows fit the table, and the stage runs once per run
 * that has occurrences, with that run's rows - a window of the rows the sweeps read, not uploaded again - as the
 * table, its consensus and its PSSMs' row origins going up. No occurrence goes to the wavefront-per-pair kernels
 * because the chunk as a whole is large. Sub-chunks inside a run are sized as the plain stage sizes them. A PSSM of
 * more than 64 rows runs through miopalSearchPssmOccurrencesAligned's own path inside the call.
 * miopalLastBatchOccurrenceAlignRouting reports the stages (counts[2]: sub-chunks over all runs).
 * Not part of this call: what miopalSearchPssmBatchOccurrences leaves out. Thread safety as miopalSearch.
 */
int miopalSearchPssmBatchOccurrencesAligned(MiopalDb* db, const int* rowScores, const unsigned char* consensus,
                                            const int64_t* rowOffsets, int nPssms, int gapOpen, int gapExt,
                                            int alphabetLength, int mode, int64_t start, int64_t end,
                                            const int* minScore, const int* window, int64_t maxHits,
                                            int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget,
                                            int** endQuery, int** startTarget, int** startQuery,
                                            unsigned char** alignments, int64_t** alignmentOffsets);

/*
 * The significant hits of a query: miopalSearchHits with the cut stated as an E-value, the statistics gathered on the
 * device from the search's own scores (almost all targets of a database search are unrelated to the query: the search
 * is its own calibration sample). No table of Karlin-Altschul parameters is involved.
 *   Length bins: a target of length L falls into bin 0 for L = 0, otherwise into bin 1 + 4 e + m with e = floor(log2 L)
 *     and m the two bits below the leading one of L (quarter octaves; at most 124 for 32-bit lengths).
 *   Statistics: per bin the device sums n, score and score^2 of the slice's targets as 64-bit integers (exact, the
 *     same in any order), and the targets and the sum of their lengths (binTargets, binLength).
 *   Fit (host, doubles), over the bins 1 .. 127 that hold targets: x_b = ln(binLength[b] / binTargets[b]); the weighted
 *     least-squares line mean_b = intercept + slope x_b through the scores (slope 0 and intercept the mean when all
 *     targets share one bin); sigma^2 = sum_b (sum s^2 - 2 mean_b sum s + n_b mean_b^2) / (used - 2).
 *   Refits: with excludeZ > 0 the statistics are taken again leaving out every target with score > ceiling[b] =
 *     floor(mean_b + excludeZ sigma) - related sequences inflate the spread; only the upper tail is cut - and the fit
 *     repeated, until the ceilings repeat or MIOPAL_FIT_MAX_REFITS refits are done. The ceilings of a refit apply to
 *     all targets and replace the ones before. excludeZ <= 0: one pass.
 *   Tail: z = (score - mean_b) / sigma; P = 1 - exp(-exp(-(pi / sqrt 6) z - gamma)), the tail of a Gumbel variable with
 *     mean 0 and variance 1; E = targets x P, targets the non-empty targets of the slice. The z-score holds for any
 *     mode; the Gumbel tail is the one of local (OPAL_MODE_SW) scores - for the other modes E is a ranking on the same
 *     scale, not a calibrated expectation.
 *   Hits: with P* = maxEvalue / targets, zCut = -(ln(-log1p(-P*)) + gamma) sqrt 6 / pi and threshold[b] =
 *     ceil(mean_b + zCut sigma), clamped to int32; a target of bin b is a hit iff score >= threshold[b]. P* >= 1:
 *     threshold[b] = INT_MIN for the bins that hold targets (every non-empty target; zCut = -infinity). Bin 0 (empty
 *     targets) and bins without targets: INT_MAX, never a hit.
 *   Degenerate: fewer than 3 targets in the fit, a residual sum that is not positive, or a value that is not finite -
 *     degenerate = 1, every threshold INT_MAX, no hits, and the call returns 0.
 * The outputs are miopalSearchHits' (database order, malloc'ed arrays, maxHits and MIOPAL_ERR_TOO_MANY_HITS - *fit is
 * filled then, too) with *evalue beside them: the E-value of hit i, malloc'ed, NULL without hits. The score rows stay
 * in HBM: per pass 3 KB of sums come back, the 512-byte table goes up, and only the hits cross PCIe.
 * Checks: miopalSearchHits' in their order, then a NULL fit or evalue, a maxEvalue that is not finite and positive, an
 * excludeZ that is NaN: MIOPAL_ERR_BAD_ARGUMENT. An empty slice is checked and answered with *count = 0, NULL arrays and
 * a zeroed fit with degenerate = 1 (no ceilings, every threshold INT_MAX), nothing launched. The score pass takes the
 * kernels miopalSearch takes (miopalLastRouting reports the same). Thread-safe like miopalSearch; the handle builds its
 * bin per target on the device at its first call of this family.
 */
#define MIOPAL_STAT_BINS 128
#define MIOPAL_FIT_MAX_REFITS 3
typedef struct MiopalScoreFit {
    int64_t targets, used;            /* non-empty targets of the slice; targets the last fit rests on */
    int32_t passes, degenerate;       /* 1 + refits done */
    double  intercept, slope, sigma, zCut;
    int64_t binTargets[MIOPAL_STAT_BINS], binLength[MIOPAL_STAT_BINS];   /* n_b, sum of lengths */
    int64_t all[MIOPAL_STAT_BINS][3];    /* n, sum, sum of squares: every target */
    int64_t kept[MIOPAL_STAT_BINS][3];   /* the same under `ceiling` (= all when no refit ran) */
    int32_t ceiling[MIOPAL_STAT_BINS];   /* of the last pass; INT_MAX: none */
    int32_t threshold[MIOPAL_STAT_BINS]; /* a target of bin b is a hit iff score >= threshold[b] */
} MiopalScoreFit;
int miopalSearchSignificant(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                            const int* scoreMatrix, int alphabetLength, int searchType, int mode,
                            int64_t start, int64_t end, double maxEvalue, double excludeZ, int64_t maxHits,
                            MiopalScoreFit* fit, int64_t* count, int64_t** targetIndex, int** score,
                            int** endTarget, int** endQuery, double** evalue);

/*
 * miopalSearchSignificant with a position-specific scoring matrix in the place of (query, scoreMatrix): rowScores as in
 * miopalSearchPssm, no consensus - the inclusion step of an iterated profile search, stated as "E below 1e-3".
 * miopalSearchSignificant's contract holds to the letter. Checked before any device call in miopalSearchPssmHits' order:
 * what needs no handle first (the fit and evalue outputs, maxEvalue and excludeZ behind the null outputs), then the
 * handle, the alphabet length against it, the slice, and the 32-bit range check (OPAL_ERR_OVERFLOW).
 */
int miopalSearchPssmSignificant(MiopalDb* db, const int* rowScores, int queryLength,
                                int gapOpen, int gapExt, int alphabetLength, int searchType, int mode,
                                int64_t start, int64_t end, double maxEvalue, double excludeZ, int64_t maxHits,
                                MiopalScoreFit* fit, int64_t* count, int64_t** targetIndex, int** score,
                                int** endTarget, int** endQuery, double** evalue);

/*
 * miopalSearchSignificant of every query of a batch, with one cut per query (maxEvalue[nQueries]) and one fit per query
 * (fits[nQueries], the caller's): miopalSearchBatchHits' chunks, each chunk's statistics taken for all its rows in one
 * launch, the fits made, the tables uploaded and the rows compacted before they leave. The answer is
 * miopalSearchBatchHits' CSR with *evalue beside the arrays; entries hitOffsets[i] .. hitOffsets[i + 1] and fits[i]
 * equal miopalSearchSignificant of query i alone. maxHits bounds the total; with more, MIOPAL_ERR_TOO_MANY_HITS with
 * hitOffsets and fits filled and nothing allocated. Checks: miopalSearchBatchHits' in their order, then a NULL evalue,
 * a NULL maxEvalue or fits with nQueries > 0, every maxEvalue[i] and excludeZ as in miopalSearchSignificant. nQueries =
 * 0 or an empty slice: checked, hitOffsets all 0, NULL arrays, every fit as for an empty slice, 0.
 */
int miopalSearchBatchSignificant(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                                 int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                                 int mode, int64_t start, int64_t end, const double* maxEvalue, double excludeZ,
                                 int64_t maxHits, MiopalScoreFit* fits, int64_t* hitOffsets, int64_t** targetIndex,
                                 int** score, int** endTarget, int** endQuery, double** evalue);

/*
 * The m best QUERIES of every target of the slice, selected on the device: the selection of miopalSearchBatchTop turned
 * round - which barcode, adapter, primer or motif of a batch matches each read best, and by what margin over the
 * runner-up. queries and queryOffsets as in miopalSearchBatch; all four modes; OPAL_SEARCH_SCORE and
 * OPAL_SEARCH_SCORE_END. For target t of [start, end) the candidates are the queries q with score(q, t) >= minScore
 * (INT_MIN: no bound), score(q, t) being what miopalSearch returns for query q alone; they are ordered by score
 * descending, then query index ascending - a total order: the answer does not depend on how the batch is cut into
 * chunks. count[t - start] = min(m, candidates); queryIndex, score and - for OPAL_SEARCH_SCORE_END - endTarget /
 * endQuery are [end - start][m] row-major, best first, -1 in the slots count .. m - 1 of every array. queryIndex is
 * int32_t: with the target indices it goes straight into miopalAlignPairs as pairQuery. 1 <= m <=
 * MIOPAL_MAX_TARGET_TOP; m > nQueries is allowed. The batch runs through miopalSearchBatch's chunks and single-query
 * path (miopalLastBatchRouting reports what miopalSearchBatch reports for the same inputs); every chunk's
 * [queries][targets] rows are folded into m x (end - start) running entries on the device, and only count and the
 * [end - start][m] arrays cross PCIe.
 * Checks, in this order: OPAL_SEARCH_ALIGNMENT refused with OPAL_ERR_INVALID_MODE; the query list and every query with
 * miopalSearchBatch's checks and codes (OPAL_ERR_OVERFLOW as miopalSearch); m outside its range and null outputs
 * (endTarget / endQuery only for OPAL_SEARCH_SCORE_END): MIOPAL_ERR_BAD_ARGUMENT. An empty slice: checked, 0, nothing
 * written, nothing launched. nQueries = 0 on a slice that is not empty: count all 0, every slot -1, nothing launched.
 * On an error every output is as it was. Thread-safe like miopalSearch: the running state belongs to the call.
 */
#define MIOPAL_MAX_TARGET_TOP 8
int miopalSearchBatchTargetTop(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                               int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                               int mode, int64_t start, int64_t end, int m, int minScore,
                               int* count, int32_t* queryIndex, int* score, int* endTarget, int* endQuery);

/*
 * A list of (query, target) pairs in one call: pair p aligns query pairQuery[p] (queries / queryOffsets as in
 * miopalSearchBatch) with target pairTarget[p] (absolute index into the handle). Any order, repeats allowed; all three
 * search types and all four modes. No reference counterpart (its callers loop over queries); an extension of the
 * resident-handle ABI like miopalSearchBatch.
 * Every output has nPairs entries, in pair order, and entry p equals what miopalSearch returns for query pairQuery[p]
 * against the slice [pairTarget[p], pairTarget[p] + 1) with the same search type, mode, gaps and matrix - score, end
 * and start locations, operations, and the -1 locations / empty operations of an empty alignment (empty queries and
 * targets included). The alignments have miopalSearchFlat's shape: ONE malloc'ed buffer (*operations, caller frees)
 * and operationOffsets[nPairs + 1]. Arrays a search type does not produce may be NULL.
 * Checked before any work, with miopalSearch's codes: every query, the matrix and the alphabet, pairQuery[p] in
 * [0, nQueries) and pairTarget[p] in [0, miopalDbCount) (MIOPAL_ERR_BAD_ARGUMENT, the message names the first bad
 * pair), null outputs, and miopalSearch's 32-bit range check for the longest query and the longest target the list
 * names (OPAL_ERR_OVERFLOW). nPairs = 0: the arguments are checked, nothing is launched, operationOffsets[0] = 0,
 * *operations = NULL, 0. Thread-safe like miopalSearch. Device memory is bounded whatever the list's length: the list
 * is processed in chunks sized from the workspace budgets of an OPAL_SEARCH_ALIGNMENT search.
 */
int miopalAlignPairs(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                     const int32_t* pairQuery, const int64_t* pairTarget, int64_t nPairs,
                     int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength,
                     int searchType, int mode,
                     int* score, int* endTarget, int* endQuery, int* startTarget, int* startQuery,
                     unsigned char** operations, int64_t* operationOffsets);

/*
 * miopalAlignPairs with a list of position-specific scoring matrices in the place of (queries, scoreMatrix): PSSM m
 * holds the rows rowOffsets[m] .. rowOffsets[m + 1] of rowScores (nPssms + 1 offsets, alphabetLength ints per row),
 * and consensus is indexed in the same row coordinates (entries: a residue or 255; required for
 * OPAL_SEARCH_ALIGNMENT, may be NULL otherwise). Pair p aligns PSSM pairPssm[p] with target pairTarget[p], and entry p
 * of every output equals what miopalSearchPssm returns for that PSSM against the slice [pairTarget[p],
 * pairTarget[p] + 1) - the -1 locations and empty operations of an empty alignment, empty PSSMs and empty targets
 * included. Outputs, the nPairs = 0 behaviour, chunking and thread safety as miopalAlignPairs; any order, repeats
 * allowed, all three search types and four modes. miopalLastPairRouting reports the call like a plain pair list.
 * Checked before any work, with the existing codes: mode and search type; the offsets (non-negative, non-decreasing,
 * at most INT32_MAX - 64 rows in total); NULL rowScores; the alphabet length's range; the consensus (NULL for an
 * alignment search, an entry that is neither a residue nor 255); pairPssm[p] in [0, nPssms) (the message names the
 * first bad pair); null outputs; then the handle, the alphabet length against it, pairTarget[p] in
 * [0, miopalDbCount); and the 32-bit range check with the extreme entries of the rows, the tallest PSSM and the
 * longest target the list names (OPAL_ERR_OVERFLOW).
 * One lane per pair - the forward pass as well as the start-cell scan and the direction pass of
 * OPAL_SEARCH_ALIGNMENT - keeps the rows of ALL the list's PSSMs in LDS: it is taken when
 * (total rows + 1) * (alphabetLength + 1) * 4 bytes fit 64 KB less 256 (493 rows at 32 letters, 651 at 24), under
 * miopalAlignPairs' cost estimates. A list with more rows runs one wavefront per pair throughout (counts[0] of
 * miopalLastPairRouting is 0): the same results, more slowly for large lists.
 * Out of scope: a table per workgroup for lists whose rows do not fit.
 */
int miopalAlignPairsPssm(MiopalDb* db, const int* rowScores, const unsigned char* consensus,
                         const int64_t* rowOffsets, int nPssms,
                         const int32_t* pairPssm, const int64_t* pairTarget, int64_t nPairs,
                         int gapOpen, int gapExt, int alphabetLength, int searchType, int mode,
                         int* score, int* endTarget, int* endQuery, int* startTarget, int* startQuery,
                         unsigned char** operations, int64_t* operationOffsets);

/*
 * How the calling thread's most recent miopalAlignPairs / miopalAlignPairsPssm ran (diagnostics for tests):
 *   counts[0] pairs whose forward pass ran in the lane-per-pair kernel (pairlist_forward_kernel)
 *   counts[1] pairs whose forward pass ran in the wavefront-per-pair kernel
 *   counts[2] pairs answered without a DP (empty query or target)
 *   counts[3] chunks
 */
void miopalLastPairRouting(int64_t counts[4]);

/*
 * Query-anchored profile columns from hits: the step between two rounds of an iterated profile search. The
 * alignments of one query - (query, scoreMatrix), or for miopalProfileColumnsPssm the PSSM (rowScores, consensus) of
 * miopalSearchPssm - with the targets targets[0 .. nTargets) (absolute indices, any order, repeats allowed) are
 * projected onto the query's rows, counted and weighted on the device; the operations never cross PCIe.
 * Members: member 0 is the query itself (row: query[i], or consensus[i], 255 = no residue); member 1 + p is target
 * targets[p], aligned as miopalAlignPairs / miopalAlignPairsPssm align that pair with OPAL_SEARCH_ALIGNMENT.
 * A member's row[0 .. queryLength): every entry 255 (not covered), then, walking the operations from (startQuery,
 * startTarget): OPAL_ALIGN_MATCH / MISMATCH at query row i with target residue t: row[i] = t; OPAL_ALIGN_DEL (a query
 * residue against a gap): row[i] = alphabetLength, the gap letter; OPAL_ALIGN_INS: nothing is recorded. An empty
 * alignment (an empty target, a Smith-Waterman score of 0) leaves the row all 255.
 * Outputs (host arrays of the caller), with A = alphabetLength:
 *   counts[queryLength][A + 1]    members with row[i] == a; index A is the gap letter
 *   memberWeight[nTargets + 1]    with k_i the letters a < A that occur in column i and term[i][a] =
 *                                 floor(2^32 / (k_i counts[i][a])) for those letters (64-bit unsigned division): the sum
 *                                 of term[i][row[i]] over the member's rows with a letter - Henikoff position-based
 *                                 weights in 32.32 fixed point (MIOPAL_PROFILE_WEIGHT_ONE is 1.0)
 *   weighted[queryLength][A + 1]  the sum of memberWeight over the members with row[i] == a
 *   msa[nTargets + 1][queryLength] the rows (NULL: not wanted - the multiple alignment then never leaves the device)
 * All integer sums, the same in any order; none exceeds queryLength * 2^32.
 * Checked before any device call, with the existing codes: the checks of miopalAlignPairs / miopalAlignPairsPssm in
 * that function's order (the messages name "target p"); then NULL counts / weighted / memberWeight; then
 * (nTargets + 1) * queryLength above 4 GiB (MIOPAL_ERR_BAD_ARGUMENT, the message states the bytes). nTargets = 0: the
 * profile of the query alone, answered on the host. queryLength = 0: nothing is written. On an error every output is as
 * it was. miopalLastPairRouting reports the call like a plain pair list. Thread safety as miopalSearch.
 */
#define MIOPAL_PROFILE_WEIGHT_ONE (1ll << 32)
int miopalProfileColumns(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                         const int* scoreMatrix, int alphabetLength, int mode,
                         const int64_t* targets, int64_t nTargets,
                         int64_t* counts, int64_t* weighted, int64_t* memberWeight, unsigned char* msa);
int miopalProfileColumnsPssm(MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength,
                             int gapOpen, int gapExt, int alphabetLength, int mode,
                             const int64_t* targets, int64_t nTargets,
                             int64_t* counts, int64_t* weighted, int64_t* memberWeight, unsigned char* msa);

/*
 * How the calling thread's most recent miopalSearchBatch ran (diagnostics for tests):
 *   counts[0] (query, target) pairs settled by the batch kernels
 *   counts[1] (query, target) pairs run by the wavefront-per-pair kernel
 *   counts[2] queries sent to the single-query path
 *   counts[3] launches of the batch kernels
 */
void miopalLastBatchRouting(int64_t counts[4]);

/*
 * How the passes BEHIND the score / end pass of the calling thread's most recent OPAL_SEARCH_ALIGNMENT
 * search ran (diagnostics for tests; no reference counterpart). Bits:
 *   1  start cells: one lane per pair          2  ... in the query-profile form (perpair_profile_kernel)
 *   4  directions: one lane per pair           8  ... in the query-profile form
 *  16  operations copied to the host batch by batch beside the next batch
 *  32  start cells by persistent wavefronts whose lanes take the next pair when they are done
 *      (perpair_scan_refill_kernel: queries of one 64-row strip)
 *  64  directions: two pairs per lane on 16-bit halves (perpair_packed.hip)
 * 128  start cells: two pairs per lane on 16-bit halves
 * 256  directions: one launch of the packed kernel per group of traceback batches
 * 0: no such search yet, or one whose traceback batches were built on the host.
 */
int miopalLastFullRouting(void);

/* Result-struct form, identical in shape to opalSearchDatabase but against
 * the resident mirror (what the platform plugin calls). */
int miopalSearchResults(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen,
                        int gapExt, const int* scoreMatrix, int alphabetLength,
                        OpalSearchResult* results[], int searchType, int mode,
                        int overflowMethod, int64_t start, int64_t end);

/*
 * Host-side self tests of the scheduler that need no device (test hook; no reference counterpart).
 *   which = 1  the packed-view cache survives a builder that throws: the placeholder is dropped, the
 *              call returns MIOPAL_ERR_INTERNAL, waiters are woken and the same slice can be built
 *              afterwards (a leaked placeholder would block every later search of the slice).
 * Returns 0 when the property holds, a positive step number otherwise.
 */
int miopalSelfTest(int which);

/*
 * Fault injection for the time-out escapes of the strip hand-over (test hook; no reference
 * counterpart; an argument of the NEXT search of the calling thread, not an environment switch):
 *   kind 1  unit `unit` of the pair-table strips kernels (Smith-Waterman or NW / HW / OV of several
 *           strips) publishes nothing: the units below it give up after `spinCap` polls, flag their
 *           lanes, and the int32 kernel returns the right scores;
 *   kind 2  unit `unit` of the wavefront-per-pair strips kernel publishes nothing: the search returns
 *           MIOPAL_ERR_INTERNAL and the handle stays usable.
 * spinCap = 0 keeps the kernels' own patience (about a second).
 */
void miopalTestInjectFault(int kind, int unit, int spinCap);

/*
 * Tuning switches (diagnostics and A/B levers; pyopal_amd/csrc/tuning.h lists them). Each is MIOPAL_<NAME>
 * in the environment, which the library reads ONCE, at its first use of any switch; afterwards a switch
 * only changes through miopalSetTuning. Nothing on the search path calls getenv: the searches run without
 * the GIL on many threads (src/pyopal/lib.pyx:1364) and getenv racing another thread's putenv is a data
 * race in the C library. `name` with or without the MIOPAL_ prefix; value NULL = unset. The change is seen
 * by searches that start after the call. No reference counterpart.
 */
int miopalSetTuning(const char* name, const char* value);
const char* miopalGetTuning(const char* name);   /* NULL: unset or unknown */

/*
 * Per-handle options: the two product knobs among the switches, as arguments instead of process-wide
 * environment (value -1 = back to the process default):
 *   "reserve_cus"   compute units kept out of the persistent search launches - the pair-table kernels of one
 *                   query and the batch kernels; at least one workgroup is always launched -, so that the
 *                   kernels of a collective that gathers the previous search's scores (one process per GPU,
 *                   RCCL) find room beside the search (bench.py, multi-GPU ranks: 8); default
 *                   MIOPAL_RESERVE_CUS / none. miopalLastLaunchShape reports the width a launch got.
 *   "small_search"  1: searches of few targets may take the wavefront-per-pair kernel (shorter start-up),
 *                   0: they stay on the lane-per-target kernels; default 1 unless MIOPAL_NO_SMALL_SEARCH
 */
int miopalDbSetOption(MiopalDb* db, const char* name, int64_t value);

/*
 * Test hook: `count` > 0 makes miopalDeviceCount() report that many devices, ordinals 0 .. count - 1 mapped
 * round-robin onto the physical gfx950 devices, so that the multi-device path of a one-process caller
 * (pyopal_amd.align: a handle, mirror and stream set per ordinal, hipSetDevice per call,
 * src/pyopal/_align.py:150-170) runs on a box with one GPU. 0 restores the physical devices.
 */
int miopalTestSetLogicalDevices(int count);

/*
 * Test hook: the device top-k selection of miopalSearchTop / miopalSearchBatchTop alone, on rows of int32 scores the
 * caller supplies (any int32 values), with no search and no handle in front of it. score, and endTarget / endQuery
 * (both or neither), are host arrays [rows][stride]; entry i of a row has the index start + i. The rows are uploaded
 * to device 0, selected by the production kernels exactly as a search's rows are (order, minScore, count and the -1
 * of the slots past the count: miopalSearchTop's), and the outputs downloaded: count[rows], the others [rows][k]
 * (outEndTarget / outEndQuery may be NULL without end arrays). *gaveUp receives the number of blocks that gave up
 * waiting for the blocks before them (0 unless the device is broken; a search turns it into MIOPAL_ERR_INTERNAL).
 * MIOPAL_ERR_BAD_ARGUMENT, before any device call: rows < 1, stride < 1, k outside [1, MIOPAL_MAX_TOP], a null
 * input or output, one end array without the other, rows x stride above 2^27.
 */
int miopalTestSelectTop(const int* score, const int* endTarget, const int* endQuery,
                        int rows, int64_t stride, int k, int minScore, int64_t start,
                        int* count, int64_t* targetIndex, int* outScore, int* outEndTarget, int* outEndQuery,
                        int* gaveUp);

/*
 * Test hook: the device compaction of miopalSearchHits and its forms alone, on rows of int32 scores the caller
 * supplies (any int32 values), with no search and no handle in front of it. score, and endTarget / endQuery (both or
 * neither), are host arrays [rows][stride]; entry i of a row has the index start + i; row r keeps its entries >=
 * minScore[r]. The rows are uploaded to device 0 and compacted by the production kernels exactly as a search's rows
 * are; the answer is miopalSearchBatchHits' CSR: hitOffsets[rows + 1] (the caller's) and malloc'ed arrays (NULL
 * without hits; outEndTarget / outEndQuery may be NULL without end arrays).
 * MIOPAL_ERR_BAD_ARGUMENT, before any device call: rows < 1, stride < 1, a null input or output, one end array
 * without the other, rows x stride above 2^27.
 */
int miopalTestSelectHits(const int* score, const int* endTarget, const int* endQuery,
                         int rows, int64_t stride, const int* minScore, int64_t start,
                         int64_t* hitOffsets, int64_t** targetIndex, int** outScore, int** outEndTarget,
                         int** outEndQuery);

/*
 * Test hook: the statistics kernels of miopalSearchSignificant alone, on rows of int32 scores the caller supplies (any
 * int32 values), with no search and no handle in front of them. score is a host array [rows][stride]; column i belongs
 * to a target of length[i] (>= 0). The device turns the lengths into bins and sums, per (row, bin), n, score and
 * score^2 of the entries with score <= ceiling[row][bin] (ceiling [rows][MIOPAL_STAT_BINS], or NULL: every entry) as
 * 64-bit two's-complement integers that wrap; rows with skip[row] != 0 (skip may be NULL) are not read and stay 0.
 * Outputs: stats [rows][MIOPAL_STAT_BINS][3] and the device's bin[stride]. Device 0.
 * MIOPAL_ERR_BAD_ARGUMENT, before any device call: rows < 1, stride < 1, a null input or output, a negative length,
 * rows x stride above 2^27.
 */
int miopalTestRowStats(const int* score, int rows, int64_t stride, const int32_t* length, const int32_t* ceiling,
                       const int* skip, int64_t* stats, unsigned char* bin);

/*
 * Test hook: miopalTestSelectHits with length[stride] (>= 0) and threshold[rows][MIOPAL_STAT_BINS] in the place of
 * minScore: entry i of row r is kept iff score >= threshold[r][bin of length[i]] - the binned compaction of
 * miopalSearchSignificant alone. Everything else, the checks included, as miopalTestSelectHits (a null length or
 * threshold and a negative length: MIOPAL_ERR_BAD_ARGUMENT).
 */
int miopalTestSelectHitsBinned(const int* score, const int* endTarget, const int* endQuery,
                               int rows, int64_t stride, const int32_t* length, const int32_t* threshold,
                               int64_t start, int64_t* hitOffsets, int64_t** targetIndex, int** outScore,
                               int** outEndTarget, int** outEndQuery);

/*
 * Test hook: the occurrence picker of miopalSearchOccurrences alone, with no alignment in front of it. value is a host
 * array [rows][stride] of int32 (any values); columns 0 .. length[r] - 1 of row r are valid; valueRow, of the same
 * shape, holds the row reported with each column, or is NULL: -1 throughout. Row r is picked by the rule of
 * miopalSearchOccurrences with minScore and window, by the production picker through the launchers the search uses -
 * count, offsets, write - one lane per row on device 0. The answer is a CSR like miopalTestSelectHits': hitOffsets
 * [rows + 1] (the caller's) and the malloc'ed *column, *score, *row (NULL without occurrences).
 * MIOPAL_ERR_BAD_ARGUMENT, before any device call: rows < 1, stride < 1, a null pointer (valueRow excepted), rows x
 * stride above 2^27, a length outside [0, stride], a negative window.
 */
int miopalTestPickOccurrences(const int* value, const int* valueRow, int rows, int64_t stride, const int32_t* length,
                              int minScore, int window, int64_t* hitOffsets, int32_t** column, int** score, int** row);

/*
 * Test hook: the device selection of miopalSearchBatchTargetTop alone - the m best rows of every column - on rows of
 * int32 scores the caller supplies (any int32 values), with no search and no handle in front of it. score, and
 * endTarget / endQuery (both or neither), are host arrays [rows][stride]. The rows are uploaded to device 0 and folded
 * by the production kernels, piece by piece in the order of the list: piece p is rows pieceFirst[p] .. pieceFirst[p] +
 * pieceCount[p] - 1 (at least one row), with base query index pieceFirst[p]; a row may appear in at most one piece, and
 * rows in no piece are not part of the answer. skip (one byte per row, or NULL): skip[r] != 0 - row r is never read.
 * The answer is miopalSearchBatchTargetTop's: count[stride], the others [stride][m] (outEndTarget / outEndQuery may be
 * NULL without end arrays), best first (score descending, row ascending), -1 past the count.
 * MIOPAL_ERR_BAD_ARGUMENT, before any device call: rows < 1, stride < 1, m outside [1, MIOPAL_MAX_TARGET_TOP], a null
 * input or output, one end array without the other, a piece outside [0, rows), rows x stride above 2^27.
 */
int miopalTestSelectColumns(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride,
                            const int32_t* pieceFirst, const int32_t* pieceCount, int pieces,
                            const unsigned char* skip, int m, int minScore,
                            int* count, int32_t* queryIndex, int* outScore, int* outEndTarget, int* outEndQuery);

/*
 * Test hook: the count / terms / member weights / weighted kernels of miopalProfileColumns alone, on device 0, on a
 * host multiple alignment msa[members][queryLength] whose entries are a letter (< alphabetLength), the gap
 * (== alphabetLength) or 255. counts, weighted ([queryLength][alphabetLength + 1]) and memberWeight ([members]) as
 * miopalProfileColumns returns them.
 * MIOPAL_ERR_BAD_ARGUMENT, before any device call: members < 1, queryLength < 1, an alphabet length out of range, a
 * null pointer, members x queryLength above 2^27, an entry that is neither a letter, the gap nor 255.
 */
int miopalTestProfileColumns(const unsigned char* msa, int64_t members, int queryLength, int alphabetLength,
                             int64_t* counts, int64_t* weighted, int64_t* memberWeight);

#ifdef __cplusplus
}
#endif
#endif /* MIOPAL_H */
