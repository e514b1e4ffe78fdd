// Tuning switches of the library: read from the environment ONCE (first use), kept in a process-wide
// table of atomics, changed afterwards only through miopalSetTuning (include/miopal.h). Nothing on the
// search path calls getenv: the C ABI is called without the GIL from many threads
// (src/pyopal/lib.pyx:1364) and getenv racing another thread's putenv is a data race in the C library.
//
// Every switch is MIOPAL_<NAME> in the environment. Switches are diagnostics and A/B levers; the two
// product knobs among them (CUs kept out of the persistent launch for a collective, the routing of small
// searches) are also per-handle options (miopalDbSetOption), which take precedence.
#pragma once
#include <atomic>

namespace miopal {

#define MIOPAL_TUNING_SWITCHES(X)                                                                          \
    X(BATCH_OCCURRENCE_ENTRIES) X(BATCH_OCCURRENCE_WORKGROUPS_PER_CU)                                      \
    X(COLUMN_SPLIT) X(DEVICE) X(FORCE_LANE_PER_PAIR) X(HOST_THREADS) X(HOST_TRACEBACK) X(NO_ASYNC_SHARES) X(NO_BIASED)     \
    X(NO_CALLER_PINNED) X(NO_DIAG_SHIFT) X(NO_DIRECT_SCATTER) X(NO_EARLY_HOST_SHARE) X(NO_GLOBAL_STRIPS)   \
    X(NO_HOST_SCATTER) X(NO_HUGEPAGE) X(NO_HYBRID_TRACE) X(NO_JOBS_AHEAD) X(NO_ONE_LAUNCH)                 \
    X(NO_PACKED_HW_SCAN) X(NO_PACKED_SCAN) X(NO_PACKED_TRACE) X(NO_PAIR_STRIPS) X(NO_PAIR_STRIP_UNITS)     \
    X(NO_PAIR_TABLE) X(NO_PERPAIR) X(NO_PERPAIR_PROFILE) X(NO_SCAN_ORDER) X(NO_SCAN_REFILL)                \
    X(NO_SEGMENTS) X(NO_SIDE_COPIES) X(NO_SIDE_STREAM) X(NO_SMALL_SEARCH) X(NO_SORT_BY_ROWS)               \
    X(NO_SW_SHIFT) X(NO_TWO_PASS_ENDS) X(NO_UNPACK_CREW) X(NO_VIEW_PREFETCH) X(ONE_LAUNCH_GROUP)           \
    X(PAIR_STRIPS) X(PARKED_WORKSPACE_MB) X(PHASE_TIMING) X(RESERVE_CUS) X(SEARCH_UNDER_UPLOAD)            \
    X(SPARE_HANDLE_MB) X(STRIPS) X(STRIP_TIMING) X(TAIL_THROTTLE) X(TEST_REFUSE_PAIR_LAUNCH)               \
    X(TEST_SPLIT_EPOCH) X(TEST_WINDOW_STRIDE)                                                              \
    X(TWO_PASS_ENDS) X(UNITS) X(UPLOAD_PIECE_KB) X(UPLOAD_STREAMS) X(UPLOAD_THREADS) X(VERBOSE)            \
    X(VIEW_CACHE_MB)

enum class Tune : int {
#define X(name) name,
    MIOPAL_TUNING_SWITCHES(X)
#undef X
    kCount
};

// The value of a switch (a NUL-terminated string that lives for the rest of the process), or null when it
// is not set - what getenv("MIOPAL_<NAME>") returned when the table was filled, unless changed since.
const char* tuned(Tune key);

}  // namespace miopal
