// Host-side scheduler behind the C ABI of include/opal.h and include/miopal.h.
//
// Plays the role of the scalar driver code of opalSearchDatabase (declared
// src/pyopal/opal.pxd:38-52, called src/pyopal/platform/pyx.in:76-91): argument
// checks, choice of lane width per target (the reference's 8/16/32-bit ladder,
// src/pyopal/lib.pyx:1283-1289, becomes packed-16 / 32 here), the score pass,
// the reversed-prefix pass for start locations and the traceback, all against
// a device-resident database.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <exception>
#include <ctime>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <sys/mman.h>
#include <thread>
#include <vector>

#include "../../include/miopal.h"
#include "common.h"
#include "full_plan_selftest.h"
#include "launch_layer_selftest.h"
#include "occurrences.h"
#include "occurrences_batch.h"
#include "occurrence_align.h"
#include "occurrence_align_batch.h"
#include "occurrence_plan_selftest.h"
#include "profile_columns.h"
#include "score_ranges_selftest.h"
#include "select_columns.h"
#include "select_hits.h"
#include "select_stats.h"
#include "select_top.h"
#include "tuning.h"

using namespace miopal;

// ---------------------------------------------------------------------------
// tuning switches (tuning.h): the environment is read here, once, and nowhere else
// ---------------------------------------------------------------------------
namespace miopal {
namespace {
const char* const kTuningNames[] = {
#define X(name) "MIOPAL_" #name,
    MIOPAL_TUNING_SWITCHES(X)
#undef X
};
struct Tuning {
    std::atomic<const char*> value[(int)Tune::kCount];
    Tuning() { fromEnv(); }
    // (copies: a later putenv of the process may not pull a string from under a search)
    void fromEnv() {
        for (int k = 0; k < (int)Tune::kCount; ++k) {
            const char* v = getenv(kTuningNames[k]);
            value[k].store(v ? strdup(v) : nullptr, std::memory_order_release);
        }
    }
    static Tuning& table() {
        static Tuning t;   // (thread-safe initialisation)
        return t;
    }
    static int find(const char* name) {
        if (!name) return -1;
        if (strncmp(name, "MIOPAL_", 7) == 0) name += 7;
        for (int k = 0; k < (int)Tune::kCount; ++k)
            if (strcmp(kTuningNames[k] + 7, name) == 0) return k;
        return -1;
    }
};
}  // namespace
const char* tuned(Tune key) { return Tuning::table().value[(int)key].load(std::memory_order_acquire); }
}  // namespace miopal

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
namespace {

thread_local std::string g_lastError;
thread_local int64_t g_lastRouting[4] = {0, 0, 0, 0};  // miopalLastRouting
thread_local int64_t g_lastWindowPlan[4] = {0, 0, 0, 0};  // miopalLastWindowPlan
thread_local int64_t g_lastLaunchShape[4] = {0, 0, 0, 0};  // miopalLastLaunchShape
thread_local int64_t g_lastBatchRouting[4] = {0, 0, 0, 0};  // miopalLastBatchRouting
thread_local int g_lastFullRouting = 0;                // miopalLastFullRouting
thread_local int g_fault[3] = {0, 0, 0};               // miopalTestInjectFault: kind, unit, spin cap
// miopalTestSetLogicalDevices: > 0 = that many device ordinals, mapped round-robin onto the physical
// devices (the multi-device code of a one-process caller - a handle, a stream set, a mirror per
// ordinal, hipSetDevice per call - on a box with one GPU)
std::atomic<int> g_logicalDevices{0};

// HIP ordinals of the gfx950 devices, in order: the only ones the kernels were built for. Device ordinals of this
// library index THIS list (on a box with nothing but MI355X: the identity).
const std::vector<int>& usableDevices() {
    static const std::vector<int> list = [] {
        std::vector<int> v;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) return v;
        for (int d = 0; d < n; ++d) {
            hipDeviceProp_t p;
            if (hipGetDeviceProperties(&p, d) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) v.push_back(d);
        }
        return v;
    }();
    return list;
}
int physicalDeviceCount() { return (int)usableDevices().size(); }

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_lastError = buf;
    return code;
}

// the range check of the 32-bit kernels (score_ranges.h), as every entry point reports it
int checkInt32Range(const ScoreModel& m, int64_t Q, int64_t maxLen) {
    const int64_t bound = int32Bound(m, Q, maxLen);
    if (!int32Fits(bound))
        return fail(OPAL_ERR_OVERFLOW, "scores may exceed the 32-bit range (bound %lld)", (long long)bound);
    return 0;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(MIOPAL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                               \
    } while (0)

#define RC_TRY(expr)          \
    do {                      \
        int _rc = (expr);     \
        if (_rc) return _rc;  \
    } while (0)

// The two events around a timed launch: destroyed unless they were handed to the workspace's list
// (the score pass has early returns between the first record and the hand-over).
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    std::pair<hipEvent_t, hipEvent_t> release() {
        std::pair<hipEvent_t, hipEvent_t> p(e0, e1);
        e0 = e1 = nullptr;
        return p;
    }
};

// Device memory and a stream of a call that runs without a handle (the test hooks of the selection kernels, the
// handle's length bins while they are built): released on every way out
struct DeviceBytes {
    void* p = nullptr;
    DeviceBytes() = default;
    DeviceBytes(const DeviceBytes&) = delete;
    DeviceBytes& operator=(const DeviceBytes&) = delete;
    ~DeviceBytes() {
        if (p) (void)hipFree(p);
    }
};
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

struct PhaseTimer {
    bool on;
    double t0;
    static double now() {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec + 1e-9 * ts.tv_nsec;
    }
    PhaseTimer() : on(tuned(Tune::PHASE_TIMING) != nullptr), t0(now()) {}
    void mark(const char* what) {
        if (!on) return;
        const double t = now();
        fprintf(stderr, "[miopal] %-28s %8.3f ms\n", what, (t - t0) * 1e3);
        t0 = t;
    }
};

// Streams that only carry uploads (database pieces, view construction) are created at the LOWEST
// priority: the runtime multiplexes streams onto four hardware queues per priority level, and every
// stream left at the default level makes it likelier that two workspaces' search streams share one.
inline hipError_t createUploadStream(hipStream_t* s) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
        (void)hipGetLastError();
        least = greatest = 0;
    }
    if (least > 0) return hipStreamCreateWithPriority(s, hipStreamNonBlocking, least);
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

constexpr int kLongTarget = 8192;          // longer targets always take the intra-sequence path
static_assert(kPlanLanes == kLanes, "full_plan.h counts in wavefronts of kLanes");   // (kDirBudget, kDirBudgetOneLaunch: full_plan.h)
constexpr int kMaxDirectRecompute = 2048;  // lanes that left their range and are sent straight to int32: at least this many (see directLimit)
// A lane that owns a whole target walks its columns one after the other (about 0.8 us per
// column of 56 rows): whatever the number of targets, the lane-per-target kernels need
// (longest target) x that. Few targets of a one-strip query are done sooner by the
// wavefront-per-pair kernel, whose anti-diagonal step is ~10x shorter and which still has a
// wavefront for every pair at this count.
constexpr int64_t kSmallSearch = 4096;
constexpr size_t kParkedWorkspaceFloor = 4ull << 30;   // idle per-handle workspaces kept: this, or four times the database (host_types.inc)
constexpr size_t kMaxCachedViews = 64;                 // packed views per handle (beside the byte budget)

// malloc-backed byte buffer: grows without zero-filling, and its storage can be handed to the
// caller of the C ABI (who frees it with free()).
struct HostBytes {
    uint8_t* data = nullptr;
    size_t size = 0, cap = 0;
    // `data` is a buffer the caller of the C ABI lent for this search (miopalSearchFlatInto): written in
    // place when it is large enough, never freed or moved here - a search that needs more leaves it alone
    // and returns a buffer of its own
    bool lent = false;
    HostBytes() = default;
    HostBytes(const HostBytes&) = delete;
    HostBytes& operator=(const HostBytes&) = delete;
    ~HostBytes() {
        if (!lent) free(data);
    }
    void lend(uint8_t* buffer, size_t capacity) {
        if (!buffer || capacity == 0) return;
        data = buffer;
        cap = capacity;
        size = 0;
        lent = true;
    }
    bool reserve(size_t want) {
        if (want <= cap) return true;
        want = std::max(want, cap + cap / 2);
        uint8_t* keep = nullptr;   // a lent buffer that is too small: its contents move, it stays the caller's
        if (lent) {
            keep = data;
            data = nullptr;
            lent = false;
            want += want / 4;   // (the next search of this kind fits the buffer it gets back)
        } else if (!data && want >= (8u << 20)) {
            // (a first large buffer too: lent back, it is judged against the NEXT search's worst case - a query of the
            // same length whose longest window rounds sixteen columns up must not find it too small)
            want += want / 4;
        }
        const bool hugePages = !tuned(Tune::NO_HUGEPAGE);
        if (!data && want >= (8u << 20) && hugePages) {
            // a large result buffer is written once, front to back: ask for huge pages so that
            // first touch costs tens of faults instead of tens of thousands
            void* p = nullptr;
            if (posix_memalign(&p, 2u << 20, want) == 0) {
                madvise(p, want, MADV_HUGEPAGE);
                data = (uint8_t*)p;
                if (keep && size) memcpy(data, keep, size);
                cap = want;
                return true;
            }
        }
        uint8_t* p = (uint8_t*)realloc(data, want);
        if (!p) {
            if (keep) {   // (as before the call)
                data = keep;
                lent = true;
            }
            return false;
        }
        if (keep && size) memcpy(p, keep, size);
        data = p;
        cap = want;
        return true;
    }
    bool resize(size_t n) {
        if (!reserve(std::max<size_t>(n, 1))) return false;
        size = n;
        return true;
    }
    bool append(const uint8_t* src, size_t n) {
        if (!reserve(size + n)) return false;
        memcpy(data + size, src, n);
        size += n;
        return true;
    }
    // the storage leaves for the caller (a lent buffer goes back the same way); `capacity`: its size in bytes
    uint8_t* release(size_t* capacity = nullptr) {
        uint8_t* p = data;
        if (capacity) *capacity = cap;
        data = nullptr;
        size = cap = 0;
        lent = false;
        return p;
    }
};

#include "host_workspace.inc"
#include "host_types.inc"
#include "host_upload.inc"
#include "host_view.inc"
#include "host_search.inc"
#include "host_handle.inc"
// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int miopalDeviceCount(void) {
    const int physical = physicalDeviceCount();
    const int logical = g_logicalDevices.load(std::memory_order_relaxed);
    return (logical > 0 && physical > 0) ? logical : physical;
}

int miopalTestSetLogicalDevices(int count) {
    if (count < 0 || count > 64) return fail(MIOPAL_ERR_BAD_ARGUMENT, "logical device count %d not in 0..64", count);
    g_logicalDevices.store(count, std::memory_order_relaxed);
    return 0;
}

int miopalSetTuning(const char* name, const char* value) {
    const int k = Tuning::find(name);
    if (k < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "unknown tuning switch %s", name ? name : "(null)");
    // (the old string is left alone: a search on another thread may be reading it)
    Tuning::table().value[k].store(value ? strdup(value) : nullptr, std::memory_order_release);
    return 0;
}

const char* miopalGetTuning(const char* name) {
    const int k = Tuning::find(name);
    return k < 0 ? nullptr : tuned((Tune)k);
}

int miopalDbSetOption(MiopalDb* db, const char* name, int64_t value) {
    if (!db || !name) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null handle / option name");
    if (strcmp(name, "reserve_cus") == 0) {
        if (value < -1 || value > 4096) return fail(MIOPAL_ERR_BAD_ARGUMENT, "reserve_cus %lld out of range", (long long)value);
        db->optReserveCus.store((int)value, std::memory_order_relaxed);
        return 0;
    }
    if (strcmp(name, "small_search") == 0) {
        if (value < -1 || value > 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "small_search takes -1 (default), 0 or 1");
        db->optSmallSearch.store((int)value, std::memory_order_relaxed);
        return 0;
    }
    return fail(MIOPAL_ERR_BAD_ARGUMENT, "unknown handle option %s", name);
}

const char* miopalLastError(void) { return g_lastError.c_str(); }

int miopalDbCreate(MiopalDb** out, const unsigned char* const* sequences, const int* lengths,
                   int64_t count, int alphabetLength, int device) {
    return guarded([&]() -> int {
    if (!out || count < 0 || (count > 0 && (!sequences || !lengths)))
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad arguments to miopalDbCreate");
    if (alphabetLength <= 0 || alphabetLength > kMaxAlphabet)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d not in 1..32", alphabetLength);
    if (count >= INT32_MAX) return fail(MIOPAL_ERR_BAD_ARGUMENT, "too many sequences");
    std::vector<int64_t> offsets((size_t)count + 1, 0);
    for (int64_t k = 0; k < count; ++k) {
        if (lengths[k] < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative sequence length");
        offsets[(size_t)k + 1] = offsets[(size_t)k] + lengths[k];
    }
    for (int64_t k = 0; k < count; ++k)
        if (lengths[k] > 0 && !sequences[k]) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null sequence %lld", (long long)k);
    ResidueSource src;
    src.sequences = sequences;
    return createCommon(out, src, std::move(offsets), count, alphabetLength, device);
    });
}

int miopalDbCreateFlat(MiopalDb** out, const unsigned char* residues, const int64_t* offsets,
                       int64_t count, int alphabetLength, int device) {
    return guarded([&]() -> int {
    if (!out || count < 0 || !offsets) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad arguments to miopalDbCreateFlat");
    if (alphabetLength <= 0 || alphabetLength > kMaxAlphabet)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d not in 1..32", alphabetLength);
    if (count >= INT32_MAX) return fail(MIOPAL_ERR_BAD_ARGUMENT, "too many sequences");
    std::vector<int64_t> off(offsets, offsets + count + 1);
    if (off[0] != 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "offsets must start at 0");
    for (int64_t k = 0; k < count; ++k)
        if (off[(size_t)k + 1] < off[(size_t)k] || off[(size_t)k + 1] - off[(size_t)k] > INT32_MAX)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "offsets must be non-decreasing");
    if (off[(size_t)count] > 0 && !residues) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null residues");
    ResidueSource src;
    src.flat = residues;
    return createCommon(out, src, std::move(off), count, alphabetLength, device);
    });
}

int miopalDbCreateSubset(MiopalDb** out, const MiopalDb* parent, const int64_t* indices, int64_t count) {
    return guarded([&]() -> int {
    if (!out) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null output handle");
    *out = nullptr;
    if (!parent) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null parent handle");
    if (count < 0 || (count > 0 && !indices) || count >= INT32_MAX) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad subset");
    std::vector<int64_t> offsets((size_t)count + 1, 0), srcStart((size_t)std::max<int64_t>(count, 1), 0);
    for (int64_t k = 0; k < count; ++k) {
        const int64_t id = indices[k];
        if (id < 0 || id >= parent->count) return fail(MIOPAL_ERR_BAD_ARGUMENT, "subset index %lld outside the database", (long long)id);
        srcStart[(size_t)k] = parent->offsets[(size_t)id];
        offsets[(size_t)k + 1] = offsets[(size_t)k] + (parent->offsets[(size_t)id + 1] - parent->offsets[(size_t)id]);
    }
    std::unique_ptr<MiopalDb> db;
    RC_TRY(newHandle(&db, parent->device));
    db->alphabet = parent->alphabet;
    db->count = count;
    db->total = offsets[(size_t)count];
    for (int64_t k = 0; k < count; ++k) db->maxLen = std::max(db->maxLen, offsets[(size_t)k + 1] - offsets[(size_t)k]);
    const size_t wantRes = (size_t)db->total + 64, wantOff = (size_t)(count + 1) * sizeof(int64_t);
    HIP_TRY(hipMalloc(&db->d_residues, wantRes));
    db->residueCap = wantRes;
    HIP_TRY(hipMalloc(&db->d_offsets, wantOff));
    db->offsetsCap = wantOff;
    RC_TRY(uploadOnce(db->device, db->d_offsets, offsets.data(), wantOff));
    if (count > 0) {
        // the residues never leave the device: gathered from the parent's resident copy
        // (on a stream of its own: the null stream would serialise against every blocking stream of the process)
        struct Scratch {
            int64_t* d_src = nullptr;
            hipStream_t stream = nullptr;
            ~Scratch() {
                if (stream) (void)hipStreamDestroy(stream);
                if (d_src) (void)hipFree(d_src);
            }
        } scratch;
        HIP_TRY(hipMalloc(&scratch.d_src, (size_t)count * sizeof(int64_t)));
        HIP_TRY(createUploadStream(&scratch.stream));
        RC_TRY(uploadOnce(db->device, scratch.d_src, srcStart.data(), (size_t)count * sizeof(int64_t)));
        hipError_t e = launchGatherSequences(parent->d_residues, scratch.d_src, db->d_offsets, count, db->d_residues, scratch.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(scratch.stream);
        if (e != hipSuccess) return fail(MIOPAL_ERR_HIP, "gathering the subset failed: %s", hipGetErrorString(e));
    }
    db->offsets = std::move(offsets);
    *out = db.release();
    return 0;
    });
}

void miopalDbDestroy(MiopalDb* db) { delete db; }

void miopalReleaseCaches(void) {
    std::vector<std::unique_ptr<MiopalDb>> handles;
    {
        SpareHandles& sp = spareHandles();
        std::lock_guard<std::mutex> g(sp.m);
        handles.swap(sp.idle);
    }
    handles.clear();
    std::vector<std::unique_ptr<UploadKit>> kits;
    {
        StagingPool& pool = stagingPool();
        std::lock_guard<std::mutex> g(pool.m);
        kits.swap(pool.free);
        pool.freeStreams.clear();
    }
    kits.clear();
    // (idle workspaces of every live handle)
    std::vector<MiopalDb*> none;
    MiopalDb::liveHandles(nullptr, 0, &none);
}

static int64_t releaseIdleWorkspaces(MiopalDb* db);


void MiopalDb::liveHandles(MiopalDb* db, int what, std::vector<MiopalDb*>* out) {
    // (never destroyed: handles parked in the spare pool are destroyed at exit, after function-local statics of
    // this kind would have been)
    static std::mutex& m = *new std::mutex;
    static std::vector<MiopalDb*>& live = *new std::vector<MiopalDb*>;
    std::lock_guard<std::mutex> g(m);
    if (what > 0) live.push_back(db);
    else if (what < 0) live.erase(std::remove(live.begin(), live.end(), db), live.end());
    else if (out) {
        // (under the lock: a handle cannot be destroyed while its idle workspaces are released)
        for (MiopalDb* h : live) (void)releaseIdleWorkspaces(h);
    }
}

static int64_t releaseIdleWorkspaces(MiopalDb* db) {
    std::vector<std::unique_ptr<Workspace>> idle;
    {
        std::lock_guard<std::mutex> g(db->wsMutex);
        idle.swap(db->ownedFree);
    }
    int64_t bytes = 0;
    for (const auto& w : idle) bytes += (int64_t)w->bytes();
    {
        // (the kernel timings of the last profiled search live in its workspace: miopalLastKernelTime)
        std::lock_guard<std::mutex> g(db->timingMutex);
        for (const auto& w : idle)
            if (db->lastTimed == w.get()) db->lastTimed = nullptr;
    }
    (void)hipSetDevice(db->device);
    idle.clear();   // (workspaces in use by running searches are not in the list: they come back and are kept)
    return bytes;
}

int64_t miopalDbReleaseWorkspaces(MiopalDb* db) {
    if (!db) return 0;
    return releaseIdleWorkspaces(db);
}

int64_t miopalDbCount(const MiopalDb* db) { return db ? db->count : 0; }
int64_t miopalDbTotalLength(const MiopalDb* db) { return db ? db->total : 0; }
int64_t miopalDbDeviceBytes(const MiopalDb* db) {
    if (!db) return 0;
    MiopalDb* m = const_cast<MiopalDb*>(db);
    int64_t t = db->total + 64 + (db->count + 1) * 8;
    {
        std::lock_guard<std::mutex> g(m->viewMutex);
        for (auto& v : m->views) t += v.view ? (int64_t)v.view->deviceBytes : 0;
    }
    return t;
}

void miopalSetProfiling(MiopalDb* db, int enabled) {
    if (db) db->profiling.store(enabled ? 1 : 0);
}

void miopalTestInjectFault(int kind, int unit, int spinCap) {
    g_fault[0] = kind;
    g_fault[1] = unit;
    g_fault[2] = spinCap;
}

int miopalSelfTest(int which) {
    return guarded([&]() -> int {
        if (which == 2) {
            // the operations' way back from two bits each (unpack::, host_workspace.inc): every code path of this CPU -
            // bit by bit, the table, pdep, AVX-512 VBMI, several threads, the crew started beforehand - against the
            // definition, on ranges that start and end anywhere
            const int64_t n = (9 << 20) + 37;
            std::vector<uint8_t> ops((size_t)n), packed((size_t)(n + 3) / 4 + 64, 0), out((size_t)n + 64);
            uint32_t x = 12345;
            for (int64_t p = 0; p < n; ++p) {
                x = x * 1664525u + 1013904223u;
                ops[(size_t)p] = (uint8_t)(x >> 30);
                packed[(size_t)(p >> 2)] |= (uint8_t)(ops[(size_t)p] << (2 * (p & 3)));
            }
            auto same = [&](int64_t from, int64_t to) {
                for (int64_t p = from; p < to; ++p)
                    if (out[(size_t)p] != ops[(size_t)p]) return false;
                return true;
            };
            const int64_t cuts[][2] = {{0, n}, {1, n - 1}, {5, 77}, {63, 64}, {64, 64}, {7, 8 << 20}, {4097, n}, {n - 3, n}};
            for (const auto& c : cuts) {
                std::fill(out.begin(), out.end(), 9);
                unpack::ops(out.data(), packed.data(), c[0], c[1], 8);
                if (!same(c[0], c[1])) return 21;
                if (c[0] > 0 && out[(size_t)c[0] - 1] != 9) return 22;   // (nothing written outside the range)
                if (out[(size_t)c[1]] != 9) return 23;
                std::fill(out.begin(), out.end(), 9);
                unpack::rangePlain(out.data(), packed.data(), c[0], c[1]);
                if (!same(c[0], c[1]) || out[(size_t)c[1]] != 9) return 24;
                std::fill(out.begin(), out.end(), 9);
                {
                    unpack::Crew crew(7);
                    crew.run(out.data(), packed.data(), c[0], c[1]);
                }
                if (!same(c[0], c[1])) return 100 + (int)(&c - &cuts[0]);   // (100 + the range's number: the crew left operations out)
                if (out[(size_t)c[1]] != 9 || (c[0] > 0 && out[(size_t)c[0] - 1] != 9)) return 200 + (int)(&c - &cuts[0]);
            }
            { unpack::Crew unused(3); }   // (a crew that is never run goes away quietly)
            return 0;
        }
        if (which == 3) {
            // the launch layer's once-per-device logic (eight racing first calls, a failing setter, devices without a
            // bit) and its row dispatcher on every range the kernel units use: launch_layer_selftest.h
            return launchLayerSelfTest();
        }
        if (which == 4) {
            // the range model of the host router against literals worked out by hand: score_ranges_selftest.h
            return scoreRangesSelfTest();
        }
        if (which == 5) {
            // the plan of the later passes of a `full` search and of a pair list - routing bits, cost model, slot geometry,
            // traceback batches - against literals worked out from the expressions it replaced: full_plan_selftest.h
            return fullPlanSelfTest();
        }
        if (which == 6) {
            // The column split's host side. Its launch asks for the pair table, the counters behind it and the profile: within
            // the CU's 160 KB for every row count at 24 symbols, and wherever the table alone passes interseqPairFits ...
            for (int rows = 1; rows <= 64; ++rows) {
                const int qPad = (rows + 7) / 8 * 8;
                if (pairSplitLdsBytes(rows, 24, qPad) > kCuLdsBytes) return 1000 + rows;
                for (int nSym = 2; nSym <= kMaxAlphabet + 1; ++nSym)
                    if (interseqPairFits(rows, nSym) && pairSplitLdsBytes(rows, nSym, qPad) > kCuLdsBytes) return 2000 + rows;
            }
            // ... and its plan against the definition, chunk by chunk: interval w = chunks [w C / W, (w + 1) C / W) of the
            // groups' chunk sequence - equal groups, ragged ones, an interval inside one group, one chunk per wavefront
            const std::vector<std::vector<int>> cases = {{75, 75, 75, 75, 75}, {9, 7, 7, 5, 3, 3, 1, 1}, {40}, {3, 2, 1, 1, 5}};
            for (const std::vector<int>& chunks : cases) {
                std::vector<int> groupOfChunk, intoGroup;
                for (size_t g = 0; g < chunks.size(); ++g)
                    for (int c = 0; c < chunks[g]; ++c) {
                        groupOfChunk.push_back((int)g);
                        intoGroup.push_back(c);
                    }
                const int64_t C = (int64_t)groupOfChunk.size();
                for (int W = 1; W <= C; ++W) {
                    const std::vector<int4> plan = splitPlanOf(chunks.data(), (int)chunks.size(), W);
                    if ((int)plan.size() != W + 1) return 3000;
                    for (int w = 0; w <= W; ++w) {
                        const int64_t x = w * (C / W) + w * (C % W) / W;
                        const int4 e = plan[(size_t)w];
                        if (e.z != x || e.w != 0) return 3001;
                        if (x == C ? (e.x != (int)chunks.size() || e.y != 0)
                                   : (e.x != groupOfChunk[(size_t)x] || e.y != intoGroup[(size_t)x])) return 3002;
                        if (w > 0 && e.z <= plan[(size_t)w - 1].z) return 3003;   // (no empty interval)
                    }
                }
            }
            return 0;
        }
        if (which == 7) {
            // the chunk plan of the panel occurrence searches - chunk sizes, groups, row lists and entries - against
            // literals worked out by hand from occurrences_batch.h's rules: occurrence_plan_selftest.h
            return occurrencePlanSelfTest();
        }
        if (which != 1) return -1;
        // (no device call on the way: the handle is never filled, the builders are injected)
        std::unique_ptr<MiopalDb> db(new MiopalDb());
        std::shared_ptr<View> got;
        int calls = 0;
        int rc = getViewWith(db.get(), 0, 10, 0, &got, [&](std::shared_ptr<View>*) -> int {
            ++calls;
            throw std::bad_alloc();
        });
        if (rc != MIOPAL_ERR_INTERNAL) return 1;
        if (calls != 2) return 2;                  // built, views evicted, built once more
        if (!db->views.empty()) return 3;          // no placeholder left behind
        // a thread that waits for the very slice while its builder fails must come back too
        std::atomic<int> stage{0};
        int rcWaiter = -1;
        std::thread first([&] {
            std::shared_ptr<View> v;
            (void)getViewWith(db.get(), 0, 10, 0, &v, [&](std::shared_ptr<View>*) -> int {
                // (called twice: a failed build is retried once after the idle views were dropped)
                int expected = 0;
                stage.compare_exchange_strong(expected, 1);
                for (int spins = 0; stage.load() < 2 && spins < 5000; ++spins)
                    std::this_thread::sleep_for(std::chrono::milliseconds(1));
                std::this_thread::sleep_for(std::chrono::milliseconds(20));   // the waiter is in wait() by now
                throw std::runtime_error("injected");
            });
        });
        for (int spins = 0; stage.load() < 1 && spins < 5000; ++spins) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        std::thread waiter([&] {
            std::shared_ptr<View> v;
            stage.store(2);
            rcWaiter = getViewWith(db.get(), 0, 10, 0, &v, [&](std::shared_ptr<View>* out) -> int {
                out->reset(new View());
                return 0;
            });
        });
        first.join();
        waiter.join();
        if (rcWaiter != 0) return 4;
        if (db->views.size() != 1 || db->views.front().building) return 5;
        db->views.clear();
        return 0;
    });
}

void miopalLastRouting(int64_t counts[4]) {
    if (!counts) return;
    for (int k = 0; k < 4; ++k) counts[k] = g_lastRouting[k];
}

void miopalLastWindowPlan(int64_t out[4]) {
    if (!out) return;
    for (int k = 0; k < 4; ++k) out[k] = g_lastWindowPlan[k];
}

void miopalLastLaunchShape(int64_t out[4]) {
    if (!out) return;
    for (int k = 0; k < 4; ++k) out[k] = g_lastLaunchShape[k];
}

int miopalLastFullRouting(void) { return g_lastFullRouting; }

void miopalLastBatchRouting(int64_t counts[4]) {
    if (!counts) return;
    for (int k = 0; k < 4; ++k) counts[k] = g_lastBatchRouting[k];
}

int miopalLastKernelTime(MiopalDb* db, float* ms) {
    if (!db || !ms) return 0;
    std::lock_guard<std::mutex> g(db->timingMutex);
    *ms = 0.f;
    Workspace* ws = db->lastTimed;
    if (!ws) return 0;
    int n = 0;
    for (auto& ev : ws->timings) {
        float t = 0.f;
        if (hipEventSynchronize(ev.second) == hipSuccess &&
            hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) {
            *ms += t;
            ++n;
        }
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    ws->timings.clear();
    return n;
}

int miopalSearchDeviceScores(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen,
                             int gapExt, const int* scoreMatrix, int alphabetLength, int mode,
                             int64_t start, int64_t end, int* deviceScores, void* stream) {
    return guarded([&]() -> int {
    RC_TRY(validate(db, query, queryLength, scoreMatrix, alphabetLength, OPAL_SEARCH_SCORE, mode, start, end));
    if (end == start) return 0;
    if (!deviceScores) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null device score buffer");
    HIP_TRY(hipSetDevice(db->device));
    WorkspaceLease lease(db);
    RC_TRY(lease.acquireExternal((hipStream_t)stream));
    Search s{db, lease.ws, (hipStream_t)stream, query, queryLength, gapOpen, gapExt, alphabetLength,
             OPAL_SEARCH_SCORE, mode, scoreMatrix, start, end, end - start};
    RC_TRY(s.prepare());
    RC_TRY(s.scorePass((int32_t*)deviceScores, nullptr, nullptr));
    if (s.d_stripError) {
        // Long pairs went through the (pair, strip) units of the int32 kernel, whose units can give up
        // waiting (never seen): the only searches of this entry point that synchronise, so that a
        // partial answer cannot pass for a score.
        RC_TRY(lease.ws->stageDownload(&s.stripErrorHost, s.d_stripError, sizeof(int)));
        RC_TRY(lease.ws->finishDownloads());
        RC_TRY(s.checkStripError());
    }
    return 0;
    });
}

#include "host_full.inc"
#include "host_batch.inc"
#include "host_top.inc"
#include "host_hits.inc"
#include "host_stats.inc"
#include "host_columns.inc"
#include "host_pairs.inc"
#include "host_profile.inc"
#include "host_occurrences.inc"
#include "host_occurrence_align.inc"
#include "host_batch_occurrences.inc"
int miopalSearch(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                 const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                 int64_t end, int* score, int* endTarget, int* endQuery, int* startTarget,
                 int* startQuery, unsigned char** alignment, int* alignmentLength) {
    return guarded([&]() -> int {
    return searchImpl(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType, mode,
                      start, end, score, endTarget, endQuery, startTarget, startQuery, alignment,
                      alignmentLength, nullptr, nullptr);
    });
}

int miopalSearchBatch(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                      int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType, int mode,
                      int64_t start, int64_t end, int* score, int* endTarget, int* endQuery) {
    return guarded([&]() -> int {
    return searchBatchImpl(db, queries, queryOffsets, nQueries, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType,
                           mode, start, end, score, endTarget, endQuery);
    });
}

int miopalSearchTop(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                    const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start, int64_t end,
                    int k, int minScore, int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery) {
    return guarded([&]() -> int {
    return searchTopImpl(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType, mode, start,
                         end, k, minScore, 0, count, targetIndex, score, endTarget, endQuery);
    });
}

int miopalSearchBatchTop(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                         int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                         int mode, int64_t start, int64_t end, int k, int minScore,
                         int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery) {
    return guarded([&]() -> int {
    return searchBatchTopImpl(db, queries, queryOffsets, nQueries, gapOpen, gapExt, scoreMatrix, alphabetLength,
                              searchType, mode, start, end, k, minScore, count, targetIndex, score, endTarget, endQuery);
    });
}

int miopalTestSelectTop(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride, int k,
                        int minScore, int64_t start, int* count, int64_t* targetIndex, int* outScore, int* outEndTarget,
                        int* outEndQuery, int* gaveUp) {
    return guarded([&]() -> int {
    return testSelectTopImpl(score, endTarget, endQuery, rows, stride, k, minScore, start, count, targetIndex, outScore,
                             outEndTarget, outEndQuery, gaveUp);
    });
}

int miopalAlignPairs(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                     const int32_t* pairQuery, const int64_t* pairTarget, int64_t nPairs, int gapOpen, int gapExt,
                     const int* scoreMatrix, int alphabetLength, int searchType, int mode, int* score, int* endTarget,
                     int* endQuery, int* startTarget, int* startQuery, unsigned char** operations,
                     int64_t* operationOffsets) {
    return guarded([&]() -> int {
    HostBytes ops;
    const bool full = searchType == OPAL_SEARCH_ALIGNMENT;
    RC_TRY(alignPairsImpl(db, queries, queryOffsets, nQueries, pairQuery, pairTarget, nPairs, gapOpen, gapExt, scoreMatrix,
                          alphabetLength, searchType, mode, score, endTarget, endQuery, startTarget, startQuery,
                          full && operations ? &ops : nullptr, operationOffsets));
    if (full) {
        *operations = nullptr;
        if (nPairs > 0) {
            if (!ops.data && !ops.resize(0)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
            *operations = ops.release();
        }
    }
    return 0;
    });
}

void miopalLastPairRouting(int64_t counts[4]) {
    if (!counts) return;
    for (int k = 0; k < 4; ++k) counts[k] = g_lastPairRouting[k];
}

int miopalSearchFlat(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                     const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                     int64_t end, int* score, int* endTarget, int* endQuery, int* startTarget,
                     int* startQuery, unsigned char** operations, int64_t* operationOffsets) {
    return guarded([&]() -> int {
    HostBytes ops;
    const bool full = searchType == OPAL_SEARCH_ALIGNMENT;
    if (full && !operations) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null alignment outputs");
    if (operations) *operations = nullptr;
    RC_TRY(searchImpl(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType, mode,
                      start, end, score, endTarget, endQuery, startTarget, startQuery, nullptr, nullptr,
                      full ? &ops : nullptr, full ? operationOffsets : nullptr));
    if (full && end > start) {
        if (!ops.data && !ops.resize(0)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        *operations = ops.release();
    }
    return 0;
    });
}

// What the entry points that take a position-specific scoring matrix share (include/miopal.h). The order of their
// checks is deliberate and part of the header's contract: what needs no handle first (checkBeforeHandle, then the entry
// point's own refusals that need none: the consensus, alignments, k, the outputs, the fit, the cut), then the null
// handle and what depends on the handle (checkHandle) - miopalAlignPairs' order; miopalSearch looks at the handle
// first. The codes are miopalSearch's; only which error is reported when several arguments are bad differs. A caller
// without a device - it cannot hold a handle - is still told what is wrong with its PSSM. None of the checks touches
// a device. (Not validate()'s checks under another name: its messages differ.)
// (no rows: an empty query has no scores; the score source still says "position-specific")
static const int kNoRows[1] = {0};
struct PssmQuery {
    static int checkBeforeHandle(int mode, int searchType, int Q, const int* rowScores, int A) {
        if (mode < OPAL_MODE_NW || mode > OPAL_MODE_SW) return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", mode);
        if (searchType < OPAL_SEARCH_SCORE || searchType > OPAL_SEARCH_ALIGNMENT)
            return fail(OPAL_ERR_INVALID_MODE, "invalid search type %d", searchType);
        if (Q < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad query length %d", Q);
        if (Q > 0 && !rowScores) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null row scores");
        if (A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad alphabet length %d", A);
        return 0;
    }
    static int checkHandle(const MiopalDb* db, int A, int64_t start, int64_t end) {
        if (!db) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null database handle");
        if (A != db->alphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d differs from the database's %d", A, db->alphabet);
        if (start < 0 || end < start || end > db->count) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad slice [%lld, %lld)", (long long)start, (long long)end);
        return 0;
    }
    // what the implementations get where a plain search has its matrix and its query. Without a consensus - score and
    // end searches, every selection - each position is "no residue": the int32 kernels upload it with the rows and
    // never read it.
    PssmQuery(const int* rowScores, const unsigned char* consensus, int Q)
        : rows_(Q > 0 ? rowScores : kNoRows), given(consensus), none(given ? 0 : (size_t)std::max(Q, 1), 255) {}
    const int* rows() const { return rows_; }
    const unsigned char* consensus() const { return given ? given : none.data(); }
    const int* const rows_;
    const unsigned char* const given;
    const std::vector<unsigned char> none;
};

// miopalSearchFlat with a position-specific scoring matrix as the score source
int miopalSearchPssm(MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength,
                     int gapOpen, int gapExt, int alphabetLength, int searchType, int mode,
                     int64_t start, int64_t end, int* score, int* endTarget, int* endQuery,
                     int* startTarget, int* startQuery, unsigned char** operations, int64_t* operationOffsets) {
    return guarded([&]() -> int {
    const int Q = queryLength, A = alphabetLength;
    RC_TRY(PssmQuery::checkBeforeHandle(mode, searchType, Q, rowScores, A));
    const bool full = searchType == OPAL_SEARCH_ALIGNMENT;
    RC_TRY(checkConsensus(consensus, 0, Q, A, full));
    RC_TRY(PssmQuery::checkHandle(db, A, start, end));
    if (full && !operations) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null alignment outputs");
    if (operations) *operations = nullptr;
    if (end == start) return 0;
    RC_TRY(checkPssmRange(db, rowScores, Q, A, gapOpen, gapExt));
    const PssmQuery pssm(rowScores, consensus, Q);
    HostBytes ops;
    RC_TRY(searchImpl(db, pssm.consensus(), Q, gapOpen, gapExt, nullptr, A, searchType, mode, start, end, score, endTarget,
                      endQuery, startTarget, startQuery, nullptr, nullptr, full ? &ops : nullptr,
                      full ? operationOffsets : nullptr, pssm.rows()));
    if (full) {
        if (!ops.data && !ops.resize(0)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        *operations = ops.release();
    }
    return 0;
    });
}

// miopalSearchTop with a position-specific scoring matrix as the score source: the two refusals of the selection that
// need no handle - alignments, k - before the handle; then searchTopImpl with the rows where the matrix stands.
int miopalSearchPssmTop(MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt,
                        int alphabetLength, int searchType, int mode, int64_t start, int64_t end, int k, int minScore,
                        int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery) {
    return guarded([&]() -> int {
    const int Q = queryLength, A = alphabetLength;
    RC_TRY(PssmQuery::checkBeforeHandle(mode, searchType, Q, rowScores, A));
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchPssmTop: alignments are not selected on the device");
    if (k < 0 || k > MIOPAL_MAX_TOP) return fail(MIOPAL_ERR_BAD_ARGUMENT, "k = %d outside [0, %d]", k, MIOPAL_MAX_TOP);
    RC_TRY(PssmQuery::checkHandle(db, A, start, end));
    const PssmQuery pssm(rowScores, nullptr, Q);
    return searchTopImpl(db, pssm.consensus(), Q, gapOpen, gapExt, nullptr, A, searchType, mode, start, end, k, minScore, 0,
                         count, targetIndex, score, endTarget, endQuery, pssm.rows());
    });
}

// miopalSearchHits: miopalSearchTop's checks in its order (the handle, the query and the matrix, the slice; alignments;
// the outputs), then the score pass and the compaction
int miopalSearchHits(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                     const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start, int64_t end,
                     int minScore, int64_t maxHits, int64_t* count, int64_t** targetIndex, int** score, int** endTarget,
                     int** endQuery) {
    return guarded([&]() -> int {
    RC_TRY(validate(db, query, queryLength, scoreMatrix, alphabetLength, searchType, mode, start, end));
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchHits: alignments are not selected on the device");
    RC_TRY(checkHitsOutputs(searchType, count, targetIndex, score, endTarget, endQuery));
    HitRows rows;
    RC_TRY(searchHitsImpl(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType, mode, start, end,
                          minScore, maxHits, &rows));
    return finishHits(rows, searchType, maxHits, count, targetIndex, score, endTarget, endQuery);
    });
}

// miopalSearchPssmHits: miopalSearchPssmTop's checks in its order - what needs no handle first, the refusal of
// alignments and the outputs (where the top form checks k) among it - then searchHitsImpl with the rows where the
// matrix stands
int miopalSearchPssmHits(MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt, int alphabetLength,
                         int searchType, int mode, int64_t start, int64_t end, int minScore, int64_t maxHits,
                         int64_t* count, int64_t** targetIndex, int** score, int** endTarget, int** endQuery) {
    return guarded([&]() -> int {
    const int Q = queryLength, A = alphabetLength;
    RC_TRY(PssmQuery::checkBeforeHandle(mode, searchType, Q, rowScores, A));
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchPssmHits: alignments are not selected on the device");
    RC_TRY(checkHitsOutputs(searchType, count, targetIndex, score, endTarget, endQuery));
    RC_TRY(PssmQuery::checkHandle(db, A, start, end));
    const PssmQuery pssm(rowScores, nullptr, Q);
    HitRows rows;
    RC_TRY(searchHitsImpl(db, pssm.consensus(), Q, gapOpen, gapExt, nullptr, A, searchType, mode, start, end, minScore,
                          maxHits, &rows, pssm.rows()));
    return finishHits(rows, searchType, maxHits, count, targetIndex, score, endTarget, endQuery);
    });
}

// miopalSearchOccurrences: miopalSearchHits' checks in its order - miopalSearch's (the handle first), then, where that
// function refuses alignments, the mode, the window and the SW cut, then the outputs - and the two sweeps
// (host_occurrences.inc)
int miopalSearchOccurrences(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                            const int* scoreMatrix, int alphabetLength, int mode, int64_t start, int64_t end, int minScore,
                            int window, int64_t maxHits, int64_t* count, int64_t** targetIndex, int** score,
                            int** endTarget, int** endQuery) {
    return guarded([&]() -> int {
    const OccurrenceOutputs out{count, targetIndex, score, endTarget, endQuery};
    RC_TRY(validate(db, query, queryLength, scoreMatrix, alphabetLength, OPAL_SEARCH_SCORE_END, mode, start, end));
    RC_TRY(checkOccurrenceRule(mode, 1, &minScore, &window, nullptr));
    RC_TRY(out.check());
    return searchOccurrencesCall(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits},
                                 OccurrenceQuery{query, queryLength, scoreMatrix, nullptr, minScore, window}, out);
    });
}

// miopalSearchOccurrencesAligned: miopalSearchOccurrences' checks in its order, the new null outputs with the others;
// the sweeps, and behind them the later passes of a `full` pair list on the occurrences (host_occurrence_align.inc)
int miopalSearchOccurrencesAligned(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                                   const int* scoreMatrix, int alphabetLength, int mode, int64_t start, int64_t end,
                                   int minScore, int window, int64_t maxHits, int64_t* count, int64_t** targetIndex,
                                   int** score, int** endTarget, int** endQuery, int** startTarget, int** startQuery,
                                   unsigned char** alignments, int64_t** alignmentOffsets) {
    return guarded([&]() -> int {
    const OccurrenceOutputs out{count, targetIndex, score, endTarget, endQuery, true, startTarget, startQuery, alignments, alignmentOffsets};
    RC_TRY(validate(db, query, queryLength, scoreMatrix, alphabetLength, OPAL_SEARCH_SCORE_END, mode, start, end));
    RC_TRY(checkOccurrenceRule(mode, 1, &minScore, &window, nullptr));
    RC_TRY(out.check());
    return searchOccurrencesCall(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits},
                                 OccurrenceQuery{query, queryLength, scoreMatrix, nullptr, minScore, window}, out);
    });
}

// miopalSearchPssmOccurrences(Aligned): miopalSearchPssmHits' checks in its order - what needs no handle first, the
// occurrence rule where that function refuses alignments, the outputs, in the aligned form the consensus as
// miopalAlignPairsPssm requires it, and the PSSM's height among it - then the same
static int searchPssmOccurrencesEntry(const OccurrenceRequest& rq, const int* rowScores, const unsigned char* consensus, int Q,
                                      int minScore, int window, const OccurrenceOutputs& out) {
    RC_TRY(PssmQuery::checkBeforeHandle(rq.mode, OPAL_SEARCH_SCORE_END, Q, rowScores, rq.A));
    RC_TRY(checkOccurrenceRule(rq.mode, 1, &minScore, &window, nullptr));
    RC_TRY(out.check());
    if (out.aligned) RC_TRY(checkConsensus(consensus, 0, Q, rq.A, out.alignments != nullptr));
    RC_TRY(checkOccurrenceTableFits(Q, rq.A));
    RC_TRY(PssmQuery::checkHandle(rq.db, rq.A, rq.start, rq.end));
    if (rq.end > rq.start) RC_TRY(checkPssmRange(rq.db, rowScores, Q, rq.A, rq.open, rq.ext));
    const PssmQuery pssm(rowScores, out.aligned ? consensus : nullptr, Q);
    return searchOccurrencesCall(rq, OccurrenceQuery{pssm.consensus(), Q, nullptr, pssm.rows(), minScore, window}, out);
}

int miopalSearchPssmOccurrences(MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt,
                                int alphabetLength, int mode, int64_t start, int64_t end, int minScore, int window,
                                int64_t maxHits, int64_t* count, int64_t** targetIndex, int** score, int** endTarget,
                                int** endQuery) {
    return guarded([&]() -> int {
    return searchPssmOccurrencesEntry(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits}, rowScores,
                                      nullptr, queryLength, minScore, window,
                                      OccurrenceOutputs{count, targetIndex, score, endTarget, endQuery});
    });
}

int miopalSearchPssmOccurrencesAligned(MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength,
                                       int gapOpen, int gapExt, int alphabetLength, int mode, int64_t start, int64_t end,
                                       int minScore, int window, int64_t maxHits, int64_t* count, int64_t** targetIndex,
                                       int** score, int** endTarget, int** endQuery, int** startTarget, int** startQuery,
                                       unsigned char** alignments, int64_t** alignmentOffsets) {
    return guarded([&]() -> int {
    return searchPssmOccurrencesEntry(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits}, rowScores,
                                      consensus, queryLength, minScore, window,
                                      OccurrenceOutputs{count, targetIndex, score, endTarget, endQuery, true, startTarget, startQuery,
                                                        alignments, alignmentOffsets});
    });
}

// miopalSearchBatchOccurrences(Aligned): miopalSearchOccurrences' checks for every query of the list, in its order,
// before any device work, the aligned form's null outputs behind its own; then the panel kernels - in the aligned form
// with the alignment stage behind every write sweep (host_batch_occurrence_align.inc) - and, for queries of more than
// 64 rows, the single-query search (host_batch_occurrences.inc)
int miopalSearchBatchOccurrences(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                                 int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int mode,
                                 int64_t start, int64_t end, const int* minScore, const int* window, int64_t maxHits,
                                 int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget, int** endQuery) {
    return guarded([&]() -> int {
    return searchBatchOccurrencesImpl(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits},
                                      PanelSide{queries, queryOffsets, nQueries, scoreMatrix, nullptr, minScore, window},
                                      OccurrenceOutputs{hitOffsets, targetIndex, score, endTarget, endQuery});
    });
}

int miopalSearchBatchOccurrencesAligned(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets,
                                        int nQueries, int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength,
                                        int mode, int64_t start, int64_t end, const int* minScore, const int* window,
                                        int64_t maxHits, int64_t* hitOffsets, int64_t** targetIndex, int** score,
                                        int** endTarget, int** endQuery, int** startTarget, int** startQuery,
                                        unsigned char** alignments, int64_t** alignmentOffsets) {
    return guarded([&]() -> int {
    return searchBatchOccurrencesImpl(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits},
                                      PanelSide{queries, queryOffsets, nQueries, scoreMatrix, nullptr, minScore, window},
                                      OccurrenceOutputs{hitOffsets, targetIndex, score, endTarget, endQuery, true, startTarget,
                                                        startQuery, alignments, alignmentOffsets});
    });
}

// miopalSearchPssmBatchOccurrences, miopalSearchPssmBatchOccurrencesAligned: the panel calls with a list of PSSMs, passed
// as miopalAlignPairsPssm takes it (host_batch_occurrences.inc: searchPssmBatchOccurrencesImpl, its checks and their order)
int miopalSearchPssmBatchOccurrences(MiopalDb* db, const int* rowScores, const int64_t* rowOffsets, int nPssms, int gapOpen,
                                     int gapExt, int alphabetLength, int mode, int64_t start, int64_t end,
                                     const int* minScore, const int* window, int64_t maxHits, int64_t* hitOffsets,
                                     int64_t** targetIndex, int** score, int** endTarget, int** endQuery) {
    return guarded([&]() -> int {
    return searchPssmBatchOccurrencesImpl(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits},
                                          PanelSide{nullptr, rowOffsets, nPssms, nullptr, rowScores, minScore, window},
                                          OccurrenceOutputs{hitOffsets, targetIndex, score, endTarget, endQuery});
    });
}

int miopalSearchPssmBatchOccurrencesAligned(MiopalDb* db, const int* rowScores, const unsigned char* consensus,
                                            const int64_t* rowOffsets, int nPssms, int gapOpen, int gapExt,
                                            int alphabetLength, int mode, int64_t start, int64_t end, const int* minScore,
                                            const int* window, int64_t maxHits, int64_t* hitOffsets, int64_t** targetIndex,
                                            int** score, int** endTarget, int** endQuery, int** startTarget,
                                            int** startQuery, unsigned char** alignments, int64_t** alignmentOffsets) {
    return guarded([&]() -> int {
    return searchPssmBatchOccurrencesImpl(OccurrenceRequest{db, gapOpen, gapExt, alphabetLength, mode, start, end, maxHits},
                                          PanelSide{consensus, rowOffsets, nPssms, nullptr, rowScores, minScore, window},
                                          OccurrenceOutputs{hitOffsets, targetIndex, score, endTarget, endQuery, true, startTarget,
                                                            startQuery, alignments, alignmentOffsets});
    });
}

// what the family's reporters say: the thread's last single-query call, its last aligned one, its last panel call
static void copyFigures(int64_t* to, const int64_t* from, int n) {
    if (!to) return;
    for (int k = 0; k < n; ++k) to[k] = from[k];
}
void miopalLastOccurrenceRouting(int64_t counts[4]) { copyFigures(counts, g_lastOccurrenceRouting, 4); }
void miopalLastOccurrenceAlignRouting(int64_t counts[4]) { copyFigures(counts, g_lastOccurrenceAlignRouting, 4); }
void miopalLastBatchOccurrenceRouting(int64_t counts[4]) { copyFigures(counts, g_lastBatchOccurrenceRouting, 4); }
void miopalLastBatchOccurrenceGroups(int64_t counts[3]) { copyFigures(counts, g_lastBatchOccurrenceGroups, 3); }
void miopalLastBatchOccurrenceAlignRouting(int64_t counts[4]) { copyFigures(counts, g_lastBatchOccurrenceAlignRouting, 4); }

int miopalTestPickOccurrences(const int* value, const int* valueRow, int rows, int64_t stride, const int32_t* length,
                              int minScore, int window, int64_t* hitOffsets, int32_t** column, int** score, int** row) {
    return guarded([&]() -> int {
    return testPickOccurrencesImpl(value, valueRow, rows, stride, length, minScore, window, hitOffsets, column, score, row);
    });
}

int miopalSearchBatchHits(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                          int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType, int mode,
                          int64_t start, int64_t end, const int* minScore, int64_t maxHits, int64_t* hitOffsets,
                          int64_t** targetIndex, int** score, int** endTarget, int** endQuery) {
    return guarded([&]() -> int {
    return searchBatchHitsImpl(db, queries, queryOffsets, nQueries, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType,
                               mode, start, end, minScore, maxHits, hitOffsets, targetIndex, score, endTarget, endQuery);
    });
}

int miopalTestSelectHits(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride,
                         const int* minScore, int64_t start, int64_t* hitOffsets, int64_t** targetIndex, int** outScore,
                         int** outEndTarget, int** outEndQuery) {
    return guarded([&]() -> int {
    return testSelectHitsImpl(score, endTarget, endQuery, rows, stride, minScore, start, hitOffsets, targetIndex, outScore,
                              outEndTarget, outEndQuery);
    });
}

// miopalSearchSignificant: miopalSearchHits' checks in its order, then the fit and E-value outputs and the cut, then the
// score pass, the statistics, the fit and the binned compaction (host_stats.inc)
int miopalSearchSignificant(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                            const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                            int64_t end, double maxEvalue, double excludeZ, int64_t maxHits, MiopalScoreFit* fit,
                            int64_t* count, int64_t** targetIndex, int** score, int** endTarget, int** endQuery,
                            double** evalue) {
    return guarded([&]() -> int {
    RC_TRY(validate(db, query, queryLength, scoreMatrix, alphabetLength, searchType, mode, start, end));
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchSignificant: alignments are not selected on the device");
    RC_TRY(checkHitsOutputs(searchType, count, targetIndex, score, endTarget, endQuery));
    RC_TRY(checkSignificantArgs(fit, evalue));
    RC_TRY(checkEvalueCut(maxEvalue, excludeZ));
    HitRows rows;
    std::vector<double> ev;
    SliceLengths lengths;
    RC_TRY(searchSignificantImpl(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType, mode, start,
                                 end, maxEvalue, excludeZ, maxHits, &lengths, fit, &rows, &ev));
    return finishSignificant(rows, ev, searchType, maxHits, count, targetIndex, score, endTarget, endQuery, evalue);
    });
}

// miopalSearchPssmSignificant: miopalSearchPssmHits' checks in its order - the fit and E-value outputs and the cut among
// what needs no handle - then searchSignificantImpl with the rows where the matrix stands
int miopalSearchPssmSignificant(MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt,
                                int alphabetLength, int searchType, int mode, int64_t start, int64_t end, double maxEvalue,
                                double excludeZ, int64_t maxHits, MiopalScoreFit* fit, int64_t* count,
                                int64_t** targetIndex, int** score, int** endTarget, int** endQuery, double** evalue) {
    return guarded([&]() -> int {
    const int Q = queryLength, A = alphabetLength;
    RC_TRY(PssmQuery::checkBeforeHandle(mode, searchType, Q, rowScores, A));
    if (searchType == OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "miopalSearchPssmSignificant: alignments are not selected on the device");
    RC_TRY(checkHitsOutputs(searchType, count, targetIndex, score, endTarget, endQuery));
    RC_TRY(checkSignificantArgs(fit, evalue));
    RC_TRY(checkEvalueCut(maxEvalue, excludeZ));
    RC_TRY(PssmQuery::checkHandle(db, A, start, end));
    const PssmQuery pssm(rowScores, nullptr, Q);
    HitRows rows;
    std::vector<double> ev;
    SliceLengths lengths;
    RC_TRY(searchSignificantImpl(db, pssm.consensus(), Q, gapOpen, gapExt, nullptr, A, searchType, mode, start, end, maxEvalue,
                                 excludeZ, maxHits, &lengths, fit, &rows, &ev, pssm.rows()));
    return finishSignificant(rows, ev, searchType, maxHits, count, targetIndex, score, endTarget, endQuery, evalue);
    });
}

int miopalSearchBatchSignificant(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                                 int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                                 int mode, int64_t start, int64_t end, const double* maxEvalue, double excludeZ,
                                 int64_t maxHits, MiopalScoreFit* fits, int64_t* hitOffsets, int64_t** targetIndex,
                                 int** score, int** endTarget, int** endQuery, double** evalue) {
    return guarded([&]() -> int {
    return searchBatchSignificantImpl(db, queries, queryOffsets, nQueries, gapOpen, gapExt, scoreMatrix, alphabetLength,
                                      searchType, mode, start, end, maxEvalue, excludeZ, maxHits, fits, hitOffsets,
                                      targetIndex, score, endTarget, endQuery, evalue);
    });
}

int miopalTestRowStats(const int* score, int rows, int64_t stride, const int32_t* length, const int32_t* ceiling,
                       const int* skip, int64_t* stats, unsigned char* bin) {
    return guarded([&]() -> int { return testRowStatsImpl(score, rows, stride, length, ceiling, skip, stats, bin); });
}

int miopalTestSelectHitsBinned(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride,
                               const int32_t* length, const int32_t* threshold, int64_t start, int64_t* hitOffsets,
                               int64_t** targetIndex, int** outScore, int** outEndTarget, int** outEndQuery) {
    return guarded([&]() -> int {
    return testSelectHitsImpl(score, endTarget, endQuery, rows, stride, nullptr, start, hitOffsets, targetIndex, outScore,
                              outEndTarget, outEndQuery, true, length, threshold);
    });
}

int miopalSearchBatchTargetTop(MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,
                               int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType,
                               int mode, int64_t start, int64_t end, int m, int minScore,
                               int* count, int32_t* queryIndex, int* score, int* endTarget, int* endQuery) {
    return guarded([&]() -> int {
    return searchBatchTargetTopImpl(db, queries, queryOffsets, nQueries, gapOpen, gapExt, scoreMatrix, alphabetLength,
                                    searchType, mode, start, end, m, minScore, count, queryIndex, score, endTarget, endQuery);
    });
}

int miopalTestSelectColumns(const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride,
                            const int32_t* pieceFirst, const int32_t* pieceCount, int pieces,
                            const unsigned char* skip, int m, int minScore,
                            int* count, int32_t* queryIndex, int* outScore, int* outEndTarget, int* outEndQuery) {
    return guarded([&]() -> int {
    return testSelectColumnsImpl(score, endTarget, endQuery, rows, stride, pieceFirst, pieceCount, pieces, skip, m, minScore,
                                 count, queryIndex, outScore, outEndTarget, outEndQuery);
    });
}

// miopalAlignPairs with a list of position-specific scoring matrices as the score source: what needs no handle is
// checked here, in miopalSearchPssm's order, then alignPairsImpl with the rows where the matrix stands, the
// consensus where the queries stand and the row offsets where the query offsets stand.
// (Its own checks, not PssmQuery's: the list's checks sit between the search type and the rows, the rows are counted
// over the whole list, the filler consensus is indexed in the offsets' coordinates, and alignPairsImpl makes the
// handle's checks with the pair list's. Only kNoRows is shared.)
int miopalAlignPairsPssm(MiopalDb* db, const int* rowScores, const unsigned char* consensus, const int64_t* rowOffsets,
                         int nPssms, const int32_t* pairPssm, const int64_t* pairTarget, int64_t nPairs, int gapOpen,
                         int gapExt, int alphabetLength, int searchType, int mode, int* score, int* endTarget,
                         int* endQuery, int* startTarget, int* startQuery, unsigned char** operations,
                         int64_t* operationOffsets) {
    return guarded([&]() -> int {
    const int A = alphabetLength;
    if (mode < OPAL_MODE_NW || mode > OPAL_MODE_SW) return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", mode);
    if (searchType < OPAL_SEARCH_SCORE || searchType > OPAL_SEARCH_ALIGNMENT)
        return fail(OPAL_ERR_INVALID_MODE, "invalid search type %d", searchType);
    if (nPssms < 0 || (nPssms > 0 && !rowOffsets)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad PSSM list");
    for (int m = 0; m < nPssms; ++m)
        if (rowOffsets[m] < 0 || rowOffsets[m + 1] < rowOffsets[m])
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad row offsets at %d", m);
    const int64_t first = nPssms > 0 ? rowOffsets[0] : 0, totalRows = nPssms > 0 ? rowOffsets[nPssms] - first : 0;
    if (totalRows > INT32_MAX - 64) return fail(MIOPAL_ERR_BAD_ARGUMENT, "the PSSMs of a pair list hold 2^31 - 65 rows at most");
    if (totalRows > 0 && !rowScores) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null row scores");
    if (A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad alphabet length %d", A);
    const bool full = searchType == OPAL_SEARCH_ALIGNMENT;
    RC_TRY(checkConsensus(consensus, first, totalRows, A, full));
    // (without a consensus - score and end lists - every position is "no residue": the kernels never read it)
    std::vector<unsigned char> none;
    if (!consensus) {
        none.assign((size_t)(first + std::max<int64_t>(totalRows, 1)), 255);   // (indexed in the offsets' coordinates)
        consensus = none.data();
    }
    HostBytes ops;
    RC_TRY(alignPairsImpl(db, consensus, rowOffsets, nPssms, pairPssm, pairTarget, nPairs, gapOpen, gapExt, nullptr, A,
                          searchType, mode, score, endTarget, endQuery, startTarget, startQuery,
                          full && operations ? &ops : nullptr, operationOffsets,
                          totalRows > 0 ? rowScores + (size_t)first * A : kNoRows));
    if (full) {
        *operations = nullptr;
        if (nPairs > 0) {
            if (!ops.data && !ops.resize(0)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
            *operations = ops.release();
        }
    }
    return 0;
    });
}

// miopalProfileColumns: miopalAlignPairs' checks in its order for the list (query, targets[p]), then the outputs and
// the size of the multiple alignment, then the pair list with the projection in the place of gather + download and the
// column kernels (host_profile.inc)
int miopalProfileColumns(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                         const int* scoreMatrix, int alphabetLength, int mode, const int64_t* targets, int64_t nTargets,
                         int64_t* counts, int64_t* weighted, int64_t* memberWeight, unsigned char* msa) {
    return guarded([&]() -> int {
    return profileColumnsImpl(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, mode, targets, nTargets,
                              counts, weighted, memberWeight, msa, nullptr);
    });
}

// ... with a position-specific scoring matrix: what needs no handle is checked here, in miopalAlignPairsPssm's order
// (one PSSM of queryLength rows; an alignment search, so the consensus is required), then the same.
// (Its own checks, not PssmQuery's: no search type, and the cap on the rows sits between the length and the rows;
// profileColumnsImpl's pair list makes the handle's checks. Only kNoRows is shared.)
int miopalProfileColumnsPssm(MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength,
                             int gapOpen, int gapExt, int alphabetLength, int mode, const int64_t* targets,
                             int64_t nTargets, int64_t* counts, int64_t* weighted, int64_t* memberWeight,
                             unsigned char* msa) {
    return guarded([&]() -> int {
    const int Q = queryLength, A = alphabetLength;
    if (mode < OPAL_MODE_NW || mode > OPAL_MODE_SW) return fail(OPAL_ERR_INVALID_MODE, "invalid alignment mode %d", mode);
    if (Q < 0) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad query length %d", Q);
    if (Q > INT32_MAX - 64) return fail(MIOPAL_ERR_BAD_ARGUMENT, "a PSSM holds 2^31 - 65 rows at most");
    if (Q > 0 && !rowScores) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null row scores");
    if (A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad alphabet length %d", A);
    RC_TRY(checkConsensus(consensus, 0, Q, A, true));
    return profileColumnsImpl(db, consensus, Q, gapOpen, gapExt, nullptr, A, mode, targets, nTargets, counts, weighted,
                              memberWeight, msa, Q > 0 ? rowScores : kNoRows);
    });
}

int miopalTestProfileColumns(const unsigned char* msa, int64_t members, int queryLength, int alphabetLength,
                             int64_t* counts, int64_t* weighted, int64_t* memberWeight) {
    return guarded([&]() -> int {
    return testProfileColumnsImpl(msa, members, queryLength, alphabetLength, counts, weighted, memberWeight);
    });
}

int miopalSearchFlatInto(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt,
                         const int* scoreMatrix, int alphabetLength, int searchType, int mode, int64_t start,
                         int64_t end, int* score, int* endTarget, int* endQuery, int* startTarget,
                         int* startQuery, unsigned char** operations, int64_t* operationsCapacity,
                         int64_t* operationOffsets) {
    return guarded([&]() -> int {
    HostBytes ops;
    const bool full = searchType == OPAL_SEARCH_ALIGNMENT;
    if (full && (!operations || !operationsCapacity)) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null alignment outputs");
    if (full && *operations && *operationsCapacity > 0) ops.lend(*operations, (size_t)*operationsCapacity);
    RC_TRY(searchImpl(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType, mode,
                      start, end, score, endTarget, endQuery, startTarget, startQuery, nullptr, nullptr,
                      full ? &ops : nullptr, full ? operationOffsets : nullptr));
    if (full && end > start) {
        if (!ops.data && !ops.resize(0)) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
        size_t capacity = 0;
        *operations = ops.release(&capacity);
        *operationsCapacity = (int64_t)capacity;
    }
    return 0;
    });
}

int miopalSearchResults(MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen,
                        int gapExt, const int* scoreMatrix, int alphabetLength,
                        OpalSearchResult* results[], int searchType, int mode, int overflowMethod,
                        int64_t start, int64_t end) {
    return guarded([&]() -> int {
    (void)overflowMethod;
    if (!db) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null database handle");
    if (end > db->count) end = db->count;
    const int64_t n = end - start;
    if (n <= 0) return n < 0 ? fail(MIOPAL_ERR_BAD_ARGUMENT, "bad slice") : 0;
    if (!results) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null results");
    // (not a vector: a million zeros written first cost as much as the copy that overwrites them)
    std::unique_ptr<int[]> scoreOwner(new int[(size_t)n]);
    int* const score = scoreOwner.get();
    std::vector<int> et, eq, st, sq, alen;
    std::vector<unsigned char*> aln;
    if (searchType >= OPAL_SEARCH_SCORE_END) { et.resize((size_t)n); eq.resize((size_t)n); }
    if (searchType == OPAL_SEARCH_ALIGNMENT) { st.resize((size_t)n); sq.resize((size_t)n); alen.resize((size_t)n); aln.resize((size_t)n, nullptr); }
    int rc = miopalSearch(db, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, searchType,
                          mode, start, end, score, et.empty() ? nullptr : et.data(),
                          eq.empty() ? nullptr : eq.data(), st.empty() ? nullptr : st.data(),
                          sq.empty() ? nullptr : sq.data(), aln.empty() ? nullptr : aln.data(),
                          alen.empty() ? nullptr : alen.data());
    if (rc) {
        for (auto p : aln) free(p);
        return rc;
    }
    PhaseTimer pt;
    // (a million scattered 40-byte records behind a million pointers: memory latency, more threads help)
    const int nSlices = hostThreads((size_t)n, 65536, 8);
    parallelSlices(nSlices, [&](int t) {
        for (int64_t k = n * t / nSlices; k < n * (t + 1) / nSlices; ++k) {
            OpalSearchResult* r = results[k];
            r->scoreSet = 1;
            r->score = score[(size_t)k];
            if (searchType >= OPAL_SEARCH_SCORE_END) {
                r->endLocationTarget = et[(size_t)k];
                r->endLocationQuery = eq[(size_t)k];
            }
            if (searchType == OPAL_SEARCH_ALIGNMENT) {
                r->startLocationTarget = st[(size_t)k];
                r->startLocationQuery = sq[(size_t)k];
                r->alignment = alen[(size_t)k] > 0 ? aln[(size_t)k] : nullptr;
                if (alen[(size_t)k] == 0) free(aln[(size_t)k]);
                r->alignmentLength = alen[(size_t)k];
            }
        }
    });
    pt.mark("result structs");
    return 0;
    });
}

// ---- opal.h ---------------------------------------------------------------
void opalInitSearchResult(OpalSearchResult* r) {
    r->scoreSet = 0;
    r->score = 0;
    r->endLocationTarget = r->endLocationQuery = -1;
    r->startLocationTarget = r->startLocationQuery = -1;
    r->alignment = nullptr;
    r->alignmentLength = 0;
}

int opalSearchResultIsEmpty(const OpalSearchResult r) { return !r.scoreSet; }

void opalSearchResultSetScore(OpalSearchResult* r, int score) {
    r->scoreSet = 1;
    r->score = score;
}

int opalSearchDatabase(unsigned char query[], int queryLength, unsigned char* db[], int dbLength,
                       int dbSeqLengths[], int gapOpen, int gapExt, int* scoreMatrix,
                       int alphabetLength, OpalSearchResult* results[], const int searchType, int mode,
                       int overflowMethod) {
    return guarded([&]() -> int {
    if (dbLength <= 0) return 0;
    int device = 0;
    if (const char* env = tuned(Tune::DEVICE)) device = atoi(env);
    const bool verbose = tuned(Tune::VERBOSE) != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    if (!db || !dbSeqLengths) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad arguments to opalSearchDatabase");
    if (alphabetLength <= 0 || alphabetLength > kMaxAlphabet)
        return fail(MIOPAL_ERR_BAD_ARGUMENT, "alphabet length %d not in 1..32", alphabetLength);
    // offsets = prefix sums of the lengths, in slices worked on side by side (a million targets: 12 MB read)
    std::vector<int64_t> offsets((size_t)dbLength + 1);
    {
        const int nSlices = hostThreads((size_t)dbLength, 65536);
        std::vector<int64_t> sliceSum((size_t)nSlices + 1, 0);
        std::vector<int> sliceBad((size_t)nSlices, 0);
        auto lo = [&](int t) { return (int)((int64_t)dbLength * t / nSlices); };
        parallelSlices(nSlices, [&](int t) {
            int64_t sum = 0;
            for (int k = lo(t); k < lo(t + 1); ++k) {
                if (dbSeqLengths[k] < 0) { sliceBad[(size_t)t] = 1; return; }
                if (dbSeqLengths[k] > 0 && !db[k]) { sliceBad[(size_t)t] = 2; return; }
                sum += dbSeqLengths[k];
            }
            sliceSum[(size_t)t + 1] = sum;
        });
        for (int t = 0; t < nSlices; ++t) {
            if (sliceBad[(size_t)t] == 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "negative sequence length");
            if (sliceBad[(size_t)t] == 2) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null sequence in the database");
            sliceSum[(size_t)t + 1] += sliceSum[(size_t)t];
        }
        parallelSlices(nSlices, [&](int t) {
            int64_t at = sliceSum[(size_t)t];
            for (int k = lo(t); k < lo(t + 1); ++k) {
                offsets[(size_t)k] = at;
                at += dbSeqLengths[k];
            }
        });
        offsets[(size_t)dbLength] = sliceSum[(size_t)nSlices];
    }
    // a handle of an earlier call, or a new one
    std::unique_ptr<MiopalDb> h;
    {
        SpareHandles& sp = spareHandles();
        std::lock_guard<std::mutex> g(sp.m);
        for (size_t k = sp.idle.size(); k-- > 0;)
            if (sp.idle[k]->device == device) {
                h = std::move(sp.idle[k]);
                sp.idle.erase(sp.idle.begin() + (long)k);
                break;
            }
    }
    if (!h) RC_TRY(newHandle(&h, device));
    ResidueSource src;
    src.sequences = (const unsigned char* const*)db;
    // Round 4, opt-in (MIOPAL_SEARCH_UNDER_UPLOAD=1): the search UNDER the upload. The lengths are all a packed
    // view's lists need, so the database is cut into a few contiguous segments (by residues: 30 / 30 / 25 / 15 %,
    // the last one short); a segment is packed and searched, and its result structs are written, as soon as its
    // residues are on the device, while the later segments still cross PCIe. Measured (1M x 300, profiles/
    // r04_search_under_upload.txt): 10.3-10.4 ms per call against 10.5-10.6 with the search behind the upload on one
    // box, 11.2-11.9 against 11.2-12.2 on another - the host-to-device copies slow down beside the search kernels by
    // what the overlap saves (upload 7.3 -> 9.2 ms), whatever the number of host threads or CUs left free. Not the
    // default for that reason; kept, with its test, because the arithmetic is right for a host whose copies do not
    // share the device with the kernels. Large databases of short targets only (those whose view lists are built
    // ahead: fillHandle); targets are independent, so the results are those of one search of the whole database
    // (src/pyopal/_align.py:150-170 cuts the same way over its threads).
    int64_t longest = 0;
    if (tuned(Tune::SEARCH_UNDER_UPLOAD)) {
        const int nSlices = hostThreads((size_t)dbLength, 65536);
        std::vector<int> sliceMax((size_t)nSlices, 0);
        parallelSlices(nSlices, [&](int t) {
            int m = 0;
            for (int k = (int)((int64_t)dbLength * t / nSlices); k < (int)((int64_t)dbLength * (t + 1) / nSlices); ++k) m = std::max(m, dbSeqLengths[k]);
            sliceMax[(size_t)t] = m;
        });
        for (int m : sliceMax) longest = std::max<int64_t>(longest, m);
    }
    const int64_t totalResidues = offsets[(size_t)dbLength];
    const bool under = tuned(Tune::SEARCH_UNDER_UPLOAD) && dbLength >= 262144 && totalResidues >= (96ll << 20) &&
                       longest <= 256 + 128 && queryLength > 0 && !tuned(Tune::NO_VIEW_PREFETCH);
    int rc = 0;
    auto t1 = t0;
    if (under) {
        std::vector<int64_t> bounds{0};
        for (double share : {0.30, 0.60, 0.85}) {
            const int64_t goal = (int64_t)(share * (double)totalResidues);
            int64_t k = std::upper_bound(offsets.begin(), offsets.end(), goal) - offsets.begin() - 1;
            k = std::min<int64_t>(std::max<int64_t>(k, bounds.back()), dbLength);
            if (k > bounds.back()) bounds.push_back(k);
        }
        if (bounds.back() < dbLength) bounds.push_back(dbLength);
        std::vector<int64_t> segEndByte;
        for (size_t k = 1; k < bounds.size(); ++k) segEndByte.push_back(offsets[(size_t)bounds[k]]);
        UploadProgress progress;
        bool ready = false;
        int fillRc = 0;
        std::string fillError;
        MiopalDb* const hd = h.get();
        std::thread filler([&, hd] {
            // (errors are per thread: this one's message is handed to the caller's)
            fillRc = guarded([&] { return fillHandle(hd, src, std::move(offsets), dbLength, alphabetLength, true, &bounds, &progress, &ready); });
            if (fillRc) fillError = g_lastError;
            progress.finish();
        });
        struct Join {
            std::thread& t;
            ~Join() { if (t.joinable()) t.join(); }
        } joinFiller{filler};
        {
            std::unique_lock<std::mutex> g(progress.m);
            progress.cv.wait(g, [&] { return ready || progress.finished; });
        }
        for (size_t k = 0; k + 1 < bounds.size() && rc == 0; ++k) {
            if (!progress.waitFor((size_t)segEndByte[k])) break;   // (the upload ended early: its error is reported below)
            if (k == 0) (void)hipSetDevice(h->device);
            rc = miopalSearchResults(hd, query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength,
                                     results + bounds[k], searchType, mode, overflowMethod, bounds[k], bounds[k + 1]);
        }
        filler.join();
        t1 = std::chrono::steady_clock::now();
        if (fillRc) {
            g_lastError = fillError;
            rc = fillRc;
        }
    } else {
        rc = fillHandle(h.get(), src, std::move(offsets), dbLength, alphabetLength, /*prefetchView=*/true);
        t1 = std::chrono::steady_clock::now();
        if (rc == 0)
            rc = miopalSearchResults(h.get(), query, queryLength, gapOpen, gapExt, scoreMatrix, alphabetLength, results,
                                     searchType, mode, overflowMethod, 0, dbLength);
    }
    const auto t2 = std::chrono::steady_clock::now();
    {
        // view lists built ahead that no search of this call asked for (another overlap, a search that built its own
        // before the list was ready, a loop that stopped on an error) would otherwise keep their device blocks, and
        // stay out of handleDeviceBytes, until the handle is filled again
        std::lock_guard<std::mutex> g(h->viewMutex);
        h->prefetched.clear();
    }
    if (rc == 0) {
        int64_t keepMb = 4096;
        if (const char* env = tuned(Tune::SPARE_HANDLE_MB)) keepMb = atoll(env);
        if (handleDeviceBytes(h.get()) <= (keepMb << 20)) {
            SpareHandles& sp = spareHandles();
            std::lock_guard<std::mutex> g(sp.m);
            if (sp.idle.size() < kSpareHandles) sp.idle.emplace_back(std::move(h));
        }
    }
    if (h) {
        (void)hipSetDevice(h->device);
        h.reset();
    }
    if (verbose) {
        const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "miopal: opalSearchDatabase: upload %.1f ms, search + results %.1f ms, release %.1f ms\n",
                ms(t0, t1), ms(t1, t2), ms(t2, std::chrono::steady_clock::now()));
    }
    return rc;
    });
}

int opalSearchDatabaseCharSW(unsigned char query[], int queryLength, unsigned char** db, int dbLength,
                             int dbSeqLengths[], int gapOpen, int gapExt, int* scoreMatrix,
                             int alphabetLength, OpalSearchResult* results[]) {
    return opalSearchDatabase(query, queryLength, db, dbLength, dbSeqLengths, gapOpen, gapExt, scoreMatrix,
                              alphabetLength, results, OPAL_SEARCH_SCORE, OPAL_MODE_SW, OPAL_OVERFLOW_BUCKETS);
}

}  // extern "C"
