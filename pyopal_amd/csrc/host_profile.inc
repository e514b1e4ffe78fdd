// Part of host.hip (included there, not a translation unit of its own): miopalProfileColumns and its PSSM form, the
// step between two rounds of an iterated profile search - the alignments of one query (or PSSM) with a list of targets
// projected onto the query's rows, counted and weighted on the device (profile_columns.hip). Only the [Q][A + 1] tables,
// one weight per member and, when asked for, the multiple alignment cross PCIe.
//
// The alignments are alignPairsImpl's: the list (query 0, targets[p]) as a `full` pair list with a consumer in the
// place of gather + download. Per chunk the consumer projects the walk's operation slots into the rows of the call's
// msa buffer, on the chunk's stream behind the walk; alignPairsImpl waits for that stream when it takes the chunk's
// small arrays down, so a chunk's rows are final before the next chunk starts, whatever stream that one runs on.
// Where the state lives: in a workspace the call leases for itself at its first chunk and holds to its end (slots
// kProfileMsa, kProfileTables); the member indices of a chunk in the workspace that produced the chunk
// (kProfileMember). The column kernels run once, on the call's own stream, after the last chunk.

namespace {

// The profile of the query alone, beside `others` members that cover nothing (no targets, or empty alignments only):
// every covered row has one letter, k = 1 and the term 2^32. Host; nothing is launched.
void profileQueryAlone(const unsigned char* row, int Q, int A, int64_t others, int64_t* counts, int64_t* weighted,
                       int64_t* memberWeight, unsigned char* msa) {
    const size_t cells = (size_t)Q * (size_t)(A + 1);
    std::fill(counts, counts + cells, (int64_t)0);
    std::fill(weighted, weighted + cells, (int64_t)0);
    std::fill(memberWeight, memberWeight + 1 + others, (int64_t)0);
    int64_t covered = 0;
    for (int i = 0; i < Q; ++i) covered += row[i] < A ? 1 : 0;
    memberWeight[0] = covered * MIOPAL_PROFILE_WEIGHT_ONE;
    for (int i = 0; i < Q; ++i) {
        if (row[i] >= A) continue;
        counts[(size_t)i * (A + 1) + row[i]] = 1;
        weighted[(size_t)i * (A + 1) + row[i]] = memberWeight[0];
    }
    if (msa) {
        memset(msa, kProfileUncovered, (size_t)(1 + others) * (size_t)Q);
        for (int i = 0; i < Q; ++i) msa[i] = row[i] < A ? row[i] : kProfileUncovered;
    }
}

// The state of one call: the msa buffer and the tables, in slots of a workspace of its own
struct ProfileFold {
    MiopalDb* db;
    const unsigned char* row;   // member 0: the query's residues, or the consensus (255: no residue)
    int Q, A;
    int64_t members;
    std::unique_ptr<WorkspaceLease> mine;
    uint8_t* d_msa = nullptr;
    std::vector<int64_t> member;

    // the msa buffer all "not covered" but row 0: complete on return (the first chunk may run on any stream)
    int begin() {
        mine.reset(new WorkspaceLease(db));
        RC_TRY(mine->acquireInternal());
        Workspace* own = mine->ws;
        const size_t bytes = (size_t)members * (size_t)Q;
        void* p;
        RC_TRY(own->get(kProfileMsa, bytes, &p));
        HIP_TRY(hipMemsetAsync(p, kProfileUncovered, bytes, own->stream));
        std::vector<unsigned char> first(row, row + Q);
        for (auto& r : first)
            if (r >= A) r = kProfileUncovered;
        RC_TRY(own->stageUpload(p, first.data(), (size_t)Q, own->stream));
        HIP_TRY(hipStreamSynchronize(own->stream));
        d_msa = (uint8_t*)p;
        return 0;
    }
    // one chunk of the pair list: its operation slots into the rows of its members, behind the walk
    int chunk(const PairChunk& c) {
        if (!d_msa) RC_TRY(begin());
        member.resize((size_t)c.count);
        for (int k = 0; k < c.count; ++k) member[(size_t)k] = 1 + c.pairs[k];
        void* pm;
        RC_TRY(c.ws->get(kProfileMember, sizeof(int64_t) * (size_t)c.count, &pm));
        RC_TRY(c.ws->stageUpload(pm, member.data(), sizeof(int64_t) * (size_t)c.count, c.ws->stream));
        ProjectArgs a{};
        a.slots = c.slots;
        a.slotOps = c.slotOps;
        a.opsLen = c.opsLen;
        a.startQ = c.startQ;
        a.startT = c.startT;
        a.tOff = c.tOff;
        a.member = (const int64_t*)pm;
        a.nPairs = c.count;
        a.residues = db->d_residues;
        a.residueCount = db->total;
        a.msa = d_msa;
        a.queryLength = Q;
        a.alphabet = A;
        const hipError_t e = launchProfileProject(a, c.ws->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "profile projection launch: %s", hipGetErrorString(e));
        }
        return 0;
    }
    // msa -> the caller's tables, on the call's own stream (every chunk is complete)
    int finish(int64_t* counts, int64_t* weighted, int64_t* memberWeight, unsigned char* msa) {
        Workspace* own = mine->ws;
        const size_t cells = (size_t)Q * (size_t)(A + 1);
        void* p;
        RC_TRY(own->get(kProfileTables, sizeof(int64_t) * (2 * cells + (size_t)members) + profileScratchBytes(Q, A), &p));
        int64_t* dCounts = (int64_t*)p;
        int64_t* dWeighted = dCounts + cells;
        int64_t* dMember = dWeighted + cells;
        HIP_TRY(hipMemsetAsync(dCounts, 0, sizeof(int64_t) * 2 * cells, own->stream));
        const hipError_t e = launchProfileColumns(d_msa, members, Q, A, dCounts, dWeighted, dMember, dMember + members, own->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIOPAL_ERR_HIP, "profile columns launch: %s", hipGetErrorString(e));
        }
        // (staged, with room for all four reserved in one go so that none is drained before the last has arrived: the
        // caller's arrays are written when everything has)
        auto staged = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
        RC_TRY(own->reserveStaging(2 * staged(sizeof(int64_t) * cells) + staged(sizeof(int64_t) * (size_t)members) +
                                   (msa ? staged((size_t)members * (size_t)Q) : 0)));
        RC_TRY(own->stageDownload(counts, dCounts, sizeof(int64_t) * cells));
        RC_TRY(own->stageDownload(weighted, dWeighted, sizeof(int64_t) * cells));
        RC_TRY(own->stageDownload(memberWeight, dMember, sizeof(int64_t) * (size_t)members));
        if (msa) RC_TRY(own->stageDownload(msa, d_msa, (size_t)members * (size_t)Q));
        return own->finishDownloads();
    }
};

}  // namespace

// `row`: the query (matrix given) or the consensus (pssmRows given). The entry points have made the checks that come
// before alignPairsImpl's.
static int profileColumnsImpl(MiopalDb* db, const unsigned char* row, int Q, int open, int ext, const int* matrix, int A,
                              int mode, const int64_t* targets, int64_t n, int64_t* counts, int64_t* weighted,
                              int64_t* memberWeight, unsigned char* msa, const int* pssmRows) {
    const int64_t offsets[2] = {0, Q};
    const size_t held = (size_t)std::max<int64_t>(n, 0);
    // the list (query 0, targets[p]) and the per-pair answers nobody asked for (the checks of the walk read them): zero
    // pages nobody touches before the list has passed its checks
    struct Zeroed {
        void* p;
        explicit Zeroed(size_t count, size_t size) : p(calloc(std::max<size_t>(count, 1), size)) {}
        Zeroed(const Zeroed&) = delete;
        Zeroed& operator=(const Zeroed&) = delete;
        ~Zeroed() { free(p); }
    };
    Zeroed pairQuery(held, sizeof(int32_t)), score(held, sizeof(int)), endT(held, sizeof(int)), endQ(held, sizeof(int)),
        startT(held, sizeof(int)), startQ(held, sizeof(int)), opsOff(held + 1, sizeof(int64_t));
    for (const Zeroed* z : {&pairQuery, &score, &endT, &endQ, &startT, &startQ, &opsOff})
        if (!z->p) return fail(MIOPAL_ERR_INTERNAL, "out of host memory");
    HostBytes noOps;
    ProfileFold fold{db, row, Q, A, n + 1};
    PairChunkConsumer consumer;
    consumer.noun = "target";
    consumer.checks = [&]() -> int {
        if (!counts || !weighted || !memberWeight)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "null counts / weighted / member weight outputs");
        if (Q > 0 && n + 1 > (4ll << 30) / Q)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "the multiple alignment of %lld members x %d rows holds %.0f bytes: 4 GiB at most",
                        (long long)(n + 1), Q, (double)(n + 1) * (double)Q);
        return 0;
    };
    consumer.chunk = [&](const PairChunk& c) -> int { return fold.chunk(c); };
    static const unsigned char kNoResidue[1] = {0};
    RC_TRY(alignPairsImpl(db, row ? row : (Q == 0 ? kNoResidue : nullptr), offsets, 1, (const int32_t*)pairQuery.p, targets,
                          n, open, ext, matrix, A, OPAL_SEARCH_ALIGNMENT, mode, (int*)score.p, (int*)endT.p, (int*)endQ.p,
                          (int*)startT.p, (int*)startQ.p, &noOps, (int64_t*)opsOff.p, pssmRows, &consumer));
    if (Q == 0) return 0;
    if (!fold.d_msa) {
        // no target, or no pair with a DP: the query alone (nothing was launched)
        profileQueryAlone(row, Q, A, n, counts, weighted, memberWeight, msa);
        return 0;
    }
    return fold.finish(counts, weighted, memberWeight, msa);
}

// miopalTestProfileColumns (test hook): the count / terms / weights / weighted kernels alone, as ProfileFold::finish
// launches them, on a multiple alignment the caller supplies. Device 0.
static int testProfileColumnsImpl(const unsigned char* msa, int64_t members, int Q, int A, int64_t* counts,
                                  int64_t* weighted, int64_t* memberWeight) {
    constexpr int64_t kMaxEntries = (int64_t)1 << 27;
    if (members < 1 || Q < 1) return fail(MIOPAL_ERR_BAD_ARGUMENT, "members = %lld, rows = %d: both at least 1", (long long)members, Q);
    if (A <= 0 || A > kMaxAlphabet) return fail(MIOPAL_ERR_BAD_ARGUMENT, "bad alphabet length %d", A);
    if (!msa || !counts || !weighted || !memberWeight) return fail(MIOPAL_ERR_BAD_ARGUMENT, "null multiple alignment / outputs");
    if (members > kMaxEntries / Q) return fail(MIOPAL_ERR_BAD_ARGUMENT, "%lld members x %d rows: more than 2^27", (long long)members, Q);
    const size_t entries = (size_t)members * (size_t)Q;
    for (size_t x = 0; x < entries; ++x)
        if (msa[x] > A && msa[x] != kProfileUncovered)
            return fail(MIOPAL_ERR_BAD_ARGUMENT, "entry %d at %lld is neither a letter, the gap (%d) nor 255", msa[x], (long long)x, A);
    if (physicalDeviceCount() < 1) return fail(OPAL_ERR_NO_SIMD_SUPPORT, "no usable gfx950 device");
    HIP_TRY(hipSetDevice(usableDevices()[0]));

    const size_t cells = (size_t)Q * (size_t)(A + 1);
    const size_t tableBytes = sizeof(int64_t) * (2 * cells + (size_t)members) + profileScratchBytes(Q, A);
    DeviceBytes dMsa, dTables;
    OwnedStream stream;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&dMsa.p, entries));
    HIP_TRY(hipMalloc(&dTables.p, tableBytes));
    int64_t* dCounts = (int64_t*)dTables.p;
    int64_t* dWeighted = dCounts + cells;
    int64_t* dMember = dWeighted + cells;
    HIP_TRY(hipMemcpyAsync(dMsa.p, msa, entries, hipMemcpyHostToDevice, stream.s));
    HIP_TRY(hipMemsetAsync(dCounts, 0, sizeof(int64_t) * 2 * cells, stream.s));
    const hipError_t e = launchProfileColumns((const uint8_t*)dMsa.p, members, Q, A, dCounts, dWeighted, dMember,
                                              dMember + members, stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream.s);
        return fail(MIOPAL_ERR_HIP, "profile columns launch: %s", hipGetErrorString(e));
    }
    // (into a vector of the call: on an error the caller's arrays are as they were)
    std::vector<int64_t> host(2 * cells + (size_t)members);
    const hipError_t c = hipMemcpyAsync(host.data(), dCounts, sizeof(int64_t) * host.size(), hipMemcpyDeviceToHost, stream.s);
    const hipError_t d = hipStreamSynchronize(stream.s);   // (drained whatever happened: the vector goes away with the call)
    if (c != hipSuccess || d != hipSuccess)
        return fail(MIOPAL_ERR_HIP, "profile columns download: %s", hipGetErrorString(c != hipSuccess ? c : d));
    memcpy(counts, host.data(), sizeof(int64_t) * cells);
    memcpy(weighted, host.data() + cells, sizeof(int64_t) * cells);
    memcpy(memberWeight, host.data() + 2 * cells, sizeof(int64_t) * (size_t)members);
    return 0;
}
