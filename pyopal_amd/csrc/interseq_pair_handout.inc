// The hand-out of groups in the one-strip pair-table kernels (interseq_pair_biased_kernel without the column split,
// interseq_pair_global_kernel), included as text in two parts (as functions or a struct the first round and its tier
// tables changed the kernels' code objects, profiles/pair_table_parts_device_code.txt).
//   #define MIOPAL_PAIR_HANDOUT_PART 1   behind the table's barrier and the pacing's set-up: wave, simd, tier,
//                                        firstDynamic, firstRound
//   #define MIOPAL_PAIR_HANDOUT_PART 2   in the group loop, with `int g` declared: the wavefront's next group in g
//                                        (continue: none in the first round; break: none is left)
// The including kernel provides a, lane, simdTaken (4 ints in LDS, zeroed) and kHandoutWaves (12 or 8 wavefronts).
// Groups are sorted longest first. First round: static and striped, so that every CU, and every SIMD inside it
// (wavefronts w, w+4, w+8 share one), starts with a mix of long and short groups: wavefront w takes tier
// kTier[w % 4][w / 4] of gridDim.x groups each, in snake order across workgroups. Later rounds: nextGroup
// (interseq_pair_parts.h), whoever finishes pulls the next group, so wavefronts finish together.
#if MIOPAL_PAIR_HANDOUT_PART == 1
    // (wave-uniform by construction; said so, or everything derived from it would sit in VGPRs)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int kTier12[4][3] = {{0, 6, 11}, {1, 7, 8}, {2, 5, 9}, {3, 4, 10}};
    constexpr int kTier8[4][2] = {{0, 7}, {1, 6}, {2, 5}, {3, 4}};
    const int tier = kHandoutWaves == 12 ? kTier12[wave & 3][wave >> 2] : kTier8[wave & 3][(wave >> 2) & 1];
    const int firstDynamic = kHandoutWaves * gridDim.x;
    // HW_REG_HW_ID (4), SIMD_ID = bits 5:4
    const int simd = (int)__builtin_amdgcn_s_getreg(4 | (4 << 6) | ((2 - 1) << 11)) & 3;
    bool firstRound = true;
#elif MIOPAL_PAIR_HANDOUT_PART == 2
        if (firstRound) {
            g = tier * gridDim.x + ((tier & 1) ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x);
            firstRound = false;
            if (lane == 0 && a.tailThrottle > 0) atomicAdd(&simdTaken[simd], 1);
            if (g >= a.nGroups) continue;
            g += a.groupBase;
        } else {
            g = nextGroup(simdTaken, simd, a.tailThrottle, a.workCounter, firstDynamic, lane);
            if (g >= a.nGroups) break;
            g += a.groupBase;
        }
#else
#error "MIOPAL_PAIR_HANDOUT_PART: 1 or 2"
#endif
#undef MIOPAL_PAIR_HANDOUT_PART
