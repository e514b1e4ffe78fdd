// The CPU-only checks of the host router's range model (pyopal_amd/csrc/score_ranges_selftest.h: the biased band, the
// NW / HW / OV ranges, the 32-bit bound, the int16 lane fits, against literals) as a program of its own, for the host
// sanitizers:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -Ipyopal_amd/csrc tools/score_ranges_check.cpp -o score_ranges_check && ./score_ranges_check
//   (as HIP, host side only: score_ranges.h takes its constants from common.h, which also declares device code.)
//   Calls nothing of the HIP runtime: no device needed.
#include <cstdio>
#include "score_ranges_selftest.h"

int main() {
    const int rc = miopal::scoreRangesSelfTest();
    std::printf(rc == 0 ? "score ranges self-test: ok\n" : "score ranges self-test: check %d FAILED\n", rc);
    return rc == 0 ? 0 : 1;
}
