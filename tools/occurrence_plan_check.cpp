// The CPU-only checks of the panel occurrence search's chunk plan (pyopal_amd/csrc/occurrence_plan_selftest.h: the
// chunk sizes, the groups the count sweep wants, and one chunk's row list, entries and groups, against literals) as a
// program of its own, for the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ipyopal_amd/csrc tools/occurrence_plan_check.cpp -o occurrence_plan_check
//   ./occurrence_plan_check
//   (occurrence_plan.h includes nothing of HIP: any host compiler does.) No device needed.
#include <cstdio>
#include "occurrence_plan_selftest.h"

int main() {
    const int rc = miopal::occurrencePlanSelfTest();
    std::printf(rc == 0 ? "occurrence plan self-test: ok\n" : "occurrence plan self-test: check %d FAILED\n", rc);
    return rc == 0 ? 0 : 1;
}
