// The CPU-only checks of the later passes' plan (pyopal_amd/csrc/full_plan_selftest.h: the routing bits, the cost model,
// the slot geometry and the traceback batch plan, against literals) as a program of its own, for the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ipyopal_amd/csrc tools/full_plan_check.cpp -o full_plan_check \
//       && ./full_plan_check
//   (full_plan.h includes nothing of HIP: any host compiler does.) No device needed.
#include <cstdio>
#include "full_plan_selftest.h"

int main() {
    const int rc = miopal::fullPlanSelfTest();
    std::printf(rc == 0 ? "full plan self-test: ok\n" : "full plan self-test: check %d FAILED\n", rc);
    return rc == 0 ? 0 : 1;
}
