// The CPU-only checks of the launch layer (pyopal_amd/csrc/launch_layer_selftest.h: the once-per-device logic under
// eight threads, the row dispatcher on every range in use) as a program of its own, for the host sanitizers:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=thread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -Ipyopal_amd/csrc tools/launch_layer_check.cpp -pthread -o launch_layer_check && ./launch_layer_check
//   (and once more with -fsanitize=address,undefined). Calls nothing of the HIP runtime: no device, no library.
#include <cstdio>
#include "launch_layer_selftest.h"

int main() {
    const int rc = miopal::launchLayerSelfTest();
    std::printf(rc == 0 ? "launch layer self-test: ok\n" : "launch layer self-test: check %d FAILED\n", rc);
    return rc == 0 ? 0 : 1;
}
