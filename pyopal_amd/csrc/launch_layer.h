// What every launcher of the pair-table kernels needs on the host: the dynamic LDS limit raised once per
// device, and the instantiation picked whose row count is the run-time one. No device code, and the logic
// needs no GPU: miopalSelfTest(3) and tools/launch_layer_check.cpp run launch_layer_selftest.h on the CPU.
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstdint>
#include <type_traits>

namespace miopal {

// ---- once per device --------------------------------------------------------------------------------
// `done` holds one bit per device (a kernel's attributes belong to the device). set() runs unless this
// device's bit is there, and the bit is published only after set() has returned hipSuccess: a thread that
// arrives while another one is still setting sets as well (twice is harmless) and never goes on on the other's
// promise. A failure leaves the bit clear and comes back, the next call tries again; a device outside 0..63
// has no bit and sets every time. Later calls are one atomic load.
template <typename Setter>
hipError_t oncePerDevice(std::atomic<uint64_t>& done, int device, Setter&& set) {
    const bool tracked = device >= 0 && device < 64;
    if (tracked && ((done.load(std::memory_order_acquire) >> device) & 1)) return hipSuccess;
    const hipError_t e = set();
    if (e == hipSuccess && tracked) done.fetch_or(1ull << device, std::memory_order_release);
    return e;
}

// A kernel whose table takes more than the 64 KB a launch may ask for by default: allow it the CU's 160 KB on
// the current device (hipFuncSetAttribute applies to that device only). One state per kernel instantiation.
template <auto Kernel>
hipError_t allowFullLds() {
    static std::atomic<uint64_t> done{0};
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess) device = -1;
    return oncePerDevice(done, device, [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024);
    });
}

// ---- row dispatch -----------------------------------------------------------------------------------
// f(std::integral_constant<int, R>) for the one R of kLo, kLo + kStep, ... (kCount of them, none above kMax)
// that equals `rows`; hipErrorInvalidValue for every other count. The comparison and the call share R, so a
// row count can only ever reach its own instantiation, and nothing above kMax is instantiated at all.
template <int kLo, int kStep, int kCount, int kMax = kLo + kStep * (kCount - 1), typename F>
hipError_t dispatchRows(int rows, F&& f) {
    if constexpr (kCount > 0 && kLo <= kMax) {
        if (rows == kLo) return f(std::integral_constant<int, kLo>{});
        return dispatchRows<kLo + kStep, kStep, kCount - 1, kMax>(rows, f);
    } else {
        return hipErrorInvalidValue;
    }
}
// the same for a list that is no arithmetic sequence (the batch kernels' row classes)
template <int R, int... Rest, typename F>
hipError_t dispatchRowList(int rows, F&& f) {
    if (rows == R) return f(std::integral_constant<int, R>{});
    if constexpr (sizeof...(Rest) > 0) return dispatchRowList<Rest...>(rows, f);
    else return hipErrorInvalidValue;
}

}  // namespace miopal
