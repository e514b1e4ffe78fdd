// CPU-only checks of launch_layer.h: miopalSelfTest(3) (host.hip) and tools/launch_layer_check.cpp (the same under the
// host sanitizers). 0 = fine, else the number of the check that failed.
#pragma once
#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>
#include "launch_layer.h"

namespace miopal {

// every row count of the range reaches exactly its own R, every other one from -1 to 70 is refused uncalled
template <typename Dispatch, typename Holds>
static bool rowsReachTheirOwn(Dispatch&& dispatch, Holds&& holds) {
    for (int rows = -1; rows <= 70; ++rows) {
        int got = -1, calls = 0;
        const hipError_t e = dispatch(rows, [&](auto r) {
            got = r;   // (its R)
            ++calls;
            return hipSuccess;
        });
        if (holds(rows) ? !(e == hipSuccess && calls == 1 && got == rows) : !(e == hipErrorInvalidValue && calls == 0)) return false;
    }
    return true;
}
template <int kLo, int kStep, int kCount, int kMax = kLo + kStep * (kCount - 1)>
static bool rangeReachesItsOwn() {
    return rowsReachTheirOwn([](int rows, auto&& f) { return dispatchRows<kLo, kStep, kCount, kMax>(rows, f); },
                             [](int rows) {
                                 return rows >= kLo && rows <= std::min(kMax, kLo + kStep * (kCount - 1)) && (rows - kLo) % kStep == 0;
                             });
}
template <int... Rs>
static bool listReachesItsOwn() {
    return rowsReachTheirOwn([](int rows, auto&& f) { return dispatchRowList<Rs...>(rows, f); },
                             [](int rows) { return ((rows == Rs) || ...); });
}

inline int launchLayerSelfTest() {
    // ---- (a) once per device ----
    {
        // eight first calls at once: nobody comes back before a setter call has completed successfully
        constexpr int kThreads = 8;
        std::atomic<uint64_t> done{0};
        std::atomic<int> ready{0}, calls{0}, completed{0}, early{0}, failed{0};
        std::vector<std::thread> threads;
        for (int t = 0; t < kThreads; ++t)
            threads.emplace_back([&] {
                ready.fetch_add(1);
                while (ready.load() < kThreads) std::this_thread::yield();
                const hipError_t e = oncePerDevice(done, 3, [&] {
                    calls.fetch_add(1);
                    std::this_thread::sleep_for(std::chrono::milliseconds(20));
                    completed.fetch_add(1);
                    return hipSuccess;
                });
                if (completed.load() < 1) early.fetch_add(1);
                if (e != hipSuccess) failed.fetch_add(1);
            });
        for (auto& t : threads) t.join();
        if (early.load() != 0) return 1;
        if (failed.load() != 0 || calls.load() < 1 || calls.load() > kThreads) return 2;
        if (done.load() != (1ull << 3)) return 3;
        // afterwards nobody sets again
        if (oncePerDevice(done, 3, [&] { calls.fetch_add(100); return hipSuccess; }) != hipSuccess || calls.load() > kThreads) return 4;
    }
    {
        std::atomic<uint64_t> done{0};
        int calls = 0;
        hipError_t next = hipErrorOutOfMemory;
        auto set = [&] {
            ++calls;
            return next;
        };
        // a failure comes back and leaves the bit clear; the next call tries again
        if (oncePerDevice(done, 0, set) != hipErrorOutOfMemory || calls != 1 || done.load() != 0) return 5;
        next = hipSuccess;
        if (oncePerDevice(done, 0, set) != hipSuccess || calls != 2 || done.load() != 1) return 6;
        if (oncePerDevice(done, 0, set) != hipSuccess || calls != 2) return 7;
        // a second device gets a call of its own
        if (oncePerDevice(done, 5, set) != hipSuccess || calls != 3 || done.load() != 0x21) return 8;
        if (oncePerDevice(done, 5, set) != hipSuccess || calls != 3) return 9;
        // a device that has no bit sets every time
        for (int k = 1; k <= 3; ++k)
            if (oncePerDevice(done, 64, set) != hipSuccess || calls != 3 + k || done.load() != 0x21) return 10;
        if (oncePerDevice(done, -1, set) != hipSuccess || calls != 7 || done.load() != 0x21) return 11;
        if (oncePerDevice(done, 63, set) != hipSuccess || oncePerDevice(done, 63, set) != hipSuccess || calls != 8) return 12;
    }
    // ---- (b) the row dispatcher, on every range the kernel units use ----
    // general kernel and the int16 / half pair table; the biased Smith-Waterman units; the NW / HW / OV units (even ones)
    if (!rangeReachesItsOwn<8, 8, 8>()) return 20;
    if (!rangeReachesItsOwn<1, 2, 8>() || !rangeReachesItsOwn<17, 2, 8>() || !rangeReachesItsOwn<33, 2, 8>() || !rangeReachesItsOwn<49, 2, 8>()) return 21;
    if (!rangeReachesItsOwn<2, 2, 8>() || !rangeReachesItsOwn<18, 2, 8>() || !rangeReachesItsOwn<34, 2, 8>() || !rangeReachesItsOwn<50, 2, 8>()) return 22;
    // the strips units under their maxima: scores, with end locations, the known-optimum pass
    if (!rangeReachesItsOwn<32, 2, 8, 52>() || !rangeReachesItsOwn<48, 2, 8, 52>()) return 23;
    if (!rangeReachesItsOwn<32, 2, 8, 48>() || !rangeReachesItsOwn<48, 2, 8, 48>()) return 24;
    if (!rangeReachesItsOwn<32, 2, 8, 40>()) return 25;
    // the units' first row counts (interseq.hip)
    if (!rangeReachesItsOwn<1, 16, 4>() || !rangeReachesItsOwn<2, 16, 4>() || !rangeReachesItsOwn<32, 16, 2>() || !rangeReachesItsOwn<32, 16, 1>()) return 26;
    // the batch units' row classes
    if (!listReachesItsOwn<8, 16, 24, 32, 40, 48, 56, 60, 64>() || !listReachesItsOwn<8, 16, 24, 32>() || !listReachesItsOwn<40, 48, 56, 60, 64>()) return 27;
    return 0;
}

}  // namespace miopal
