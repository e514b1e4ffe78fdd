// The picker of the occurrence searches, shared by the translation units whose kernels run it (occurrences.hip and,
// through it, occurrences_pssm.hip; occurrences_batch.hip). include/miopal.h, miopalSearchOccurrences, states the rule.
#pragma once
#include <hip/hip_runtime.h>

namespace miopal {

// Greedy peak picking with a suppression window, left to right over one target's columns: the candidate is the
// first column of the highest value seen since the last emission; it is emitted once a column more than `window`
// behind it is reached, or at the end.
struct OccurrencePicker {
    int minScore, window;
    int cj = -1, cv = 0, cr = 0;   // the candidate (cj < 0: none)
    __device__ OccurrencePicker(int minScore_, int window_) : minScore(minScore_), window(window_) {}
    template <typename Emit>
    __device__ void feed(int j, int v, int r, Emit&& emit) {
        if (cj >= 0 && j - cj > window) {
            emit(cj, cv, cr);
            cj = -1;
        }
        if (v >= minScore && (cj < 0 || v > cv)) {
            cj = j;
            cv = v;
            cr = r;
        }
    }
    template <typename Emit>
    __device__ void finish(Emit&& emit) {
        if (cj >= 0) emit(cj, cv, cr);
        cj = -1;
    }
};

}  // namespace miopal
