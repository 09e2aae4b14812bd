// irbpp_metrics.h -- the arithmetic of the trainer's logged episode metrics (trainer.py:145-147, 168-178, 215-222), shared by the
// window kernels of irbpp_metrics.hip and, compiled for the host, by tests/host/metrics_host.cpp:
//   - py_round6: Python's round(x, 6), the Monitor's 'r' (monitor.py:64) -- NOT np.round (round6 of irbpp_kernels.hip);
//   - np_sum:    the float64 sum np.mean forms over a list (numpy's pairwise summation), so that sum / n is np.mean bit for bit;
//   - tail_merge: the newest n entries of up to 64 sorted snapshots (one per part: group or rank), one wave.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef IRBPP_HD
#define IRBPP_HD __host__ __device__
#endif
#ifndef IRBPP_WAVE_FN
#define IRBPP_WAVE_FN __device__      // code that needs a wave's lanes (the host test runs 64 threads in lockstep instead)
#endif

namespace irbpp {

// Python's round(x, 6): the EXACT value x * 10^6 rounded half-to-even to an integer m, then m / 10^6 correctly rounded (what
// CPython's dtoa-based float.__round__ returns).  p = x * 1e6 is the product rounded; e = fma(x, 1e6, -p) is its exact error,
// so p + e is the exact product.  rint(p) is already m unless p itself lies exactly half-way between two integers: then the
// sign of e decides, and e == 0 is a true tie that rint has settled to the even side.  (For |x| < 2^52 / 1e6, where p - rint(p)
// is exact; episode rewards are far below that.)
IRBPP_HD inline double py_round6(double x) {
    const double p = x * 1e6;
    const double e = fma(x, 1e6, -p);
    double m = rint(p);
    const double d = p - m;
    if (d == 0.5 && e > 0.0) m += 1.0;
    else if (d == -0.5 && e < 0.0) m -= 1.0;
    return m / 1e6;
}

// numpy's pairwise summation of a contiguous float64 run (pairwise_sum_DOUBLE, numpy/_core/src/umath/loops_utils.h.src):
// below 8 elements a plain running sum, up to 128 eight interleaved accumulators combined as ((0+1)+(2+3))+((4+5)+(6+7)) and the
// remainder added one by one, above that the two halves split at a multiple of 8.  D bounds the recursion at compile time
// (no call stack on the device): D = 6 covers every n <= 1024 (1023 already needs four levels of halving).
template <int D>
IRBPP_HD inline double np_pairwise(const double* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128 || D == 0) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise<(D > 0 ? D - 1 : 0)>(a, n2) + np_pairwise<(D > 0 ? D - 1 : 0)>(a + n2, n - n2);
}

// np.add.reduce of a 1-d float64 array (what np.mean sums): the reduction starts from the add identity 0.0 and adds the
// pairwise sum of all n elements.  n <= 1024 (the window's limit).
IRBPP_HD inline double np_sum(const double* a, int n) { return 0.0 + np_pairwise<6>(a, n); }

#ifndef IRBPP_METRICS_HOST_WAVE
__device__ inline int64_t metrics_wave_max(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}
__device__ inline uint64_t metrics_ballot(bool p) { return __ballot(p); }
#endif

// The P-way merge from the tails (one wave; lane p < P holds part p, whose snapshot lists `fill` entries in ascending key
// order, keys read through key_at(i)): n picks, each the largest key still at some lane's tail (the lowest lane on equal
// keys, which distinct global bins never produce).  Pick k is the (k+1)-th newest entry of the union: emit(i, n - 1 - k)
// hands the picking lane's entry i its slot in the merged window, oldest first.  Any entry of the union's newest W is among
// the newest W of its own part, so the parts' windows are all the merge needs.  Requires n <= the sum of the fills.
template <class KeyAt, class Emit>
IRBPP_WAVE_FN inline void tail_merge(int lane, int P, int fill, int n, KeyAt key_at, Emit emit) {
    int idx = lane < P ? fill - 1 : -1;
    int64_t key = idx >= 0 ? key_at(idx) : (int64_t)-1;
    for (int k = 0; k < n; ++k) {
        const int64_t best = metrics_wave_max(key);
        const uint64_t who = metrics_ballot(key == best);
        if (lane == __builtin_ctzll(who)) {
            emit(idx, n - 1 - k);
            --idx;
            key = idx >= 0 ? key_at(idx) : (int64_t)-1;
        }
    }
}

}  // namespace irbpp
