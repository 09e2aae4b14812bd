// Host harness (test infrastructure): the episode-metric routines of irbpp_amd/csrc/irbpp_metrics.h compiled for the CPU --
// Python's round(x, 6), numpy's summation order, and the wave's P-way tail merge run by 64 threads in lockstep, each
// cross-lane operation (wave max, ballot) an exchange through a shared array between two barriers.
#include <pthread.h>
#include <stdint.h>

#include <thread>
#include <vector>

#define __host__
#define __device__
#define IRBPP_WAVE_FN
#define IRBPP_METRICS_HOST_WAVE

static pthread_barrier_t g_bar;
static thread_local int g_lane;
static int64_t g_x[64];

static inline int64_t metrics_wave_max(int64_t v) {
    g_x[g_lane] = v;
    pthread_barrier_wait(&g_bar);
    int64_t m = g_x[0];
    for (int i = 1; i < 64; ++i) m = g_x[i] > m ? g_x[i] : m;
    pthread_barrier_wait(&g_bar);
    return m;
}
static inline uint64_t metrics_ballot(bool p) {
    g_x[g_lane] = p ? 1 : 0;
    pthread_barrier_wait(&g_bar);
    uint64_t b = 0;
    for (int i = 0; i < 64; ++i) b |= (uint64_t)(g_x[i] != 0) << i;
    pthread_barrier_wait(&g_bar);
    return b;
}

#include "../../irbpp_amd/csrc/irbpp_metrics.h"

extern "C" {

void host_py_round6(const double* x, double* out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = irbpp::py_round6(x[i]);
}

double host_np_mean(const double* a, int n) { return irbpp::np_sum(a, n) / (double)n; }

// keys [P][W] (part p's first fills[p] ascending), n picks -> out_part / out_idx [n]: the merged window, oldest first
void host_tail_merge(const int64_t* keys, const int* fills, int P, int W, int n, int* out_part, int* out_idx) {
    pthread_barrier_init(&g_bar, nullptr, 64);
    std::vector<std::thread> lanes;
    for (int lane = 0; lane < 64; ++lane)
        lanes.emplace_back([=]() {
            g_lane = lane;
            const int64_t* mine = keys + (size_t)(lane < P ? lane : 0) * W;
            irbpp::tail_merge(lane, P, lane < P ? fills[lane] : 0, n, [&](int i) { return mine[i]; },
                              [&](int i, int slot) { out_part[slot] = lane; out_idx[slot] = i; });
        });
    for (auto& t : lanes) t.join();
    pthread_barrier_destroy(&g_bar);
}

}
