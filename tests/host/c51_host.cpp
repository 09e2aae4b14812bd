// Host harness (test infrastructure): the two kernels of irbpp_amd/csrc/irbpp_c51.hip run on the CPU, one workgroup at a
// time, by 64 threads in lockstep: __syncthreads is a real barrier, __shfl_xor an exchange through a shared array between
// two barriers, static __shared__ arrays are statics and the dynamic LDS tile is a buffer of the harness.  The kernels'
// own source is compiled, so their indexing, staging and reduction are what the CPU suite checks against the numpy
// definition; float arithmetic is IEEE float32 on both sides (build with -ffp-contract=off).
#include <math.h>
#include <pthread.h>
#include <stdint.h>

#include <thread>
#include <vector>

#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(n)
#define HIP_DYNAMIC_SHARED(type, var) type* var = (type*)g_tile;

static thread_local struct { unsigned x; } threadIdx;
static struct { unsigned x; } blockIdx;
static pthread_barrier_t g_bar;
static float g_tile[64 * 129];
static int g_xi[64];
static float g_xf[64];

static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline int __shfl_xor(int v, int o) {
    g_xi[threadIdx.x] = v;
    pthread_barrier_wait(&g_bar);
    const int r = g_xi[threadIdx.x ^ o];
    pthread_barrier_wait(&g_bar);
    return r;
}
static inline float __shfl_xor(float v, int o) {
    g_xf[threadIdx.x] = v;
    pthread_barrier_wait(&g_bar);
    const float r = g_xf[threadIdx.x ^ o];
    pthread_barrier_wait(&g_bar);
    return r;
}

#include "../../irbpp_amd/csrc/irbpp_c51.hip"

template <typename F>
static void run_blocks(int blocks, F body) {
    pthread_barrier_init(&g_bar, nullptr, 64);
    for (int b = 0; b < blocks; ++b) {
        blockIdx.x = (unsigned)b;
        std::vector<std::thread> lanes;
        for (int l = 0; l < 64; ++l)
            lanes.emplace_back([&, l] { threadIdx.x = (unsigned)l; body(); });
        for (auto& t : lanes) t.join();
    }
    pthread_barrier_destroy(&g_bar);
}

extern "C" void host_c51_act(const float* p, long long env_stride, long long row_stride, const float* support, int atoms,
                             const float* obs, int obs_stride, int s_rows, int n_env, int64_t* action, float* q_out,
                             long long q_stride) {
    run_blocks(n_env, [&] {
        irbpp::irbpp_c51_act_kernel(p, env_stride, row_stride, support, atoms, obs, obs_stride, s_rows, action, q_out, q_stride);
    });
}

extern "C" void host_c51_target(const float* p_on, long long on_env, long long on_row, const float* p_tg, long long tg_env,
                                long long tg_row, const float* returns, const float* nonterminals, const float* support,
                                int atoms, int s_rows, int batch, float gamma_n, float v_min, float v_max, float delta_z, float* m,
                                int64_t* a_star) {
    run_blocks(batch, [&] {
        irbpp::irbpp_c51_target_kernel(p_on, on_env, on_row, p_tg, tg_env, tg_row, returns, nonterminals, support, atoms, s_rows,
                                       gamma_n, v_min, v_max, delta_z, m, a_star);
    });
}
