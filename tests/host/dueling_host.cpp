// Host harness (test infrastructure): the two kernels of irbpp_amd/csrc/irbpp_dueling.hip run on the CPU, one workgroup at a
// time, by 512 threads in lockstep (the workgroup's size): __syncthreads is a real barrier, __shfl_xor an exchange through a
// shared array between two barriers (every thread of the workgroup takes part, partners 64-aligned as in a wave), static
// __shared__ objects are statics and the dynamic LDS tile is a buffer of the harness.  The kernels' own source is compiled,
// so their staging, indexing, reductions and both forms (resident block / staged in chunks) are what the CPU suite checks
// against the numpy definition; float arithmetic is IEEE float32 on both sides (build with -ffp-contract=off).
// With -DDUELING_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs both kernels over a few shapes,
// either form included, and prints a checksum.
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>

#include <thread>
#include <vector>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(n)
#define HIP_DYNAMIC_SHARED(type, var) type* var = (type*)g_tile;

constexpr int HOST_THREADS = 512;
static thread_local struct { unsigned x; } threadIdx;
static struct { unsigned x; } blockIdx;
static pthread_barrier_t g_bar;
static float g_tile[144 * 1024 / 4];
static int g_xi[HOST_THREADS];
static float g_xf[HOST_THREADS];

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

#include "../../irbpp_amd/csrc/irbpp_dueling.hip"

static_assert(irbpp::DUELING_THREADS == HOST_THREADS, "the harness runs as many threads as the workgroup has");
static_assert(sizeof g_tile == irbpp::DUELING_TILE_BYTES, "the harness tile is the kernels' dynamic LDS");

template <typename F>
static void run_blocks(int blocks, F body) {
    pthread_barrier_init(&g_bar, nullptr, HOST_THREADS);
    for (int b = 0; b < blocks; ++b) {
        blockIdx.x = (unsigned)b;
        std::vector<std::thread> lanes;
        for (int l = 0; l < HOST_THREADS; ++l)
            lanes.emplace_back([&, l] { threadIdx.x = (unsigned)l; body(); });
        for (auto& t : lanes) t.join();
    }
    pthread_barrier_destroy(&g_bar);
}

extern "C" int host_dueling_tile_rows(int s_rows, int atoms) { return irbpp::dueling_tile_rows(s_rows, atoms); }

extern "C" void host_dueling_act(const float* v, long long v_stride, const float* a, long long env_stride, long long row_stride,
                                 const float* support, int atoms, const float* obs, int obs_stride, int s_rows, int n_env,
                                 int64_t* action, float* q_out, long long q_stride, float* p_out) {
    run_blocks(n_env, [&] {
        irbpp::irbpp_dueling_act_kernel(v, v_stride, a, env_stride, row_stride, support, atoms, obs, obs_stride, s_rows, action, q_out,
                                        q_stride, p_out);
    });
}

extern "C" void host_dueling_target(const float* v_on, long long von_stride, const float* a_on, long long on_env, long long on_row,
                                    const float* v_tg, long long vtg_stride, const float* a_tg, long long tg_env, long long tg_row,
                                    const float* returns, const float* nonterminals, const float* support, int atoms, int s_rows,
                                    int batch, float gamma_n, float v_min, float v_max, float delta_z, float* m, int64_t* a_star) {
    run_blocks(batch, [&] {
        irbpp::irbpp_dueling_target_kernel(v_on, von_stride, a_on, on_env, on_row, v_tg, vtg_stride, a_tg, tg_env, tg_row, returns,
                                           nonterminals, support, atoms, s_rows, gamma_n, v_min, v_max, delta_z, m, a_star);
    });
}

#ifdef DUELING_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    const int shapes[][3] = {{1, 2, 2}, {3, 2, 3}, {65, 31, 2}, {500, 31, 1}, {129, 128, 1}, {300, 128, 2}, {1024, 128, 1}};
    uint32_t rng = 12345u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 8.0f - 4.0f; };
    double sum = 0;
    for (const auto& sh : shapes) {
        const int s = sh[0], atoms = sh[1], n = sh[2];
        std::vector<float> v((size_t)n * atoms), a((size_t)n * s * atoms), v2(v.size()), a2(a.size()), z(atoms), obs((size_t)n * s * 5),
            q((size_t)n * s), p((size_t)n * s * atoms), ret(n), nt(n), m((size_t)n * atoms);
        std::vector<int64_t> act(n), star(n);
        for (auto* x : {&v, &a, &v2, &a2}) for (auto& f : *x) f = next();
        a[0] = 200.0f;                                   // most of that row's e are exactly 0
        for (int k = 0; k < atoms; ++k) z[k] = -1.0f + 9.0f * k / (atoms - 1);
        for (size_t i = 0; i < obs.size(); ++i) obs[i] = (i % 5 == 4 && (i / 5) % 3 == 0) ? 0.0f : 1.0f;
        for (int e = 0; e < n; ++e) { ret[e] = next() * 3; nt[e] = (float)(e & 1); }
        host_dueling_act(v.data(), atoms, a.data(), (long long)s * atoms, atoms, z.data(), atoms, obs.data(), s * 5, s, n, act.data(),
                         q.data(), s, p.data());
        host_dueling_act(v.data(), atoms, a.data(), (long long)s * atoms, atoms, z.data(), atoms, nullptr, 0, s, n, act.data(), nullptr,
                         0, nullptr);
        host_dueling_target(v.data(), atoms, a.data(), (long long)s * atoms, atoms, v2.data(), atoms, a2.data(), (long long)s * atoms,
                            atoms, ret.data(), nt.data(), z.data(), atoms, s, n, 0.97f, -1.0f, 8.0f, 9.0f / (atoms - 1), m.data(),
                            star.data());
        for (int e = 0; e < n; ++e) sum += (double)act[e] + (double)star[e];
        for (float f : q) sum += f;
        for (float f : p) sum += f;
        for (float f : m) sum += f;
        printf("S %d atoms %d n %d tile rows %d: checksum %.9g\n", s, atoms, n, irbpp::dueling_tile_rows(s, atoms), sum);
    }
    return 0;
}
#endif
