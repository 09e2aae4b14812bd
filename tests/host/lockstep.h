// Host shim (test infrastructure) of the head's harnesses (c51_host.cpp, dueling_host.cpp, dueling_loss_host.cpp,
// streams_host.cpp) and of the replay kernels' (replay_host.cpp): what a kernel file needs to compile for the CPU and run one
// workgroup at a time, its threads in lockstep.  __syncthreads is a real barrier, __shfl_xor (int, float, long long) an
// exchange through a shared array between two barriers (partners 64-aligned as in a wave), static __shared__ objects are
// statics and the dynamic LDS tile is g_tile, a buffer of LOCKSTEP_TILE_FLOATS floats (define it before including this file;
// 1 where the kernels use none).  Include this file, then the .hip under test; float arithmetic is IEEE float32 on both sides
// (build with -ffp-contract=off).
//
// run_grid<THREADS> is the head harnesses' launch: every thread of the workgroup takes part in every shuffle.  lockstep_launch
// is the general one -- a thread count chosen at run time, up to 1024 -- with two options (LockstepLaunch):
//   dynamic_lds  the dynamic LDS is a heap block of exactly that many bytes, allocated once for the launch, instead of g_tile:
//                pass what the C API passes to hipLaunchKernelGGL, and a sanitizer build sees a kernel that walks past it;
//   wave_shuffles  a shuffle waits for the 64 lanes of its own wave only (one barrier per wave), as the hardware does: for
//                kernels in which whole waves return before the others shuffle (a workgroup-wide barrier would wait for ever).
// __builtin_amdgcn_wave_barrier is a real barrier over the calling thread's wave, atomicOr a real atomic, __clz the count of
// leading zeros with __clz(0) == 32.
#pragma once
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

#include <thread>
#include <vector>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(n)
#define HIP_DYNAMIC_SHARED(type, var) type* var = (type*)(g_dynamic_lds ? g_dynamic_lds : (void*)g_tile);
#define __builtin_amdgcn_wave_barrier() lockstep_wave_barrier()

#ifndef LOCKSTEP_TILE_FLOATS
#define LOCKSTEP_TILE_FLOATS 1
#endif
constexpr int LOCKSTEP_MAX_THREADS = 1024;
constexpr int LOCKSTEP_WAVE = 64;

static thread_local struct { unsigned x; } threadIdx;
static struct { unsigned x, y; } blockIdx;
static pthread_barrier_t g_bar;
static pthread_barrier_t g_wave_bar[LOCKSTEP_MAX_THREADS / LOCKSTEP_WAVE];
static bool g_wave_shuffles = false;
static void* g_dynamic_lds = nullptr;
static float g_tile[LOCKSTEP_TILE_FLOATS];
static int g_xi[LOCKSTEP_MAX_THREADS];
static float g_xf[LOCKSTEP_MAX_THREADS];
static long long g_xl[LOCKSTEP_MAX_THREADS];

static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline void lockstep_wave_barrier() { pthread_barrier_wait(&g_wave_bar[threadIdx.x / LOCKSTEP_WAVE]); }
static inline pthread_barrier_t* lockstep_shuffle_barrier() {
    return g_wave_shuffles ? &g_wave_bar[threadIdx.x / LOCKSTEP_WAVE] : &g_bar;
}
template <typename T>
static inline T lockstep_shfl_xor(T* slots, T v, int o) {
    pthread_barrier_t* bar = lockstep_shuffle_barrier();
    slots[threadIdx.x] = v;
    pthread_barrier_wait(bar);
    const T r = slots[threadIdx.x ^ o];
    pthread_barrier_wait(bar);
    return r;
}
static inline int __shfl_xor(int v, int o) { return lockstep_shfl_xor(g_xi, v, o); }
static inline float __shfl_xor(float v, int o) { return lockstep_shfl_xor(g_xf, v, o); }
static inline long long __shfl_xor(long long v, int o) { return lockstep_shfl_xor(g_xl, v, o); }
static inline int atomicOr(int32_t* address, int32_t v) { return __atomic_fetch_or(address, v, __ATOMIC_RELAXED); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }

struct LockstepLaunch {
    long long dynamic_lds = -1;          // bytes of dynamic LDS as an exact heap block; -1: the kernels' tile is g_tile
    bool wave_shuffles = false;          // shuffles wait for their own wave only
};

// a grid of gx * gy workgroups of `threads` threads, one workgroup after the other
template <typename F>
static void lockstep_launch(int threads, int gx, int gy, F body, LockstepLaunch how = LockstepLaunch()) {
    if (threads < 1 || threads > LOCKSTEP_MAX_THREADS) abort();
    const int waves = (threads + LOCKSTEP_WAVE - 1) / LOCKSTEP_WAVE;
    pthread_barrier_init(&g_bar, nullptr, threads);
    for (int w = 0; w < waves; ++w) {
        const int lanes = threads - w * LOCKSTEP_WAVE < LOCKSTEP_WAVE ? threads - w * LOCKSTEP_WAVE : LOCKSTEP_WAVE;
        pthread_barrier_init(&g_wave_bar[w], nullptr, lanes);
    }
    g_wave_shuffles = how.wave_shuffles;
    g_dynamic_lds = how.dynamic_lds >= 0 ? malloc((size_t)how.dynamic_lds) : nullptr;
    if (how.dynamic_lds >= 0 && !g_dynamic_lds) abort();
    // the host threads live for the whole launch: between two workgroups they meet at a barrier of their own, and thread 0
    // moves blockIdx on while the others wait there
    pthread_barrier_t between;
    pthread_barrier_init(&between, nullptr, threads);
    std::vector<std::thread> lanes;
    for (int l = 0; l < threads; ++l)
        lanes.emplace_back([&, l] {
            threadIdx.x = (unsigned)l;
            for (int y = 0; y < gy; ++y)
                for (int x = 0; x < gx; ++x) {
                    if (l == 0) blockIdx.x = (unsigned)x, blockIdx.y = (unsigned)y;
                    pthread_barrier_wait(&between);
                    body();
                    pthread_barrier_wait(&between);
                }
        });
    for (auto& t : lanes) t.join();
    pthread_barrier_destroy(&between);
    free(g_dynamic_lds);
    g_dynamic_lds = nullptr;
    g_wave_shuffles = false;
    for (int w = 0; w < waves; ++w) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_bar);
}

template <int THREADS, typename F>
static void run_grid(int gx, int gy, F body) {
    static_assert(THREADS <= LOCKSTEP_MAX_THREADS, "the shuffle arrays hold one value per thread");
    lockstep_launch(THREADS, gx, gy, body);
}
