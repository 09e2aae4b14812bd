// Host shim (test infrastructure) of the head's harnesses (c51_host.cpp, dueling_host.cpp, dueling_loss_host.cpp): what a
// kernel file needs to compile for the CPU and run one workgroup at a time, its threads in lockstep.  __syncthreads is a real
// barrier, __shfl_xor an exchange through a shared array between two barriers (every thread of the workgroup takes part,
// partners 64-aligned as in a wave), static __shared__ objects are statics and the dynamic LDS tile is g_tile, a buffer of
// LOCKSTEP_TILE_FLOATS floats (define it before including this file; 1 where the kernels use none).  Include this file, then
// the one .hip under test; float arithmetic is IEEE float32 on both sides (build with -ffp-contract=off).
#pragma once
#include <math.h>
#include <pthread.h>
#include <stdint.h>

#include <thread>
#include <vector>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(n)
#define HIP_DYNAMIC_SHARED(type, var) type* var = (type*)g_tile;

#ifndef LOCKSTEP_TILE_FLOATS
#define LOCKSTEP_TILE_FLOATS 1
#endif
constexpr int LOCKSTEP_MAX_THREADS = 512;

static thread_local struct { unsigned x; } threadIdx;
static struct { unsigned x, y; } blockIdx;
static pthread_barrier_t g_bar;
static float g_tile[LOCKSTEP_TILE_FLOATS];
static int g_xi[LOCKSTEP_MAX_THREADS];
static float g_xf[LOCKSTEP_MAX_THREADS];

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

// a grid of gx * gy workgroups of THREADS threads, one workgroup after the other
template <int THREADS, typename F>
static void run_grid(int gx, int gy, F body) {
    static_assert(THREADS <= LOCKSTEP_MAX_THREADS, "the shuffle arrays hold one value per thread");
    pthread_barrier_init(&g_bar, nullptr, THREADS);
    for (int y = 0; y < gy; ++y)
        for (int x = 0; x < gx; ++x) {
            blockIdx.x = (unsigned)x;
            blockIdx.y = (unsigned)y;
            std::vector<std::thread> lanes;
            for (int l = 0; l < THREADS; ++l)
                lanes.emplace_back([&, l] { threadIdx.x = (unsigned)l; body(); });
            for (auto& t : lanes) t.join();
        }
    pthread_barrier_destroy(&g_bar);
}
