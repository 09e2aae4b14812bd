// Host harness (test infrastructure): the wave routines of irbpp_amd/csrc/irbpp_itemgen_device.h (MT19937 regeneration,
// tempering, one- and two-stage selection) run on the CPU by 64 threads in lockstep, as tests/host/wave_host.cpp runs the
// wave-cooperative contour routines: every cross-lane operation is an exchange through a shared array between two
// barriers, and the wave barrier that orders the lanes' LDS traffic on the device is a real barrier here.
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline

static thread_local struct { unsigned x; } threadIdx;
static pthread_barrier_t g_bar;
static int g_x[64];
static unsigned long long g_bal;

static inline int __shfl(int v, int src) {
    g_x[threadIdx.x & 63] = v;
    pthread_barrier_wait(&g_bar);
    const int r = g_x[src & 63];
    pthread_barrier_wait(&g_bar);
    return r;
}
static inline unsigned long long __ballot(bool p) {
    if ((threadIdx.x & 63) == 0) g_bal = 0ull;
    pthread_barrier_wait(&g_bar);
    if (p) __atomic_fetch_or(&g_bal, 1ull << (threadIdx.x & 63), __ATOMIC_RELAXED);
    pthread_barrier_wait(&g_bar);
    const unsigned long long r = g_bal;
    pthread_barrier_wait(&g_bar);
    return r;
}
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
#define IRBPP_ITEMGEN_SYNC() pthread_barrier_wait(&g_bar)

#include "../../irbpp_amd/csrc/irbpp_itemgen_device.h"

namespace {

template <class F>
void run_wave(F body) {
    pthread_barrier_init(&g_bar, nullptr, 64);
    std::vector<std::thread> lanes;
    for (int l = 0; l < 64; ++l)
        lanes.emplace_back([&, l] {
            threadIdx.x = (unsigned)l;
            body(l);
        });
    for (auto& t : lanes) t.join();
    pthread_barrier_destroy(&g_bar);
}

struct ArraySink {
    int32_t* out;
    void operator()(int j, int32_t id) const { out[j] = id; }
};

}  // namespace

// init_genrand alone: the 624 key words of a fresh stream
extern "C" void host_mt_seed(uint32_t seed, uint32_t* key) { irbpp::mt_seed_serial(key, seed); }

// `blocks` regenerations of a stream seeded `seed`: keys = [blocks][624] the key words after each one, words = the same
// tempered (the generator's output words in order)
extern "C" void host_mt_blocks(uint32_t seed, int blocks, uint32_t* keys, uint32_t* words) {
    static uint32_t k[irbpp::MT_N];
    irbpp::mt_seed_serial(k, seed);
    run_wave([&](int lane) {
        for (int b = 0; b < blocks; ++b) {
            irbpp::mt_regenerate_wave(lane, k);
            for (int i = lane; i < irbpp::MT_N; i += 64) {
                keys[b * irbpp::MT_N + i] = k[i];
                words[b * irbpp::MT_N + i] = irbpp::mt_temper(k[i]);
            }
        }
    });
}

// One stream seeded `seed` over the given lists, drawn in n_calls calls of counts[c] items each, as the kernels call the
// routine: out receives the items back to back.  Returns the final position in the key words, or -1 if the lanes
// disagree about it.
extern "C" int host_itemgen_draw(uint32_t seed, int n_groups, const int32_t* offsets, const int32_t* members, int n_members,
                                 const int* counts, int n_calls, int32_t* out) {
    static uint32_t k[irbpp::MT_N];
    irbpp::mt_seed_serial(k, seed);
    std::vector<uint32_t> masks((size_t)(n_groups > 0 ? n_groups : 1));
    for (int g = 0; g < n_groups; ++g) masks[g] = irbpp::randint_mask((uint32_t)(offsets[g + 1] - offsets[g]) - 1u);
    irbpp::ItemGenTables G;
    G.n_groups = n_groups;
    G.n_members = n_members;
    G.offsets = offsets;
    G.members = members;
    G.group_mask = masks.data();
    G.mask0 = irbpp::randint_mask((uint32_t)(n_groups > 0 ? n_groups : n_members) - 1u);
    int final_pos[64];
    run_wave([&](int lane) {
        int pos = irbpp::MT_N;
        int32_t* at = out;
        for (int c = 0; c < n_calls; ++c) {
            ArraySink sink{at};
            pos = irbpp::itemgen_draw_wave(lane, k, pos, G, counts[c], sink);
            at += counts[c];
            pthread_barrier_wait(&g_bar);          // (a kernel boundary)
        }
        final_pos[lane] = pos;
    });
    for (int l = 1; l < 64; ++l)
        if (final_pos[l] != final_pos[0]) return -1;
    return final_pos[0];
}
