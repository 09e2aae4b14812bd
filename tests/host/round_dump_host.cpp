// Host harness (test infrastructure): the two forms in which a trace wave's borders reach the polygon kernel
// (irbpp_amd/csrc/irbpp_rounds.h) run on the CPU by 64 threads in lockstep, as tests/host/wave_host.cpp runs the segmented
// Douglas-Peucker: every cross-lane operation (v_readlane, ds_bpermute via __shfl, the DPP controls of the inclusive scans,
// ballots) is an exchange through a shared array between two barriers.  One call plays the end of one trace chunk and the
// polygon waves that take its rounds, once per form, and returns the positions each form hands to approx_convex_segmented.
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline
struct uint2 { unsigned x, y; };
static inline int __ffs(int v) { return __builtin_ffs(v); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline unsigned __brev(unsigned v) { unsigned r = 0; for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i); return r; }
static inline unsigned atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }

static thread_local struct { unsigned x; } threadIdx;
static pthread_barrier_t g_bar;
static int g_x[64];

static inline int xchg(int v, int src) {                  // value of lane `src` (per-lane src allowed)
    g_x[threadIdx.x & 63] = v;
    pthread_barrier_wait(&g_bar);
    const int r = g_x[src & 63];
    pthread_barrier_wait(&g_bar);
    return r;
}
// v_mov_b32_dpp with the controls the device code uses (CDNA ISA: quad_perm 0x00-0xFF, row_shr:n 0x111-0x11F, row_mirror
// 0x140, row_half_mirror 0x141, row_bcast15 0x142, row_bcast31 0x143); a lane without a source, or in a row outside
// row_mask, keeps `old`
static inline int emu_dpp(int old, int v, int ctrl, int row_mask) {
    const int lane = threadIdx.x & 63, row = lane >> 4;
    int src = lane;
    bool has_src = true;
    if (ctrl <= 0xFF) src = (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3);
    else if (ctrl >= 0x111 && ctrl <= 0x11F) { has_src = (lane & 15) >= (ctrl & 15); src = lane - (ctrl & 15); }
    else if (ctrl == 0x140) src = (lane & ~15) | (15 - (lane & 15));
    else if (ctrl == 0x141) src = (lane & ~7) | (7 - (lane & 7));
    else if (ctrl == 0x142) { has_src = row >= 1; src = row * 16 - 1; }
    else if (ctrl == 0x143) { has_src = row >= 2; src = 31; }
    const int got = xchg(v, has_src ? src : lane);
    return (((row_mask >> row) & 1) && has_src) ? got : old;
}
#define __builtin_amdgcn_readlane(v, l) xchg((v), (l))
#define __builtin_amdgcn_readfirstlane(v) xchg((v), 0)
#define __builtin_amdgcn_update_dpp(old, v, ctrl, rm, bm, bc) emu_dpp((old), (v), (ctrl), (rm))
#define __shfl(v, l) xchg((v), (l))
#define IRBPP_WAVE_SYNC() pthread_barrier_wait(&g_bar)
static unsigned long long g_bal;
static inline unsigned long long __ballot(bool p) {
    if ((threadIdx.x & 63) == 0) g_bal = 0ull;
    pthread_barrier_wait(&g_bar);
    if (p) __atomic_fetch_or(&g_bal, 1ull << (threadIdx.x & 63), __ATOMIC_RELAXED);
    pthread_barrier_wait(&g_bar);
    const unsigned long long r = g_bal;
    pthread_barrier_wait(&g_bar);
    return r;
}
static inline unsigned atomicMax(uint32_t* p, uint32_t v) {
    uint32_t o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
static inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }

#include "../../irbpp_amd/csrc/irbpp_rounds.h"

using namespace irbpp;

constexpr int PP = TRACE_P, NPOS = 64 * PP;
constexpr int WAVE = 1, WAVES = 3;                        // the chunk's wave in a w_big of three regions: the index is used

template <int CPW>
static int run_forms(const uint8_t* slot_bytes, const uint8_t* spill_bytes, const int* my_n_in, const int* rk_in, int max_rounds,
                     int32_t* out_rec, int32_t* out_dump, int32_t* lane_plan, uint64_t* sels) {
    alignas(16) static uint8_t slots[64 * TRACE_SLOT];                // the trace wave's LDS slots (CPW of them are its own)
    static uint32_t dps[NPOS];
    static std::vector<uint8_t> w_big, entries_rec, entries_dump;
    w_big.assign((size_t)WAVES * TRACE_WAVE_BYTES + 16, 0xEE);
    entries_rec.assign((size_t)(max_rounds + 1) * ROUND_BYTES + 16, 0xEE);
    entries_dump.assign((size_t)(max_rounds + 1) * ROUND_BYTES + 16, 0xEE);
    uint8_t* const big = w_big.data() + ((16 - ((uintptr_t)w_big.data() & 15)) & 15);           // 16-byte aligned like hipMalloc's
    uint8_t* const erec = entries_rec.data() + ((16 - ((uintptr_t)entries_rec.data() & 15)) & 15);
    uint8_t* const edump = entries_dump.data() + ((16 - ((uintptr_t)entries_dump.data() & 15)) & 15);
    uint8_t* const region = big + (size_t)WAVE * TRACE_WAVE_BYTES;
    memset(slots, 0xEE, sizeof slots);
    memcpy(slots, slot_bytes, (size_t)CPW * TRACE_SLOT);
    memcpy(region + TRACE_SPILL_OFF, spill_bytes, 64 * TRACE_SPILL);
    int n_rec = -1, n_dump = -2, over = 0;
    pthread_barrier_init(&g_bar, nullptr, 64);
    std::vector<std::thread> lanes;
    for (int l = 0; l < 64; ++l)
        lanes.emplace_back([&, l] {
            threadIdx.x = (unsigned)l;
            const int lane = l, my_n = lane < CPW ? my_n_in[lane] : 0, rk = lane < CPW ? rk_in[lane] : 0;
            const bool spilled = __ballot(my_n > TRACE_LDS_CAP) != 0ull;
            const uint8_t* const wave_spill = region + TRACE_SPILL_OFF;
            // ---- the counting pass (both forms)
            int my_round, my_start;
            unsigned long long my_sel;
            const int n_rounds = count_rounds(lane, my_n, my_round, my_start, my_sel);
            lane_plan[2 * lane] = my_round;
            lane_plan[2 * lane + 1] = my_start;
            if (lane < n_rounds && lane < max_rounds) sels[lane] = my_sel;
            if (n_rounds > max_rounds) { if (lane == 0) over = 1; return; }              // (uniform)
            // ---- RECORD form, trace side: the trace wave's own gather, round by round
            int left = my_n, n_dp = 0;
            for (int cls = 0; cls < 2; ++cls)
                for (;;) {
                    int wn, excl, base = 0;
                    const unsigned long long sel = next_round(cls, left, wn, excl, base);
                    if (sel == 0ull) break;
                    bool live[PP];
                    int pv[PP], jj[PP], nn[PP], sbq[PP], prk[PP], owner[PP];
                    round_positions<PP>(lane, sel, wn, excl - base, rk, slots, wave_spill, spilled, dps, live, pv, jj, nn, sbq, prk, owner);
                    round_record_store<PP>(lane, erec + (size_t)n_dp * ROUND_BYTES, live, pv, nn, sbq, prk);
                    if ((sel >> lane) & 1ull) left = 0;
                    ++n_dp;
                }
            if (lane == 0) n_rec = n_dp;
            // ---- DUMP form, trace side
            if (n_rounds > 0) {
                round_dump_store<CPW>(lane, region, slots, my_n, rk, my_round, my_start);
                round_headers_store(lane, edump, n_rounds, WAVE, spilled, my_sel);
            }
            if (lane == 0) n_dump = n_rounds;
            IRBPP_WAVE_SYNC();
            // ---- polygon side, either form: what goes into approx_convex_segmented
            for (int form = 0; form < 2; ++form) {
                const uint8_t* const entries = form ? edump : erec;
                int32_t* const out = form ? out_dump : out_rec;
                for (int r = 0; r < n_rounds; ++r) {
                    const uint8_t* const rec = entries + (size_t)r * ROUND_BYTES;
                    bool live[PP];
                    int pv[PP], jj[PP], nn[PP], sbq[PP], prk[PP];
                    const RoundWord4 h = *(const RoundWord4*)rec;
                    if (((h.x & ROUND_FORM_DUMP) != 0u) != (form == 1)) { if (lane == 0) over = 2; }
                    if (h.x & ROUND_FORM_DUMP) round_dump_load<PP>(lane, h, big, dps, live, pv, jj, nn, sbq, prk);
                    else round_record_load<PP>(lane, rec, live, pv, jj, nn, sbq, prk);
                    for (int u = 0; u < PP; ++u) {
                        int32_t* const o = out + (size_t)r * 6 * NPOS + u * 64 + lane;
                        o[0] = live[u] ? 1 : 0; o[NPOS] = pv[u]; o[2 * NPOS] = jj[u]; o[3 * NPOS] = nn[u]; o[4 * NPOS] = sbq[u]; o[5 * NPOS] = prk[u];
                    }
                    IRBPP_WAVE_SYNC();
                }
            }
        });
    for (auto& t : lanes) t.join();
    pthread_barrier_destroy(&g_bar);
    if (over) return -over;
    if (n_rec != n_dump) return -3;
    // the dump wrote its own region only, and nothing behind the last header
    for (int w = 0; w < WAVES; ++w)
        if (w != WAVE)
            for (int i = 0; i < TRACE_WAVE_BYTES; ++i) if (big[(size_t)w * TRACE_WAVE_BYTES + i] != 0xEE) return -4;
    for (int i = TRACE_DUMP_SLOTS + CPW * TRACE_SLOT; i < TRACE_DUMP_TABLE; ++i) if (region[i] != 0xEE) return -5;
    for (int i = 0; i < ROUND_BYTES; ++i) if (edump[(size_t)n_dump * ROUND_BYTES + i] != 0xEE || erec[(size_t)n_rec * ROUND_BYTES + i] != 0xEE) return -6;
    return n_rec;
}

extern "C" {

// out[0..5] = TRACE_P, TRACE_LDS_CAP, TRACE_CAP, TRACE_SLOT, TRACE_SPILL, TRACE_SHORT
void host_round_constants(int* out) {
    out[0] = TRACE_P; out[1] = TRACE_LDS_CAP; out[2] = TRACE_CAP; out[3] = TRACE_SLOT; out[4] = TRACE_SPILL; out[5] = TRACE_SHORT;
}

// One trace chunk of cpw (64 / 32 / 16) lanes.  slot_bytes [64][TRACE_SLOT]: the lanes' LDS slots; spill_bytes [64][TRACE_SPILL];
// my_n, rk [64].  out_rec / out_dump [max_rounds][6][64 * TRACE_P]: live, pv, jj, nn, sbq, prk per round and position, from the
// RECORD and from the DUMP form; lane_plan [64][2]: the round and start position the counting pass gave each lane; sels
// [max_rounds]: the rounds' lanes.  Returns the number of rounds; negative: more than max_rounds (-1), a header of the wrong
// form (-2), the forms disagree on the number of rounds (-3), a store outside its region (-4 .. -6).
int host_round_forms(int cpw, const uint8_t* slot_bytes, const uint8_t* spill_bytes, const int* my_n, const int* rk, int max_rounds,
                     int32_t* out_rec, int32_t* out_dump, int32_t* lane_plan, uint64_t* sels) {
    if (cpw == 64) return run_forms<64>(slot_bytes, spill_bytes, my_n, rk, max_rounds, out_rec, out_dump, lane_plan, sels);
    if (cpw == 32) return run_forms<32>(slot_bytes, spill_bytes, my_n, rk, max_rounds, out_rec, out_dump, lane_plan, sels);
    if (cpw == 16) return run_forms<16>(slot_bytes, spill_bytes, my_n, rk, max_rounds, out_rec, out_dump, lane_plan, sels);
    return -100;
}

}  // extern "C"

#ifdef ROUND_DUMP_MAIN
// Stand-alone run (e.g. built with -fsanitize=address,undefined): a few constructed waves through both forms.
#include <stdio.h>
int main() {
    static uint8_t slots[64 * TRACE_SLOT], spill[64 * TRACE_SPILL];
    static int32_t a[64 * 6 * NPOS], b[64 * 6 * NPOS], plan[128];
    static uint64_t sels[64];
    int my_n[64], rk[64], bad = 0;
    uint32_t rng = 12345u;
    for (int rep = 0; rep < 40; ++rep) {
        for (int l = 0; l < 64; ++l) {
            rng = rng * 1664525u + 1013904223u;
            const int kind = (rep + l) % 7;
            my_n[l] = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? TRACE_LDS_CAP + 1 : kind == 3 && l % 16 == 0 ? TRACE_CAP : (int)((rng >> 8) % 40u);
            if (rep == 1) my_n[l] = l == 7 ? 64 * TRACE_P > TRACE_CAP ? TRACE_CAP : 64 * TRACE_P : 0;
            rk[l] = (int)(rng >> 12);
            for (int j = 0; j < TRACE_SLOT; ++j) slots[l * TRACE_SLOT + j] = (uint8_t)(rng >> (j % 24));
            for (int j = 0; j < TRACE_SPILL; ++j) spill[l * TRACE_SPILL + j] = (uint8_t)((rng >> (j % 20)) + 1u);
        }
        const int cpw = rep % 3 == 0 ? 64 : rep % 3 == 1 ? 32 : 16;
        const int n = host_round_forms(cpw, slots, spill, my_n, rk, 64, a, b, plan, sels);
        if (n < 0 || memcmp(a, b, (size_t)n * 6 * NPOS * sizeof(int32_t)) != 0) { printf("rep %d: %d\n", rep, n); ++bad; }
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
