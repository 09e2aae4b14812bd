// irbpp_rounds.h -- polygon rounds: how the borders a trace wave has followed reach approx_convex_segmented.
//
// A trace wave ends a chunk with up to 64 closed borders (lane l: my_n points, the first TRACE_LDS_CAP of them in its LDS
// slot, the rest in the wave's spill bytes in global scratch).  They are served in ROUNDS of 64 * TRACE_P contour
// positions, borders packed back to back (greedy, in lane order, optionally in two classes: next_round / count_rounds).
// Every round is one entry of an XCD's list in State::w_round and one work item of irbpp_polygon_kernel.  An entry
// starts with a header of ROUND_HDR bytes; its word 0 says which of two forms the entry has:
//   RECORD (bit 0 clear)  the trace wave has gathered the round's positions itself and the entry holds them:
//                         [points | border length | border start][64 * TRACE_P] bytes, then the vertex-row words.  A serial
//                         chain of cross-lane operations per round, paid by the wave that sets the trace kernel's duration.
//   DUMP   (bit 0 set)    the trace wave has written its slots as they lie and a 64-entry lane table ONCE per chunk into its
//                         own region of State::w_big (wide coalesced stores), and the entry is the header alone: the wave of
//                         the polygon kernel that takes the round rebuilds the positions (round_positions, the very routine
//                         the RECORD form runs in the trace wave) with the point bytes read from the dump.
// Everything here compiles for the device and, under the lockstep emulation of tests/host/round_dump_host.cpp, for the host.
#pragma once
#include "contours_device.h"
#include "irbpp_device.h"

namespace irbpp {

#ifndef IRBPP_TRACE_SHORT
#define IRBPP_TRACE_SHORT 0
#endif
constexpr int TRACE_P = IRBPP_TRACE_P;                                // contour points per lane and polygon round
constexpr int TRACE_CAP = 128;                                        // points of a border the wave-parallel path takes
constexpr int TRACE_LDS_CAP = 56, TRACE_SLOT = TRACE_LDS_CAP + 4;     // of which in the lane's slot in LDS (15 dwords: odd stride); the rest
constexpr int TRACE_SPILL = TRACE_CAP - TRACE_LDS_CAP;                //   in global scratch (a border of more than 56 points: one in ~10^3)
constexpr int TRACE_SHORT = IRBPP_TRACE_SHORT;                        // borders of up to this many points get rounds of their own, ahead of the
                                                                      // long ones (0 = one class: measured 27.46 vs 27.25 M steps/s for 8)
static_assert(TRACE_CAP <= 64 * TRACE_P, "a border must fit one polygon round");
static_assert(ROUND_POINTS == 64 * TRACE_P, "a round record holds one polygon round");
static_assert(TRACE_CAP <= 255 && 64 * TRACE_P <= 256, "border length and start position travel as bytes");
constexpr int TRACE_BIG = 768;                                        // point capacity of the sequential redo (global scratch)
constexpr int TRACE_BIG_BYTES = 6 * TRACE_BIG + 64;                   // scratch of the sequential redo: points, polygon, stack, 16-bit image
// per wave of the trace grid (State::w_big): the redo's scratch, the lanes' spill bytes, the dump of the wave's FIRST chunk
// (its slots, then the lane table: {n | start << 8 | round << 16, vertex-row index} per lane)
constexpr int TRACE_SPILL_OFF = TRACE_BIG_BYTES;
constexpr int TRACE_DUMP_SLOTS = TRACE_SPILL_OFF + 64 * TRACE_SPILL;
constexpr int TRACE_DUMP_TABLE = TRACE_DUMP_SLOTS + 64 * TRACE_SLOT;
constexpr int TRACE_WAVE_BYTES = TRACE_DUMP_TABLE + 64 * 8;
static_assert(TRACE_DUMP_SLOTS % 16 == 0 && TRACE_DUMP_TABLE % 16 == 0 && TRACE_WAVE_BYTES % 16 == 0 && ROUND_BYTES % 16 == 0,
              "dump and headers are written as 16-byte words");
// header word 0 of a round entry
constexpr uint32_t ROUND_FORM_DUMP = 1u, ROUND_SPILLED = 2u;          // (round index within its chunk: bits 8..15)

struct alignas(16) RoundWord4 { uint32_t x, y, z, w; };               // one 16-byte load / store
struct alignas(8) RoundWord2 { uint32_t x, y; };

// wave64 inclusive scans on the DPP network (no LDS round trips): prefix inside each row of 16 lanes by four
// row shifts, then the row totals are carried over with the two row broadcasts.  Operands are >= 0, so the
// 0 that a shift brings in from outside the row is the identity of both sum and max.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_shift(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false); }
__device__ __forceinline__ int wave_inclusive_sum(int v) {
    v += dpp_shift<0x111, 0xF>(v);           // row_shr:1
    v += dpp_shift<0x112, 0xF>(v);           // row_shr:2
    v += dpp_shift<0x114, 0xF>(v);           // row_shr:4
    v += dpp_shift<0x118, 0xF>(v);           // row_shr:8
    v += dpp_shift<0x142, 0xA>(v);           // row_bcast15 into rows 1 and 3
    v += dpp_shift<0x143, 0xC>(v);           // row_bcast31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int wave_inclusive_max(int v) {
    v = imax(v, dpp_shift<0x111, 0xF>(v));
    v = imax(v, dpp_shift<0x112, 0xF>(v));
    v = imax(v, dpp_shift<0x114, 0xF>(v));
    v = imax(v, dpp_shift<0x118, 0xF>(v));
    v = imax(v, dpp_shift<0x142, 0xA>(v));
    v = imax(v, dpp_shift<0x143, 0xC>(v));
    return v;
}

// The next round of the greedy partition: lanes with `left` points still to serve, class `cls` (0: borders of up to
// TRACE_SHORT points, 1: everything left).  Returns the lanes of the round (0: none left in this class); per lane wn =
// points it still has in this class, excl - base = position of its first point if it is in the round.
__device__ __forceinline__ unsigned long long next_round(int cls, int left, int& wn, int& excl, int& base) {
    wn = (cls == 0 ? left <= TRACE_SHORT : true) ? left : 0;
    const int incl = wave_inclusive_sum(wn);
    excl = incl - wn;
    if (__builtin_amdgcn_readlane(incl, 63) == 0) return 0ull;
    const unsigned long long todo = __ballot(wn > 0);
    base = __builtin_amdgcn_readlane(excl, __ffsll((long long)todo) - 1);
    return __ballot(wn > 0 && incl - base <= 64 * TRACE_P);
}

// The counting pass: rounds of a wave's borders.  Per lane with my_n > 0: the round it was assigned and the position of its
// first point there; lane i < rounds additionally gets round i's lanes in my_sel.
__device__ __forceinline__ int count_rounds(int lane, int my_n, int& my_round, int& my_start, unsigned long long& my_sel) {
    int n_rounds = 0, left = my_n;
    my_round = my_start = 0;
    my_sel = 0ull;
    for (int cls = 0; cls < 2; ++cls)
        for (;;) {
            int wn, excl, base = 0;
            const unsigned long long sel = next_round(cls, left, wn, excl, base);
            if (sel == 0ull) break;
            if ((sel >> lane) & 1ull) { left = 0; my_round = n_rounds; my_start = excl - base; }
            if (lane == n_rounds) my_sel = sel;
            ++n_rounds;
        }
    return n_rounds;
}

// The positions of one round, as approx_convex_segmented takes them.  sel: the round's lanes; per lane of sel: wn = points
// of its border, start = position of its first point, rk = its vertex-row index.  Which border does the point at position
// q = u * 64 + lane belong to: border lanes drop their id at the position of their first point, a running maximum over
// the positions spreads it.  slots: the 64 lanes' point bytes, TRACE_SLOT apart (LDS in the trace wave, the dump in the
// polygon wave); spill: [64][TRACE_SPILL] points TRACE_LDS_CAP.. of the lanes' borders, read only if `spilled`;
// dps: 64 * PP words of LDS private to this wave.  owner[u]: the lane whose border position u belongs to (0 if none).
template <int PP>
__device__ __forceinline__ void round_positions(int lane, unsigned long long sel, int wn, int start, int rk, const uint8_t* slots,
                                                const uint8_t* spill, bool spilled, uint32_t* dps, bool (&live)[PP], int (&pv)[PP],
                                                int (&jj)[PP], int (&nn)[PP], int (&sbq)[PP], int (&prk)[PP], int (&owner)[PP]) {
    constexpr int LCAP = TRACE_LDS_CAP;
#pragma unroll
    for (int u = 0; u < PP; ++u) dps[u * 64 + lane] = 0u;
    IRBPP_WAVE_SYNC();
    if ((sel >> lane) & 1ull) dps[start] = (uint32_t)lane + 1u;
    IRBPP_WAVE_SYNC();
    int mark[PP];
#pragma unroll
    for (int u = 0; u < PP; ++u) mark[u] = (int)dps[u * 64 + lane];
    IRBPP_WAVE_SYNC();
    int carry = 0;
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int run = imax(wave_inclusive_max(mark[u]), carry);
        carry = __builtin_amdgcn_readlane(run, 63);
        const int own = run - 1;                                      // lane that traced this position's border
        const int on = own >= 0 ? own : 0;
        const int ns = __shfl(wn | (start << 8), on);                 // (one gather for both: wn <= 128, start < 256)
        nn[u] = ns & 255;
        sbq[u] = ns >> 8;
        prk[u] = __shfl(rk, on);
        live[u] = own >= 0 && u * 64 + lane < sbq[u] + nn[u];
        owner[u] = on;
        jj[u] = u * 64 + lane - sbq[u];
        if (!live[u]) { nn[u] = 1; sbq[u] = 0; jj[u] = 0; }
        pv[u] = live[u] ? (int)slots[on * TRACE_SLOT + (jj[u] < LCAP ? jj[u] : LCAP)] : 0;
        if (spilled && live[u] && jj[u] >= LCAP) pv[u] = (int)spill[on * TRACE_SPILL + jj[u] - LCAP];
    }
}

// RECORD form, trace side: the round's positions into its entry
template <int PP>
__device__ __forceinline__ void round_record_store(int lane, uint8_t* entry, const bool (&live)[PP], const int (&pv)[PP],
                                                   const int (&nn)[PP], const int (&sbq)[PP], const int (&prk)[PP]) {
    if (lane == 0) *(uint32_t*)entry = 0u;
    uint8_t* const rec = entry + ROUND_HDR;                           // [pts | n | sb][64 * PP] bytes, then rk words
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int q = u * 64 + lane;
        rec[q] = (uint8_t)pv[u];
        rec[64 * PP + q] = (uint8_t)(live[u] ? nn[u] : 0);             // 0: no point at this position
        rec[2 * 64 * PP + q] = (uint8_t)sbq[u];
        ((uint32_t*)(rec + 3 * 64 * PP))[q] = (uint32_t)prk[u];
    }
}
// ... an entry without points (a reserved entry of a full list, whose borders the trace wave approximated itself)
template <int PP>
__device__ __forceinline__ void round_record_store_empty(int lane, uint8_t* entry) {
    if (lane == 0) *(uint32_t*)entry = 0u;
#pragma unroll
    for (int u = 0; u < PP; ++u) entry[ROUND_HDR + 64 * PP + u * 64 + lane] = 0;
}
// RECORD form, polygon side
template <int PP>
__device__ __forceinline__ void round_record_load(int lane, const uint8_t* entry, bool (&live)[PP], int (&pv)[PP], int (&jj)[PP],
                                                  int (&nn)[PP], int (&sbq)[PP], int (&prk)[PP]) {
    const uint8_t* const rec = entry + ROUND_HDR;
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int q = u * 64 + lane;
        pv[u] = rec[q];
        nn[u] = rec[64 * PP + q];
        sbq[u] = rec[2 * 64 * PP + q];
        prk[u] = (int)((const uint32_t*)(rec + 3 * 64 * PP))[q];
        live[u] = nn[u] > 0;
        jj[u] = q - sbq[u];
        if (!live[u]) { nn[u] = 1; sbq[u] = 0; jj[u] = 0; pv[u] = 0; }
    }
}

// DUMP form, trace side: the wave's slots as they lie (CPW * TRACE_SLOT bytes of LDS) and its lane table into the wave's
// region of State::w_big, then one header per round into the rounds' entries (entry0: the first of n_rounds reserved ones).
template <int CPW>
__device__ __forceinline__ void round_dump_store(int lane, uint8_t* region, const uint8_t* slots, int my_n, int rk, int my_round,
                                                 int my_start) {
    constexpr int WORDS = CPW * TRACE_SLOT / 16;
    static_assert(CPW * TRACE_SLOT % 16 == 0, "the slots are dumped as 16-byte words");
    RoundWord4* const dst = (RoundWord4*)(region + TRACE_DUMP_SLOTS);
    const RoundWord4* const src = (const RoundWord4*)slots;
#pragma unroll
    for (int i = 0; i < (WORDS + 63) / 64; ++i)
        if (i * 64 + lane < WORDS) dst[i * 64 + lane] = src[i * 64 + lane];
    RoundWord2 e;
    e.x = (uint32_t)my_n | ((uint32_t)my_start << 8) | ((uint32_t)my_round << 16);
    e.y = (uint32_t)rk;
    ((RoundWord2*)(region + TRACE_DUMP_TABLE))[lane] = e;
}
__device__ __forceinline__ void round_headers_store(int lane, uint8_t* entry0, int n_rounds, int wave, bool spilled,
                                                    unsigned long long my_sel) {
    if (lane < n_rounds) {
        RoundWord4 h;
        h.x = ROUND_FORM_DUMP | (spilled ? ROUND_SPILLED : 0u) | ((uint32_t)lane << 8);
        h.y = (uint32_t)wave;
        h.z = (uint32_t)my_sel;
        h.w = (uint32_t)(my_sel >> 32);
        *(RoundWord4*)(entry0 + (size_t)lane * ROUND_BYTES) = h;
    }
}
// DUMP form, polygon side: the positions of the round whose header is h (uniform), rebuilt from the dump in w_big
template <int PP>
__device__ __forceinline__ void round_dump_load(int lane, const RoundWord4& h, const uint8_t* w_big, uint32_t* dps, bool (&live)[PP],
                                                int (&pv)[PP], int (&jj)[PP], int (&nn)[PP], int (&sbq)[PP], int (&prk)[PP]) {
    const uint8_t* const region = w_big + (size_t)h.y * TRACE_WAVE_BYTES;
    const RoundWord2 e = ((const RoundWord2*)(region + TRACE_DUMP_TABLE))[lane];
    const unsigned long long sel = (unsigned long long)h.z | ((unsigned long long)h.w << 32);
    int owner[PP];
    round_positions<PP>(lane, sel, (int)(e.x & 255u), (int)((e.x >> 8) & 255u), (int)e.y, region + TRACE_DUMP_SLOTS,
                        region + TRACE_SPILL_OFF, (h.x & ROUND_SPILLED) != 0u, dps, live, pv, jj, nn, sbq, prk, owner);
}

}  // namespace irbpp
