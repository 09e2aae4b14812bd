// irbpp_itemgen_device.h -- the item streams of irbpp_itemgen.h, drawn by a wave on the device.
//
// The same numbers as the host generator (and so as numpy's legacy RandomState and the reference's random item creators):
// init_genrand seeding, the 624-word regeneration, tempering, and RandomState.randint(0, n) = words masked with the
// smallest 2^k - 1 >= n - 1 and rejected while above n - 1, no word at all for n == 1; two stages (name, then member of
// that name's list) when the creator has groups, one stage otherwise.
//
// A wave owns a stream.  Its 624 key words lie in LDS while it works:
//   * regeneration: word i becomes k[(i + 397) % 624] ^ f(k[i], k[i + 1]).  In 64-word chunks taken in rising order, with
//     every lane loading before any lane stores, each load sees exactly what the serial loop sees: k[i] and k[i + 1] are
//     old (k[i + 1] is this chunk's or a later one's), k[i + 397] for i < 227 lies in a later chunk (old), and
//     k[i - 227] for i >= 227 lies at least 163 words back, in a chunk that is finished (new).  Word 623 needs the new
//     k[0] and goes last, alone.  (The three ranges [0,227), [227,454), [454,623) of the serial code need no separate
//     treatment: a chunk that straddles 227 or 454 still reads only finished or untouched words.)
//   * tempering: per chunk, in registers, as the selection reads the words.
//   * selection, one stage: one mask for the whole stream, so the accepted words of a chunk are a ballot and an item's
//     place in the output is a prefix count.
//   * selection, two stages: the member mask depends on the name just drawn, so the chunk's words are walked by a
//     wave-uniform state machine: the next accepted word at or after the cursor is the lowest set bit of a ballot.
//
// Compiles with g++ as well (tests/host/itemgen_host.cpp: 64 threads in lockstep, every cross-lane operation an exchange
// between barriers), like contours_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef IRBPP_ITEMGEN_SYNC      // lanes talk through LDS: program order within the wave, and no compiler motion across
#define IRBPP_ITEMGEN_SYNC()                                  \
    do {                                                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
    } while (0)
#endif

namespace irbpp {

constexpr int MT_N = 624, MT_M = 397;

// what all streams of a generator share (device memory)
struct ItemGenTables {
    int32_t n_groups;             // 0: one stage over members
    int32_t n_members;
    const int32_t* offsets;       // [n_groups + 1] into members
    const int32_t* members;
    const uint32_t* group_mask;   // [n_groups] rejection mask of a draw among group g's members
    uint32_t mask0;               // rejection mask of the first stage (names, or all members when there are no groups)
};

__host__ __device__ __forceinline__ uint32_t randint_mask(uint32_t rng) {       // smallest 2^k - 1 >= rng
    uint32_t mask = rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    return mask;
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// init_genrand: serial by nature, one thread per stream
__device__ inline void mt_seed_serial(uint32_t* key, uint32_t seed) {
    for (int i = 0; i < MT_N; ++i) {
        key[i] = seed;
        seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)i + 1u;
    }
}

__device__ __forceinline__ uint32_t mt_twist(uint32_t hi, uint32_t lo, uint32_t far) {
    const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// the 624-word regeneration of mt19937_next by one wave; k: the stream's key words in LDS
__device__ inline void mt_regenerate_wave(int lane, uint32_t* k) {
    IRBPP_ITEMGEN_SYNC();
    for (int base = 0; base < MT_N - 1; base += 64) {
        const int i = base + lane;
        const bool live = i < MT_N - 1;
        uint32_t v = 0u;
        if (live) v = mt_twist(k[i], k[i + 1], k[i < MT_N - MT_M ? i + MT_M : i + MT_M - MT_N]);
        IRBPP_ITEMGEN_SYNC();                  // every lane has loaded ...
        if (live) k[i] = v;
        IRBPP_ITEMGEN_SYNC();                  // ... and stored before the next chunk loads
    }
    if (lane == 0) k[MT_N - 1] = mt_twist(k[MT_N - 1], k[0], k[MT_M - 1]);
    IRBPP_ITEMGEN_SYNC();
}

// Append `count` items of one stream.  k: its key words in LDS, pos: the next word (624 = regenerate first); every lane
// calls with the same arguments.  sink(j, id) is called by ONE lane for the j-th item of this call, 0 <= j < count.
// Returns the new pos.
template <class Sink>
__device__ inline int itemgen_draw_wave(int lane, uint32_t* k, int pos, const ItemGenTables& G, int count, Sink& sink) {
    const bool two = G.n_groups > 0;
    const uint32_t rng0 = (uint32_t)(two ? G.n_groups : G.n_members) - 1u;
    const uint32_t mask0 = G.mask0;
    int done = 0;
    if (!two && rng0 == 0u) {                                 // choice of a one-element list: no word is consumed
        const int32_t id = G.members[0];
        for (int j = lane; j < count; j += 64) sink(j, id);
        return pos;
    }
    // two stages: the state between two words
    int stage = 0, lo = 0;
    uint32_t rng1 = 0u, mask1 = 0u;
    while (done < count) {
        if (two && stage == 0 && rng0 == 0u) {                // one name only: nothing drawn for it
            lo = G.offsets[0];
            rng1 = (uint32_t)(G.offsets[1] - lo) - 1u;
            mask1 = G.group_mask[0];
            stage = 1;
        }
        if (two && stage == 1 && rng1 == 0u) {                // a one-member list: nothing drawn for it
            if (lane == 0) sink(done, G.members[lo]);
            ++done;
            stage = 0;
            continue;
        }
        if (pos == MT_N) {
            mt_regenerate_wave(lane, k);
            pos = 0;
        }
        const int at = pos + lane;
        const bool live = at < MT_N;
        const uint32_t w = live ? mt_temper(k[at]) : 0u;
        const int avail = MT_N - pos < 64 ? MT_N - pos : 64;   // words of this chunk
        if (!two) {
            const uint32_t v = w & mask0;
            const bool ok = live && v <= rng0;
            const unsigned long long bal = __ballot(ok);
            const int before = __popcll(bal & ((1ull << lane) - 1ull));
            const int want = count - done;
            if (ok && before < want) sink(done + before, G.members[v]);
            const int got = __popcll(bal);
            if (got >= want) {                                 // the call ends at its last accepted word
                const unsigned long long last = __ballot(ok && before == want - 1);
                pos += __ffsll((long long)last);
                done = count;
            } else {
                pos += avail;
                done += got;
            }
            continue;
        }
        int p = 0;                                             // cursor into the chunk
        while (done < count) {
            if (stage == 0 && rng0 == 0u) {
                lo = G.offsets[0];
                rng1 = (uint32_t)(G.offsets[1] - lo) - 1u;
                mask1 = G.group_mask[0];
                stage = 1;
            }
            if (stage == 1 && rng1 == 0u) {
                if (lane == 0) sink(done, G.members[lo]);
                ++done;
                stage = 0;
                continue;
            }
            const uint32_t rng = stage == 0 ? rng0 : rng1;
            const uint32_t v = w & (stage == 0 ? mask0 : mask1);
            unsigned long long bal = __ballot(live && v <= rng);
            bal = p < 64 ? bal & (~0ull << p) : 0ull;
            if (bal == 0ull) { p = avail; break; }             // the rest of the chunk is rejected
            const int l = __ffsll((long long)bal) - 1;
            const uint32_t pick = (uint32_t)__shfl((int)v, l);
            p = l + 1;
            if (stage == 0) {
                lo = G.offsets[pick];
                rng1 = (uint32_t)(G.offsets[pick + 1] - lo) - 1u;
                mask1 = G.group_mask[pick];
                stage = 1;
            } else {
                if (lane == 0) sink(done, G.members[lo + (int)pick]);
                ++done;
                stage = 0;
            }
        }
        pos += p;
    }
    return pos;
}

}  // namespace irbpp
