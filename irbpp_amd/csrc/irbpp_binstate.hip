// irbpp_binstate.hip -- save, restore and fork bins: the rows of irbpp_binstate.h's segment table copied between bins and a blob
// (irbpp_save_bins, irbpp_load_bins) or between bins, of one environment or two (irbpp_copy_bins).  A plain streaming copy, off the
// step's path: one 256-thread workgroup per (source, destination) pair, 16 bytes per thread and trip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irbpp.h"
#include "irbpp_binstate.h"

namespace irbpp {

enum BinCopyMode : int { BINS_TO_BLOB = 0, BLOB_TO_BINS = 1, BINS_TO_BINS = 2 };
constexpr int BINSTATE_THREADS = 256;

__device__ __forceinline__ uint8_t* bin_array_base(const State& S, int array) {
    switch (array) {
        case BA_HM: return (uint8_t*)S.hm;
        case BA_QUEUE: return (uint8_t*)S.queue;
        case BA_CAND: return (uint8_t*)S.cand;
        case BA_BS: return (uint8_t*)S.bs;
        case BA_W_POSZ: return (uint8_t*)S.w_posz;
        case BA_W_VALID: return (uint8_t*)S.w_valid;
        case BA_TOTALS: return (uint8_t*)S.totals;
        case BA_LOG_META: return (uint8_t*)S.log_meta;
        case BA_LOG_Z: return (uint8_t*)S.log_z;
        default: return nullptr;
    }
}

// Pair i = blockIdx.x: source bin src_bins[i] (or blob row i) -> destination bin dst_bins[i] (or blob row i).  An index outside its
// environment's bins makes the pair a no-op and raises IRBPP_DEVERR_BAD_BIN in the destination environment's error word (saving:
// the environment's own).  n_src / n_dst: bins of the two environments.
template <int MODE>
__global__ __launch_bounds__(BINSTATE_THREADS) void irbpp_binstate_kernel(const BinSegTable tab, const State src, const State dst,
                                                                          const int32_t* __restrict__ src_bins,
                                                                          const int32_t* __restrict__ dst_bins, uint8_t* blob,
                                                                          const int32_t n_src, const int32_t n_dst, const int32_t same_env) {
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int s = MODE == BLOB_TO_BINS ? 0 : src_bins[i];
    const int d = MODE == BINS_TO_BLOB ? 0 : dst_bins[i];
    const bool bad = (MODE != BLOB_TO_BINS && (s < 0 || s >= n_src)) || (MODE != BINS_TO_BLOB && (d < 0 || d >= n_dst));
    if (bad) {                                       // (workgroup-uniform)
        if (tid == 0) atomicOr(dst.err, IRBPP_DEVERR_BAD_BIN);
        return;
    }
    if (MODE == BINS_TO_BINS && same_env && s == d) return;         // a bin paired with itself
    uint8_t* const row = blob + (size_t)i * (size_t)tab.bytes_per_bin;
    for (int k = 0; k < tab.n; ++k) {
        const BinSegment g = tab.seg[k];
        if (MODE == BINS_TO_BINS && !bin_array_in_fork(g.array)) continue;
        const uint8_t* sp = MODE == BLOB_TO_BINS ? row + g.offset : bin_array_base(src, g.array) + (size_t)s * (size_t)g.row_bytes;
        uint8_t* dp = MODE == BINS_TO_BLOB ? row + g.offset : bin_array_base(dst, g.array) + (size_t)d * (size_t)g.row_bytes;
        if ((((uintptr_t)sp | (uintptr_t)dp | (uintptr_t)g.row_bytes) & 15u) == 0) {
            const uint4* s4 = (const uint4*)sp;
            uint4* d4 = (uint4*)dp;
            const int n4 = g.row_bytes >> 4;
            for (int e = tid; e < n4; e += BINSTATE_THREADS) d4[e] = s4[e];
        } else {                                     // a row that is no multiple of 16 bytes (a queue of one item, an odd S): dwords
            const uint32_t* s1 = (const uint32_t*)sp;
            uint32_t* d1 = (uint32_t*)dp;
            const int n1 = g.row_bytes >> 2;
            for (int e = tid; e < n1; e += BINSTATE_THREADS) d1[e] = s1[e];
            if (MODE == BINS_TO_BLOB)                // the blob's padding up to the next 16 bytes
                for (int e = n1 + tid; e < (g.bytes >> 2); e += BINSTATE_THREADS) d1[e] = 0u;
        }
    }
}

}  // namespace irbpp
