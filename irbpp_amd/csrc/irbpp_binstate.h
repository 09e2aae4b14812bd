// irbpp_binstate.h -- what "the state of a bin" is: the ONE table irbpp_save_bins, irbpp_load_bins and irbpp_copy_bins go by, on the
// host (blob sizes, the keys a blob or a second environment is checked against) and in the kernel (irbpp_binstate.hip), which
// gets it by value.  Plain C++: compiles with g++ (tests/host/binstate_host.cpp) as well as hipcc.
//
// The rule: an array belongs to a bin's state iff a later irbpp_step / irbpp_step_cells / irbpp_heuristic_step /
// irbpp_get_action_candidates / irbpp_get_all_possible_observation / irbpp_heuristic_action / irbpp_reset_bins ON THAT BIN reads
// what an earlier call on that bin wrote there.  By that rule (DESIGN.md section 2 has the table with the readers and writers):
//   in   hm        the heightmap
//   in   queue     the item buffer
//   in   cand      the candidate keys of the last location observation: irbpp_step turns its action into a cell through them
//   in   bs        the bin's line of scalars -- cursor, episode, observed item, np.sum(naiveMask), chosen slot, counters, the episode's
//                  sums and traj_row, the trajectory row of the RUNNING episode: a copy goes on drawing its source's items
//   in   w_posz    the drop heights of the last observation: the apply kernels' posZmap[rot, lx, ly], the heuristic selection's scores
//   in   w_valid   naiveMask of the last observation as bit rows: says where w_posz is current
//   in   totals    the finished episodes' sums -- save / load only; a fork leaves the destination's alone (in_fork), or a finished
//                  episode would be counted twice
//   in   log_meta, log_z   the placement-log rows, when a log is attached: the running episode's entries
//   out  w_meta    written by the transition kernel's hand-over (split_handover) and read by the emit kernels of the SAME call only: the
//                  apply kernels and the heuristic selection take the observed item and np.sum(naiveMask) from bs (cur_item, nvalid)
//   out  w_vmask, w_img, w_imgrot, w_cand, w_round, w_nround, w_heavy, w_total, w_big   hand-over between the kernels of one observation
//   out  order     rewritten by irbpp_item_order_kernel in front of every launch that reads it
//   out  err       the environment's sticky error word, no bin's
// The capacity path (Params::wide) has the same arrays with vrow = 32 words per rotation of w_valid and up to 1024 cells per
// rotation of w_posz: the sizes below come from Params, nothing is path-specific.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "irbpp_device.h"

namespace irbpp {

constexpr int32_t BIN_BLOB_VERSION = 1;      // layout version of the table: irbpp_bin_blob_info::version

enum BinArray : int32_t {
    BA_HM = 0, BA_QUEUE, BA_CAND, BA_BS, BA_W_POSZ, BA_W_VALID, BA_TOTALS, BA_LOG_META, BA_LOG_Z, BA_COUNT
};

// One array's share of a bin: `row_bytes` is the bin's row in the State array (element size x elements, a multiple of 4: a queue of
// one item is 4 bytes); `bytes` is its room in the per-bin blob, row_bytes rounded up to 16 (the rest is written as zero), at `offset`.
// offset and bytes are multiples of 16, the segments follow each other without gaps, bytes_per_bin is their sum.
struct BinSegment { int32_t array, row_bytes, bytes, offset; };
struct BinSegTable { int32_t n, bytes_per_bin; BinSegment seg[BA_COUNT]; };

constexpr bool bin_array_in_fork(int32_t array) { return array != BA_TOTALS; }
inline const char* bin_array_name(int32_t array) {
    constexpr const char* names[BA_COUNT] = {"hm", "queue", "cand", "bs", "w_posz", "w_valid", "totals", "log_meta", "log_z"};
    return array >= 0 && array < BA_COUNT ? names[array] : "?";
}

// log_cap: State::log_cap (0: no placement log attached)
constexpr BinSegTable bin_segments(const Params& P, int32_t log_cap) {
    BinSegTable t{};
    const int32_t rows[BA_COUNT] = {
        P.Hc * 8,                   // hm        f64 [Hc]
        P.K * 4,                    // queue     i32 [K]
        P.S * 4,                    // cand      u32 [S]
        (int32_t)sizeof(BinState),  // bs
        P.R * P.AC * 8,             // w_posz    f64 [R][AC]
        P.R * P.vrow * 4,           // w_valid   u32 [R][vrow]
        4 * 8,                      // totals    f64 [4]
        log_cap * 4,                // log_meta  u32 [log_cap]
        log_cap * 8,                // log_z     f64 [log_cap]
    };
    int32_t off = 0;
    for (int32_t a = 0; a < BA_COUNT; ++a) {
        if (rows[a] <= 0) continue;
        t.seg[t.n] = BinSegment{a, rows[a], align16(rows[a]), off};
        off += t.seg[t.n].bytes;
        ++t.n;
    }
    t.bytes_per_bin = off;
    return t;
}

// FNV-1a, 64 bit, chained through `h`
constexpr uint64_t FNV_OFFSET = 0xcbf29ce484222325ull;
inline uint64_t fnv1a(const void* data, size_t bytes, uint64_t h = FNV_OFFSET) {
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < bytes; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

// Every Params field the table and the kernels' reading of a bin's rows depend on.  Not the number of bins, not global_offset /
// global_bins: a search environment of N x B bins beside a root environment of N bins has the same key.
inline uint64_t bin_geometry_key(const Params& P, int32_t log_cap) {
    const int32_t ints[] = {BIN_BLOB_VERSION, P.Hx, P.Hy, P.Ax, P.Ay, P.step, P.R, P.S, P.K, P.wide, P.vrow, log_cap};
    const double reals[] = {P.res_a, P.res_h, P.res_z, P.bin_x, P.bin_y, P.bin_z};
    return fnv1a(reals, sizeof reals, fnv1a(ints, sizeof ints));
}

// What irbpp_load_shapes / irbpp_load_sequences were given, argument array by argument array.
inline uint64_t bin_shapes_key(int32_t n_shapes, int32_t n_rot, const double* extents, const double* volumes, const int32_t* dims,
                               const int64_t* offsets, int64_t pool_len, const double* height_top, const double* height_bottom,
                               const double* mask_top, const double* mask_bottom) {
    const size_t nr = (size_t)n_shapes * (size_t)n_rot, pool = (size_t)pool_len * sizeof(double);
    uint64_t h = fnv1a(&n_shapes, sizeof n_shapes);
    h = fnv1a(&n_rot, sizeof n_rot, h);
    h = fnv1a(extents, nr * 3 * sizeof(double), h);
    h = fnv1a(volumes, (size_t)n_shapes * sizeof(double), h);
    h = fnv1a(dims, nr * 2 * sizeof(int32_t), h);
    h = fnv1a(offsets, nr * sizeof(int64_t), h);
    h = fnv1a(height_top, pool, h);
    h = fnv1a(height_bottom, pool, h);
    h = fnv1a(mask_top, pool, h);
    return fnv1a(mask_bottom, pool, h);
}
inline uint64_t bin_sequences_key(const int32_t* ids, int32_t n_traj, int32_t length) {
    uint64_t h = fnv1a(&n_traj, sizeof n_traj);
    h = fnv1a(&length, sizeof length, h);
    return fnv1a(ids, (size_t)n_traj * (size_t)length * sizeof(int32_t), h);
}
inline uint64_t bin_tables_key(uint64_t shapes_key, uint64_t sequences_key) {
    const uint64_t both[2] = {shapes_key, sequences_key};
    return fnv1a(both, sizeof both);
}

}  // namespace irbpp
