// irbpp_plan.h -- the launch plan of a transition: which kernels go out, in which order, with which grid, workgroup size,
// dynamic LDS and `mode` argument.  plan_transition() is a pure function of its arguments: no HIP runtime call, no function
// pointer, nothing read from or written to an environment -- irbpp_capi.hip executes the plan (launch_group), advances
// heavy_turn by it (launch_env) and renders it (irbpp_debug_kernel_info), so what the library says it launches is what it
// launches; tests/host/launch_plan_host.cpp compiles this header for the host and prints plans.  Every size threshold of the
// launch decision lives here, with the measurements that put it where it is.
#pragma once
#include "../../include/irbpp.h"
#include "irbpp_device.h"

namespace irbpp {

// ---------------------------------------------------------------------------------------------------------------------
// The kernels of a transition (and the two others whose dynamic-LDS limit is raised), ONCE: X(id, scope, name, threads per
// workgroup, needs the raised dynamic-LDS limit).  XS: a kernel that only exists where the specialised builds do (not under
// IRBPP_NO_SPEC).  irbpp_capi.hip expands the same list into the function pointers (kernel_registry).
// ---------------------------------------------------------------------------------------------------------------------
#define IRBPP_KERNEL_LIST(X, XS)                                    \
    X(K_ENV, , irbpp_env_kernel, 256, 1)                            \
    X(K_ENV_WIDE, , irbpp_env_kernel_wide, 256, 1)                  \
    X(K_ENV_BOX, , irbpp_env_kernel_box, 256, 1)                    \
    X(K_ENV_BOX8, , irbpp_env_kernel_box8, 256, 1)                  \
    X(K_ENV_GENERIC, , irbpp_env_kernel_generic, 256, 1)            \
    X(K_ENV_GENERIC8, , irbpp_env_kernel_generic8, 256, 1)          \
    X(K_ENV_MIXED8, , irbpp_env_kernel_mixed8, 256, 1)              \
    X(K_ENV_GENERIC_W512, wg512::, irbpp_env_kernel_generic_w512, 512, 1) \
    XS(K_ENV_S1, , irbpp_env_kernel_s1, 256, 1)                     \
    XS(K_ENV_S2, , irbpp_env_kernel_s2, 256, 1)                     \
    XS(K_ENV_S3, , irbpp_env_kernel_s3, 256, 1)                     \
    XS(K_ENV_S4, , irbpp_env_kernel_s4, 256, 1)                     \
    XS(K_ENV_S5, , irbpp_env_kernel_s5, 256, 1)                     \
    XS(K_ENV_S1_W128, wg128::, irbpp_env_kernel_s1_w128, 128, 1)    \
    XS(K_ENV_S4_W512, wg512::, irbpp_env_kernel_s4_w512, 512, 1)    \
    XS(K_ENV_S4_W512C, wg512::, irbpp_env_kernel_s4_w512c, 512, 1)  \
    X(K_CHAIN, , irbpp_env_kernel_chain, 256, 1)                    \
    XS(K_CHAIN_S1, , irbpp_env_kernel_chain_s1, 256, 1)             \
    X(K_WIDE, , irbpp_wide_kernel, 256, 1)                          \
    X(K_TRACE, , irbpp_trace_kernel, 64, 0)                         \
    X(K_TRACE_C32, , irbpp_trace_kernel_c32, 64, 0)                 \
    X(K_TRACE_C16, , irbpp_trace_kernel_c16, 64, 0)                 \
    X(K_TRACE_REFILL, , irbpp_trace_kernel_refill, 64, 0)           \
    X(K_POLYGON, , irbpp_polygon_kernel, 64, 0)                     \
    X(K_EMIT, , irbpp_emit_kernel, 256, 1)                          \
    XS(K_EMIT_S1, , irbpp_emit_kernel_s1, 256, 1)                   \
    XS(K_EMIT_S2, , irbpp_emit_kernel_s2, 256, 1)                   \
    XS(K_EMIT_S3, , irbpp_emit_kernel_s3, 256, 1)                   \
    XS(K_EMIT_S4, , irbpp_emit_kernel_s4, 256, 1)                   \
    XS(K_EMIT_S5, , irbpp_emit_kernel_s5, 256, 1)                   \
    X(K_EMIT_WAVE, , irbpp_emit_wave_kernel, 256, 1)                \
    XS(K_EMIT_WAVE_S1, , irbpp_emit_wave_kernel_s1, 256, 1)         \
    XS(K_EMIT_WAVE_S2, , irbpp_emit_wave_kernel_s2, 256, 1)         \
    XS(K_EMIT_WAVE_S5, , irbpp_emit_wave_kernel_s5, 256, 1)         \
    X(K_APPLY, , irbpp_apply_kernel, 256, 0)                        \
    X(K_APPLY_WG, , irbpp_apply_wg_kernel, 256, 0)                  \
    X(K_APPLY_CELLS, , irbpp_apply_cells_kernel, 256, 0)            \
    X(K_APPLY_CELLS_WG, , irbpp_apply_cells_wg_kernel, 256, 0)      \
    X(K_APPLY_HEUR, , irbpp_apply_heur_kernel, 256, 0)              \
    X(K_APPLY_HEUR_WG, , irbpp_apply_heur_wg_kernel, 256, 0)        \
    X(K_HEURISTIC, , irbpp_heuristic_kernel, 256, 1)                \
    X(K_ITEM_ORDER, , irbpp_item_order_kernel, 1024, 0)             \
    X(K_HULL, , irbpp_hull_kernel, 256, 1)

enum KernelId : int {
#define IRBPP_X(id, scope, name, threads, lds) id,
    IRBPP_KERNEL_LIST(IRBPP_X, IRBPP_X)
#undef IRBPP_X
    N_KERNELS
};
struct KernelInfo { const char* name; int threads; bool raise_lds; };
inline constexpr KernelInfo KERNEL_INFO[N_KERNELS] = {
#define IRBPP_X(id, scope, name, threads, lds) {#name, threads, lds != 0},
    IRBPP_KERNEL_LIST(IRBPP_X, IRBPP_X)
#undef IRBPP_X
};
constexpr const KernelInfo& kernel_info(int id) { return KERNEL_INFO[id]; }
constexpr bool is_apply_kernel(int id) { return id >= K_APPLY && id <= K_APPLY_HEUR_WG; }

// (irbpp_kernels.hip's ApplyKey and TRACE_REFILL_BATCH, which this header cannot see: irbpp_capi.hip asserts that they agree)
constexpr int PLAN_KEY_CAND = 0, PLAN_KEY_CELLS = 1, PLAN_KEY_HEUR = 2;
constexpr int PLAN_KEY_HEUR_HM = 3;         // KEY_HEUR with StepIO::heur_method 4 (HM): the scorer kernel in front of the cells apply
constexpr int PLAN_TRACE_REFILL_BATCH = 128;

constexpr int TRACE_SMALL_GRID = 8192;      // waves of a trace launch over few bins (16 or 32 candidates per wave)
constexpr int TRACE_CPW16_BINS = 0;         // launches over at most this many bins trace 16 candidates per wave ...
constexpr int TRACE_CPW32_BINS = 1024;      // ... 32 per wave (profiles/r04 session 41: +1.5 ... 1.9 % at 512 / 1024 bins, -0.3 % at 2048; 16 per wave loses everywhere)

// radix counters / sort keys of the emit routine's > S selection, behind the transition kernel's carve-up (CHAIN builds): the
// emit kernel's own e_hist region (irbpp_device.h: layout_lds)
inline int chain_extra_lds(const Params& P) {
    int npad = 64;
    while (npad < P.S) npad <<= 1;
    return align16(10 * npad > 1024 ? 10 * npad : 1024);
}
// lattice data through and through (every rotation on the block path) or box data: what the wave-per-bin emit kernel and the
// early split of the apply phase are for; a data set with list rotations (PATH_MIXED) is treated like free-form data there
inline bool all_block(const Params& P) { return P.block_b > 0 && P.block_rots == (1 << P.R) - 1; }
inline bool lattice_or_box(const Params& P) { return all_block(P) || P.box != 0; }
// ... except in what its level images look like: unions of rectangles with a few dozen candidates per bin, practically never more
// than S of them -- the wave-per-bin emit kernel's case, not the speckled free-form images the heavy-first list is for
inline bool lattice_images(const Params& P) { return P.block_b > 0 || P.box != 0; }

// waves of the largest trace grid a launch over this environment's bins can ask for (16 candidates per wave: four waves per
// bin), at most TRACE_SMALL_GRID of them beyond one per bin: State::w_big holds one scratch per wave of the grid (13 KB each:
// a 1-bin probe environment allocates 55 KB, not 112 MB)
inline int trace_grid_cap(int N) {
    const int small = 4 * N < TRACE_SMALL_GRID ? 4 * N : TRACE_SMALL_GRID;
    return N > small ? N : small;
}

// Specialised builds (irbpp_device.h): SPEC index whose compile-time constants equal this environment's Params, or 0.
inline int pick_spec(const Params& P, int tuning) {
#if defined(IRBPP_NO_SPEC) || defined(IRBPP_ABLATE)
    (void)P; (void)tuning;
    return 0;
#else
    if (tuning & (IRBPP_TUNE_NO_SPECIALISED | IRBPP_TUNE_WIDE_KERNEL | IRBPP_TUNE_NARROW_KERNEL)) return 0;
    static constexpr Params spec[N_SPECS] = {Params{}, spec_params(SPEC_KEYS[1]), spec_params(SPEC_KEYS[2]), spec_params(SPEC_KEYS[3]),
                                         spec_params(SPEC_KEYS[4]), spec_params(SPEC_KEYS[5])};
    static_assert(N_SPECS == 6, "one table entry and one kernel per SPEC_KEYS row");
    for (int i = 1; i < N_SPECS; ++i)
        if (spec_matches(P, spec[i])) return i;
    return 0;
#endif
}

// step(): the actions are applied by irbpp_apply_kernel (a wave per bin) and the transition kernel only observes
// (MODE_OBSERVE), unless the stability proxy is on (it rates the placement on the LDS tile) or the caller asks for the fused form
// -- from the launch size on at which that pays.  The apply kernel costs a launch and one pass of its dependent reads
// (~9 us at any size, 15 us with free-form footprints); inside the transition kernel the same chain is paid once per ROUND
// of workgroups (eight per CU), hidden in part behind the other workgroups' arithmetic.  Measured on the specialised builds
// (profiles/r05/s6, placement-steps/s split vs fused): BlockOut 2048 / 4096 / 6144 / 8192 / 16384 bins -4 % / 0 / +1.7 /
// +3.0 / +6.1 %; cube 4096 / 8192: 0 / +2.7 %; free-form solids at R = 8: 4096 -1.1 %, 8192 +0.3 % (BlockOut at R = 8: 0 /
// +1.6 %); the 64 x 64 heightmap (four workgroups per CU, footprints of up to 1600 cells): -2 % at two and at four rounds;
// a buffered step (K > 1: the apply phase and a float32 copy of the tile) with a WAVE per bin: -22 % / -52 % (one wave takes
// 16 dependent round trips to copy the tile) -- with a WORKGROUP per bin (irbpp_apply_wg_kernel: wave 0 applies, all four
// waves copy; no LDS tile, no overlap-test code in the kernel) it wins at every size, see profiles/r05/s25.  With a second
// group of bins on another stream the split pays a round earlier (BlockOut as two groups of 4096: 59.1 -> 60.5 M,
// profiles/r05/s10).  Hence, for online steps: lattice and box data from two rounds of workgroups on, cell lists from four
// rounds on where eight workgroups share a CU.
// (Re-measured with the observe-only lattice launch reducing the heightmap in registers, profiles/register_tile: BlockOut as one
// group, split vs fused at 2048 / 3072 / 4096 bins -3.1 % / +2.6 % / +3.0 % -- the crossover now lies between one and one and a
// half rounds.  The threshold stays at two rounds: one run per point, and tests/test_launch_plan_host.py pins it.)
inline bool split_apply(const Params& P, int tuning, int n) {
    if (P.stability != 0 || (tuning & IRBPP_TUNE_FUSED_APPLY)) return false;
    if (tuning & IRBPP_TUNE_SPLIT_APPLY) return true;
    if (P.K > 1) return true;                 // buffered: the workgroup-per-bin form (apply + order observation), at every size
    const int per_cu = (160 * 1024) / (P.lds_bytes > 0 ? P.lds_bytes : 1);
    if (per_cu < 8) return false;
    const bool lists = !lattice_or_box(P);
    return n >= (lists ? 4 : 2) * 256 * 8;
}

// The transition kernel is compiled once per overlap path (lattice blocks, solid boxes, generic cell lists), with and
// without the 64-VGPR cap that makes eight workgroups per CU resident, plus one build that decides at run time.
inline int pick_env_kernel(const Params& P, int t) {
    const bool lds_allows_8 = 8 * P.lds_bytes <= 160 * 1024;
    // Generic path where the tile is so large that at most four 256-thread workgroups fit a CU's LDS (the 64 x 64 heightmap:
    // 40 KB per bin): 512-thread workgroups, eight waves on one tile (irbpp::wg512, the second pass of irbpp_kernels.hip)
    const bool generic = P.block_b == 0 && !P.box;
    const bool mixed = P.block_b > 0 && !all_block(P);
    const int spec = pick_spec(P, t);
#if !defined(IRBPP_NO_SPEC) && !defined(IRBPP_ABLATE)
    if (generic && (t & IRBPP_TUNE_NARROW_KERNEL) && (t & IRBPP_TUNE_WG512) && spec_matches(P, spec_params(SPEC_KEYS[4])))
        return K_ENV_S4_W512C;      // (A/B: under the 64-VGPR cap)
#endif
    const bool wg512 = generic && !(t & (IRBPP_TUNE_NO_WG512 | IRBPP_TUNE_WIDE_KERNEL | IRBPP_TUNE_NARROW_KERNEL)) &&
                       ((t & IRBPP_TUNE_WG512) || 5 * P.lds_bytes > 160 * 1024);
    // (under the 64-VGPR cap four such workgroups share a CU instead of three: level at 2048 bins, +10 % at 8192, profiles/r05/s30)
    if (wg512 && spec == 4) return P.N >= 4096 ? K_ENV_S4_W512C : K_ENV_S4_W512;
    if (wg512 && (spec == 0 || (t & IRBPP_TUNE_WG512))) return K_ENV_GENERIC_W512;
    if ((t & IRBPP_TUNE_WG128) && spec == 1) return K_ENV_S1_W128;        // (A/B: two waves per bin)
    switch (spec) {            // (a key fixes the overlap path: block_b and box are pinned fields)
        case 1: return K_ENV_S1;
        case 2: return K_ENV_S2;
        case 3: return K_ENV_S3;
        case 4: return K_ENV_S4;
        case 5: return K_ENV_S5;
        default: break;
    }
    if (mixed) return (t & IRBPP_TUNE_WIDE_KERNEL) ? K_ENV_WIDE : K_ENV_MIXED8;
    if (P.block_b > 0) return ((t & IRBPP_TUNE_WIDE_KERNEL) || 6 * P.lds_bytes > 150 * 1024) ? K_ENV_WIDE : K_ENV;
    if (P.box) {
        if (t & IRBPP_TUNE_WIDE_KERNEL) return K_ENV_BOX;
        return ((t & IRBPP_TUNE_NARROW_KERNEL) || lds_allows_8) ? K_ENV_BOX8 : K_ENV_BOX;
    }
    // generic path: the build under the 64-VGPR cap where the LDS lets an eighth workgroup onto the CU (general 15.1 vs
    // 14.9 M steps/s, blockout at R = 8 20.4 vs 20.1 M with the blocked and pipelined loop; before it the seven-wave
    // build was ahead, 12.9 vs 12.2 M); a 64 x 64 heightmap (40 KB, four workgroups) gains nothing from the cap
    if (t & IRBPP_TUNE_WIDE_KERNEL) return K_ENV_GENERIC;
    return ((t & IRBPP_TUNE_NARROW_KERNEL) || lds_allows_8) ? K_ENV_GENERIC8 : K_ENV_GENERIC;
}

// Border following: candidates per wave and grid of a launch over n bins.  A bin averages a few dozen candidate starts; at
// full width (thousands of bins) 64 per wave fill every SIMD and fewer, shorter-lived waves only add scheduling overhead
// (measured at 4096 bins: 28.3 / 26.8 / 24.3 M steps/s for 64 / 32 / 16); a launch over few bins leaves SIMDs idle, and a
// wave lasts as long as the longest of its borders, so there the candidates are spread over more waves.
inline int pick_trace_cpw(int t, int n) {
    if (t & IRBPP_TUNE_TRACE_CPW64) return 64;
    if (t & IRBPP_TUNE_TRACE_CPW32) return 32;
    if (t & IRBPP_TUNE_TRACE_CPW16) return 16;
    if (t & IRBPP_TUNE_TRACE_REFILL) return PLAN_TRACE_REFILL_BATCH;
    // (lane refill -- a wave owns a batch of 128 candidates and hands a lane the next one as borders close, trace_refill_body --
    // is OPT-IN: measured slower at every size, profiles/r06/LOG.md session 2: 8192 BlockOut bins 54.9 -> 51.4 M as one group,
    // 63.8 -> 59.0 M as two, the kernel 36.2 -> 46.0 us.  The chip has as many lane slots as a launch has candidates, so a
    // refilled lane's work is taken from another wave, not from idleness, and one wave then pays every refill's latencies in turn)
    return n <= TRACE_CPW16_BINS ? 16 : (n <= TRACE_CPW32_BINS ? 32 : 64);
}

// One kernel per observation (OPT-IN, IRBPP_TUNE_CHAIN): the bin's own workgroup finishes its observation (CHAIN builds of the
// transition kernel: contour stage and candidate rows in LDS, no trace / polygon / emit launches).  Built for launches of up to
// ~2048 bins, where a step is a chain of launch and drain latencies whatever the number of bins, and measured SLOWER there
// (profiles/r06/LOG.md session 6, placement-steps/s one kernel vs four): a buffered placement at 512 / 1024 / 2048 bins 8.1 vs
// 9.0 / 12.8 vs 16.3 / 16.5 vs 25.9 M, BlockOut online at 1024 / 2048 bins 14.4 vs 18.7 / 18.0 vs 29.7 M, free-form solids at
// 1024 bins 3.2 vs 8.7 M; only the Cube set gains (26.7 vs 24.4 M at 1024 bins).  A bin's observation is ~25 borders to follow
// and approximate: inside its own workgroup that is one serial latency chain per bin on a CU with nobody else to issue,
// while the split kernels spread the borders of ALL bins over every SIMD of the chip; the launch boundaries they pay
// (~3 us each) are the smaller price.
inline bool chain_launch(const Params& P, int t) {
    if (!(t & IRBPP_TUNE_CHAIN) || P.stability != 0) return false;
    if (t & (IRBPP_TUNE_TRACE_CPW64 | IRBPP_TUNE_TRACE_CPW32 | IRBPP_TUNE_TRACE_CPW16 | IRBPP_TUNE_TRACE_REFILL | IRBPP_TUNE_INLINE_POLYGON |
             IRBPP_TUNE_BLOCK_EMIT | IRBPP_TUNE_WAVE_EMIT | IRBPP_TUNE_SPLIT_APPLY | IRBPP_TUNE_GRAPH | IRBPP_TUNE_WG512 | IRBPP_TUNE_NARROW_KERNEL))
        return false;                                          // (a caller that forces a shape of the split pipeline gets the split pipeline)
    if (P.lds_bytes > 32 * 1024) return false;            // (the 64 x 64 heightmap: 512-thread workgroups on a 40 KB tile, not this)
    return true;
}

struct Launch { int kernel, grid, block, lds, mode; };
constexpr int LDS_WIDE_LAYOUT = -1;     // Launch::lds of irbpp_wide_kernel: wide_layout(P).bytes (irbpp_wide.hip), filled in by the executor
enum ObsRows : int { ROWS_NONE = 0, ROWS_TRACK = 1, ROWS_FORGET = 2 };
struct Plan {
    Launch launch[8];
    int n_launches;
    // what the executor puts into StepIO / Params, and what the environment keeps
    int use_order;         // StepIO::use_order: the item-order kernel is the plan's first launch
    int heavy_first;       // the emit grid serves the heavy-first list: env->heavy_turn flips once the launches have gone out
    int heavy_turn;        // StepIO::heavy_turn (-1: none)
    int inline_polygon;    // the trace launch gets Params::round_cap = 0 (and there is no polygon launch)
    int obs_rows;          // a registered observation buffer: ROWS_TRACK hand its per-bin row counts to the kernels (StepIO::obs_rows),
                           // ROWS_FORGET mark them unknown (the launch writes rows the counts do not describe)
};

// The launches of one transition over n launch slots (all bins, or the `listed` ones of a reset), in order.
//   tuning          irbpp_config::tuning                       key             PLAN_KEY_*: where a step's placement comes from
//   listed          a reset of the bins of StepIO::bin_list
//   registered_obs  StepIO::obs is a registered observation buffer (irbpp_register_obs_buffer)
//   heavy_turn      the environment's State::w_heavy list of the next observing launch
//   item_order      the data set launches its online steps grouped by observed item per die (irbpp_load_shapes)
// key != PLAN_KEY_CAND (irbpp_step_cells / irbpp_heuristic_step): always the apply kernel followed by MODE_OBSERVE, whatever the size.
inline Plan plan_transition(const Params& P, int tuning, int mode, int n, int key, bool listed, bool registered_obs, int heavy_turn,
                            bool item_order) {
    Plan plan{};
    plan.heavy_turn = -1;
    auto add = [&plan](int kernel, int grid, int lds, int mode_arg) {
        plan.launch[plan.n_launches++] = Launch{kernel, grid, kernel_info(kernel).threads, lds, mode_arg};
    };
    if (mode == MODE_STEP && item_order && n == P.N) {
        add(K_ITEM_ORDER, 1, 0, mode);
        plan.use_order = 1;
    }
    const bool observes = mode == MODE_CANDS || ((mode == MODE_RESET || mode == MODE_STEP) && P.K == 1);
    // reset_specific writes a row per LISTED bin and a buffered environment's step / reset write the order
    // observation: through a registered pointer either leaves the per-bin row counts meaningless
    if (registered_obs) plan.obs_rows = (observes && !(mode == MODE_RESET && listed)) ? ROWS_TRACK : ROWS_FORGET;
    // The apply phase of a split step over n launch slots: a wave per bin, or (buffered environments below 2048 bins) a workgroup per
    // bin; `key` says where the placements' cells come from (ApplyKey: candidate rows, the caller's cells, the heuristic's choice).
    // irbpp_heuristic_step's selection is fused into the placing wave (irbpp_apply_heur_kernel) for MINZ / DBLF / FIRSTFIT (as a kernel
    // of its own in front of the cell apply it measured slower at every size, DESIGN.md "Placing at grid cells"); HM keeps the
    // recomputing scorer (it needs the heightmap window sums): it writes the triples to env->heur_cells, which
    // irbpp_apply_cells_kernel reads behind it on the same stream.  The scorer indexes bins by workgroup, without block_off: a
    // heuristic step always covers the whole environment (launch_env refuses any other grid for KEY_HEUR).
    auto add_apply = [&](int k) {
        if (k == PLAN_KEY_HEUR_HM) {
            add(K_HEURISTIC, P.N, P.lds_bytes_full, mode);
            k = PLAN_KEY_CELLS;
        }
        // a buffered step: a workgroup per bin at launches of fewer than 2048 bins (a wave per bin leaves most of the chip
        // to one dependent chain per CU there: 15.7 vs 15.3 M at 1024 bins), a wave per bin from there on (every bin resident
        // at once: 8192 bins as two groups 50.6 -> 55.2 M, 4096 bins 40.0 -> 41.6 M; profiles/r05/s27)
        const bool wg = P.K > 1 && n < 2048;
        const int kernel = k == PLAN_KEY_CELLS ? (wg ? K_APPLY_CELLS_WG : K_APPLY_CELLS)
                         : k == PLAN_KEY_HEUR ? (wg ? K_APPLY_HEUR_WG : K_APPLY_HEUR) : (wg ? K_APPLY_WG : K_APPLY);
        add(kernel, wg ? n : (n + 3) / 4, 0, mode);
    };
    if (P.wide) {                     // irbpp_wide.hip: [the geometry-free apply kernel,] then ONE kernel per observation
        if (mode == MODE_STEP) {
            add_apply(key);
            if (P.K > 1) return plan;
        }
        add(K_WIDE, n, LDS_WIDE_LAYOUT, mode == MODE_STEP ? MODE_OBSERVE : mode);
        return plan;
    }
    // split pipeline: a location observation is finished by the trace kernel (one wave per 64 candidate starts of
    // the launch's flat list) and the emit kernel (one workgroup per bin), on the same stream
    const bool chain = observes && mode != MODE_POSSIBLE && chain_launch(P, tuning);
    const bool split = P.split && observes && !chain;
    // expensive bins first in the emit kernel: free-form level images only (lattice and box data never get there), not for a
    // listed reset (its observation rows go by list position)
    const bool heavy_first = split && P.heavy_cap > 0 && !lattice_images(P) && !listed && !(tuning & IRBPP_TUNE_NO_HEAVY_FIRST);
    plan.heavy_first = heavy_first ? 1 : 0;
    if (heavy_first) plan.heavy_turn = heavy_turn;
    const int spec = pick_spec(P, tuning);
    if (chain && !(mode == MODE_STEP && P.K > 1)) {
        // (a buffered step is the apply kernel below: it observes nothing)
        add(spec == 1 ? K_CHAIN_S1 : K_CHAIN, n, P.lds_bytes + chain_extra_lds(P), mode);
        return plan;
    }
    int env_mode = mode;
    if (mode == MODE_STEP && (key != PLAN_KEY_CAND || split_apply(P, tuning, n))) {
        add_apply(key);
        env_mode = MODE_OBSERVE;         // (a buffered step ends with the apply kernel: it wrote the order observation)
    }
    if (!(env_mode == MODE_OBSERVE && P.K > 1)) add(pick_env_kernel(P, tuning), n, P.lds_bytes, env_mode);
    if (!split) return plan;
    // the grid covers an average of up to 64 candidates per bin and strides over the chunks beyond that
    // one trace wave per 64 candidates a bin may average, two polygon waves per bin; the kernels stride over anything
    // beyond (half / a third of either grid with striding measured -4 ... -9 %)
    const int cpw = pick_trace_cpw(tuning, n), pgrid = 2 * n;
    // (IRBPP_TUNE_INLINE_POLYGON: every trace wave runs approxPolyDP on the borders it followed itself -- the path a full
    // record list takes -- and no polygon kernel is launched.  Measured at 1024 / 2048 / 4096 bins: 11.8 / 20.2 / 28.8 M
    // steps/s against 13.9 / - / 31.1 M: the approximation stretches the slowest trace waves.  For the parity tests.)
    plan.inline_polygon = (tuning & IRBPP_TUNE_INLINE_POLYGON) ? 1 : 0;
    int tgrid = cpw > 64 ? (n * 64 + cpw - 1) / cpw : n * (64 / cpw);
    if (tgrid > trace_grid_cap(P.N)) tgrid = trace_grid_cap(P.N);      // (w_big holds one scratch per wave of the grid)
    add(cpw > 64 ? K_TRACE_REFILL : cpw == 64 ? K_TRACE : (cpw == 32 ? K_TRACE_C32 : K_TRACE_C16), tgrid, 0, mode);
    if (!plan.inline_polygon) add(K_POLYGON, pgrid, 0, mode);
    // lattice and box data (practically never more than S candidates per bin): a wave per bin, four bins per workgroup
    // -- from 2048 bins on: a launch over 1024 bins is one such workgroup per CU, 2.6 % slower than a workgroup per bin (profiles/r05/s7)
    const bool wave_emit = lattice_images(P) && !heavy_first && !(tuning & IRBPP_TUNE_BLOCK_EMIT) &&
                           (n >= 2048 || (tuning & IRBPP_TUNE_WAVE_EMIT));
    int emit = wave_emit ? K_EMIT_WAVE : K_EMIT;
    switch (spec) {
        case 1: emit = wave_emit ? K_EMIT_WAVE_S1 : K_EMIT_S1; break;
        case 2: emit = wave_emit ? K_EMIT_WAVE_S2 : K_EMIT_S2; break;
        case 3: emit = K_EMIT_S3; break;
        case 4: emit = K_EMIT_S4; break;
        case 5: emit = wave_emit ? K_EMIT_WAVE_S5 : K_EMIT_S5; break;
        default: break;
    }
    add(emit, wave_emit ? (n + 3) / 4 : n + (heavy_first ? P.heavy_cap : 0), P.emit_lds_bytes, mode);
    return plan;
}

}  // namespace irbpp
