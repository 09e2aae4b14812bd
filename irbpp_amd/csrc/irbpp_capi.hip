// irbpp_capi.hip -- host side of libirbpp_hip.so: the C ABI declared in include/irbpp.h.
//
// Owns the per-device state in HBM (heightmaps, item queues, candidate keys, counters), packs
// the shotInfo tables and trajectories once, and launches the transition kernel on the
// caller's stream.  No torch types, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/irbpp.h"
#include "irbpp_device.h"
#include "irbpp_rotalias.h"
#include "irbpp_kernels.hip"     // single translation unit: kernels + host ABI
#include "irbpp_wide.hip"         // action grids of 17 .. 32 cells a side: the capacity path
#include "irbpp_replay.hip"
#include "irbpp_replay_pool.hip"    // the N memories sampled and updated as one pooled memory (irbpp_replay_pool_sample / _gather / _update)
#include "irbpp_itemgen.hip"        // the item streams of irbpp_itemgen.h drawn on the device (irbpp_itemgen_dev_*, irbpp_stream_refill)
#include "irbpp_c51.hip"            // the distributional head around the network (irbpp_categorical_act, irbpp_categorical_target)
#include "irbpp_dueling.hip"        // the same from the network's logits: dueling combine + softmax fused in (irbpp_dueling_act, irbpp_dueling_target)
#include "irbpp_dueling_loss.hip"   // the loss that carries the gradient, forward and backward from the logits (irbpp_dueling_loss, irbpp_dueling_loss_backward)
#include "irbpp_optim.hip"          // the optimiser step: gradient-norm clip and Adam over all parameter tensors, two launches (irbpp_clipped_adam_step)
#include "irbpp_streams.hip"        // the four noisy layers of the value and advantage streams in front of the dueling head (irbpp_noisy_weights, irbpp_streams_act)
#include "irbpp_streams_mfma.hip"   // the same launch with the advantage stream on the matrix cores, the same bits (irbpp_streams_act_mfma)
#include "irbpp_shapefeat.hip"      // the shape branch in front of the network: sampled points to shape features (irbpp_shape_features)
#include "irbpp_shapefeat_grad.hip" // the same with a gradient: the arg record and the backward routed through it (irbpp_shape_features_arg, _backward)
#include "irbpp_streams_grad.hip"   // the backward of the streams' four noisy layers: dx, dxg and the sixteen parameter gradients (irbpp_streams_backward)
#include "irbpp_embed.hip"          // the embedding stage: heightmap CNN, candidate rows, masked mean (irbpp_embed)
#include "irbpp_embed_mfma.hip"     // the same stage with the three per-row layers on the matrix cores, the same bits (irbpp_embed_mfma)
#include "irbpp_order_embed.hip"   // the order network's embedding stage: CNN, k buffered items, one attention layer, mean (irbpp_order_embed)
#include "irbpp_order_embed_mfma.hip"   // the same stage with its eight linear layers on the matrix cores, the same bits (irbpp_order_embed_mfma)
#include "irbpp_metrics.hip"        // the trainer's episode metrics (irbpp_set_episode_window)
#include "irbpp_itemgen.h"
#include "irbpp_plan.h"             // which kernels a transition launches: the registry of kernels and plan_transition
#include "irbpp_binstate.hip"       // save, restore and fork bins (irbpp_save_bins, irbpp_load_bins, irbpp_copy_bins) by irbpp_binstate.h's table

using namespace irbpp;

struct irbpp_env {
    irbpp_config cfg;
    Params P;
    Tables T;
    State S;
    bool shapes_loaded = false, seq_loaded = false, was_reset = false;
    bool transition_launched = false;      // launch_env went out at least once (irbpp_debug_round_cap is refused from then on)
    int32_t round_cap_alloc = 0;           // Params::round_cap as irbpp_create computed it: what State::w_round was allocated for
    int32_t* round_snap = nullptr;         // irbpp_debug_round_counts: State::w_nround as the trace kernel left it (null: not recorded)
    bool item_order = false;               // launch slots grouped by observed item, one contiguous range per XCD (generic path)
    long long* phase_cycles = nullptr;
    int32_t* auto_actions = nullptr;       // irbpp_set_auto_policy
    int heavy_turn = 0;                    // State::w_heavy list of the next observing launch
    int32_t* err_mirror = nullptr;         // irbpp_step_out::err_dev of the last step: every error bit is ORed into it as it is raised
    std::vector<std::pair<const float*, int32_t*>> obs_buffers;   // irbpp_register_obs_buffer: buffer -> rows per bin
    std::vector<hipEvent_t> timing;        // tooling: event pairs around irbpp_env_kernel (ring)
    size_t timing_next = 0, timing_used = 0;
    int timing_every = 1, timing_phase = 0;   // events go around every timing_every-th transition only
    std::vector<void*> allocs;
    char kernel_names[256] = {0};          // irbpp_debug_kernel_info
    // small launches replayed as HIP graphs (launch_env): the launches of a transition, captured once per distinct
    // argument set on a stream of the library's own and replayed on the caller's
    struct GraphEntry { std::vector<uint8_t> key; hipGraphExec_t exec; hipGraph_t graph; uint64_t used; };
    std::vector<GraphEntry> graphs;
    hipStream_t cap_stream = nullptr;
    uint64_t graph_clock = 0, graph_replays = 0;
    int obs_epoch = 0;                     // bumped by every (un)registration of an observation buffer: part of a graph's key
    irbpp_episode_window window{};         // irbpp_set_episode_window (window.window == 0: none attached)
    int32_t* heur_cells = nullptr;         // [N][3] irbpp_heuristic_step: the cells a scorer kernel chose, read by irbpp_apply_cells_kernel
    bool grids_current = false;            // w_posz / w_valid of EVERY bin are those of the item its next step places, on its present heightmap
    uint64_t shapes_key = 0, seq_key = 0;  // FNV-1a of what irbpp_load_shapes / irbpp_load_sequences were given (irbpp_bin_blob_info::tables_key)
};

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return IRBPP_ERR_HIP;     \
    } while (0)

namespace {

static_assert(PLAN_KEY_CAND == KEY_CAND && PLAN_KEY_CELLS == KEY_CELLS && PLAN_KEY_HEUR == KEY_HEUR &&
              PLAN_TRACE_REFILL_BATCH == TRACE_REFILL_BATCH, "irbpp_plan.h restates these constants of irbpp_kernels.hip");
// the function behind every KernelId of irbpp_plan.h's list (nullptr: a specialised build this library was compiled without)
#define IRBPP_X(id, scope, name, threads, lds) (const void*)scope name,
#ifdef IRBPP_NO_SPEC
#define IRBPP_XS(id, scope, name, threads, lds) nullptr,
#else
#define IRBPP_XS IRBPP_X
#endif
const void* const kernel_registry[N_KERNELS] = {IRBPP_KERNEL_LIST(IRBPP_X, IRBPP_XS)};
#undef IRBPP_X
#undef IRBPP_XS

template <typename T>
int dev_alloc(irbpp_env* env, T** out, size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, count * sizeof(T) > 0 ? count * sizeof(T) : sizeof(T)) != hipSuccess) return IRBPP_ERR_NOMEM;
    if (hipMemset(p, 0, count * sizeof(T)) != hipSuccess) { hipFree(p); return IRBPP_ERR_HIP; }
    env->allocs.push_back(p);
    *out = (T*)p;
    return IRBPP_OK;
}

template <typename T>
int dev_upload(irbpp_env* env, const T** out, const T* host, size_t count) {
    T* p = nullptr;
    int rc = dev_alloc(env, &p, count);
    if (rc != IRBPP_OK) return rc;
    if (count && hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return IRBPP_ERR_HIP;
    *out = p;
    return IRBPP_OK;
}

inline double round6_host(double x) { return nearbyint(x * 1e6) / 1e6; }   // np.round(x, 6)
// dynamic-LDS carve-up of the transition kernel: irbpp::layout_lds (irbpp_device.h, shared with the specialised builds)
void layout_lds_host(Params& P) {
    int pad = 0;
#ifdef IRBPP_ABLATE
    if (const char* e = getenv("IRBPP_LDS_PAD")) pad = atoi(e);   // tooling build only: caps workgroups per CU
#endif
    irbpp::layout_lds(P, pad);
}

// The dynamic-LDS limit is an attribute of the kernel on the device, not of an environment: always raise it to the
// CU's 160 KiB, so that a later, smaller environment cannot lower it under one that is still alive.
int raise_lds_limits() {
    for (int id = 0; id < N_KERNELS; ++id)
        if (kernel_info(id).raise_lds && kernel_registry[id] != nullptr &&
            hipFuncSetAttribute(kernel_registry[id], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return IRBPP_ERR_HIP;
    return IRBPP_OK;
}

}  // namespace

extern "C" {

const char* irbpp_status_string(int status) {
    switch (status) {
        case IRBPP_OK: return "ok";
        case IRBPP_ERR_ARG: return "bad argument or unsupported configuration";
        case IRBPP_ERR_HIP: return "HIP runtime error";
        case IRBPP_ERR_STATE: return "call out of order (load shapes and sequences, reset, then step)";
        case IRBPP_ERR_DEVICE: return "device-side error word set";
        case IRBPP_ERR_NOMEM: return "out of device memory";
        default: return "unknown status";
    }
}

int irbpp_version(void) { return 610; }      // 61x: device item generator (irbpp_itemgen_dev_*, irbpp_stream_refill); 3xx: irbpp_config::tuning / item_stream, unregister / invalidate_obs_buffer, stream ring, itemgen; 5xx: source hash, overlap path, specialised builds

#ifndef IRBPP_SOURCE_HASH
#define IRBPP_SOURCE_HASH "unstamped"
#endif
// (the marker lets build.py find the stamp in the file without loading the library)
const char* irbpp_source_hash(void) { static const char stamp[] = "irbpp-source-hash:" IRBPP_SOURCE_HASH; return stamp + 18; }

int irbpp_create(const irbpp_config* cfg, irbpp_env** out) {
    if (!cfg || !out) return IRBPP_ERR_ARG;
    if (cfg->num_bins > MAX_BINS) return IRBPP_ERR_ARG;
    if (cfg->num_bins < 1 || cfg->n_rot < 1 || cfg->n_rot > 8 || cfg->selected < 1 || cfg->selected > 1024 ||
        cfg->buffer_size < 1 || cfg->buffer_size > 16)
        return IRBPP_ERR_ARG;
    if (!(cfg->resolution_a > 0) || !(cfg->resolution_h > 0) || !(cfg->resolution_z > 0)) return IRBPP_ERR_ARG;
    irbpp_env* env = new (std::nothrow) irbpp_env();
    if (!env) return IRBPP_ERR_NOMEM;
    env->cfg = *cfg;
    memset(&env->T, 0, sizeof(Tables));
    memset(&env->S, 0, sizeof(State));
    Params& P = env->P;
    memset(&P, 0, sizeof(Params));
    P.N = cfg->num_bins;
    P.R = cfg->n_rot;
    P.S = cfg->selected;
    P.K = cfg->buffer_size;
    P.res_a = cfg->resolution_a;
    P.res_h = cfg->resolution_h;
    P.res_z = cfg->resolution_z;
    P.inv_res_z = 1.0 / cfg->resolution_z;
    for (int k = 0; k < 32; ++k) P.txs[k] = round6_host((double)k * cfg->resolution_a);
    P.bin_x = cfg->bin[0];
    P.bin_y = cfg->bin[1];
    P.bin_z = cfg->bin[2];
    P.bin_vol = cfg->bin[0] * cfg->bin[1] * cfg->bin[2];             // np.prod(bin_dimension)
    P.scale_z = cfg->scale_z;
    P.ibin_z = round6_host(cfg->bin[2] * cfg->scale_z);              // Interface.py:39-40
    // Space.__init__ (space.py:19-24)
    P.step = (int)(cfg->resolution_a / cfg->resolution_h);
    if ((double)P.step != cfg->resolution_a / cfg->resolution_h || P.step < 1) { delete env; return IRBPP_ERR_ARG; }
    P.Hx = (int)ceil(cfg->bin[0] / cfg->resolution_h);
    P.Hy = (int)ceil(cfg->bin[1] / cfg->resolution_h);
    P.Ax = (int)ceil(cfg->bin[0] / cfg->resolution_a);
    P.Ay = (int)ceil(cfg->bin[1] / cfg->resolution_a);
    P.Hc = P.Hx * P.Hy;
    P.AC = P.Ax * P.Ay;
    if (P.Ax > 32 || P.Ay > 32 || P.Ax < 1 || P.Ay < 1 || P.Hc > 128 * 128) { delete env; return IRBPP_ERR_ARG; }
    // height levels (cvTools.py:78): a placement height never exceeds bin_z, so floor(bin_z / resolution_z) levels cover it.  The
    // tuned pipeline codes them in 6 bits (level + 32), the capacity path in 8 (TUNED_MAX_LEVELS, MAX_LEVELS)
    const double levels = floor(cfg->bin[2] / cfg->resolution_z + 1e-9);
    if (!(levels <= (double)MAX_LEVELS)) { delete env; return IRBPP_ERR_ARG; }
    const bool deep = levels > (double)TUNED_MAX_LEVELS;
    // 17 .. 32 action cells a side (resolutionA = 0.01), or more than 31 height levels (resolutionZ = 0.005 on the 0.30 m bin): the
    // capacity path of irbpp_wide.hip -- one kernel per observation, every stage in the bin's workgroup; no stability proxy, no item
    // streams' extras are affected, the stage-level tooling entry points (possible_position, heuristic_action, convex_hull_actions)
    // answer IRBPP_ERR_ARG
    P.wide = (P.Ax > 16 || P.Ay > 16 || deep) ? 1 : 0;
    P.vrow = P.wide ? WIDE_VROW : 16;
    if (P.wide && (P.Hc > 64 * 64 || cfg->stability != 0)) { delete env; return IRBPP_ERR_ARG; }
    if (P.Hx != P.Ax * P.step || P.Hy != P.Ay * P.step) { delete env; return IRBPP_ERR_ARG; }   // phase-plane tile layout
    P.traj_start = cfg->traj_start;
    P.goff = cfg->global_offset;
    P.gbins = cfg->global_bins > 0 ? cfg->global_bins : cfg->num_bins;
    P.obs_len1 = 5 * P.S + 9 + P.Hc;
    P.obs_len0 = P.K > 1 ? P.K + P.Hc : P.obs_len1;
#ifdef IRBPP_ABLATE
    if (const char* rep = getenv("IRBPP_DEBUG_REPEAT")) P.dbg_repeat = atoi(rep);   // tooling build only (tools/build_variant.sh)
#endif
    P.split = 1;                                            // transition -> trace -> emit kernels
    P.stability = cfg->stability < 0 ? 0 : (cfg->stability > 2 ? 2 : cfg->stability);
    P.rect = (cfg->tuning & IRBPP_TUNE_RECT) ? 1 : 0;
    P.lds_tile = (cfg->tuning & IRBPP_TUNE_LDS_TILE) ? 1 : 0;
    P.round_dump = (cfg->tuning & IRBPP_TUNE_TRACE_PACK) ? 0 : 1;
    P.wimg = P.R * (deep ? (((int)levels + 33 + 31) & ~31) : 64);   // level + 32 for levels up to `levels`, in whole words of 32 codes
    P.seg_cap = P.wide ? 64 : 2 * ((P.N + NXCD - 1) / NXCD) * P.R * P.AC;      // (the wide path hands nothing over between kernels)
    P.round_cap = P.wide ? 16 : (P.N / NXCD + 64) * 16;
    env->round_cap_alloc = P.round_cap;
    layout_lds_host(P);                 // redone by irbpp_load_shapes if the block path applies
    if (P.lds_bytes_full > 160 * 1024 || (P.wide && wide_layout(P).bytes > 160 * 1024)) { delete env; return IRBPP_ERR_ARG; }

    if (hipSetDevice(cfg->device) != hipSuccess) { delete env; return IRBPP_ERR_HIP; }
    if (raise_lds_limits() != IRBPP_OK) { delete env; return IRBPP_ERR_HIP; }
    State& S = env->S;
    const size_t N = (size_t)P.N;
    int rc = IRBPP_OK;
#define ALLOC(field, count) if (rc == IRBPP_OK) rc = dev_alloc(env, &S.field, (count))
    ALLOC(hm, N * P.Hc);
    ALLOC(queue, N * P.K);
    ALLOC(cand, N * P.S);
    ALLOC(bs, N);
    ALLOC(totals, N * 4);
    ALLOC(order, N);
    ALLOC(err, 1);
    ALLOC(w_posz, N * P.R * P.AC);
    ALLOC(w_valid, N * P.R * P.vrow);
    ALLOC(w_vmask, N * P.R * 16);
    ALLOC(w_meta, N * WMETA);
    ALLOC(w_img, P.wide ? 16 : N * P.wimg * 16);
    ALLOC(w_imgrot, P.wide ? 16 : N * P.wimg);
    ALLOC(w_cand, (size_t)NXCD * P.seg_cap);
    ALLOC(w_big, P.wide ? N * wide_scratch_bytes(P) : (size_t)trace_grid_cap(P.N) * TRACE_WAVE_BYTES);   // one scratch per wave of the trace grid (wide: per bin)
    ALLOC(w_total, NXCD * XCD_STRIDE);
    ALLOC(w_nround, NXCD * XCD_STRIDE);
    ALLOC(w_round, (size_t)NXCD * P.round_cap * ROUND_BYTES);
    P.heavy_cap = P.N >= 64 ? P.N / 8 : 0;                 // expensive bins the emit kernel serves first (generic data only, see launch_group)
    P.heavy_thr = (P.S * 3) / 5;                          // (with the run-level start filter a > S bin has >= 0.70 S starts + isolated pixels, 99 % of the others < 0.65 S)
    ALLOC(w_heavy, 2 * (size_t)(XCD_STRIDE + P.heavy_cap));
#undef ALLOC
    if (rc == IRBPP_OK) rc = dev_alloc(env, &env->heur_cells, N * 3);
    if (rc != IRBPP_OK) { irbpp_destroy(env); return rc; }
    {   // identity launch order until an ordering pass writes another one
        std::vector<int32_t> ident(N);
        for (size_t i = 0; i < N; ++i) ident[i] = (int32_t)i;
        if (hipMemcpy(S.order, ident.data(), N * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { irbpp_destroy(env); return IRBPP_ERR_HIP; }
    }
    *out = env;
    return IRBPP_OK;
}

int irbpp_destroy(irbpp_env* env) {
    if (!env) return IRBPP_OK;
    hipSetDevice(env->cfg.device);
    for (void* p : env->allocs) hipFree(p);
    for (hipEvent_t e : env->timing) hipEventDestroy(e);
    for (auto& g : env->graphs) { if (g.exec) hipGraphExecDestroy(g.exec); if (g.graph) hipGraphDestroy(g.graph); }
    if (env->cap_stream) hipStreamDestroy(env->cap_stream);
    delete env;
    return IRBPP_OK;
}

int irbpp_load_shapes(irbpp_env* env, int32_t n_shapes, const double* extents, const double* volumes,
                      const int32_t* dims, const int64_t* offsets, int64_t pool_len,
                      const double* height_top, const double* height_bottom,
                      const double* mask_top, const double* mask_bottom) {
    if (!env || n_shapes < 1 || !extents || !volumes || !dims || !offsets || pool_len < 1 || !height_top ||
        !height_bottom || !mask_top || !mask_bottom)
        return IRBPP_ERR_ARG;
    if (env->shapes_loaded) return IRBPP_ERR_STATE;
    const Params& P = env->P;
    HIP_TRY(hipSetDevice(env->cfg.device));
    const int R = P.R;
    std::vector<ShapeRot> sr((size_t)n_shapes * R);
    std::vector<Cell> bcell, tcell, blkcell;
    std::vector<GCell> gcell;
    for (int64_t i = 0; i < (int64_t)n_shapes * R; ++i) {               // table shapes and offsets first: the scans below trust them
        const int64_t fx = dims[i * 2], fy = dims[i * 2 + 1];
        if (fx < 1 || fy < 1 || fx > 4096 || fy > 4096 || offsets[i] < 0 || offsets[i] + fx * fy > pool_len) return IRBPP_ERR_ARG;
    }
    env->shapes_key = bin_shapes_key(n_shapes, R, extents, volumes, dims, offsets, pool_len, height_top, height_bottom, mask_top, mask_bottom);
    // Block path: the largest b (multiple of step, <= 8) such that every footprint of the dataset is a
    // union of b x b tiles that are fully masked out or fully masked in with one bottom height -- decided per ROTATION:
    // if every rotation qualifies the data set is pure lattice data (BlockOut at R = 4); if only some do (BlockOut at the
    // README's eight rotations: the four lattice rotations, not the 45-degree ones) those take the block loop and the
    // others their cell lists, in one kernel (PATH_MIXED); b = the largest size with the most rotations.
    int block_b = 0, block_rots = 0;
    if (!(env->cfg.tuning & IRBPP_TUNE_NO_BLOCK_PATH) && !P.wide) {
        int best_count = 0;
        for (int b = 8; b >= 2; --b) {
            if (b % P.step != 0 || (P.Hx - b) % P.step != 0 || (P.Hy - b) % P.step != 0) continue;
            int mask = 0;
            for (int r = 0; r < R; ++r) {
                bool ok = true;
                for (int64_t k = 0; k < n_shapes && ok; ++k) {
                    const int64_t i = k * R + r;
                    const int fx = dims[i * 2], fy = dims[i * 2 + 1];
                    if (fx % b != 0 || fy % b != 0) { ok = false; break; }
                    for (int ti = 0; ti < fx / b && ok; ++ti)
                        for (int tj = 0; tj < fy / b && ok; ++tj) {
                            const int64_t e0 = offsets[i] + (int64_t)(ti * b) * fy + tj * b;
                            for (int u = 0; u < b && ok; ++u)
                                for (int v = 0; v < b && ok; ++v) {
                                    const int64_t e = offsets[i] + (int64_t)(ti * b + u) * fy + tj * b + v;
                                    if (mask_bottom[e] != mask_bottom[e0] ||
                                        (mask_bottom[e0] != 0.0 && height_bottom[e] != height_bottom[e0]))
                                        ok = false;
                                }
                        }
                }
                if (ok) mask |= 1 << r;
            }
            const int count = __builtin_popcount((unsigned)mask);
            if (count > best_count) { best_count = count; block_b = b; block_rots = mask; }
            if (count == R) break;
        }
        // (a single lattice rotation among many list rotations is not worth the block-max grid; IRBPP_TUNE_NO_MIXED_PATH: A/B)
        if (block_rots != (1 << R) - 1 && (2 * best_count < R || (env->cfg.tuning & IRBPP_TUNE_NO_MIXED_PATH))) { block_b = 0; block_rots = 0; }
    }
    const bool mixed = block_b > 0 && block_rots != (1 << R) - 1;
    // Box path: every footprint of the dataset is a solid box -- maskB the rectangle [0,bx) x [0,by), one bottom height
    // over it (the Cube dataset: bottom 0, the ceil-fuzz row of space.py:105 masked out).  max over the window of (H - c)
    // is (max H) - c exactly, and the max over a rectangle is separable: row maxima first, then column maxima.
    bool box = block_b == 0 && !(env->cfg.tuning & IRBPP_TUNE_NO_BOX_PATH) && !P.wide;
    for (int64_t i = 0; i < (int64_t)n_shapes * R && box; ++i) {
        const int fx = dims[i * 2], fy = dims[i * 2 + 1];
        const double* mb = mask_bottom + offsets[i];
        const double* hb = height_bottom + offsets[i];
        int bx = 0, by = 0;
        while (bx < fx && mb[(int64_t)bx * fy] != 0.0) ++bx;
        while (by < fy && mb[by] != 0.0) ++by;
        if (bx == 0 || by == 0) { box = false; break; }
        for (int ci = 0; ci < fx && box; ++ci)
            for (int cj = 0; cj < fy && box; ++cj) {
                const bool in = ci < bx && cj < by;
                if ((mb[(int64_t)ci * fy + cj] != 0.0) != in || (in && hb[(int64_t)ci * fy + cj] != hb[0])) box = false;
            }
    }
    const int mb_h = block_b ? (P.Hx - block_b) / P.step + 1 : 0, mb_w = block_b ? (P.Hy - block_b) / P.step + 1 : 0;
    for (int k = 0; k < n_shapes; ++k) {
        for (int r = 0; r < R; ++r) {
            const size_t i = (size_t)k * R + r;
            ShapeRot& s = sr[i];
            memset(&s, 0, sizeof(s));
            s.ext_x = extents[i * 3 + 0];
            s.ext_y = extents[i * 3 + 1];
            s.ext_z = extents[i * 3 + 2];
            const double bx = round6_host(s.ext_x), by = round6_host(s.ext_y);     // space.py:104
            s.ext_z_r = round6_host(s.ext_z);
            s.fx = (int32_t)ceil(bx / P.res_h);                                   // space.py:105
            s.fy = (int32_t)ceil(by / P.res_h);
            s.ax = (int32_t)ceil(bx / P.res_a);                                   // space.py:106
            s.ay = (int32_t)ceil(by / P.res_a);
            const int64_t off = offsets[i];
            if (s.fx != dims[i * 2] || s.fy != dims[i * 2 + 1]) return IRBPP_ERR_ARG;   // table shape must match
            if (s.fx < 1 || s.fy < 1 || s.fx > s.ax * P.step || s.fy > s.ay * P.step) return IRBPP_ERR_ARG;
            if (off < 0 || off + (int64_t)s.fx * s.fy > pool_len) return IRBPP_ERR_ARG;
            // compact lists of the masked-in cells, row-major
            s.ob = (int32_t)bcell.size();
            s.ot = (int32_t)tcell.size();
            for (int ci = 0; ci < s.fx; ++ci) {
                for (int cj = 0; cj < s.fy; ++cj) {
                    const int64_t e = off + (int64_t)ci * s.fy + cj;
                    const double mt = mask_top[e], mb = mask_bottom[e];
                    if ((mt != 0.0 && mt != 1.0) || (mb != 0.0 && mb != 1.0)) return IRBPP_ERR_ARG;
                    const int32_t ij = ci | (cj << 16);
                    if (mb != 0.0) bcell.push_back(Cell{height_bottom[e], ij, ci * s.fy + cj});
                    else s.has_out = 1;
                    if (mt != 0.0) tcell.push_back(Cell{height_top[e], ij, ci * s.fy + cj});
                }
            }
            s.nb = (int32_t)bcell.size() - s.ob;
            s.nt = (int32_t)tcell.size() - s.ot;
            {   // centre of mass of the solid between bottom and top table (columns hit from both sides)
                double mass = 0.0, mx = 0.0, my = 0.0;
                for (int ci = 0; ci < s.fx; ++ci)
                    for (int cj = 0; cj < s.fy; ++cj) {
                        const int64_t e = off + (int64_t)ci * s.fy + cj;
                        if (mask_top[e] != 0.0 && mask_bottom[e] != 0.0) {
                            const double w = height_top[e] - height_bottom[e] > 0.0 ? height_top[e] - height_bottom[e] : 0.0;
                            mass += w; mx += w * (ci + 0.5); my += w * (cj + 0.5);
                        }
                    }
                s.com_x = mass > 0.0 ? mx / mass : 0.5 * s.fx;
                s.com_y = mass > 0.0 ? my / mass : 0.5 * s.fy;
            }
            s.oblk = (int32_t)blkcell.size();
            if (block_b && ((block_rots >> r) & 1))
                for (int ti = 0; ti < s.fx / block_b; ++ti)
                    for (int tj = 0; tj < s.fy / block_b; ++tj) {
                        const int64_t e0 = off + (int64_t)(ti * block_b) * s.fy + tj * block_b;
                        if (mask_bottom[e0] != 0.0)
                            blkcell.push_back(Cell{height_bottom[e0], (ti * block_b / P.step) * mb_w + tj * block_b / P.step, 0});
                    }
            s.nblk = (int32_t)blkcell.size() - s.oblk;
            // generic path: the masked-in bottom cells again, as (height, byte offset in the LDS tile relative to the
            // action cell's own entry): cell (ci, cj) of an item on action cell (X, Y) is heightmap cell
            // (X*step + ci, Y*step + cj) = plane (ci % step, cj % step), entry (X + ci / step) * Ay + Y + cj / step
            if (!box && (!block_b || mixed))
                for (int e = 0; e < s.nb; ++e) {
                    const Cell& c = bcell[s.ob + e];
                    const int ci = c.ij & 0xFFFF, cj = c.ij >> 16;
                    const int off = ((ci % P.step) * P.step + cj % P.step) * P.AC + (ci / P.step) * P.Ay + cj / P.step;
                    gcell.push_back(GCell{c.v, off * 8, 0});
                }
            if (box) {
                while (s.bx < s.fx && mask_bottom[off + (int64_t)s.bx * s.fy] != 0.0) ++s.bx;
                while (s.by < s.fy && mask_bottom[off + s.by] != 0.0) ++s.by;
                s.bc = height_bottom[off];
            }
            if (s.nb == 0 && !s.has_out) return IRBPP_ERR_ARG;
        }
    }
    // Rotations of one shape whose observation inputs are bit-identical (symmetric polycubes: a fifth of BlockOut's rotations):
    // the later one reuses the earlier one's overlap results and vertex bits (irbpp_rotalias.h).  Identity on the
    // capacity path and under IRBPP_TUNE_NO_ROT_ALIAS, and for every rotation that walks its cell list (generic path, the list
    // rotations of PATH_MIXED): only the block and box loops of the overlap test skip aliased rotations -- with the skip in the list
    // loop as well the capped generic builds went 4 to 8 bytes over their scratch budget (tests/test_kernel_asm.py).
    {
        const bool off = P.wide || (env->cfg.tuning & IRBPP_TUNE_NO_ROT_ALIAS) || R > 8;
        std::vector<RotView> views((size_t)R);
        std::vector<int32_t> alias((size_t)R);
        for (int k = 0; k < n_shapes; ++k) {
            for (int r = 0; r < R; ++r) {
                const size_t i = (size_t)k * R + r;
                views[r] = RotView{sr[i].fx, sr[i].fy, sr[i].ax, sr[i].ay, sr[i].has_out, sr[i].ext_z_r, mask_bottom + offsets[i], height_bottom + offsets[i]};
            }
            rot_aliases(views.data(), R, alias.data());
            for (int r = 0; r < R; ++r) {
                const int c = alias[r];
                const bool skips = box || (((block_rots >> r) & 1) && ((block_rots >> c) & 1));
                sr[(size_t)k * R + r].alias = (off || !skips) ? r : c;
            }
        }
    }
    if (bcell.empty()) bcell.push_back(Cell{0.0, 0, 0});
    if (tcell.empty()) tcell.push_back(Cell{0.0, 0, 0});
    if (blkcell.empty()) blkcell.push_back(Cell{0.0, 0, 0});
    // gcell mirrors bcell index for index; on the block / box paths nobody reads it
    if (gcell.empty()) gcell.push_back(GCell{0.0, 0, 0});
    // (the walk requests the next four cells while it works on the current four: up to seven cells past a list's end
    // are loaded and ignored)
    for (int i = 0; i < 8; ++i) gcell.push_back(GCell{0.0, 0, 0});
    Tables& T = env->T;
    int rc = dev_upload(env, &T.sr, sr.data(), sr.size());
    if (rc == IRBPP_OK) rc = dev_upload(env, &T.bcell, (const Cell*)bcell.data(), bcell.size());
    if (rc == IRBPP_OK) rc = dev_upload(env, &T.tcell, (const Cell*)tcell.data(), tcell.size());
    if (rc == IRBPP_OK) rc = dev_upload(env, &T.blkcell, (const Cell*)blkcell.data(), blkcell.size());
    if (rc == IRBPP_OK) rc = dev_upload(env, &T.gcell, (const GCell*)gcell.data(), gcell.size());
    if (rc == IRBPP_OK) rc = dev_upload(env, &T.volume, volumes, (size_t)n_shapes);
    if (rc != IRBPP_OK) return rc;
    T.n_shapes = n_shapes;
    if (block_b || box) {                        // switch the overlap test to the block / box path
        env->P.block_b = block_b;
        env->P.block_rots = block_rots;
        env->P.mb_h = mb_h;
        env->P.mb_w = mb_w;
        env->P.box = box ? 1 : 0;
        layout_lds_host(env->P);
        if (env->P.lds_bytes_full > 160 * 1024) return IRBPP_ERR_ARG;
        if (raise_lds_limits() != IRBPP_OK) return IRBPP_ERR_HIP;
    }
    // generic path on a data set whose footprint lists do not fit a die's L2: online steps launch the bins grouped by
    // observed item per die (irbpp_item_order_kernel)
    env->item_order = (!block_b || mixed) && !box && gcell.size() * sizeof(GCell) > (size_t)8 << 20 && env->P.N % NXCD == 0 &&
                      env->P.N >= 64 * NXCD && env->P.K == 1 && !(env->cfg.tuning & IRBPP_TUNE_NO_ITEM_ORDER);
    env->shapes_loaded = true;
    return IRBPP_OK;
}

int irbpp_load_sequences(irbpp_env* env, const int32_t* ids, int32_t n_traj, int32_t length) {
    if (!env || !ids || n_traj < 1 || length < 1) return IRBPP_ERR_ARG;
    if (env->seq_loaded) return IRBPP_ERR_STATE;
    HIP_TRY(hipSetDevice(env->cfg.device));
    int rc = dev_upload(env, &env->T.seq, ids, (size_t)n_traj * length);
    if (rc != IRBPP_OK) return rc;
    env->T.n_traj = n_traj;
    env->T.seq_len = length;
    env->T.stream = env->cfg.item_stream ? 1 : 0;
    env->seq_key = bin_sequences_key(ids, n_traj, length);
    env->seq_loaded = true;
    return IRBPP_OK;
}

int irbpp_stream_cursors(irbpp_env* env, int32_t* cursors_dev, int32_t set, void* stream) {
    if (!env || !cursors_dev) return IRBPP_ERR_ARG;
    if (!env->cfg.item_stream || !env->seq_loaded) return IRBPP_ERR_STATE;
    hipLaunchKernelGGL(irbpp_stream_cursor_kernel, dim3((env->P.N + 255) / 256), dim3(256), 0, (hipStream_t)stream, env->S.bs,
                       cursors_dev, env->P.N, set);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_stream_write(irbpp_env* env, const int32_t* ids_dev, const int32_t* first_dev, const int32_t* count_dev, int32_t width,
                       void* stream) {
    if (!env || !ids_dev || !first_dev || !count_dev || width < 0) return IRBPP_ERR_ARG;
    if (!env->cfg.item_stream || !env->seq_loaded) return IRBPP_ERR_STATE;
    if (width > env->T.seq_len) return IRBPP_ERR_ARG;
    if (width == 0) return IRBPP_OK;
    env->err_mirror = nullptr;                    // the caller may have cleared a STREAM_DRY condition: seed the next step's word anew
    const long long n = (long long)env->T.n_traj * width;
    hipLaunchKernelGGL(irbpp_stream_write_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       const_cast<int32_t*>(env->T.seq), env->T.n_traj, env->T.seq_len, ids_dev, first_dev, count_dev, width);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_stream_table(irbpp_env* env, int32_t* table_dev, void* stream) {
    if (!env || !table_dev) return IRBPP_ERR_ARG;
    if (!env->cfg.item_stream || !env->seq_loaded) return IRBPP_ERR_STATE;
    HIP_TRY(hipMemcpyAsync(table_dev, env->T.seq, (size_t)env->T.n_traj * env->T.seq_len * sizeof(int32_t), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return IRBPP_OK;
}

int irbpp_stream_refill(irbpp_env* env, irbpp_itemgen_dev* gen, int32_t first_stream, void* stream) {
    if (!env || !gen || first_stream < 0) return IRBPP_ERR_ARG;
    if (!env->cfg.item_stream || !env->seq_loaded) return IRBPP_ERR_STATE;
    if ((long long)first_stream + env->P.N > gen->n_streams) return IRBPP_ERR_ARG;
    if (env->T.n_traj != env->P.N || gen->device != env->cfg.device) return IRBPP_ERR_ARG;   // a ring per bin, on the generator's device
    env->err_mirror = nullptr;                    // (as irbpp_stream_write; a STREAM_DRY raised here reaches S.err, which seeds the next step's word)
    return irbpp::itemgen_launch_refill(gen, env->S.bs, const_cast<int32_t*>(env->T.seq), env->P.N, env->T.seq_len, first_stream,
                                        env->S.err, (hipStream_t)stream);
}

int irbpp_obs_len(const irbpp_env* env, int32_t which) {
    if (!env) return IRBPP_ERR_ARG;
    return which == 0 ? env->P.obs_len0 : env->P.obs_len1;
}

typedef void (*env_kernel_fn)(const Params, const Tables, const State, const StepIO, const int);
typedef void (*trace_kernel_fn)(const Params, const State, long long*);

// One launch group: the launches of a transition's plan (irbpp_plan.h: plan_transition) over n launch slots, on one stream;
// `rows`: the per-bin row counts of io.obs where that is a registered observation buffer, else null.
// Most kernels take (Params, Tables, State, StepIO, mode); the few that do not have their own case.
static void launch_group(irbpp_env* env, StepIO io, const Plan& plan, int32_t* rows, hipStream_t st, int n) {
    io.block_off = 0;
    io.n_slots = n;
    io.auto_action = env->auto_actions;
    io.use_order = plan.use_order;
    io.heavy_turn = plan.heavy_turn;
    io.obs_rows = plan.obs_rows == ROWS_TRACK ? rows : nullptr;
    if (plan.obs_rows == ROWS_FORGET) hipMemsetAsync(rows, 0xFF, (size_t)env->P.N * sizeof(int32_t), st);
    const int32_t* const actions = io.actions;
    for (int i = 0; i < plan.n_launches; ++i) {
        const Launch& l = plan.launch[i];
        const void* fn = kernel_registry[l.kernel];
        switch (l.kernel) {
            case K_ITEM_ORDER:
                hipLaunchKernelGGL(irbpp_item_order_kernel, dim3(l.grid), dim3(l.block), l.lds, st, env->T, env->S, n);
                break;
            case K_HEURISTIC: {          // HM's scorer: its triples are the cells of the apply kernel behind it (of that launch alone)
                StepIO sel = io;
                sel.heur_out = env->heur_cells;
                hipLaunchKernelGGL(irbpp_heuristic_kernel, dim3(l.grid), dim3(l.block), l.lds, st, env->P, env->T, env->S, sel);
                io.actions = env->heur_cells;
                break;
            }
            case K_TRACE: case K_TRACE_C32: case K_TRACE_C16: case K_TRACE_REFILL: {
                Params Pt = env->P;
                if (plan.inline_polygon) Pt.round_cap = 0;
                hipLaunchKernelGGL((trace_kernel_fn)fn, dim3(l.grid), dim3(l.block), l.lds, st, Pt, env->S, env->phase_cycles);
                if (env->round_snap)     // tooling: the emit kernel behind it retires the counters, so they are copied here
                    (void)hipMemcpyAsync(env->round_snap, env->S.w_nround, NXCD * XCD_STRIDE * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
                                         // (an error is sticky: launch_env's hipGetLastError reports it, as for the launches)
                break;
            }
            case K_POLYGON:
#ifdef IRBPP_AB_POLY_ACCOUNT
                hipLaunchKernelGGL(irbpp_polygon_kernel, dim3(l.grid), dim3(l.block), l.lds, st, env->P, env->S, env->phase_cycles);
#else
                hipLaunchKernelGGL(irbpp_polygon_kernel, dim3(l.grid), dim3(l.block), l.lds, st, env->P, env->S);
#endif
                break;
            default:
                hipLaunchKernelGGL((env_kernel_fn)fn, dim3(l.grid), dim3(l.block), l.lds == LDS_WIDE_LAYOUT ? wide_layout(env->P).bytes : l.lds,
                                   st, env->P, env->T, env->S, io, l.mode);
                io.actions = actions;
        }
    }
}

// A transition of `grid` launch slots (all bins, or the listed ones) on the caller's stream.  (Cutting it into
// groups on library-owned streams, forked from and joined to the caller's stream with events, was measured and
// dropped: the eight cross-queue dependencies per step cost more than the overlapped launch tails give back,
// 18.5 -> 11.8 M steps/s.  Overlap across sub-batches is offered one level up instead, where no join is needed:
// vec_env.GroupedPackingEnv steps independent groups of bins on their own streams.)
// Transitions as HIP graphs -- OPT-IN (IRBPP_TUNE_GRAPH), because on this runtime (ROCm 7.2) it LOSES at every size measured:
// a buffered placement at 1024 bins 15.3 -> 13.1 M steps/s, BlockOut online 1024 / 2048 bins 17.8 -> 16.4 / 28.4 -> 26.2 M,
// the 64 x 64 heightmap at 2048 bins 6.34 -> 6.22 M, 8192 BlockOut bins as two groups 60.8 -> 58.8 M (profiles/r05/s14): what
// hipGraphLaunch puts between the kernel nodes of a linear chain costs more than the host's launch calls and the dispatch
// gaps it removes (~7 us of a 66 us placement).  The mechanism stays for runtimes where that changes: the chain of a
// transition is captured ONCE per distinct argument set (mode, every pointer and flag of StepIO, the host-side state the
// launch code branches on) on a stream of the library's own and replayed on the caller's stream with one hipGraphLaunch.
// An argument set is captured when it is seen the SECOND time: a caller that hands over a fresh observation tensor every
// step never repeats one and is launched directly.  Everything issued while the caller's stream is itself being captured
// is launched directly too (into the caller's capture).
constexpr int GRAPH_CACHE = 24;
// A captured graph holds Params / Tables / State BY VALUE in its kernel nodes: every setter that changes one of them after
// graphs may exist (the placement log's pointers, a tooling switch) drops the cache; the next launches capture again.
static void drop_graphs(irbpp_env* env) {
    for (auto& g : env->graphs) { if (g.exec) hipGraphExecDestroy(g.exec); if (g.graph) hipGraphDestroy(g.graph); }
    env->graphs.clear();
}
static bool graph_wanted(const irbpp_env* env, int) { return (env->cfg.tuning & IRBPP_TUNE_GRAPH) != 0; }

static int launch_env(irbpp_env* env, StepIO io, int mode, void* stream, int grid = 0, int key = KEY_CAND) {
    if (grid <= 0) grid = env->P.N;
    if (key == KEY_HEUR && grid != env->P.N) return IRBPP_ERR_ARG;     // (HM's scorer covers all bins: plan_transition)
    env->transition_launched = true;
    io.phase_cycles = env->phase_cycles;
    hipStream_t st = (hipStream_t)stream;
    size_t pairs = env->timing.size() / 2;
    const size_t slot = env->timing_next;
    if (pairs && (env->timing_phase++ % env->timing_every) != 0) pairs = 0;       // not a sampled launch
    if (pairs) hipEventRecord(env->timing[2 * slot], st);
    int32_t* rows = nullptr;               // the row counts of io.obs, if it is a registered observation buffer
    for (auto& rb : env->obs_buffers)
        if (io.obs != nullptr && rb.first == io.obs) rows = rb.second;
    const Plan plan = plan_transition(env->P, env->cfg.tuning, mode, grid, key == KEY_HEUR && io.heur_method == 4 ? PLAN_KEY_HEUR_HM : key,
                                      io.bin_list != nullptr, rows != nullptr, env->heavy_turn, env->item_order);
    bool launched = false;
    if (graph_wanted(env, grid) && (mode == MODE_STEP || mode == MODE_CANDS) && key == KEY_CAND) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) cs = hipStreamCaptureStatusActive;
        if (cs == hipStreamCaptureStatusNone) {
            // everything launch_group reads: the arguments and the host-side state it branches on
            struct Key { StepIO io; int mode, grid, heavy_turn, obs_epoch; int32_t* auto_actions; } k;
            memset(&k, 0, sizeof k);
            k.io = io; k.mode = mode; k.grid = grid; k.heavy_turn = env->heavy_turn; k.obs_epoch = env->obs_epoch;
            k.auto_actions = env->auto_actions;
            const uint8_t* kb = (const uint8_t*)&k;
            irbpp_env::GraphEntry* hit = nullptr;
            for (auto& g : env->graphs)
                if (g.key.size() == sizeof k && memcmp(g.key.data(), kb, sizeof k) == 0) { hit = &g; break; }
            if (hit == nullptr) {                        // first sight: remember it, launch directly
                if (env->graphs.size() >= (size_t)GRAPH_CACHE) {       // (the least recently used entry makes room)
                    size_t lru = 0;
                    for (size_t i = 1; i < env->graphs.size(); ++i) if (env->graphs[i].used < env->graphs[lru].used) lru = i;
                    if (env->graphs[lru].exec) hipGraphExecDestroy(env->graphs[lru].exec);
                    if (env->graphs[lru].graph) hipGraphDestroy(env->graphs[lru].graph);
                    env->graphs.erase(env->graphs.begin() + lru);
                }
                env->graphs.push_back({std::vector<uint8_t>(kb, kb + sizeof k), nullptr, nullptr, ++env->graph_clock});
            } else {
                hit->used = ++env->graph_clock;
                if (hit->exec == nullptr) {              // second sight: capture the chain on the library's own stream
                    if (env->cap_stream == nullptr && hipStreamCreateWithFlags(&env->cap_stream, hipStreamNonBlocking) != hipSuccess)
                        env->cap_stream = nullptr;
                    if (env->cap_stream != nullptr && hipStreamBeginCapture(env->cap_stream, hipStreamCaptureModeRelaxed) == hipSuccess) {
                        launch_group(env, io, plan, rows, env->cap_stream, grid);
                        hipGraph_t graph = nullptr;
                        if (hipStreamEndCapture(env->cap_stream, &graph) == hipSuccess && graph != nullptr &&
                            hipGraphInstantiate(&hit->exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                            hit->graph = graph;
                        } else {
                            if (graph) hipGraphDestroy(graph);
                            hit->exec = nullptr;
                        }
                        (void)hipGetLastError();
                    }
                }
                if (hit->exec != nullptr && hipGraphLaunch(hit->exec, st) == hipSuccess) {
                    launched = true;
                    ++env->graph_replays;
                }
            }
        }
    }
    if (!launched) launch_group(env, io, plan, rows, st, grid);
    if (plan.heavy_first) env->heavy_turn ^= 1;      // (the one place it advances: behind a transition that went out, replayed or direct)
    if (pairs) {
        hipEventRecord(env->timing[2 * slot + 1], st);
        env->timing_next = (slot + 1) % pairs;
        if (env->timing_used < pairs) env->timing_used++;
    }
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    // are the grids of the last observation (w_posz / w_valid) those of the item every bin places next?  A launch over all
    // bins that observes makes them so (MODE_CANDS of irbpp_get_all_possible_observation too: the grids are the last slot's,
    // and so are BinState::cur_item / nvalid, which the selection and prejudge go by); a buffered step or reset moves the
    // heightmap / the queue on without observing.  Only launches that went out count.
    if (io.bin_list == nullptr && mode != MODE_POSSIBLE)
        env->grids_current = mode == MODE_CANDS || env->P.K == 1;
    return IRBPP_OK;
}

int irbpp_reset(irbpp_env* env, float* obs_dev, void* stream) {
    if (!env || !obs_dev) return IRBPP_ERR_ARG;
    if (!env->shapes_loaded || !env->seq_loaded) return IRBPP_ERR_STATE;
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.obs = obs_dev;
    io.obs_stride = env->P.obs_len0;
    io.reset_next = env->was_reset ? 1 : 0;       // a later reset() moves every bin on to its next trajectory (IRcreator.py:86-92)
    env->err_mirror = nullptr;                    // bits a reset raises reach S.err only: the next step seeds its error word again
    const int rc = launch_env(env, io, MODE_RESET, stream);
    if (rc == IRBPP_OK) env->was_reset = true;
    return rc;
}

int irbpp_reset_bins(irbpp_env* env, const int32_t* bins_dev, int32_t count, float* obs_dev, void* stream) {
    if (!env || count < 0 || count > env->P.N || (count > 0 && (!bins_dev || !obs_dev))) return IRBPP_ERR_ARG;
    if (!env->was_reset) return IRBPP_ERR_STATE;
    if (count == 0) return IRBPP_OK;
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.obs = obs_dev;
    io.obs_stride = env->P.obs_len0;
    io.bin_list = bins_dev;
    env->err_mirror = nullptr;                    // (as irbpp_reset)
    return launch_env(env, io, MODE_RESET, stream, count);
}

// irbpp_step and its two siblings: `key` says what actions_dev holds (KEY_CAND: candidate rows; KEY_CELLS: int32[N][3] cells;
// KEY_HEUR: nothing, the heuristic (method, dir_idx) chooses)
static int step_common(irbpp_env* env, const int32_t* actions_dev, float* obs_dev, const irbpp_step_out* out, void* stream, int key,
                       int method = 0, int dir_idx = 0) {
    const bool windowed = env->window.window > 0;
    if (windowed && (!out || !out->done_dev || !out->ep_reward_dev || !out->ratio_dev || !out->counter_dev)) return IRBPP_ERR_ARG;
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.actions = actions_dev;
    io.heur_method = method;
    io.heur_dir = dir_idx;
    io.obs = obs_dev;
    io.obs_stride = env->P.obs_len0;
    if (out) {
        io.reward = out->reward_dev;
        io.done = out->done_dev;
        io.counter = out->counter_dev;
        io.ratio = out->ratio_dev;
        io.ep_reward = out->ep_reward_dev;
        io.ep_len = out->ep_len_dev;
        io.stable = out->stable_dev;
        // The error word of the outputs.  Online (K == 1): stored by the emit kernel, the step's last one.  Buffered (K > 1):
        // the transition kernel is the last one and may raise bits itself, so every kernel ORs a bit into S.err AND into
        // this word as it raises it (raise_error), and the emit kernel of get_action_candidates stores S.err into it; the
        // word only needs seeding when the caller hands over a new one.  (A 4-byte device-to-device copy per step -- a
        // 5 us kernel to move one int -- did this before: 3.3 % of the GPU time of a buffered step at 1024 bins.)
        io.err_out = out->err_dev;
        if (out->err_dev != env->err_mirror) {
            if (out->err_dev != nullptr)
                HIP_TRY(hipMemcpyAsync(out->err_dev, env->S.err, sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
            env->err_mirror = out->err_dev;
        }
    } else {
        env->err_mirror = nullptr;
    }
    const int rc = launch_env(env, io, MODE_STEP, stream, 0, key);
    if (rc != IRBPP_OK || !windowed) return rc;
    // the episode window (irbpp_metrics.hip): one workgroup behind the step's kernels, reading the outputs they wrote
    return irbpp_episode_window_update(&env->window, out->done_dev, out->ep_reward_dev, out->ratio_dev, out->counter_dev, env->P.N,
                                       env->cfg.global_offset, stream);
}

int irbpp_step(irbpp_env* env, const int32_t* actions_dev, float* obs_dev, const irbpp_step_out* out, void* stream) {
    if (!env || !actions_dev || !obs_dev) return IRBPP_ERR_ARG;
    if (!env->was_reset) return IRBPP_ERR_STATE;
    return step_common(env, actions_dev, obs_dev, out, stream, KEY_CAND);
}

// a step whose placement does not come from a candidate row is always the apply kernel + MODE_OBSERVE: configurations that
// apply inside the transition kernel cannot take it
static bool applies_in_transition(const irbpp_env* env) {
    return env->P.stability != 0 || (env->cfg.tuning & IRBPP_TUNE_FUSED_APPLY) || chain_launch(env->P, env->cfg.tuning);
}

int irbpp_step_cells(irbpp_env* env, const int32_t* cells_dev, float* obs_dev, const irbpp_step_out* out, void* stream) {
    if (!env || !cells_dev || !obs_dev || applies_in_transition(env)) return IRBPP_ERR_ARG;
    if (!env->was_reset) return IRBPP_ERR_STATE;
    return step_common(env, cells_dev, obs_dev, out, stream, KEY_CELLS);
}

int irbpp_heuristic_step(irbpp_env* env, int32_t method, int32_t dir_idx, float* obs_dev, const irbpp_step_out* out, void* stream) {
    if (!env || !obs_dev || method < 1 || method > 4 || dir_idx < 0 || dir_idx > 3 || applies_in_transition(env)) return IRBPP_ERR_ARG;
    if (method == 4 && env->P.wide) return IRBPP_ERR_ARG;          // HM: the recomputing scorer, which the capacity path lacks
    if (!env->was_reset || !env->grids_current) return IRBPP_ERR_STATE;
    return step_common(env, nullptr, obs_dev, out, stream, KEY_HEUR, method, dir_idx);
}

int irbpp_get_action_candidates(irbpp_env* env, const int32_t* order_actions_dev, float* loc_obs_dev, void* stream) {
    if (!env || !order_actions_dev || !loc_obs_dev) return IRBPP_ERR_ARG;
    if (!env->was_reset) return IRBPP_ERR_STATE;
    if (env->P.K < 2) return IRBPP_ERR_ARG;
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.actions = order_actions_dev;
    io.obs = loc_obs_dev;
    io.obs_stride = env->P.obs_len1;
    io.err_out = env->err_mirror;          // the error word of the step outputs follows S.err through this call too
    return launch_env(env, io, MODE_CANDS, stream);
}

int irbpp_get_all_possible_observation(irbpp_env* env, float* loc_obs_dev, void* stream) {
    if (!env || !loc_obs_dev) return IRBPP_ERR_ARG;
    if (!env->was_reset) return IRBPP_ERR_STATE;
    if (env->P.K < 2) return IRBPP_ERR_ARG;
    // one full-width transition per buffer slot, all on the caller's stream: slot j of every bin is observed into row
    // [b][j] of the [N][k][obs_len(1)] block (row stride k * obs_len(1)); like the reference's loop the last slot's
    // candidates are the ones a following step would index, and the chosen slot (orderAction) is not touched
    for (int j = 0; j < env->P.K; ++j) {
        StepIO io;
        memset(&io, 0, sizeof(io));
        io.fixed_slot = j + 1;
        io.obs = loc_obs_dev + (size_t)j * env->P.obs_len1;
        io.obs_stride = env->P.K * env->P.obs_len1;
        io.err_out = env->err_mirror;
        const int rc = launch_env(env, io, MODE_CANDS, stream);
        if (rc != IRBPP_OK) return rc;
    }
    return IRBPP_OK;
}

int irbpp_policy_minz(irbpp_env* env, const float* loc_obs_dev, int32_t obs_stride, int32_t* actions_dev, void* stream) {
    if (!env || !loc_obs_dev || !actions_dev || obs_stride < 5 * env->P.S) return IRBPP_ERR_ARG;
    const int waves_per_block = 4;
    const int grid = (env->P.N + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(irbpp_policy_minz_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, loc_obs_dev,
                       obs_stride, env->P.S, env->P.N, actions_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_set_auto_policy(irbpp_env* env, int32_t* actions_dev) {
    if (!env) return IRBPP_ERR_ARG;
    env->auto_actions = actions_dev;
    return IRBPP_OK;
}

int irbpp_register_obs_buffer(irbpp_env* env, float* obs_dev) {
    if (!env || !obs_dev) return IRBPP_ERR_ARG;
    HIP_TRY(hipSetDevice(env->cfg.device));
    env->obs_epoch++;
    for (auto& rb : env->obs_buffers)
        if (rb.first == obs_dev) {           // registered again (e.g. a new allocation at an old address): contents unknown
            HIP_TRY(hipMemset(rb.second, 0xFF, (size_t)env->P.N * sizeof(int32_t)));
            return IRBPP_OK;
        }
    int32_t* rows = nullptr;
    for (auto& rb : env->obs_buffers)        // a slot freed by irbpp_unregister_obs_buffer keeps its row counts' memory
        if (rb.first == nullptr && rows == nullptr) { rows = rb.second; rb.first = obs_dev; }
    if (rows == nullptr) {
        if (env->obs_buffers.size() >= 8) return IRBPP_ERR_ARG;
        int rc = dev_alloc(env, &rows, (size_t)env->P.N);
        if (rc != IRBPP_OK) return rc;
        env->obs_buffers.emplace_back(obs_dev, rows);
    }
    HIP_TRY(hipMemset(rows, 0xFF, (size_t)env->P.N * sizeof(int32_t)));      // -1: contents unknown, write everything once
    return IRBPP_OK;
}

int irbpp_unregister_obs_buffer(irbpp_env* env, float* obs_dev) {
    if (!env || !obs_dev) return IRBPP_ERR_ARG;
    env->obs_epoch++;
    for (auto& rb : env->obs_buffers)
        if (rb.first == obs_dev) { rb.first = nullptr; return IRBPP_OK; }
    return IRBPP_ERR_ARG;
}

int irbpp_invalidate_obs_buffer(irbpp_env* env, float* obs_dev, void* stream) {
    if (!env) return IRBPP_ERR_ARG;
    bool found = obs_dev == nullptr;
    for (auto& rb : env->obs_buffers)
        if (rb.first != nullptr && (obs_dev == nullptr || rb.first == obs_dev)) {
            HIP_TRY(hipMemsetAsync(rb.second, 0xFF, (size_t)env->P.N * sizeof(int32_t), (hipStream_t)stream));
            found = true;
        }
    return found ? IRBPP_OK : IRBPP_ERR_ARG;
}

int irbpp_possible_position(irbpp_env* env, const int32_t* item_ids_dev, double* posz_dev, uint8_t* mask_dev, void* stream) {
    if (!env || !item_ids_dev || !posz_dev || !mask_dev || env->P.wide) return IRBPP_ERR_ARG;
    if (!env->shapes_loaded) return IRBPP_ERR_STATE;
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.actions = item_ids_dev;
    io.posz_out = posz_dev;
    io.mask_out = mask_dev;
    return launch_env(env, io, MODE_POSSIBLE, stream);
}

int irbpp_heuristic_action(irbpp_env* env, int32_t method, int32_t dir_idx, int32_t* out_dev, void* stream) {
    if (!env || !out_dev || method < 1 || method > 4 || dir_idx < 0 || dir_idx > 3 || env->P.wide) return IRBPP_ERR_ARG;
    if (!env->was_reset) return IRBPP_ERR_STATE;
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.heur_out = out_dev;
    io.heur_method = method;
    io.heur_dir = dir_idx;
    hipLaunchKernelGGL(irbpp_heuristic_kernel, dim3(env->P.N), dim3(256), env->P.lds_bytes_full, (hipStream_t)stream, env->P,
                       env->T, env->S, io);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_shot_item(const double* verts_dev, const int32_t* faces_dev, int32_t n_faces, int32_t fx, int32_t fy,
                    double resolution_h, double shift, double extent_z, double* top_dev, double* bottom_dev,
                    double* mask_top_dev, double* mask_bottom_dev, int32_t* scratch_dev, void* stream) {
    if (!verts_dev || !faces_dev || n_faces < 1 || fx < 1 || fy < 1 || !top_dev || !bottom_dev || !mask_top_dev ||
        !mask_bottom_dev || !scratch_dev)
        return IRBPP_ERR_ARG;
    HIP_TRY(hipMemsetAsync(scratch_dev, 0, sizeof(int32_t), (hipStream_t)stream));
    const int n = fx * fy, grid = (n + 255) / 256;
    hipLaunchKernelGGL(irbpp_shot_item_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, verts_dev, faces_dev,
                       n_faces, fx, fy, resolution_h, shift, top_dev, bottom_dev, mask_top_dev, mask_bottom_dev,
                       scratch_dev);
    hipLaunchKernelGGL(irbpp_shot_item_fallback_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, extent_z,
                       top_dev, bottom_dev, mask_top_dev, mask_bottom_dev, scratch_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_convex_hull_actions(irbpp_env* env, int32_t n_grids, const double* posz_valid_dev, const uint8_t* mask_dev,
                              uint32_t* vertex_rows_dev, void* stream) {
    if (!env || n_grids < 1 || !posz_valid_dev || !mask_dev || !vertex_rows_dev || env->P.wide) return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_hull_kernel, dim3(n_grids), dim3(256), env->P.lds_bytes, (hipStream_t)stream, env->P,
                       env->S, posz_valid_dev, mask_dev, vertex_rows_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_get_heightmaps(irbpp_env* env, double* hm_dev, void* stream) {
    if (!env || !hm_dev) return IRBPP_ERR_ARG;
    HIP_TRY(hipMemcpyAsync(hm_dev, env->S.hm, (size_t)env->P.N * env->P.Hc * sizeof(double), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return IRBPP_OK;
}

int irbpp_set_heightmaps(irbpp_env* env, const double* hm_dev, void* stream) {
    if (!env || !hm_dev) return IRBPP_ERR_ARG;
    HIP_TRY(hipMemcpyAsync(env->S.hm, hm_dev, (size_t)env->P.N * env->P.Hc * sizeof(double), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    // the drop heights of the last observation (w_posz, marked by w_valid) belong to the OLD maps: a step that follows
    // without a new observation recomputes its drop height from the footprint's bottom cells instead
    HIP_TRY(hipMemsetAsync(env->S.w_valid, 0, (size_t)env->P.N * env->P.R * env->P.vrow * sizeof(uint32_t), (hipStream_t)stream));
    env->grids_current = false;            // (irbpp_heuristic_step answers IRBPP_ERR_STATE until the next observation of all bins)
    return IRBPP_OK;
}

// ---- save, restore and fork bins (irbpp_binstate.h: the segment table; irbpp_binstate.hip: the kernel) ----
static void bin_blob_info_of(const irbpp_env* env, irbpp_bin_blob_info* out) {
    memset(out, 0, sizeof *out);
    out->version = BIN_BLOB_VERSION;
    out->bytes_per_bin = bin_segments(env->P, env->S.log_cap).bytes_per_bin;
    out->geometry_key = bin_geometry_key(env->P, env->S.log_cap);
    out->tables_key = bin_tables_key(env->shapes_key, env->seq_key);
    out->grids_current = env->grids_current ? 1 : 0;
}

extern "C++" {
template <int MODE>
static int launch_binstate(const irbpp_env* src, const irbpp_env* dst, const int32_t* src_bins, const int32_t* dst_bins, void* blob,
                           int32_t count, void* stream) {
    HIP_TRY(hipSetDevice(dst->cfg.device));
    hipLaunchKernelGGL(irbpp_binstate_kernel<MODE>, dim3((unsigned)count), dim3(BINSTATE_THREADS), 0, (hipStream_t)stream,
                       bin_segments(dst->P, dst->S.log_cap), src->S, dst->S, src_bins, dst_bins, (uint8_t*)blob, src->P.N, dst->P.N,
                       src == dst ? 1 : 0);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}
}  // extern "C++"

int irbpp_bin_blob_info_get(const irbpp_env* env, irbpp_bin_blob_info* out) {
    if (!env || !out) return IRBPP_ERR_ARG;
    if (!env->shapes_loaded || !env->seq_loaded) return IRBPP_ERR_STATE;
    bin_blob_info_of(env, out);
    return IRBPP_OK;
}

int irbpp_save_bins(irbpp_env* env, const int32_t* bins_dev, int32_t count, void* blob_dev, void* stream) {
    if (!env || count < 0 || (count > 0 && (!bins_dev || !blob_dev))) return IRBPP_ERR_ARG;
    if (count == 0) return IRBPP_OK;                 // (answered before the environment is looked at)
    if (env->cfg.item_stream) return IRBPP_ERR_ARG;
    if (!env->was_reset) return IRBPP_ERR_STATE;
    return launch_binstate<BINS_TO_BLOB>(env, env, bins_dev, nullptr, blob_dev, count, stream);
}

int irbpp_load_bins(irbpp_env* env, const irbpp_bin_blob_info* info, const int32_t* bins_dev, int32_t count, const void* blob_dev,
                    void* stream) {
    if (!env || !info || count < 0 || (count > 0 && (!bins_dev || !blob_dev))) return IRBPP_ERR_ARG;
    if (count == 0) return IRBPP_OK;
    if (env->cfg.item_stream) return IRBPP_ERR_ARG;
    if (!env->shapes_loaded || !env->seq_loaded || !env->was_reset) return IRBPP_ERR_STATE;
    irbpp_bin_blob_info own;
    bin_blob_info_of(env, &own);
    if (info->version != own.version || info->bytes_per_bin != own.bytes_per_bin || info->geometry_key != own.geometry_key ||
        info->tables_key != own.tables_key)
        return IRBPP_ERR_ARG;
    const int rc = launch_binstate<BLOB_TO_BINS>(env, env, nullptr, bins_dev, const_cast<void*>(blob_dev), count, stream);
    // the loaded bins' stored grids are as current as they were at the save; every other host-side flag stays: the graph cache (no
    // pointer a captured node holds changes -- the setters that drop it change Params / Tables / State), err_mirror, the episode window
    if (rc == IRBPP_OK) env->grids_current = env->grids_current && info->grids_current != 0;
    return rc;
}

int irbpp_copy_bins(irbpp_env* dst, const int32_t* dst_bins_dev, irbpp_env* src, const int32_t* src_bins_dev, int32_t count,
                    void* stream) {
    if (!dst || !src || count < 0 || (count > 0 && (!dst_bins_dev || !src_bins_dev))) return IRBPP_ERR_ARG;
    if (count == 0) return IRBPP_OK;
    if (dst->cfg.item_stream || src->cfg.item_stream) return IRBPP_ERR_ARG;
    if (!dst->was_reset || !src->was_reset) return IRBPP_ERR_STATE;
    if (dst != src) {
        irbpp_bin_blob_info a, b;
        bin_blob_info_of(dst, &a);
        bin_blob_info_of(src, &b);
        if (a.geometry_key != b.geometry_key || a.tables_key != b.tables_key || dst->cfg.device != src->cfg.device ||
            (dst->S.log_meta != nullptr) != (src->S.log_meta != nullptr))
            return IRBPP_ERR_ARG;
    }
    const int rc = launch_binstate<BINS_TO_BINS>(src, dst, src_bins_dev, dst_bins_dev, nullptr, count, stream);
    if (rc == IRBPP_OK) dst->grids_current = dst->grids_current && src->grids_current;      // (the other flags: as irbpp_load_bins)
    return rc;
}

int irbpp_episode_totals(irbpp_env* env, double* out_dev, void* stream) {
    if (!env || !out_dev) return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_totals_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, env->S.totals, env->P.N, out_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_set_placement_log(irbpp_env* env, uint32_t* meta_dev, double* z_dev, int32_t capacity) {
    if (!env || capacity < 0 || ((meta_dev == nullptr) != (z_dev == nullptr))) return IRBPP_ERR_ARG;
    drop_graphs(env);                      // (captured kernel nodes carry State by value)
    env->S.log_meta = meta_dev;
    env->S.log_z = z_dev;
    env->S.log_cap = meta_dev ? capacity : 0;
    return IRBPP_OK;
}

static bool window_ok(const irbpp_episode_window* w) {
    return w->ring_dev && w->snapshot_dev && w->rows_dev && w->state_dev && w->window >= 1 && w->window <= WINDOW_MAX &&
           w->history >= 1;
}

int irbpp_set_episode_window(irbpp_env* env, const irbpp_episode_window* w) {
    if (!env) return IRBPP_ERR_ARG;
    if (w == nullptr) { env->window = irbpp_episode_window{}; return IRBPP_OK; }
    if (!window_ok(w)) return IRBPP_ERR_ARG;
    env->window = *w;
    return IRBPP_OK;
}

// the one launch site of the update kernel: a windowed step (step_common) ends here too
int irbpp_episode_window_update(const irbpp_episode_window* w, const uint8_t* done_dev, const double* ep_reward_dev,
                                const double* ratio_dev, const int32_t* counter_dev, int32_t n_bins, int32_t global_offset,
                                void* stream) {
    if (!w || !done_dev || !ep_reward_dev || !ratio_dev || !counter_dev || !window_ok(w) || n_bins < 1) return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_window_update_kernel, dim3(1), dim3(WINDOW_UPDATE_THREADS), 0, (hipStream_t)stream, done_dev,
                       ep_reward_dev, ratio_dev, counter_dev, n_bins, global_offset, w->ring_dev, w->snapshot_dev, w->rows_dev,
                       w->state_dev, w->window, w->history);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_episode_metrics(const irbpp_episode_window* parts, int32_t n_parts, int32_t first_step, int32_t n_steps,
                          double* out_dev, void* stream) {
    if (!parts || !out_dev || n_parts < 1 || n_parts > WINDOW_PARTS_MAX || first_step < 1) return IRBPP_ERR_ARG;
    WindowParts wp;
    memset(&wp, 0, sizeof wp);
    wp.P = n_parts;
    wp.W = parts[0].window;
    wp.H = parts[0].history;
    if (wp.W < 1 || wp.W > WINDOW_MAX || wp.H < 1 || n_steps < 1 || n_steps > wp.H) return IRBPP_ERR_ARG;
    for (int p = 0; p < n_parts; ++p) {
        if (!parts[p].snapshot_dev || !parts[p].rows_dev || !parts[p].state_dev || parts[p].window != wp.W ||
            parts[p].history != wp.H)
            return IRBPP_ERR_ARG;
        wp.snap[p] = parts[p].snapshot_dev;
        wp.rows[p] = parts[p].rows_dev;
        wp.state[p] = parts[p].state_dev;
    }
    hipLaunchKernelGGL(irbpp_window_metrics_kernel, dim3(n_steps), dim3(64), (size_t)3 * wp.W * sizeof(double), (hipStream_t)stream,
                       wp, first_step, out_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_sumtree_find(const float* tree_dev, int32_t n_env, int32_t capacity, const float* values_dev, int32_t draws,
                       float* prob_dev, int64_t* data_idx_dev, int64_t* tree_idx_dev, void* stream) {
    if (!tree_dev || !values_dev || !prob_dev || !data_idx_dev || !tree_idx_dev || n_env < 1 || capacity < 1 || draws < 1)
        return IRBPP_ERR_ARG;
    const int n = n_env * draws;
    hipLaunchKernelGGL(irbpp_sumtree_find_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, tree_dev, n_env,
                       capacity, values_dev, draws, prob_dev, data_idx_dev, tree_idx_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_sumtree_sample(const float* tree_dev, const int64_t* index_dev, int32_t n_env, int32_t capacity, int32_t draws,
                         int32_t n_step, uint64_t seed, int32_t max_tries, float* prob_dev, int64_t* data_idx_dev,
                         int64_t* tree_idx_dev, int32_t* failed_dev, void* stream) {
    if (!tree_dev || !index_dev || !prob_dev || !data_idx_dev || !tree_idx_dev || !failed_dev || n_env < 1 || capacity < 1 ||
        draws < 1 || n_step < 0 || max_tries < 1)
        return IRBPP_ERR_ARG;
    const int n = n_env * draws;
    hipLaunchKernelGGL(irbpp_sumtree_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, tree_dev, index_dev,
                       n_env, capacity, draws, n_step, seed, max_tries, prob_dev, data_idx_dev, tree_idx_dev, failed_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_sumtree_update(float* tree_dev, float* max_dev, int32_t n_env, int32_t capacity, const int64_t* tree_idx_dev,
                         const float* priority_dev, int32_t leaves, const uint8_t* env_mask_dev, void* stream) {
    if (!tree_dev || !max_dev || !tree_idx_dev || !priority_dev || n_env < 1 || capacity < 1 || leaves < 1) return IRBPP_ERR_ARG;
    if (2 * capacity - 1 > SUMTREE_LDS) return IRBPP_ERR_ARG;        // caller keeps its host-side path for longer rows
    hipLaunchKernelGGL(irbpp_sumtree_update_kernel, dim3(n_env), dim3(64), (size_t)(2 * capacity - 1) * sizeof(float), (hipStream_t)stream, tree_dev, max_dev, capacity,
                       tree_idx_dev, priority_dev, leaves, env_mask_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_masked_argmax(const float* q_dev, int32_t q_stride, const float* obs_dev, int32_t obs_stride, int32_t selected,
                        int32_t n_env, int64_t* action_dev, void* stream) {
    if (!q_dev || !obs_dev || !action_dev || n_env < 1 || selected < 1 || q_stride < selected || obs_stride < 5 * selected)
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_masked_argmax_kernel, dim3((n_env + 3) / 4), dim3(256), 0, (hipStream_t)stream, q_dev, q_stride,
                       obs_dev, obs_stride, selected, n_env, action_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

// one [S][atoms] block per env / sample: within the head's limits, rows and envs that do not overlap
static bool head_block_ok(const float* p, int64_t env_stride, int64_t row_stride, int32_t atoms, int32_t s_rows) {
    return p && atoms >= 2 && atoms <= HEAD_MAX_ATOMS && s_rows >= 1 && s_rows <= HEAD_MAX_ROWS && row_stride >= atoms &&
           env_stride >= (int64_t)(s_rows - 1) * row_stride + atoms;
}

int irbpp_categorical_act(const float* p_dev, int64_t env_stride, int64_t row_stride, const float* support_dev, int32_t atoms,
                          const float* obs_dev, int32_t obs_stride, int32_t s_rows, int32_t n_env, int64_t* action_dev,
                          float* q_out_dev, int64_t q_stride, void* stream) {
    if (!head_block_ok(p_dev, env_stride, row_stride, atoms, s_rows) || !support_dev || !action_dev || n_env < 1 ||
        (obs_dev && obs_stride < 5 * s_rows) || (q_out_dev && q_stride < s_rows))
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_c51_act_kernel, dim3(n_env), dim3(64), (size_t)64 * (atoms | 1) * sizeof(float), (hipStream_t)stream,
                       p_dev, (long long)env_stride, (long long)row_stride, support_dev, atoms, obs_dev, obs_stride, s_rows,
                       action_dev, q_out_dev, (long long)q_stride);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_categorical_target(const float* p_online_dev, int64_t online_env_stride, int64_t online_row_stride,
                             const float* p_target_dev, int64_t target_env_stride, int64_t target_row_stride, const float* returns_dev,
                             const float* nonterminals_dev, const float* support_dev, int32_t atoms, int32_t s_rows, int32_t batch,
                             float gamma_n, float v_min, float v_max, float delta_z, float* m_dev, int64_t* a_star_dev, void* stream) {
    if (!head_block_ok(p_online_dev, online_env_stride, online_row_stride, atoms, s_rows) ||
        !head_block_ok(p_target_dev, target_env_stride, target_row_stride, atoms, s_rows) || !returns_dev || !nonterminals_dev ||
        !support_dev || !m_dev || !a_star_dev || batch < 1 || !(v_max > v_min) || !(delta_z > 0))
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_c51_target_kernel, dim3(batch), dim3(64), (size_t)64 * (atoms | 1) * sizeof(float),
                       (hipStream_t)stream, p_online_dev, (long long)online_env_stride, (long long)online_row_stride, p_target_dev,
                       (long long)target_env_stride, (long long)target_row_stride, returns_dev, nonterminals_dev, support_dev,
                       atoms, s_rows, gamma_n, v_min, v_max, delta_z, m_dev, a_star_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

static bool dueling_block_ok(const float* v, int64_t v_stride, const float* a, int64_t env_stride, int64_t row_stride, int32_t atoms,
                             int32_t s_rows) {
    return v && v_stride >= atoms && head_block_ok(a, env_stride, row_stride, atoms, s_rows);
}

// dynamic LDS of a dueling launch; above 64 KB the kernel is told (on the current device) that it may be given that much
static bool dueling_lds(const void* kernel, int32_t atoms, int32_t s_rows, size_t* bytes) {
    *bytes = (size_t)dueling_tile_rows(s_rows, atoms) * (atoms | 1) * sizeof(float);
    return *bytes <= 64 * 1024 ||
           hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DUELING_TILE_BYTES) == hipSuccess;
}

int irbpp_dueling_act(const float* v_dev, int64_t v_stride, const float* a_dev, int64_t env_stride, int64_t row_stride,
                      const float* support_dev, int32_t atoms, const float* obs_dev, int32_t obs_stride, int32_t s_rows,
                      int32_t n_env, int64_t* action_dev, float* q_out_dev, int64_t q_stride, float* p_out_dev, void* stream) {
    if (!dueling_block_ok(v_dev, v_stride, a_dev, env_stride, row_stride, atoms, s_rows) || !support_dev || !action_dev ||
        n_env < 1 || (obs_dev && obs_stride < 5 * s_rows) || (q_out_dev && q_stride < s_rows))
        return IRBPP_ERR_ARG;
    size_t lds;
    if (!dueling_lds((const void*)irbpp_dueling_act_kernel, atoms, s_rows, &lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(irbpp_dueling_act_kernel, dim3(n_env), dim3(DUELING_THREADS), lds, (hipStream_t)stream, v_dev,
                       (long long)v_stride, a_dev, (long long)env_stride, (long long)row_stride, support_dev, atoms, obs_dev,
                       obs_stride, s_rows, action_dev, q_out_dev, (long long)q_stride, p_out_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_dueling_target(const float* v_online_dev, int64_t v_online_stride, const float* a_online_dev, int64_t online_env_stride,
                         int64_t online_row_stride, const float* v_target_dev, int64_t v_target_stride, const float* a_target_dev,
                         int64_t target_env_stride, int64_t target_row_stride, const float* returns_dev,
                         const float* nonterminals_dev, const float* support_dev, int32_t atoms, int32_t s_rows, int32_t batch,
                         float gamma_n, float v_min, float v_max, float delta_z, float* m_dev, int64_t* a_star_dev, void* stream) {
    if (!dueling_block_ok(v_online_dev, v_online_stride, a_online_dev, online_env_stride, online_row_stride, atoms, s_rows) ||
        !dueling_block_ok(v_target_dev, v_target_stride, a_target_dev, target_env_stride, target_row_stride, atoms, s_rows) ||
        !returns_dev || !nonterminals_dev || !support_dev || !m_dev || !a_star_dev || batch < 1 || !(v_max > v_min) ||
        !(delta_z > 0))
        return IRBPP_ERR_ARG;
    size_t lds;
    if (!dueling_lds((const void*)irbpp_dueling_target_kernel, atoms, s_rows, &lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(irbpp_dueling_target_kernel, dim3(batch), dim3(DUELING_THREADS), lds, (hipStream_t)stream, v_online_dev,
                       (long long)v_online_stride, a_online_dev, (long long)online_env_stride, (long long)online_row_stride,
                       v_target_dev, (long long)v_target_stride, a_target_dev, (long long)target_env_stride,
                       (long long)target_row_stride, returns_dev, nonterminals_dev, support_dev, atoms, s_rows, gamma_n, v_min,
                       v_max, delta_z, m_dev, a_star_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_dueling_loss(const float* v_dev, int64_t v_stride, const float* a_dev, int64_t env_stride, int64_t row_stride,
                       const int64_t* actions_dev, const float* m_dev, int32_t atoms, int32_t s_rows, int32_t batch,
                       float* loss_out_dev, float* g_out_dev, void* stream) {
    if (!dueling_block_ok(v_dev, v_stride, a_dev, env_stride, row_stride, atoms, s_rows) || !actions_dev || !m_dev || batch < 1 ||
        !loss_out_dev || !g_out_dev)
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_dueling_loss_kernel, dim3(batch), dim3(DUELING_THREADS), 0, (hipStream_t)stream, v_dev,
                       (long long)v_stride, a_dev, (long long)env_stride, (long long)row_stride, actions_dev, m_dev, atoms, s_rows,
                       loss_out_dev, g_out_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_dueling_loss_backward(const float* g_dev, const float* grad_loss_dev, const int64_t* actions_dev, int32_t atoms,
                                int32_t s_rows, int32_t batch, float* grad_v_out_dev, float* grad_a_out_dev, void* stream) {
    if (!g_dev || !grad_loss_dev || !actions_dev || atoms < 2 || atoms > HEAD_MAX_ATOMS || s_rows < 1 ||
        s_rows > HEAD_MAX_ROWS || batch < 1)
        return IRBPP_ERR_ARG;
    if (!grad_v_out_dev && !grad_a_out_dev) return IRBPP_OK;                   // nothing asked for: nothing launched
    const int chunks = grad_a_out_dev ? (s_rows + DUELING_LOSS_CHUNK_ROWS - 1) / DUELING_LOSS_CHUNK_ROWS : 1;
    hipLaunchKernelGGL(irbpp_dueling_loss_backward_kernel, dim3(batch, chunks), dim3(DUELING_THREADS), 0, (hipStream_t)stream,
                       g_dev, grad_loss_dev, actions_dev, atoms, s_rows, grad_v_out_dev, grad_a_out_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_clipped_adam_step(const irbpp_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunks_dev, int32_t n_chunks,
                            double* partial_dev, const irbpp_adam_hyper* hyper, float* total_norm_dev, int64_t* skipped_dev,
                            void* stream) {
    if (!tensors_dev || !chunks_dev || !partial_dev || !hyper || !total_norm_dev || !skipped_dev || n_tensors < 1 ||
        n_chunks < n_tensors)
        return IRBPP_ERR_ARG;
    const int32_t f = hyper->flags;
    if ((f & ~(IRBPP_ADAM_WRITE_GRADS | IRBPP_ADAM_ZERO_GRADS | IRBPP_ADAM_SYNC_TARGET | IRBPP_ADAM_CLIP_ONLY)) ||
        ((f & IRBPP_ADAM_WRITE_GRADS) && (f & IRBPP_ADAM_ZERO_GRADS)) ||
        ((f & IRBPP_ADAM_CLIP_ONLY) && (f & (IRBPP_ADAM_ZERO_GRADS | IRBPP_ADAM_SYNC_TARGET))))
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_grad_sumsq_kernel, dim3(n_chunks), dim3(OPTIM_THREADS), 0, (hipStream_t)stream, tensors_dev, chunks_dev,
                       partial_dev);
    hipLaunchKernelGGL(irbpp_clipped_adam_kernel, dim3(n_chunks), dim3(OPTIM_THREADS), 0, (hipStream_t)stream, tensors_dev, chunks_dev,
                       (const double*)partial_dev, (int)n_chunks, *hyper, total_norm_dev, (long long*)skipped_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_noisy_weights(const float* mu, const float* sigma, const float* eps, const float* bias_mu, const float* bias_sigma,
                        const float* bias_eps, int32_t out, int32_t in, float* w_out, float* b_out, void* stream) {
    if (!mu || !sigma || !eps || !bias_mu || !bias_sigma || !bias_eps || !w_out || !b_out || out < 1 || in < 1 ||
        out > STREAMS_MAX_WIDTH || in > STREAMS_MAX_WIDTH)
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_noisy_weights_kernel, dim3((out * in + 255) / 256), dim3(256), 0, (hipStream_t)stream, mu, sigma, eps,
                       bias_mu, bias_sigma, bias_eps, out, in, w_out, b_out);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_streams_act(const irbpp_stream_weights* w, const float* xg_dev, int64_t xg_stride, const float* x_dev, int64_t env_stride,
                      int64_t row_stride, const float* support_dev, const float* obs_dev, int32_t obs_stride, int32_t s_rows,
                      int32_t n_env, int64_t* action_dev, float* q_out_dev, int64_t q_stride, float* v_out_dev, float* a_out_dev,
                      void* stream) {
    if (!w || !w->w_hv || !w->b_hv || !w->w_zv || !w->b_zv || !w->w_ha || !w->b_ha || !w->w_za || !w->b_za || w->embed < 1 ||
        w->embed > STREAMS_MAX_WIDTH || w->hidden < 1 || w->hidden > STREAMS_MAX_WIDTH || w->atoms < 2 ||
        w->atoms > HEAD_MAX_ATOMS || s_rows < 1 || s_rows > HEAD_MAX_ROWS || n_env < 1 || !xg_dev || xg_stride < w->embed ||
        !x_dev || row_stride < w->embed || env_stride < (int64_t)(s_rows - 1) * row_stride + w->embed ||
        (obs_dev && obs_stride < 5 * s_rows) || (q_out_dev && q_stride < s_rows) || ((action_dev || q_out_dev) && !support_dev) ||
        (!action_dev && !q_out_dev && !v_out_dev && !a_out_dev))
        return IRBPP_ERR_ARG;
    const bool resident = dueling_tile_rows(s_rows, w->atoms) == s_rows;
    if (!resident && !a_out_dev) return IRBPP_ERR_ARG;                         // the block needs a_out as its workspace
    StreamsArgs g;
    g.xg_stride = xg_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.q_stride = q_stride;
    g.embed = w->embed, g.hidden = w->hidden, g.atoms = w->atoms, g.obs_stride = obs_stride, g.s_rows = s_rows;
    g.x_vec4 = ((uintptr_t)x_dev % 16 == 0 && (uintptr_t)w->w_ha % 16 == 0 && env_stride % 4 == 0 && row_stride % 4 == 0 && w->embed % 4 == 0) ? 1 : 0;
    const auto kernel = w->atoms <= 32 ? irbpp_streams_act_a32_kernel : irbpp_streams_act_kernel;
    size_t lds = 0;
    if (resident && !dueling_lds((const void*)kernel, w->atoms, s_rows, &lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(kernel, dim3(n_env), dim3(DUELING_THREADS), lds, (hipStream_t)stream, w->w_hv, w->b_hv, w->w_zv, w->b_zv,
                       w->w_ha, w->b_ha, w->w_za, w->b_za, xg_dev, x_dev, support_dev, obs_dev, action_dev, q_out_dev, v_out_dev,
                       a_out_dev, g);
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    if (resident || (!action_dev && !q_out_dev)) return IRBPP_OK;
    if (!dueling_lds((const void*)irbpp_streams_finish_kernel, w->atoms, s_rows, &lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(irbpp_streams_finish_kernel, dim3(n_env), dim3(DUELING_THREADS), lds, (hipStream_t)stream, w->w_hv, w->b_hv,
                       w->w_zv, w->b_zv, xg_dev, (const float*)a_out_dev, support_dev, obs_dev, action_dev, q_out_dev, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_streams_act_mfma(const irbpp_stream_weights* w, const float* xg_dev, int64_t xg_stride, const float* x_dev,
                           int64_t env_stride, int64_t row_stride, const float* support_dev, const float* obs_dev, int32_t obs_stride,
                           int32_t s_rows, int32_t n_env, int64_t* action_dev, float* q_out_dev, int64_t q_stride, float* v_out_dev,
                           float* a_out_dev, void* stream) {
    if (!w || !w->w_hv || !w->b_hv || !w->w_zv || !w->b_zv || !w->w_ha || !w->b_ha || !w->w_za || !w->b_za || w->embed < 1 ||
        w->embed > STREAMS_MAX_WIDTH || w->hidden < 1 || w->hidden > STREAMS_MAX_WIDTH || w->embed % 4 || w->hidden % 4 ||
        w->atoms < 2 || w->atoms > HEAD_MAX_ATOMS || s_rows < 1 || s_rows > HEAD_MAX_ROWS || n_env < 1 || !xg_dev ||
        xg_stride < w->embed || !x_dev || row_stride < w->embed || env_stride < (int64_t)(s_rows - 1) * row_stride + w->embed ||
        (obs_dev && obs_stride < 5 * s_rows) || (q_out_dev && q_stride < s_rows) || ((action_dev || q_out_dev) && !support_dev) ||
        (!action_dev && !q_out_dev && !v_out_dev && !a_out_dev))
        return IRBPP_ERR_ARG;
    const bool resident = dueling_tile_rows(s_rows, w->atoms) == s_rows;
    if (!resident && !a_out_dev) return IRBPP_ERR_ARG;                         // the block needs a_out as its workspace
    StreamsArgs g;
    g.xg_stride = xg_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.q_stride = q_stride;
    g.embed = w->embed, g.hidden = w->hidden, g.atoms = w->atoms, g.obs_stride = obs_stride, g.s_rows = s_rows;
    g.x_vec4 = (((uintptr_t)x_dev % 16 == 0 && env_stride % 4 == 0 && row_stride % 4 == 0) ? STREAMS_MFMA_X16 : 0) |
               ((uintptr_t)w->w_ha % 16 == 0 ? STREAMS_MFMA_WHA16 : 0) | ((uintptr_t)w->w_za % 16 == 0 ? STREAMS_MFMA_WZA16 : 0);
    const auto kernel = w->atoms <= MFMA_TILE ? irbpp_streams_act_mfma_a32_kernel : irbpp_streams_act_mfma_kernel;
    size_t lds = 0;
    if (resident && !dueling_lds((const void*)kernel, w->atoms, s_rows, &lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(kernel, dim3(n_env), dim3(DUELING_THREADS), lds, (hipStream_t)stream, w->w_hv, w->b_hv, w->w_zv, w->b_zv,
                       w->w_ha, w->b_ha, w->w_za, w->b_za, xg_dev, x_dev, support_dev, obs_dev, action_dev, q_out_dev, v_out_dev,
                       a_out_dev, g);
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    if (resident || (!action_dev && !q_out_dev)) return IRBPP_OK;
    if (!dueling_lds((const void*)irbpp_streams_finish_kernel, w->atoms, s_rows, &lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(irbpp_streams_finish_kernel, dim3(n_env), dim3(DUELING_THREADS), lds, (hipStream_t)stream, w->w_hv, w->b_hv,
                       w->w_zv, w->b_zv, xg_dev, (const float*)a_out_dev, support_dev, obs_dev, action_dev, q_out_dev, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

static bool streams_grad_shape_bad(int32_t embed, int32_t hidden, int32_t atoms, int32_t s_rows, int32_t batch) {
    return embed < 1 || embed > STREAMS_GRAD_MAX_WIDTH || hidden < 1 || hidden > STREAMS_GRAD_MAX_WIDTH || atoms < 2 ||
           atoms > HEAD_MAX_ATOMS || s_rows < 1 || s_rows > HEAD_MAX_ROWS || batch < 1 || batch > STREAMS_GRAD_MAX_BATCH;
}

int64_t irbpp_streams_backward_workspace(int32_t embed, int32_t hidden, int32_t atoms, int32_t s_rows, int32_t batch) {
    if (streams_grad_shape_bad(embed, hidden, atoms, s_rows, batch)) return 0;
    return (int64_t)batch * streams_grad_sample_floats(embed, hidden, atoms) * (int64_t)sizeof(float);
}

int irbpp_streams_backward(const irbpp_stream_weights* w, const irbpp_stream_noise* eps, const float* xg_dev, int64_t xg_stride,
                           const float* x_dev, int64_t env_stride, int64_t row_stride, const float* ga_dev, const float* gv_dev,
                           int32_t s_rows, int32_t batch, float* workspace_dev, float* dx_dev, float* dxg_dev,
                           const irbpp_stream_grads* grads, void* stream) {
    if (!w || !grads || !w->w_hv || !w->b_hv || !w->w_zv || !w->b_zv || !w->w_ha || !w->b_ha || !w->w_za || !w->b_za ||
        streams_grad_shape_bad(w->embed, w->hidden, w->atoms, s_rows, batch) || !workspace_dev || !xg_dev ||
        xg_stride < w->embed || !x_dev || row_stride < w->embed || env_stride < (int64_t)(s_rows - 1) * row_stride + w->embed ||
        (eps && (!eps->w_hv || !eps->b_hv || !eps->w_zv || !eps->b_zv || !eps->w_ha || !eps->b_ha || !eps->w_za || !eps->b_za)))
        return IRBPP_ERR_ARG;
    const hipStream_t st = (hipStream_t)stream;
    StreamsGradArgs g;
    g.xg_stride = xg_stride, g.env_stride = env_stride, g.row_stride = row_stride;
    g.embed = w->embed, g.hidden = w->hidden, g.atoms = w->atoms, g.s_rows = s_rows, g.batch = batch;
    g.w_ha_vec4 = (w->embed % 4 == 0 && (uintptr_t)w->w_ha % 16 == 0) ? 1 : 0;
    g.w_za_vec4 = (w->hidden % 4 == 0 && (uintptr_t)w->w_za % 16 == 0) ? 1 : 0;
    if (gv_dev) {
        hipLaunchKernelGGL(irbpp_streams_grad_value_kernel, dim3(batch), dim3(STREAMS_GRAD_VALUE_THREADS), 0, st, w->w_hv, w->b_hv,
                           w->w_zv, xg_dev, gv_dev, workspace_dev, dxg_dev, g);
    } else if (dxg_dev) {
        const long long n = (long long)batch * w->embed;
        hipLaunchKernelGGL(irbpp_streams_grad_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dxg_dev, n);
    }
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    if (ga_dev) {
        const size_t lds = streams_grad_lds_bytes(w->embed, w->hidden, w->atoms);
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)irbpp_streams_grad_rows_kernel,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return IRBPP_ERR_HIP;
        hipLaunchKernelGGL(irbpp_streams_grad_rows_kernel, dim3(batch), dim3(STREAMS_GRAD_THREADS), lds, st, w->w_ha, w->b_ha, w->w_za,
                           x_dev, ga_dev, workspace_dev, dx_dev, g);
    } else if (dx_dev) {
        const long long n = (long long)batch * s_rows * w->embed;
        hipLaunchKernelGGL(irbpp_streams_grad_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dx_dev, n);
    }
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    StreamsGradOut oa, ov;
    oa.h_w_mu = grads->ha_weight_mu, oa.h_w_sigma = grads->ha_weight_sigma, oa.h_b_mu = grads->ha_bias_mu, oa.h_b_sigma = grads->ha_bias_sigma;
    oa.z_w_mu = grads->za_weight_mu, oa.z_w_sigma = grads->za_weight_sigma, oa.z_b_mu = grads->za_bias_mu, oa.z_b_sigma = grads->za_bias_sigma;
    ov.h_w_mu = grads->hv_weight_mu, ov.h_w_sigma = grads->hv_weight_sigma, ov.h_b_mu = grads->hv_bias_mu, ov.h_b_sigma = grads->hv_bias_sigma;
    ov.z_w_mu = grads->zv_weight_mu, ov.z_w_sigma = grads->zv_weight_sigma, ov.z_b_mu = grads->zv_bias_mu, ov.z_b_sigma = grads->zv_bias_sigma;
    oa.h_w_eps = eps ? eps->w_ha : nullptr, oa.h_b_eps = eps ? eps->b_ha : nullptr, oa.z_w_eps = eps ? eps->w_za : nullptr;
    oa.z_b_eps = eps ? eps->b_za : nullptr;
    ov.h_w_eps = eps ? eps->w_hv : nullptr, ov.h_b_eps = eps ? eps->b_hv : nullptr, ov.z_w_eps = eps ? eps->w_zv : nullptr;
    ov.z_b_eps = eps ? eps->b_zv : nullptr;
    const long long elems = 2 * ((long long)w->hidden * w->embed + (long long)w->atoms * w->hidden + w->hidden + w->atoms);
    hipLaunchKernelGGL(irbpp_streams_grad_reduce_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st,
                       (const float*)workspace_dev, xg_dev, gv_dev, oa, ov, ga_dev ? 1 : 0, gv_dev ? 1 : 0, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_shape_features_chunks(int32_t n_shapes, int32_t k) {
    if (n_shapes < 1 || n_shapes > SHAPE_MAX_SHAPES || k < 1 || k > SHAPE_MAX_POINTS) return 0;
    return shape_chunks(n_shapes, k);
}

int irbpp_shape_features(const float* points_dev, int32_t n_shapes, int32_t n_points, const int32_t* indices_dev, int32_t k,
                         const void* ids_dev, int32_t ids_are_float, int32_t ids_stride, int32_t m_rows,
                         const irbpp_shape_encoder* enc, float* partial_dev, int32_t partial_chunks, float* out_dev,
                         int32_t out_stride, void* stream) {
    if (!points_dev || !indices_dev || !ids_dev || !enc || !enc->w1 || !enc->b1 || !enc->w2 || !enc->b2 || !partial_dev ||
        !out_dev || enc->hidden < 1 || enc->hidden > SHAPE_MAX_WIDTH || enc->feat < 1 || enc->feat > SHAPE_MAX_WIDTH ||
        !(enc->slope >= 0.0f) || k < 1 || k > SHAPE_MAX_POINTS || n_shapes < 1 || n_shapes > SHAPE_MAX_SHAPES || n_points < 1 ||
        m_rows < 1 || ids_stride < 1 || out_stride < enc->feat || partial_chunks != shape_chunks(n_shapes, k))
        return IRBPP_ERR_ARG;
    ShapeArgs g;
    g.ids_stride = ids_stride, g.m_rows = m_rows, g.out_stride = out_stride;
    g.n_shapes = n_shapes, g.n_points = n_points, g.k = k, g.ids_are_float = ids_are_float != 0, g.hidden = enc->hidden;
    g.feat = enc->feat, g.chunk_points = shape_chunk_points(n_shapes, k), g.chunks = partial_chunks, g.slope = enc->slope;
    const int threads = shape_threads(enc->feat);
    hipLaunchKernelGGL(irbpp_shape_partial_kernel, dim3(n_shapes, partial_chunks), dim3(threads), 0, (hipStream_t)stream, points_dev,
                       indices_dev, ids_dev, enc->w1, enc->b1, enc->w2, enc->b2, partial_dev, g);
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    const long long elems = (long long)m_rows * enc->feat;
    hipLaunchKernelGGL(irbpp_shape_gather_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)partial_dev, ids_dev, out_dev, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

static bool shape_call_bad(const void* points_dev, int32_t n_shapes, int32_t n_points, const void* indices_dev, int32_t k,
                           const void* ids_dev, int32_t ids_stride, int32_t m_rows, const irbpp_shape_encoder* enc) {
    return !points_dev || !indices_dev || !ids_dev || !enc || !enc->w1 || !enc->b1 || !enc->w2 || !enc->b2 || enc->hidden < 1 ||
           enc->hidden > SHAPE_MAX_WIDTH || enc->feat < 1 || enc->feat > SHAPE_MAX_WIDTH || !(enc->slope >= 0.0f) || k < 1 ||
           k > SHAPE_MAX_POINTS || n_shapes < 1 || n_shapes > SHAPE_MAX_SHAPES || n_points < 1 || m_rows < 1 || ids_stride < 1;
}

int irbpp_shape_features_arg(const float* points_dev, int32_t n_shapes, int32_t n_points, const int32_t* indices_dev, int32_t k,
                             const void* ids_dev, int32_t ids_are_float, int32_t ids_stride, int32_t m_rows,
                             const irbpp_shape_encoder* enc, uint32_t* partial_key_dev, int32_t* partial_j_dev,
                             int32_t partial_chunks, float* out_dev, int32_t out_stride, int32_t* arg_dev, void* stream) {
    if (shape_call_bad(points_dev, n_shapes, n_points, indices_dev, k, ids_dev, ids_stride, m_rows, enc) || !partial_key_dev ||
        !partial_j_dev || !out_dev || !arg_dev || out_stride < enc->feat || partial_chunks != shape_chunks(n_shapes, k))
        return IRBPP_ERR_ARG;
    ShapeArgs g;
    g.ids_stride = ids_stride, g.m_rows = m_rows, g.out_stride = out_stride;
    g.n_shapes = n_shapes, g.n_points = n_points, g.k = k, g.ids_are_float = ids_are_float != 0, g.hidden = enc->hidden;
    g.feat = enc->feat, g.chunk_points = shape_chunk_points(n_shapes, k), g.chunks = partial_chunks, g.slope = enc->slope;
    hipLaunchKernelGGL(irbpp_shape_partial_arg_kernel, dim3(n_shapes, partial_chunks), dim3(shape_threads(enc->feat)), 0,
                       (hipStream_t)stream, points_dev, indices_dev, ids_dev, enc->w1, enc->b1, enc->w2, enc->b2, partial_key_dev,
                       partial_j_dev, g);
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    const long long elems = ((long long)m_rows + n_shapes) * enc->feat;
    hipLaunchKernelGGL(irbpp_shape_gather_arg_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t*)partial_key_dev, (const int32_t*)partial_j_dev, ids_dev, out_dev, arg_dev, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_shape_features_backward(const float* points_dev, int32_t n_shapes, int32_t n_points, const int32_t* indices_dev, int32_t k,
                                  const void* ids_dev, int32_t ids_are_float, int32_t ids_stride, int32_t m_rows,
                                  const irbpp_shape_encoder* enc, const int32_t* arg_dev, const float* grad_out_dev,
                                  float* point_d2_dev, float* first_dev, float* d_w1_dev, float* d_b1_dev, float* d_w2_dev,
                                  float* d_b2_dev, void* stream) {
    if (shape_call_bad(points_dev, n_shapes, n_points, indices_dev, k, ids_dev, ids_stride, m_rows, enc) || !arg_dev ||
        !grad_out_dev || !point_d2_dev || !first_dev || (uintptr_t)point_d2_dev % 16 != 0 || (uintptr_t)first_dev % 16 != 0 ||
        !d_w1_dev || !d_b1_dev || !d_w2_dev || !d_b2_dev)
        return IRBPP_ERR_ARG;
    ShapeGradArgs g;
    g.ids_stride = ids_stride, g.m_rows = m_rows, g.n_shapes = n_shapes, g.n_points = n_points, g.k = k;
    g.ids_are_float = ids_are_float != 0, g.hidden = enc->hidden, g.feat = enc->feat, g.slope = enc->slope;
    hipLaunchKernelGGL(irbpp_shape_backward_shape_kernel, dim3(n_shapes), dim3(SHAPE_GRAD_THREADS), 0, (hipStream_t)stream, points_dev,
                       indices_dev, ids_dev, enc->w1, enc->b1, enc->w2, enc->b2, arg_dev, grad_out_dev, (ShapeQuad*)point_d2_dev,
                       (ShapeQuad*)first_dev, g);
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    const long long elems = (long long)enc->feat * enc->hidden + enc->feat + 4LL * enc->hidden;
    hipLaunchKernelGGL(irbpp_shape_backward_reduce_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       enc->w1, enc->b1, arg_dev, (const ShapeQuad*)point_d2_dev, (const ShapeQuad*)first_dev, d_w1_dev, d_b1_dev,
                       d_w2_dev, d_b2_dev, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

// the heightmap encoder's part of irbpp_embed_weights and of irbpp_order_embed_weights is outside its limits: one of its six
// arrays missing, map_len, c1, c2 or c3 out of range, or a slope that is not >= 0 (a NaN among them: read from the bits, since
// the library is built with -fno-honor-nans, under which a comparison inside a function need not reject a NaN)
extern "C++" {
template <typename W>
static bool front_encoder_bad(const W* w) {
    uint32_t slope_bits;
    memcpy(&slope_bits, &w->slope, 4);
    return !w->w_conv1 || !w->b_conv1 || !w->w_conv2 || !w->b_conv2 || !w->w_conv3 || !w->b_conv3 || w->map_len < 8 ||
           w->map_len > EMBED_MAX_MAP || w->map_len % 4 != 0 || w->c1 < 1 || w->c1 > EMBED_MAX_C1 || w->c2 < 1 ||
           w->c2 > EMBED_MAX_C2 || w->c3 < 1 || w->c3 > EMBED_MAX_C3 || (slope_bits > 0x7f800000u && slope_bits != 0x80000000u);
}
}  // extern "C++"

// a rows kernel may be launched with `bytes` of dynamic LDS: above 64 KB the limit has to be raised first
static bool front_rows_lds(const void* kernel, size_t bytes) {
    return bytes <= 64 * 1024 || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

// the two forms of the embedding stage: the bin kernel, then `rows_kernel` (irbpp_embed_rows_kernel or its MFMA form, which
// needs the K of its three products, width_step = 4, never padded)
extern "C++" {
template <typename K>
static int embed_launch(K rows_kernel, int width_step, const irbpp_embed_weights* w, const float* obs_dev, int64_t obs_stride,
                        const float* shape_feat_dev, int64_t feat_stride, int32_t s_rows, int32_t n_env, float* base_dev,
                        float* x_dev, int64_t env_stride, int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream) {
    if (!w || front_encoder_bad(w) || !w->w_c1 || !w->b_c1 || !w->w_c2 || !w->b_c2 || !w->w_p1 || !w->b_p1 || !w->w_p2 ||
        !w->b_p2 || !obs_dev || !shape_feat_dev || !base_dev || !x_dev || !xg_dev || w->feat < 1 || w->feat > EMBED_MAX_WIDTH ||
        w->cand_embed < 1 || w->cand_embed > EMBED_MAX_WIDTH || w->proj_hidden < 1 || w->proj_hidden > EMBED_MAX_WIDTH ||
        w->embed < 1 || w->embed > EMBED_MAX_WIDTH || w->cand_hidden < 1 || w->cand_hidden > EMBED_MAX_CAND_HIDDEN || s_rows < 1 ||
        s_rows > HEAD_MAX_ROWS || n_env < 1 ||
        obs_stride < (int64_t)5 * s_rows + 9 + (int64_t)w->map_len * w->map_len || feat_stride < w->feat || row_stride < w->embed ||
        env_stride < (int64_t)(s_rows - 1) * row_stride + w->embed || xg_stride < w->embed ||
        w->cand_hidden % width_step || w->cand_embed % width_step || w->proj_hidden % width_step)
        return IRBPP_ERR_ARG;
    EmbedArgs g;
    g.obs_stride = obs_stride, g.feat_stride = feat_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.xg_stride = xg_stride;
    g.map_len = w->map_len, g.c1 = w->c1, g.c2 = w->c2, g.c3 = w->c3, g.feat = w->feat, g.cand_hidden = w->cand_hidden;
    g.cand_embed = w->cand_embed, g.proj_hidden = w->proj_hidden, g.embed = w->embed, g.s_rows = s_rows, g.slope = w->slope;
    hipLaunchKernelGGL(irbpp_embed_bin_kernel, dim3(n_env), dim3(EMBED_BIN_THREADS), 0, (hipStream_t)stream, w->w_conv1, w->b_conv1,
                       w->w_conv2, w->b_conv2, w->w_conv3, w->b_conv3, w->w_p1, w->b_p1, obs_dev, shape_feat_dev, base_dev, g);
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    const size_t lds = (size_t)embed_rows_lds_floats(w->cand_hidden, w->cand_embed, w->proj_hidden, w->embed) * sizeof(float);
    if (!front_rows_lds((const void*)rows_kernel, lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(rows_kernel, dim3(n_env), dim3(EMBED_ROW_THREADS), lds, (hipStream_t)stream, w->w_c1, w->b_c1, w->w_c2,
                       w->b_c2, w->w_p1, w->w_p2, w->b_p2, obs_dev, (const float*)base_dev, x_dev, xg_dev, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}
}  // extern "C++"

int irbpp_embed(const irbpp_embed_weights* w, const float* obs_dev, int64_t obs_stride, const float* shape_feat_dev,
                int64_t feat_stride, int32_t s_rows, int32_t n_env, float* base_dev, float* x_dev, int64_t env_stride,
                int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream) {
    return embed_launch(irbpp_embed_rows_kernel, 1, w, obs_dev, obs_stride, shape_feat_dev, feat_stride, s_rows, n_env, base_dev, x_dev,
                        env_stride, row_stride, xg_dev, xg_stride, stream);
}

int irbpp_embed_mfma(const irbpp_embed_weights* w, const float* obs_dev, int64_t obs_stride, const float* shape_feat_dev,
                     int64_t feat_stride, int32_t s_rows, int32_t n_env, float* base_dev, float* x_dev, int64_t env_stride,
                     int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream) {
    return embed_launch(irbpp_embed_rows_mfma_kernel, 4, w, obs_dev, obs_stride, shape_feat_dev, feat_stride, s_rows, n_env, base_dev,
                        x_dev, env_stride, row_stride, xg_dev, xg_stride, stream);
}

// the two forms of the order network's embedding stage: the bin kernel, then `rows_kernel` (irbpp_order_rows_kernel or its MFMA
// form, which needs the K of its eight products, width_step = 4, never padded) with `lds` bytes of dynamic LDS
extern "C++" {
template <typename K>
static int order_embed_launch(K rows_kernel, int width_step, const irbpp_order_embed_weights* w, const float* obs_dev, int64_t obs_stride,
                              const float* shape_feat_dev, int64_t feat_stride, int32_t k_slots, int32_t n_env, float* base_dev,
                              float* x_dev, int64_t env_stride, int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream) {
    if (!w || front_encoder_bad(w) || !w->w_g1 || !w->b_g1 || !w->w_g2 || !w->b_g2 || !w->w_q || !w->w_k || !w->w_v || !w->w_o ||
        !w->b_o || !w->w_f1 || !w->b_f1 || !w->w_f2 || !w->b_f2 || !obs_dev || !shape_feat_dev || !base_dev || !x_dev || !xg_dev ||
        w->feat < 1 || w->feat > ORDER_MAX_WIDTH || w->proj_hidden < 1 || w->proj_hidden > ORDER_MAX_WIDTH || w->embed < 1 ||
        w->embed > ORDER_MAX_WIDTH || w->ff_hidden < 1 || w->ff_hidden > ORDER_MAX_WIDTH || k_slots < 2 || k_slots > ORDER_MAX_SLOTS ||
        n_env < 1 || obs_stride < (int64_t)k_slots + (int64_t)w->map_len * w->map_len || feat_stride < w->feat ||
        row_stride < w->embed || env_stride < (int64_t)(k_slots - 1) * row_stride + w->embed || xg_stride < w->embed ||
        w->feat % width_step || w->proj_hidden % width_step || w->embed % width_step || w->ff_hidden % width_step)
        return IRBPP_ERR_ARG;
    OrderEmbedArgs g;
    g.obs_stride = obs_stride, g.feat_stride = feat_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.xg_stride = xg_stride;
    g.map_len = w->map_len, g.c1 = w->c1, g.c2 = w->c2, g.c3 = w->c3, g.feat = w->feat, g.proj_hidden = w->proj_hidden;
    g.embed = w->embed, g.ff_hidden = w->ff_hidden, g.k_slots = k_slots, g.n_env = n_env, g.slope = w->slope;
    g.norm = (float)(1.0 / sqrt((double)w->embed));
    hipLaunchKernelGGL(irbpp_order_bin_kernel, dim3(n_env), dim3(EMBED_BIN_THREADS), 0, (hipStream_t)stream, w->w_conv1, w->b_conv1,
                       w->w_conv2, w->b_conv2, w->w_conv3, w->b_conv3, w->w_g1, w->b_g1, obs_dev, base_dev, g);
    if (hipGetLastError() != hipSuccess) return IRBPP_ERR_HIP;
    const int lds_floats = width_step == 1 ? order_rows_lds_floats(w->feat, w->proj_hidden, w->embed, w->ff_hidden, k_slots)
                                           : order_rows_mfma_lds_floats(w->feat, w->proj_hidden, w->embed, w->ff_hidden, k_slots);
    const size_t lds = (size_t)lds_floats * sizeof(float);
    if (!front_rows_lds((const void*)rows_kernel, lds)) return IRBPP_ERR_HIP;
    hipLaunchKernelGGL(rows_kernel, dim3(order_tiles(n_env, k_slots)), dim3(EMBED_ROW_THREADS), lds, (hipStream_t)stream,
                       w->w_g1, w->w_g2, w->b_g2, w->w_q, w->w_k, w->w_v, w->w_o, w->b_o, w->w_f1, w->b_f1, w->w_f2, w->b_f2,
                       shape_feat_dev, (const float*)base_dev, x_dev, xg_dev, g);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}
}  // extern "C++"

int irbpp_order_embed(const irbpp_order_embed_weights* w, const float* obs_dev, int64_t obs_stride, const float* shape_feat_dev,
                      int64_t feat_stride, int32_t k_slots, int32_t n_env, float* base_dev, float* x_dev, int64_t env_stride,
                      int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream) {
    return order_embed_launch(irbpp_order_rows_kernel, 1, w, obs_dev, obs_stride, shape_feat_dev, feat_stride, k_slots, n_env, base_dev,
                              x_dev, env_stride, row_stride, xg_dev, xg_stride, stream);
}

int irbpp_order_embed_mfma(const irbpp_order_embed_weights* w, const float* obs_dev, int64_t obs_stride, const float* shape_feat_dev,
                           int64_t feat_stride, int32_t k_slots, int32_t n_env, float* base_dev, float* x_dev, int64_t env_stride,
                           int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream) {
    return order_embed_launch(irbpp_order_rows_mfma_kernel, 4, w, obs_dev, obs_stride, shape_feat_dev, feat_stride, k_slots, n_env,
                              base_dev, x_dev, env_stride, row_stride, xg_dev, xg_stride, stream);
}

int irbpp_replay_gather(const irbpp_replay_view* v, int32_t draws, float beta, const int64_t* data_idx_dev, const float* prob_dev,
                        float* state_dev, int64_t* action_dev, float* return_dev, float* next_state_dev, float* nonterminal_dev,
                        float* weight_dev, void* stream) {
    if (!v || !v->states_dev || !v->actions_dev || !v->rewards_dev || !v->nonterminals_dev || !v->tree_dev || !v->index_dev ||
        !v->full_dev || !v->scaling_dev || v->n_env < 1 || v->capacity < 1 || v->obs_len < 1 || v->n_step < 1 || draws < 1 ||
        draws > 256 || !data_idx_dev || !prob_dev || !state_dev || !action_dev || !return_dev || !next_state_dev ||
        !nonterminal_dev || !weight_dev)
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_replay_gather_kernel, dim3(v->n_env), dim3(256), 0, (hipStream_t)stream, v->states_dev, v->actions_dev,
                       v->rewards_dev, v->nonterminals_dev, v->tree_dev, v->index_dev, v->full_dev, v->scaling_dev, v->capacity,
                       v->obs_len, v->n_step, draws, beta, data_idx_dev, prob_dev, state_dev, action_dev, return_dev,
                       next_state_dev, nonterminal_dev, weight_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_replay_append(const irbpp_replay_store* m, const float* state_dev, int64_t state_stride, const void* action_dev,
                        int32_t action_bytes, const void* reward_dev, int32_t reward_bytes, const uint8_t* terminal_dev,
                        const uint8_t* valid_dev, void* stream) {
    if (!m || !m->states_dev || !m->actions_dev || !m->rewards_dev || !m->nonterminals_dev || !m->timesteps_dev || !m->tree_dev ||
        !m->max_dev || !m->index_dev || !m->full_dev || !m->t_dev || m->n_env < 1 || m->capacity < 1 || m->obs_len < 1 ||
        !state_dev || state_stride < m->obs_len || !action_dev || (action_bytes != 4 && action_bytes != 8) || !reward_dev ||
        (reward_bytes != 4 && reward_bytes != 8) || !terminal_dev)
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_replay_append_kernel, dim3(m->n_env), dim3(256), 0, (hipStream_t)stream, m->states_dev, m->actions_dev,
                       m->rewards_dev, m->nonterminals_dev, m->timesteps_dev, m->tree_dev, m->max_dev, m->index_dev, m->full_dev,
                       m->t_dev, m->capacity, m->obs_len, state_dev, (long long)state_stride, action_dev, action_bytes, reward_dev,
                       reward_bytes, terminal_dev, valid_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

static bool replay_view_ok(const irbpp_replay_view* v) {
    return v && v->states_dev && v->actions_dev && v->rewards_dev && v->nonterminals_dev && v->tree_dev && v->index_dev &&
           v->full_dev && v->scaling_dev && v->n_env >= 1 && v->capacity >= 1 && v->capacity <= (1 << 30) && v->obs_len >= 1 &&
           v->n_step >= 1;
}

int irbpp_replay_pool_sample(const irbpp_replay_view* v, int32_t draws, const float* values_dev, uint64_t seed, int32_t max_tries,
                             float beta, int64_t* env_dev, float* prob_dev, int64_t* data_idx_dev, int64_t* tree_idx_dev,
                             float* weight_dev, int32_t* failed_dev, void* stream) {
    if (!replay_view_ok(v) || draws < 1 || draws > POOL_MAX_DRAWS || max_tries < 1 || !env_dev || !prob_dev || !data_idx_dev ||
        !tree_idx_dev || !weight_dev || !failed_dev)
        return IRBPP_ERR_ARG;
    if (v->n_env > SUMTREE_LDS / 2) return IRBPP_ERR_ARG;            // the top tree over 8192 leaves is the LDS row
    int top_leaves = 1;
    while (top_leaves < v->n_env) top_leaves <<= 1;
    const int floats = 2 * top_leaves - 1 < 8 ? 8 : 2 * top_leaves - 1;
    hipLaunchKernelGGL(irbpp_replay_pool_sample_kernel, dim3(1), dim3(256), (size_t)floats * sizeof(float), (hipStream_t)stream,
                       v->tree_dev, v->index_dev, v->full_dev, v->n_env, v->capacity, top_leaves, draws, v->n_step, values_dev, seed,
                       max_tries, beta, env_dev, prob_dev, data_idx_dev, tree_idx_dev, weight_dev, failed_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_replay_pool_gather(const irbpp_replay_view* v, int32_t draws, const int64_t* env_dev, const int64_t* data_idx_dev,
                             float* state_dev, int64_t* action_dev, float* return_dev, float* next_state_dev,
                             float* nonterminal_dev, void* stream) {
    if (!replay_view_ok(v) || draws < 1 || !env_dev || !data_idx_dev || !state_dev || !action_dev || !return_dev ||
        !next_state_dev || !nonterminal_dev)
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_replay_pool_gather_kernel, dim3(draws), dim3(256), 0, (hipStream_t)stream, v->states_dev, v->actions_dev,
                       v->rewards_dev, v->nonterminals_dev, v->scaling_dev, v->n_env, v->capacity, v->obs_len, v->n_step, env_dev,
                       data_idx_dev, state_dev, action_dev, return_dev, next_state_dev, nonterminal_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_replay_pool_update(float* tree_dev, float* max_dev, int32_t n_env, int32_t capacity, const int64_t* env_dev,
                             const int64_t* tree_idx_dev, const float* priority_dev, int32_t count, void* stream) {
    if (!tree_dev || !max_dev || !env_dev || !tree_idx_dev || !priority_dev || n_env < 1 || capacity < 1 || capacity > (1 << 30) ||
        count < 1 || count > POOL_MAX_DRAWS)
        return IRBPP_ERR_ARG;
    hipLaunchKernelGGL(irbpp_replay_pool_update_kernel, dim3(1), dim3((count + 63) / 64 * 64), 0, (hipStream_t)stream, tree_dev,
                       max_dev, n_env, capacity, env_dev, tree_idx_dev, priority_dev, count);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_debug_phase_cycles(irbpp_env* env, int64_t* cycles_dev) {
    if (!env) return IRBPP_ERR_ARG;
    drop_graphs(env);
    env->phase_cycles = (long long*)cycles_dev;
    return IRBPP_OK;
}

int irbpp_debug_kernel_info(const irbpp_env* env, int32_t* lds_bytes, const char** kernel_name) {
    if (!env || !lds_bytes || !kernel_name) return IRBPP_ERR_ARG;
    const Params& P = env->P;
    *lds_bytes = P.lds_bytes;
    // the plan of a step over all bins of this environment, rendered: the kernels of its observation in launch order (a buffered
    // step observes nothing: the plan of the get_action_candidates behind it), then where the step's actions are applied
    const Plan step = plan_transition(P, env->cfg.tuning, MODE_STEP, P.N, PLAN_KEY_CAND, false, false, env->heavy_turn, env->item_order);
    const Plan obs = P.K > 1 ? plan_transition(P, env->cfg.tuning, MODE_CANDS, P.N, PLAN_KEY_CAND, false, false, env->heavy_turn, false) : step;
    std::string text;
    int shown = 0, last = -1, apply = -1;
    for (int i = 0; i < obs.n_launches; ++i) {
        const int k = obs.launch[i].kernel;
        if (is_apply_kernel(k) || k == K_ITEM_ORDER) continue;
        text += shown++ ? " + " : "";
        text += kernel_info(last = k).name;
    }
    for (int i = 0; i < step.n_launches; ++i)
        if (is_apply_kernel(step.launch[i].kernel)) apply = step.launch[i].kernel;
    const bool alone = apply >= 0 && step.launch[step.n_launches - 1].kernel == apply;
    const std::string applied = apply >= 0 ? kernel_info(apply).name : "";
    if (shown == 1 && last == K_WIDE) {
        // (what sends the configuration there: the grid, and / or more height levels than the tuned pipeline codes)
        const int levels = (int)floor(P.bin_z / P.res_z + 1e-9);
        text += " alone (action grid of " + std::to_string(P.Ax) + " x " + std::to_string(P.Ay) + " cells";
        if (levels > TUNED_MAX_LEVELS) text += ", " + std::to_string(levels) + " height levels";
        text += ")";
        if (alone) text += " (step: the apply kernel alone)";
        else if (apply >= 0) text += " (step: " + applied + " in front)";
    } else {
        if (shown == 1) text += " alone (observation finished in the bin's workgroup)";
        if (alone) text += " (step: " + applied + " alone)";
        else if (apply >= 0) text += " (step: " + applied + " in front, transition kernel in MODE_OBSERVE)";
    }
    snprintf(const_cast<irbpp_env*>(env)->kernel_names, sizeof env->kernel_names, "%s", text.c_str());
    *kernel_name = env->kernel_names;
    return IRBPP_OK;
}

int irbpp_overlap_path(const irbpp_env* env) {
    if (!env) return IRBPP_ERR_ARG;
    if (!env->shapes_loaded) return IRBPP_ERR_STATE;
    return env->P.block_b > 0 ? (all_block(env->P) ? 1 : 4) : (env->P.box ? 2 : 3);
}

int irbpp_debug_kernel_timing_every(irbpp_env* env, int32_t every) {
    if (!env || every < 1) return IRBPP_ERR_ARG;
    env->timing_every = every;
    env->timing_phase = 0;
    return IRBPP_OK;
}

int irbpp_debug_kernel_timing(irbpp_env* env, int32_t capacity) {
    if (!env || capacity < 0) return IRBPP_ERR_ARG;
    HIP_TRY(hipSetDevice(env->cfg.device));
    for (hipEvent_t e : env->timing) hipEventDestroy(e);
    env->timing.clear();
    env->timing_next = env->timing_used = 0;
    for (int i = 0; i < 2 * capacity; ++i) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        env->timing.push_back(e);
    }
    return IRBPP_OK;
}

int irbpp_debug_kernel_times(irbpp_env* env, float* ms_host, int32_t max_count, int32_t* count) {
    if (!env || !ms_host || !count || max_count < 0) return IRBPP_ERR_ARG;
    const size_t pairs = env->timing.size() / 2;
    size_t n = env->timing_used < (size_t)max_count ? env->timing_used : (size_t)max_count;
    for (size_t i = 0; i < n; ++i) {                   // the n latest launches, oldest first
        const size_t slot = (env->timing_next + pairs - n + i) % pairs;
        HIP_TRY(hipEventSynchronize(env->timing[2 * slot + 1]));
        HIP_TRY(hipEventElapsedTime(&ms_host[i], env->timing[2 * slot], env->timing[2 * slot + 1]));
    }
    *count = (int32_t)n;
    env->timing_next = env->timing_used = 0;
    return IRBPP_OK;
}

int irbpp_debug_round_cap(irbpp_env* env, int32_t cap) {
    if (!env || env->P.wide || cap < 1 || cap > env->round_cap_alloc) return IRBPP_ERR_ARG;
    if (env->transition_launched) return IRBPP_ERR_STATE;       // (one stride for the lists' whole life: irbpp.h)
    drop_graphs(env);
    env->P.round_cap = cap;
    return IRBPP_OK;
}

int irbpp_debug_round_counts(irbpp_env* env, int32_t out[8], void* stream) {
    static_assert(NXCD == 8, "irbpp.h documents eight lists");
    if (!env || !out || env->P.wide) return IRBPP_ERR_ARG;
    if (env->round_snap == nullptr) {                           // the first call switches the recording on
        HIP_TRY(hipSetDevice(env->cfg.device));
        drop_graphs(env);                                       // (a captured chain has no copy node yet)
        const int rc = dev_alloc(env, &env->round_snap, NXCD * XCD_STRIDE);
        if (rc != IRBPP_OK) { env->round_snap = nullptr; return rc; }
    }
    int32_t words[NXCD * XCD_STRIDE];
    HIP_TRY(hipMemcpyAsync(words, env->round_snap, sizeof words, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int s = 0; s < NXCD; ++s) out[s] = words[s * XCD_STRIDE];
    return IRBPP_OK;
}

int irbpp_device_error(irbpp_env* env, void* stream, int32_t* flags_out) {
    if (!env || !flags_out) return IRBPP_ERR_ARG;
    HIP_TRY(hipMemcpyAsync(flags_out, env->S.err, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return *flags_out ? IRBPP_ERR_DEVICE : IRBPP_OK;
}

}  // extern "C"
