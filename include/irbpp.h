/*
 * irbpp.h -- C ABI of the MI355X-native batched packing environment (libirbpp_hip.so).
 *
 * The reference (alexfrom0815/IR-BPP) has no FFI: its environment is Python behind the
 * VecEnv protocol (wrapper/vec_env.py:29-138, wrapper/shmem_vec_env.py:20-157).  This
 * header is the boundary a maintainer binds instead of spawning one process per bin:
 * each entry point names the reference interface it replaces.  INTEGRATION.md shows the
 * ctypes stub.
 *
 * Conventions
 *   - every function returns 0 (IRBPP_OK) or a negative irbpp_status; no exceptions cross
 *     the ABI; irbpp_status_string() explains a code.
 *   - "_dev" pointers are caller-owned device (HBM) memory; everything else is host memory.
 *   - launches are asynchronous on the given hipStream_t (passed as void*; NULL = the null
 *     stream); a handle is not thread-safe; one outstanding step per handle (the
 *     reference's `waiting_step` rule, shmem_vec_env.py:58-74).
 *   - observation buffers are written in full on every call, so the caller may hand a
 *     fresh buffer each step (trainer.py:184-186 keeps the previous `state` alive); a buffer
 *     handed over with irbpp_register_obs_buffer is kept complete by the library instead
 *     (same contents, fewer stores).
 *
 * Limits (irbpp_create returns IRBPP_ERR_ARG beyond them): action grid <= 32 x 32 cells, heightmap <= 128 x 128 cells with
 * resolutionA an integer multiple of resolutionH and the bin an integer number of action cells; n_rot <= 8; selected <= 1024;
 * buffer_size <= 16; floor(bin[2] / resolution_z) <= 222 height levels (cvTools.py:78; a level is coded as level + 32 in a byte,
 * 255 meaning none); num_bins <= 1048576 per device.  Item ids are < 65536 in the placement log.
 * Two regimes: up to 16 x 16 action cells AND up to 31 height levels (every README command of the reference) run the tuned
 * pipeline.  17 .. 32 cells a side (resolutionA = 0.01), or 32 .. 222 height levels at any grid size (resolution_z = 0.005 on the
 * 0.30 m bin: 60; a 0.60 m bin at 0.01: 60), run the capacity path of csrc/irbpp_wide.hip, one kernel per observation, with the
 * same results and its own limits: heightmap <= 64 x 64 cells, no stability proxy (stability must be 0), and the stage-level
 * tooling entry points irbpp_possible_position, irbpp_heuristic_action and irbpp_convex_hull_actions answer IRBPP_ERR_ARG.
 */
#ifndef IRBPP_H
#define IRBPP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct irbpp_env irbpp_env;

typedef enum {
    IRBPP_OK = 0,
    IRBPP_ERR_ARG = -1,        /* bad argument / unsupported configuration          */
    IRBPP_ERR_HIP = -2,        /* a HIP runtime call failed                          */
    IRBPP_ERR_STATE = -3,      /* call order (e.g. step before load_shapes/reset)    */
    IRBPP_ERR_DEVICE = -4,     /* a kernel raised its error word (see irbpp_device_error) */
    IRBPP_ERR_NOMEM = -5
} irbpp_status;

/* Geometry and episode parameters: PackingGame.__init__ (binPhy.py:22-116),
 * Space.__init__ (space.py:15-47), Interface.__init__ (Interface.py:33-40). */
typedef struct {
    int32_t num_bins;        /* bins simulated on this device                                   */
    int32_t n_rot;           /* ZRotNum (arguments.py:117), 1..8                                 */
    int32_t selected;        /* selectedAction S (arguments.py:79), 1..1024                      */
    int32_t buffer_size;     /* bufferSize k (arguments.py:75); >1 = hierarchical, 1..16         */
    double  resolution_a;    /* resolutionA                                                      */
    double  resolution_h;    /* resolutionH                                                      */
    double  resolution_z;    /* resolutionZ = heightResolution (arguments.py:84,125)             */
    double  bin[3];          /* np.round([0.32,0.32,0.30], 6) (arguments.py:115)                 */
    double  scale_z;         /* Interface scale[2] = 100 (arguments.py:123)                      */
    int32_t traj_start;      /* trajectory of global bin 0's first episode; 1 = LoadItemCreator
                                (IRcreator.py:86-92 increments before first use)                */
    int32_t global_offset;   /* global index of this device's bin 0 (multi-GPU sharding)         */
    int32_t global_bins;     /* bins over all ranks = trajectory stride between episodes         */
    int32_t device;          /* HIP device ordinal                                               */
    int32_t stability;       /* stand-in for the rigid-body settling the path leaves out (Interface.py:271-310):
                                0 off; 1 every accepted placement is also rated by a static support test
                                (irbpp_step_out::stable_dev), results otherwise unchanged; 2 a placement that
                                fails the test is refused like one that does not fit (episode ends)          */
    int32_t tuning;          /* bit flags, none of which changes a result (A/B measurements and the parity test that
                                plays lattice data through both overlap paths): IRBPP_TUNE_*; 0 = the library decides */
    int32_t item_stream;     /* 0: trajectories (LoadItemCreator, IRcreator.py:74-103): episode e of global bin g reads row
                                (traj_start + g + e*global_bins) % n_traj from its start.  1: one endless stream per bin
                                (RandomItemCreator / RandomInstanceCreator / RandomCateCreator, IRcreator.py:26-72): bin b
                                of this device reads row b % n_traj and a new episode goes on where the last one stopped
                                (ItemCreator.reset only clears the queue); the row is a ring the host refills
                                (irbpp_stream_cursors)                                                          */
} irbpp_config;

#define IRBPP_TUNE_NO_BLOCK_PATH  1   /* lattice data (BlockOut) through the generic overlap test too               */
#define IRBPP_TUNE_WIDE_KERNEL    2   /* transition kernel without the 64-VGPR cap                                  */
#define IRBPP_TUNE_NARROW_KERNEL  4   /* transition kernel under the 64-VGPR cap even on the generic path           */
#define IRBPP_TUNE_NO_BOX_PATH    8   /* box data (Cube) through the generic overlap test too                       */
#define IRBPP_TUNE_NO_ITEM_ORDER 16   /* launch the bins in index order instead of grouped by observed item per XCD */
#define IRBPP_TUNE_TRACE_CPW64   32   /* border following with 64 / 32 / 16 candidate starts per wave whatever the number of */
#define IRBPP_TUNE_TRACE_CPW32   64   /* bins (default: by the number of bins, see launch_group in irbpp_capi.hip)          */
#define IRBPP_TUNE_TRACE_CPW16  128
#define IRBPP_TUNE_INLINE_POLYGON 256 /* every trace wave approximates the borders it followed itself; no polygon kernel (the
                                         path a full record list takes, forced for the parity tests; measured slower at every size) */
#define IRBPP_TUNE_NO_HEAVY_FIRST 512 /* emit kernel: the bins in launch order, speckled ones not first                        */
#define IRBPP_TUNE_FUSED_APPLY 2048 /* step(): the actions applied inside the transition kernel (one 256-thread workgroup per bin, as until
                                      round 4) whatever the size of the launch ...                                              */
#define IRBPP_TUNE_SPLIT_APPLY 4096 /* ... or by irbpp_apply_kernel (one wave per bin) in front of it whatever the size (default: split
                                      from the size on at which it pays, see split_apply in irbpp_capi.hip); identical results, for
                                      A/B runs and the parity tests                                                              */
#define IRBPP_TUNE_BLOCK_EMIT 8192 /* emit kernel: one 256-thread workgroup per bin also for lattice / box data (default there, from 2048
                                     bins per launch on: one wave per bin, four bins per workgroup); identical results          */
#define IRBPP_TUNE_WAVE_EMIT 16384 /* ... or the wave-per-bin form for lattice / box data whatever the size of the launch      */
#define IRBPP_TUNE_GRAPH 32768 /* step() / get_action_candidates() replayed as HIP graphs owned by the library (one per distinct argument
                                  set, captured at its second use) instead of launched kernel by kernel.  Off by default: slower on
                                  ROCm 7.2 at every size measured (launch_env in irbpp_capi.hip); identical results                 */
#define IRBPP_TUNE_WG512 65536 /* generic overlap path: the transition kernel with 512-thread workgroups (eight waves share a bin's tile)
                                  whatever the LDS per bin; default: where at most four 256-thread workgroups fit a CU's LDS      */
#define IRBPP_TUNE_NO_WG512 131072 /* ... never                                                                                 */
#define IRBPP_TUNE_TRACE_REFILL 262144 /* border following in batches of 128 candidate starts per wave whose lanes take the next candidate as
                                         they close their borders.  Off by default: measured slower at every size (profiles/r06/LOG.md,
                                         session 2); identical results, parity-tested                                                       */
#define IRBPP_TUNE_NO_MIXED_PATH 524288 /* a data set of which only SOME rotations are lattice footprints (BlockOut at eight rotations) through
                                          the cell lists entirely, as until round 5 (default: those rotations on the block path, the others on
                                          their lists, in one kernel); identical results                                                    */
#define IRBPP_TUNE_CHAIN 1048576     /* every observation as ONE kernel: the bin's workgroup also follows its borders, approximates them and
                                        writes the candidate rows (no trace / polygon / emit launches).  Off by default: measured slower at
                                        the launch sizes it was built for (irbpp_capi.hip: chain_launch); identical results, parity-tested  */
#define IRBPP_TUNE_WG128 2097152     /* BlockOut at R = 4: the transition kernel with 128-thread workgroups (two waves per bin, two action cells
                                        per thread); identical results, for A/B runs and the parity tests                                     */
#define IRBPP_TUNE_RECT 4194304      /* the transition kernel marks the vertices of level-image components that are isolated solid rectangles
                                      * itself, as it does isolated pixels (default: the trace kernel follows them like every other border --
                                      * measured: trace -5 us, polygon -2 us, transition +6 us at 8192 BlockOut bins, profiles/r06/LOG.md s21) */
#define IRBPP_TUNE_NO_ROT_ALIAS 8388608 /* every rotation of an item builds its own observation, also where another rotation of the item has
                                         bit-identical footprint sizes, bottom table and ext_z_r (default: such a rotation reuses the other's
                                         drop heights and vertex bits, irbpp_rotalias.h); identical results, for A/B runs and the parity tests */
#define IRBPP_TUNE_LDS_TILE 16777216 /* lattice data, observe-only transition launch (behind irbpp_apply_kernel): stage the float64 heightmap
                                        tile in LDS as every other launch does (default there, on even grids with one action cell per thread:
                                        each thread reduces its own action cell's heightmap cells in registers and writes their float32 copy,
                                        no tile); identical results, for A/B runs and the parity tests                                    */
#define IRBPP_TUNE_TRACE_PACK 33554432 /* the trace kernel packs the round records of the polygon kernel itself, one gather per round in the
                                          wave that followed the borders (default: it dumps its point slots and a lane table once per chunk
                                          and the polygon wave that takes a round gathers the round's positions from the dump,
                                          irbpp_rounds.h); identical results, for A/B runs and the parity tests                            */
#define IRBPP_TUNE_NO_SPECIALISED 1024 /* the run-time builds of the transition / emit kernels even where a build with the
                                         geometry as compile-time constants exists (16 x 16 action cells, step 2 or 4, R = 2 / 4 / 8,
                                         S = 500: BASELINE.json's configs); identical results, for A/B runs and the parity tests  */

/* Per-step outputs beyond the observation: what PackingGame.step returns and what Monitor
 * adds on `done` (binPhy.py:299-311,327; monitor.py:58-75).  All device pointers, one entry
 * per bin; any pointer may be NULL to skip that output. */
typedef struct {
    double*  reward_dev;      /* reward of this step (item_ratio*10 or 0.0)                      */
    uint8_t* done_dev;        /* 1 iff the episode ended with this step                          */
    int32_t* counter_dev;     /* info['counter'] = items packed, valid where done                */
    double*  ratio_dev;       /* info['ratio']   = get_ratio(),  valid where done                */
    double*  ep_reward_dev;   /* sum of the episode's rewards (Monitor 'r' before round(.,6))    */
    int32_t* ep_len_dev;      /* Monitor 'l'                                                     */
    uint8_t* stable_dev;      /* irbpp_config::stability >= 1: 1 iff the placement of this step rests stably
                                 (0 also where the step placed nothing); NULL to skip                    */
    int32_t* err_dev;         /* copy of the device error word after this step (one int32, not per bin):
                                 callers that fetch the outputs with one D2H copy get it for free.
                                 LIFETIME: the library keeps this pointer after irbpp_step returns and ORs
                                 error bits into the word as later launches of this environment raise them
                                 (irbpp_get_action_candidates writes through it): it must stay allocated and
                                 must not be written by the caller until the next irbpp_step with another
                                 err_dev (or NULL), irbpp_reset / irbpp_reset_bins, or irbpp_destroy.  The word
                                 always holds every sticky bit of the device error word when a step's
                                 kernels have run (it is re-seeded whenever the pointer changes and after
                                 every reset / stream write)                                          */
} irbpp_step_out;

const char* irbpp_status_string(int status);
int irbpp_version(void);
/* Hash of the sources and compiler flags this binary was built from (irbpp_amd/build.py: source_hash(), passed in as
 * -DIRBPP_SOURCE_HASH); "unstamped" for a build made some other way.  The Python loader refuses a binary whose stamp is
 * not the hash of the sources lying next to it: a stale .so can then never be measured or tested by mistake. */
const char* irbpp_source_hash(void);

/* replaces: gym.make('Physics-v0', args=args) x num_processes + ShmemVecEnv.__init__
 * (envs.py:67-99, shmem_vec_env.py:25-59) */
int irbpp_create(const irbpp_config* cfg, irbpp_env** out);
/* replaces: ShmemVecEnv.close_extras (shmem_vec_env.py:83-92) */
int irbpp_destroy(irbpp_env* env);

/* replaces: args.shotInfo / args.infoDict built by shotInfoPre + load_shape_dict
 * (tools.py:227-279).  Shape id k, rotation r owns four [fx,fy] row-major float64 tables
 * starting at pool offset offsets[k*n_rot+r]; dims[(k*n_rot+r)*2 + {0,1}] = fx, fy;
 * extents[(k*n_rot+r)*3 + {0,1,2}] = mesh.extents; volumes[k] = infoDict[k][0]['volume'].
 * Masks must be exactly 0.0 or 1.0.  All host pointers; copied. */
int irbpp_load_shapes(irbpp_env* env, int32_t n_shapes,
                      const double* extents, const double* volumes,
                      const int32_t* dims, const int64_t* offsets, int64_t pool_len,
                      const double* height_top, const double* height_bottom,
                      const double* mask_top, const double* mask_bottom);

/* replaces: LoadItemCreator.item_trajs = torch.load(test_sequence.pt) (IRcreator.py:81) and
 * the pre-drawn np.random.choice stream of the Random*Creator classes (IRcreator.py:26-72).
 * ids: int32[n_traj][length] host memory, copied. */
int irbpp_load_sequences(irbpp_env* env, const int32_t* ids, int32_t n_traj, int32_t length);

/* obs_len of PackingGame (binPhy.py:87-98): which=0 the observation reset()/step() return
 * (5S+9+Hx*Hy when k==1, k+Hx*Hy when k>1); which=1 the location observation of
 * get_action_candidates (5S+9+Hx*Hy). */
int irbpp_obs_len(const irbpp_env* env, int32_t which);

/* replaces: ShmemVecEnv.reset (shmem_vec_env.py:61-68) -> PackingGame.reset (binPhy.py:128-147).
 * obs_dev: float32[num_bins][obs_len(0)].  Restarts the trajectory counters. */
int irbpp_reset(irbpp_env* env, float* obs_dev, void* stream);

/* replaces: ShmemVecEnv.reset_specific (shmem_vec_env.py:113-117): PackingGame.reset of the
 * listed bins only.  bins_dev: int32[count] distinct local bin indices (device memory);
 * obs_dev: float32[count][obs_len(0)], row i = the reset observation of bin bins_dev[i].
 * Like the reference's per-env reset the bin moves on to its next trajectory and the episode it
 * abandons enters no statistics.  An index outside [0, num_bins) is skipped and raises
 * IRBPP_DEVERR_BAD_BIN. */
int irbpp_reset_bins(irbpp_env* env, const int32_t* bins_dev, int32_t count, float* obs_dev, void* stream);

/* replaces: ShmemVecEnv.step_async+step_wait (shmem_vec_env.py:70-81) -> PackingGame.step
 * (binPhy.py:248-337, no-physics branch) + the worker's auto-reset (shmem_vec_env.py:141-144).
 * actions_dev: int32[num_bins] indices into the candidate rows of the last location
 * observation.  obs_dev: float32[num_bins][obs_len(0)]; for a finished episode it already
 * holds the next episode's first observation. */
int irbpp_step(irbpp_env* env, const int32_t* actions_dev, float* obs_dev,
               const irbpp_step_out* out, void* stream);

/* irbpp_step with the placement's cell handed in instead of a candidate row: PackingGame.step (binPhy.py:248-337) with
 * candidates[action][0:3] replaced by cells_dev[b] = (rot, lx, ly), int32[num_bins][3] -- for callers that choose from the
 * possible-position grids (Space.get_heuristic_action, search, scripted curricula), whose cell is often no contour vertex
 * and so no candidate row.  Everything else is irbpp_step: prejudge on the extents and on np.sum(naiveMask) == 0, the drop
 * height posZmap[rot, lx, ly] of the last observation (recomputed from the footprint's bottom cells where the observation
 * did not mark the cell valid), simulateHeight, heightmap update, reward / done / info, auto-reset, queue update, the next
 * (online) or order (buffered, after irbpp_get_action_candidates) observation, placement log, episode window, totals.
 * A triple outside 0 <= rot < n_rot, 0 <= lx < Ax, 0 <= ly < Ay is the reference's IndexError: it raises
 * IRBPP_DEVERR_BAD_ACTION and the step runs on the clamped cell.  Unlike row indices, negative values do NOT count from the
 * end (numpy's wrap-around is not reproduced for cells).
 * Always runs as the apply kernel followed by the observation, at every launch size and on both pipelines; configurations
 * that apply the step inside the transition kernel answer IRBPP_ERR_ARG: stability != 0, IRBPP_TUNE_FUSED_APPLY,
 * IRBPP_TUNE_CHAIN (where it takes effect). */
int irbpp_step_cells(irbpp_env* env, const int32_t* cells_dev, float* obs_dev,
                     const irbpp_step_out* out, void* stream);

/* One placement of the reference's heuristic baselines without a host round trip: per bin the cell
 * Space.get_heuristic_action (space.py:162-218) picks -- method and dir_idx as for irbpp_heuristic_action -- then
 * irbpp_step_cells on it.  MINZ, DBLF and FIRSTFIT score the posZmap / naiveMask grids the last observation stored (one
 * wave per bin, fused with the placement) on both pipelines; HM (16 x 16 grids only: IRBPP_ERR_ARG on the capacity path)
 * runs irbpp_heuristic_action's scorer in front of the cell step.  Same IRBPP_ERR_ARG cases as irbpp_step_cells.
 * The stored grids must be current: IRBPP_ERR_STATE after irbpp_set_heightmaps (it clears them), and in a buffered
 * environment after irbpp_reset / irbpp_step, until the next observation of all bins (irbpp_reset or irbpp_step online,
 * irbpp_get_action_candidates buffered; irbpp_get_all_possible_observation counts as well: after it the grids, the item and
 * np.sum(naiveMask) the step goes by are those of the LAST buffer slot, as for irbpp_step). */
int irbpp_heuristic_step(irbpp_env* env, int32_t method, int32_t dir_idx, float* obs_dev,
                         const irbpp_step_out* out, void* stream);

/* replaces: ShmemVecEnv.get_action_candidates (shmem_vec_env.py:99-102) ->
 * PackingGame.get_action_candidates (binPhy.py:161-169).  order_actions_dev: int32[num_bins]
 * buffer slots; loc_obs_dev: float32[num_bins][obs_len(1)].  Hierarchical mode only. */
int irbpp_get_action_candidates(irbpp_env* env, const int32_t* order_actions_dev,
                                float* loc_obs_dev, void* stream);

/* replaces: PackingGame.get_all_possible_observation (binPhy.py:171-180; no caller in the reference): the location
 * observation of EVERY buffer slot of every bin on the current heightmaps, loc_obs_dev: float32[num_bins][k][obs_len(1)]
 * -- per bin the concatenation the reference returns.  Hierarchical mode only.  As there, the candidate rows a following
 * irbpp_step would index are those of the LAST slot, and the slot chosen by the last irbpp_get_action_candidates
 * (self.orderAction) is left as it is.  Ignores irbpp_set_auto_policy's buffer semantics only in that the action written is
 * the last slot's. */
int irbpp_get_all_possible_observation(irbpp_env* env, float* loc_obs_dev, void* stream);

/* The scripted policy used by the benchmark and the parity tests: per bin the candidate
 * row with V==1 and the lowest H (first on ties), 0 if none.  loc_obs_dev has row stride
 * obs_stride floats.  (Stands in for agent.py:51-58 so no host round trip is timed.) */
int irbpp_policy_minz(irbpp_env* env, const float* loc_obs_dev, int32_t obs_stride,
                      int32_t* actions_dev, void* stream);

/* The same policy fused into the observation: while actions_dev is set (int32[num_bins] on the device; NULL
 * switches it off), every call that emits a location observation -- irbpp_reset, irbpp_reset_bins (listed bins
 * only), irbpp_step of an online environment, irbpp_get_action_candidates -- also writes the action
 * irbpp_policy_minz would pick on it, so that a scripted roll-out (tools.test with a heuristic, the benchmark)
 * needs no policy kernel between two steps.  The buffer may be the one the next irbpp_step reads its actions from. */
int irbpp_set_auto_policy(irbpp_env* env, int32_t* actions_dev);

/* Registers a location-observation buffer (float32[num_bins][obs_len(1)], i.e. what irbpp_reset / irbpp_step of an
 * online environment / irbpp_get_action_candidates write) that from now on ONLY this library writes: it remembers
 * how many candidate rows each bin's block holds, so a later call that is handed the same pointer stores the rows
 * that exist and clears the ones that existed before, instead of rewriting the zero tail of all `selected` rows
 * (typically 80 % of the block).  The contents delivered are the same as for an unregistered buffer.  Up to 8
 * buffers (a ring of 2-3 is what an actor loop needs); not for irbpp_reset_bins.
 * Lifetime: the registration is keyed by the pointer value, so unregister a buffer BEFORE freeing it (a later
 * allocation may reuse the address); registering a pointer again, irbpp_invalidate_obs_buffer, and any library call
 * that writes another layout through it (irbpp_step of a buffered environment) make the next emit rewrite all
 * `selected` rows.  If the caller itself writes into a registered buffer it must invalidate it afterwards. */
int irbpp_register_obs_buffer(irbpp_env* env, float* obs_dev);
int irbpp_unregister_obs_buffer(irbpp_env* env, float* obs_dev);
/* obs_dev == NULL: every registered buffer.  Asynchronous on `stream`. */
int irbpp_invalidate_obs_buffer(irbpp_env* env, float* obs_dev, void* stream);

/* item_stream = 1 only.  The position of every bin in its stream row, counted in items consumed since the row was
 * loaded (int32[num_bins], device memory): set == 0 reads them, set != 0 writes them.  The host side of the ring
 * (irbpp_amd/itemgen.py) reads the cursors, rewrites the consumed part of each row with irbpp_stream_write and never
 * lets a bin run more than `length` items ahead of what it has written. */
int irbpp_stream_cursors(irbpp_env* env, int32_t* cursors_dev, int32_t set, void* stream);
/* Row r of the stream table gets ids_dev[r][0 .. count_dev[r]) (int32[n_traj][width], device memory) at ring positions
 * (first_dev[r] + c) mod length.  Ids below -1 are stored as -1 (no item): the value -3 is the bins' own mark of a slot
 * they have consumed. */
int irbpp_stream_write(irbpp_env* env, const int32_t* ids_dev, const int32_t* first_dev, const int32_t* count_dev,
                       int32_t width, void* stream);
/* Tests and tooling: the stream table as it stands (int32[n_traj][length], device memory; -3 in a slot its bin has
 * consumed and nobody has rewritten).  Asynchronous on `stream`. */
int irbpp_stream_table(irbpp_env* env, int32_t* table_dev, void* stream);

/* replaces: RandomItemCreator / RandomInstanceCreator / RandomCateCreator.generate_item (IRcreator.py:26-72) of ONE
 * environment whose process was seeded with `seed` (= args.seed + rank, envs.py:41 -> binPhy.py:118-123): host-side,
 * the same MT19937 words, masks and rejections as np.random.choice on the legacy global generator, so the stream of
 * item ids equals the reference's.  n_groups > 0: two stages, name = choice(n_groups), item = choice(members of that
 * group) with group g = members[group_offsets[g] .. group_offsets[g+1]) in the order the reference's dict holds them;
 * n_groups == 0: one stage over `members` (RandomItemCreator).  irbpp_itemgen_draw appends `count` items. */
typedef struct irbpp_itemgen irbpp_itemgen;
int irbpp_itemgen_create(uint32_t seed, int32_t n_groups, const int32_t* group_offsets, const int32_t* members,
                         int32_t n_members, irbpp_itemgen** out);
int irbpp_itemgen_draw(irbpp_itemgen* gen, int32_t count, int32_t* out_host);
int irbpp_itemgen_destroy(irbpp_itemgen* gen);

/* The same streams drawn on the device, n_streams of them over one set of lists, stream s seeded seeds_host[s]
 * (init_genrand runs on the device, launched on `stream`; the arguments are checked like irbpp_itemgen_create's).  Per
 * stream the generator keeps the 624 key words, the position in them and `delivered`, the number of items it has
 * written so far (64-bit), all in device memory.  Every call below is asynchronous on its `stream` and reads nothing
 * back; calls that touch the same streams of a generator must be ordered by the caller (same HIP stream, or events).
 *   irbpp_itemgen_dev_draw       appends `count` items of EVERY stream: out_dev = int32[n_streams][count], device memory
 *                                (parity tests and tooling; advances the state a refill advances)
 *   irbpp_itemgen_dev_delivered  copies `delivered` to out_dev = int64[n_streams], device memory
 *   irbpp_stream_refill          item_stream = 1 with the table loaded, one row per bin (IRBPP_ERR_STATE / _ARG otherwise;
 *                                IRBPP_ERR_ARG if first_stream + num_bins > n_streams): bin b is fed by stream
 *                                s = first_stream + b.  With c the bin's cursor, w = delivered[s] and L the ring length,
 *                                the c + L - w items the bin has consumed are drawn and written to ring slots
 *                                (w + j) mod L, and delivered[s] grows by as many -- so the first refill of a new
 *                                environment fills the whole ring and its table may be loaded as a placeholder of -1.
 *                                c > w (the bin ran past what it was given) raises IRBPP_DEVERR_STREAM_DRY in the sticky
 *                                error word and writes nothing.  No host read, no synchronisation. */
typedef struct irbpp_itemgen_dev irbpp_itemgen_dev;
int irbpp_itemgen_dev_create(int32_t device, int32_t n_streams, const uint32_t* seeds_host, int32_t n_groups,
                             const int32_t* group_offsets, const int32_t* members, int32_t n_members, void* stream,
                             irbpp_itemgen_dev** out);
int irbpp_itemgen_dev_draw(irbpp_itemgen_dev* gen, int32_t count, int32_t* out_dev, void* stream);
int irbpp_itemgen_dev_delivered(irbpp_itemgen_dev* gen, int64_t* out_dev, void* stream);
int irbpp_stream_refill(irbpp_env* env, irbpp_itemgen_dev* gen, int32_t first_stream, void* stream);
int irbpp_itemgen_dev_destroy(irbpp_itemgen_dev* gen);

/* -- stage-level entry points (parity tests and tooling) ------------------------------- */

/* Space.get_possible_position (space.py:98-129) for item_ids_dev[b] on bin b's current
 * heightmap.  posz_dev: float64[num_bins][n_rot][Ax][Ay] = posZmap; mask_dev:
 * uint8[num_bins][n_rot][Ax][Ay] = naiveMask.  Does not modify the environment. */
int irbpp_possible_position(irbpp_env* env, const int32_t* item_ids_dev,
                            double* posz_dev, uint8_t* mask_dev, void* stream);

/* Space.get_heuristic_action (space.py:162-218) for the item of the last location observation on
 * the current heightmaps: method 1 MINZ, 2 DBLF, 3 FIRSTFIT, 4 HM; dir_idx 0..3 = (Xflip, Yflip)
 * as at space.py:163-166.  out_dev: int32[num_bins][3] = (rotIdx, lx, ly), the first minimum in C
 * order of np.round(score, 6) with invalid cells at 1e6.  RANDOM is not provided. */
int irbpp_heuristic_action(irbpp_env* env, int32_t method, int32_t dir_idx, int32_t* out_dev, void* stream);

/* replaces: tools.shot_item (tools.py:98-135), the per-(shape, rotation) footprint precompute that
 * shotInfoPre caches on disk (tools.py:248-279) -- trimesh ray casting in the reference, a
 * z-ray/triangle rasteriser here.  Stateless.  verts_dev: float64[n_verts][3] of the mesh already
 * rotated and translated to its bounding-box minimum; faces_dev: int32[n_faces][3]; ray (i, j)
 * passes through (i*resolution_h + shift, j*resolution_h + shift) (shift = 0.001, tools.py:81-95).
 * Outputs float64[fx][fy] each: heightMapT (highest hit), heightMapB (lowest hit), maskH, maskB;
 * if no ray hits at all: T = extent_z, B = 0, masks 1 (tools.py:112-117,126-131).
 * scratch_dev: one int32 of device memory. */
int irbpp_shot_item(const double* verts_dev, const int32_t* faces_dev, int32_t n_faces, int32_t fx, int32_t fy,
                    double resolution_h, double shift, double extent_z, double* top_dev, double* bottom_dev,
                    double* mask_top_dev, double* mask_bottom_dev, int32_t* scratch_dev, void* stream);

/* getConvexHullActions (cvTools.py:61-102) on caller-supplied grids, independent of the
 * environment state: posz_valid_dev float64[n_grids][n_rot][Ax][Ay], mask_dev
 * uint8[n_grids][n_rot][Ax][Ay].  vertex_rows_dev: uint32[n_grids][n_rot][16]; word `row` has
 * bit `col` set iff (row, col) is a candidate of that rotation (np.unique makes the candidate
 * list a set, cvTools.py:101, so the bit grid is its exact representation). */
int irbpp_convex_hull_actions(irbpp_env* env, int32_t n_grids, const double* posz_valid_dev,
                              const uint8_t* mask_dev, uint32_t* vertex_rows_dev, void* stream);

/* Space.heightmapC of every bin (space.py:26): float64[num_bins][Hx][Hy]. */
int irbpp_get_heightmaps(irbpp_env* env, double* hm_dev, void* stream);
/* (the drop heights a step takes from the last observation are forgotten with the old maps: a step that follows
 * irbpp_set_heightmaps without a new observation recomputes its drop height on the new map) */
int irbpp_set_heightmaps(irbpp_env* env, const double* hm_dev, void* stream);

/* Running totals over finished episodes since create/reset, for logging
 * (trainer.py:215-222): out_dev float64[4] = {episodes, sum ratio, sum counter, sum reward}.
 * The multi-GPU runner all-reduces these four numbers (RCCL). */
int irbpp_episode_totals(irbpp_env* env, double* out_dev, void* stream);

/* The trainer's logged episode metrics on the device (trainer.py:145-147 deque(maxlen=10) x 3, :168-178 append on done,
 * :215-222 add_scalar of their mean / max / min): a window of the last `window` finished episodes, in the order (step they
 * finished in, global bin), kept per environment and snapshotted after every step, so that the rows the trainer would have
 * logged can be computed for hundreds of steps at once without a host round trip per step.
 * An entry: r = round(ep_reward, 6) with Python's round (monitor.py:64), ratio and counter of the step outputs. */
typedef struct {
    int64_t key;              /* finish step << 32 | global bin (global_offset + b): the window's order            */
    double  r;                /* Monitor 'r': Python's round(ep_reward, 6)                                         */
    double  ratio;            /* info['ratio']                                                                      */
    int32_t counter;          /* info['counter']                                                                    */
    int32_t reserved;
} irbpp_episode_entry;
/* Caller-owned device buffers of one window (all zeroed before the first attach: a zeroed window is empty at step 0).
 * Steps are counted from 1 (trainer.py:158) since the buffers were zeroed; step T's window is snapshot row T % history. */
typedef struct {
    irbpp_episode_entry* ring_dev;      /* [window]: the live window, a ring                                        */
    irbpp_episode_entry* snapshot_dev;  /* [history][window]: the window after each step, oldest entry first         */
    int32_t* rows_dev;                  /* [history][2]: step held by the snapshot row, entries in it                */
    int32_t* state_dev;                 /* [4]: steps recorded, entries in the window, ring head, unused             */
    int32_t window;                     /* W, 1..1024 (the reference: 10)                                            */
    int32_t history;                    /* H >= 1 snapshot rows: read at least every H steps                         */
} irbpp_episode_window;
/* Attaches a window to the environment (NULL detaches): from then on every irbpp_step -- both overlap paths, online and
 * buffered -- launches one small update kernel on its stream after the step's kernels, which appends the bins finished by
 * the step (done_dev) to the window and writes the snapshot.  While attached, a step whose irbpp_step_out lacks done_dev,
 * ep_reward_dev, ratio_dev or counter_dev is IRBPP_ERR_ARG.  Works with IRBPP_TUNE_GRAPH (the launch follows the replayed
 * graph).  Detached, a step launches exactly what it launched before.  The buffers must outlive the attachment. */
int irbpp_set_episode_window(irbpp_env* env, const irbpp_episode_window* window);
/* One step of a window without an environment: appends the bins whose done_dev[b] != 0 (bin order, global bin =
 * global_offset + b) and writes the snapshot of the step, exactly as a windowed irbpp_step does behind its kernels (which
 * calls this function: it is the only launch of the update kernel).  done_dev uint8[n_bins], ep_reward_dev / ratio_dev
 * float64[n_bins], counter_dev int32[n_bins].  IRBPP_ERR_ARG for a NULL pointer, a window irbpp_set_episode_window would
 * refuse, or n_bins < 1.  Asynchronous on `stream`. */
int irbpp_episode_window_update(const irbpp_episode_window* window, const uint8_t* done_dev, const double* ep_reward_dev,
                                const double* ratio_dev, const int32_t* counter_dev, int32_t n_bins, int32_t global_offset,
                                void* stream);
/* The rows the trainer logs (trainer.py:215-222) for steps first_step .. first_step + n_steps - 1 of n_parts windows whose
 * bins together are the trainer's envs (groups of bins, ranks: any order; the global bin index orders them).  out_dev:
 * float64[n_steps][7] = (T, n, mean r, max r, min r, mean ratio, mean counter), n = len(deque) and the five statistics NaN
 * when n == 0 (the trainer logs nothing then); every mean equals np.mean over the deque bit for bit.  A step that some part
 * has not recorded yet has n = -2, a step whose snapshot row was overwritten (more than `history` steps ago) n = -1, both
 * with NaN statistics.  All parts need the same window and history; n_parts 1..64, n_steps 1..history, first_step >= 1.
 * Asynchronous on `stream`, which must follow the steps of every part. */
int irbpp_episode_metrics(const irbpp_episode_window* parts, int32_t n_parts, int32_t first_step, int32_t n_steps,
                          double* out_dev, void* stream);

/* replaces: PackingGame.packed (binPhy.py:141,296), the per-episode placement record that
 * tools.test saves to trajs.npy (tools.py:339-340).  While set, every placement of bin b, the
 * i-th of its episode (i < capacity), stores the word meta_dev[b*capacity+i] =
 *   item (bits 0..15) | rot << 16 (bits 16..19) | lx << 20 (bits 20..24) | ly << 25 (bits 25..29)
 * (bits 30..31 zero) and z_dev[b*capacity+i] = its drop height posZmap[rot,lx,ly].  Item ids must be
 * < 65535; rot < 16 and lx, ly < 32 hold for every environment the library accepts (n_rot <= 8, action
 * grids of at most 32 cells a side).
 * The REFUSED placement that ends an episode is recorded too, as entry `counter` behind the episode's
 * `counter` accepted ones (the reference appends to self.packed before it looks at `success`): its
 * fields are masked to their widths, its item field is 0xFFFF when the trajectory was exhausted (no
 * item to place), and its height is posZmap[rot,lx,ly] where the footprint lies inside the grid for
 * that rotation and 1e3 where it does not.  An index i >= capacity is dropped, never wrapped: with
 * capacity 0 nothing is written.  The index is the episode's own placement count, so a log attached
 * in the middle of an episode continues at that episode's index.  A finished episode's entries stay
 * readable until that bin's next placements overwrite them, so read them right after the step that
 * reported done.  NULL, NULL switches the log off; one NULL pointer of the two is IRBPP_ERR_ARG. */
int irbpp_set_placement_log(irbpp_env* env, uint32_t* meta_dev, double* z_dev, int32_t capacity);

/* Save, restore and fork bins on the device.
 *
 * The state of a bin is the set of per-bin rows a later call on that bin reads and an earlier call on it wrote (the segment table of
 * csrc/irbpp_binstate.h): heightmap, item queue, candidate keys of the last observation, the bin's line of
 * scalars (cursor, episode count, trajectory row of the running episode, counters and sums), the drop-height and naiveMask grids of
 * the last observation, the placement-log rows when a log is attached, and -- for save / load only -- the bin's share of
 * irbpp_episode_totals.  A per-bin blob holds these rows back to back, each padded to 16 bytes: bytes_per_bin bytes.
 *
 *   irbpp_bin_blob_info_get   what a blob of this environment is: layout version, bytes per bin, and the two keys a blob (or a second
 *                             environment) must share with an environment to be loaded into (copied to) it.  num_bins, global_offset
 *                             and global_bins take no part in the keys: a search environment of N * B bins beside a root environment
 *                             of N bins is the intended use.  A placement log's capacity is part of geometry_key (a blob saved
 *                             with a log loads only into an environment with a log of that capacity).  IRBPP_ERR_STATE before
 *                             both tables are loaded.
 *   irbpp_save_bins           blob row i = the state of bin bins_dev[i]; blob_dev: count * bytes_per_bin bytes, 16-byte aligned.
 *   irbpp_load_bins           bin bins_dev[i] = blob row i: the bin is what it was at the save, its totals included.  `info` is the
 *                             info the blob was saved with: IRBPP_ERR_ARG if its version, bytes_per_bin, geometry_key or tables_key
 *                             differ from the environment's own.
 *   irbpp_copy_bins           bin dst_bins_dev[i] of dst = bin src_bins_dev[i] of src (src may be dst).  After it the destination bin
 *                             behaves exactly as its source would, call for call, until the running episode ends: it draws the
 *                             items its source would draw (the episode's trajectory row travels).  The NEXT episode is the
 *                             destination's own: the trajectory row of its own index with the copied episode count.  The
 *                             destination's totals are untouched (a finished episode is not counted twice); the placement-log rows
 *                             of the running episode are copied.  IRBPP_ERR_ARG if the two environments differ in a key, are on
 *                             different devices, or one has a placement log and the other none.
 *
 * bins_dev: int32[count] local bin indices in device memory.  An index outside [0, num_bins) makes its pair a no-op and raises
 * IRBPP_DEVERR_BAD_BIN in the sticky error word of the destination environment (irbpp_save_bins: of env); the other pairs are served.
 * OVERLAP IS THE CALLER'S CONTRACT: within one call the destination bins are pairwise distinct, and with src == dst no bin is both
 * a source and a destination unless it is paired with itself (a no-op).  The library does not check this on the device; the Python
 * wrappers do (vec_env.GpuPackingEnv.fork_bins).
 * count == 0 is IRBPP_OK (answered first, after the NULL / negative-count checks); IRBPP_ERR_STATE before irbpp_reset.
 * Item-stream environments (item_stream = 1) answer IRBPP_ERR_ARG from all three calls: a ring row belongs to its bin AND to a feeder
 * that counts what it delivered, so copying one is a design of its own.  The stability proxy keeps nothing per bin: allowed.
 * Host-side flags: the destination's "stored grids are current" flag stays set only if the source's (the blob's grids_current) is set
 * too, otherwise irbpp_heuristic_step answers IRBPP_ERR_STATE until the next observation of all bins, as after
 * irbpp_set_heightmaps.  Registered observation buffers are the caller's memory and are not touched: a caller that copies
 * observation rows itself calls irbpp_invalidate_obs_buffer.  Replayed graphs (IRBPP_TUNE_GRAPH), the error word handed to
 * irbpp_step and an attached episode window are left as they are (a window belongs to an environment's step stream, not to a bin).
 * Asynchronous on `stream`, which must follow the steps of both environments. */
typedef struct irbpp_bin_blob_info {
    int32_t version;          /* layout version of the segment table, starts at 1 */
    int32_t bytes_per_bin;    /* multiple of 16 */
    uint64_t geometry_key;    /* hash of every Params field the table and the kernels' reading of it depend on:
                                 Hx, Hy, Ax, Ay, step, R, S, K, resolutions, bin size, wide, log capacity */
    uint64_t tables_key;      /* hash of what irbpp_load_shapes and irbpp_load_sequences were given */
    int32_t grids_current;    /* the environment's flag when the blob was written */
    int32_t reserved;
} irbpp_bin_blob_info;

int irbpp_bin_blob_info_get(const irbpp_env* env, irbpp_bin_blob_info* out);
int irbpp_save_bins(irbpp_env* env, const int32_t* bins_dev, int32_t count, void* blob_dev, void* stream);
int irbpp_load_bins(irbpp_env* env, const irbpp_bin_blob_info* info, const int32_t* bins_dev, int32_t count,
                    const void* blob_dev, void* stream);
int irbpp_copy_bins(irbpp_env* dst, const int32_t* dst_bins_dev, irbpp_env* src, const int32_t* src_bins_dev,
                    int32_t count, void* stream);

/* Caller side: the N per-env prioritised replay memories of main.py:61-63 as one tensor set.
 * replaces: SegmentTree.find/_retrieve (memory.py:72-86) for `draws` values per env.
 * tree_dev float32[n_env][2*capacity-1] (implicit heap, leaves at capacity-1..), values_dev float32[n_env][draws];
 * outputs [n_env][draws]: leaf value, data index (tree index - capacity + 1), tree index. */
int irbpp_sumtree_find(const float* tree_dev, int32_t n_env, int32_t capacity, const float* values_dev, int32_t draws,
                       float* prob_dev, int64_t* data_idx_dev, int64_t* tree_idx_dev, void* stream);
/* ReplayMemory._get_samples_from_segments (memory.py:161-176) for all envs: draws one position per (env, segment)
 * -- `draws` segments of p_total/draws each -- with the rejection loop of memory.py:170-176 run on the device
 * (redraw while the position straddles the write index index_dev[env] +- n_step / history or has probability 0).
 * Counter-based uniform numbers from `seed`; failed_dev[0] |= 1 if a draw found nothing valid in max_tries tries. */
int irbpp_sumtree_sample(const float* tree_dev, const int64_t* index_dev, int32_t n_env, int32_t capacity, int32_t draws,
                         int32_t n_step, uint64_t seed, int32_t max_tries, float* prob_dev, int64_t* data_idx_dev,
                         int64_t* tree_idx_dev, int32_t* failed_dev, void* stream);

/* replaces: SegmentTree.update/_propagate (memory.py:47-58) for `leaves` (tree index, value) pairs per env, applied
 * in list order, every ancestor recomputed as left + right in float32; max_dev float32[n_env] is SegmentTree.max.
 * env_mask_dev (may be NULL) uint8[n_env]: envs with 0 are skipped.  IRBPP_ERR_ARG if 2*capacity-1 > 16384 (the
 * caller then keeps its own path). */
int irbpp_sumtree_update(float* tree_dev, float* max_dev, int32_t n_env, int32_t capacity, const int64_t* tree_idx_dev,
                         const float* priority_dev, int32_t leaves, const uint8_t* env_mask_dev, void* stream);
/* The replay tensors of all envs (memory.py:28-36 per env): float32 states [n_env][capacity][obs_len], int64 actions,
 * float32 rewards, uint8 nonterminals [n_env][capacity], float32 tree [n_env][2*capacity-1], int64 index and uint8 full
 * [n_env], float32 scaling [n_step] = discount^k. */
typedef struct {
    const float* states_dev; const int64_t* actions_dev; const float* rewards_dev; const uint8_t* nonterminals_dev;
    const float* tree_dev; const int64_t* index_dev; const uint8_t* full_dev; const float* scaling_dev;
    int32_t n_env, capacity, obs_len, n_step;
} irbpp_replay_view;
/* replaces: ReplayMemory._get_transition_new and the batch assembly of ReplayMemory.sample (memory.py:123-139,178-204)
 * for `draws` (<= 256) positions per env found by irbpp_sumtree_find: outputs env-major rows [n_env*draws]:
 * state and next state float32 [..][obs_len], action int64, n-step return, non-terminal flag, importance weight
 * (priority_weight = beta) float32. */
int irbpp_replay_gather(const irbpp_replay_view* view, int32_t draws, float beta, const int64_t* data_idx_dev,
                        const float* prob_dev, float* state_dev, int64_t* action_dev, float* return_dev,
                        float* next_state_dev, float* nonterminal_dev, float* weight_dev, void* stream);
/* The N memories of an irbpp_replay_view sampled as ONE prioritised memory (no reference counterpart: its batch is the
 * concatenation of per-worker batches, so it cannot be smaller than n_env).  The pooled tree is a top tree over the n_env
 * row roots -- an implicit heap over P leaves, P the power of two >= n_env, padding 0, rebuilt by every call and never
 * stored -- with each env's own tree below its leaf; its root T is the pooled total.  Draw j of `draws` (<= 1024) is
 * v = j*(T/draws) + u*(T/draws), u from the counter-based generator of irbpp_sumtree_sample (its env field a constant no
 * env uses), walked by `v <= left ? left : (v - left, right)` through the top tree and on, with the residual v, through
 * that env's tree in global memory (any capacity).  A draw on a padding leaf, one that fails memory.py:175 against its
 * env's write index, or one of priority 0 is redrawn within its segment up to max_tries times; failed_dev[0] |= 1 if one
 * stays invalid.  values_dev (may be NULL) float32[draws]: positions in [0, T) used as v directly, looked up once.
 * Outputs [draws]: env and data / tree index in it (int64), leaf value, and the importance weight of memory.py:199-202 on
 * the pooled memory: (filled * prob / T)^-beta over the batch maximum, filled = the integer sum over envs of (capacity if
 * full else index) as float32.  IRBPP_ERR_ARG if n_env > 8192 (the top tree's LDS row). */
int irbpp_replay_pool_sample(const irbpp_replay_view* view, int32_t draws, const float* values_dev, uint64_t seed,
                             int32_t max_tries, float beta, int64_t* env_dev, float* prob_dev, int64_t* data_idx_dev,
                             int64_t* tree_idx_dev, float* weight_dev, int32_t* failed_dev, void* stream);
/* irbpp_replay_gather for `draws` rows (env_dev[j], data_idx_dev[j]) of a pooled sample: state and next state float32
 * [draws][obs_len], action int64, n-step return and non-terminal flag float32 [draws].  A row whose env is outside
 * [0, n_env) is written as zeros. */
int irbpp_replay_pool_gather(const irbpp_replay_view* view, int32_t draws, const int64_t* env_dev, const int64_t* data_idx_dev,
                             float* state_dev, int64_t* action_dev, float* return_dev, float* next_state_dev,
                             float* nonterminal_dev, void* stream);
/* SegmentTree.update/_propagate (memory.py:47-58) for `count` (<= 1024) triples (env, tree index, priority) applied in
 * list order: a leaf listed twice keeps its last value, max_dev[env] becomes the maximum of itself and every priority
 * listed for env, every ancestor of a touched leaf ends as left + right of its final children; nothing else of any row is
 * read or written (any capacity).  A triple whose env is outside [0, n_env) or whose tree index is no leaf of the row is
 * ignored.  Priorities are non-negative. */
int irbpp_replay_pool_update(float* tree_dev, float* max_dev, int32_t n_env, int32_t capacity, const int64_t* env_dev,
                             const int64_t* tree_idx_dev, const float* priority_dev, int32_t count, void* stream);
/* The writable side of the same tensor set (memory.py:28-36, 111): int32 timesteps [n_env][capacity], float32 max priority,
 * int32 episode timestep counter [n_env]; the others as in irbpp_replay_view. */
typedef struct {
    float* states_dev; int64_t* actions_dev; float* rewards_dev; uint8_t* nonterminals_dev; int32_t* timesteps_dev;
    float* tree_dev; float* max_dev; int64_t* index_dev; uint8_t* full_dev; int32_t* t_dev;
    int32_t n_env, capacity, obs_len;
} irbpp_replay_store;
/* replaces: ReplayMemory.append (memory.py:117-121) with SegmentTree.append (:60-70) and its _propagate (:47-52), called
 * per env at trainer.py:184-186 -- for all envs in one launch: state_dev float32 rows `state_stride` floats apart, action
 * int32 or int64 (action_bytes 4 | 8), reward float32 or float64 (reward_bytes 4 | 8; stored as float32), terminal_dev
 * uint8[n_env]; valid_dev (may be NULL = every env) uint8[n_env]: envs with 0 are skipped (a sample that is not Valid). */
int irbpp_replay_append(const irbpp_replay_store* store, const float* state_dev, int64_t state_stride, const void* action_dev,
                        int32_t action_bytes, const void* reward_dev, int32_t reward_bytes, const uint8_t* terminal_dev,
                        const uint8_t* valid_dev, void* stream);
/* replaces: the tail of Agent.act (agent.py:55-58) with get_mask_from_state (tools.py:298-299) fused in:
 * action[e] = argmax_i q[e][i] over the candidates i whose validity flag obs[e][5*i+4] is non-zero (first maximum;
 * 0x7fffffff never occurs: with no valid candidate every q is -inf and index 0 wins, like torch.argmax). */
int irbpp_masked_argmax(const float* q_dev, int32_t q_stride, const float* obs_dev, int32_t obs_stride, int32_t selected,
                        int32_t n_env, int64_t* action_dev, void* stream);
/* replaces: all of Agent.act after the network (agent.py:51-58): (q_map * support).sum(2), the mask, argmax(1) -- one
 * launch that reads the probabilities once.  p_dev float32 [n_env][s_rows][atoms], atoms contiguous, rows row_stride and
 * envs env_stride floats apart (slices of wider tensors work); support_dev float32[atoms], the caller's own
 * torch.linspace(Vmin, Vmax, atoms), never recomputed.  A row's value is the float32 sum, left to right over
 * a = 0..atoms-1, of fl32(p[a] * support[a]), multiply and add separate: reproducible bit for bit.  obs_dev / obs_stride
 * as in irbpp_masked_argmax: a row whose obs[e][5*i+4] == 0 counts as -inf; NULL = no mask (orderDQN.act(state, None),
 * trainer.py:266).  action_dev int64[n_env]: the first maximum; index 0 if every row is masked or -inf.  q_out_dev (may
 * be NULL) float32 rows q_stride floats apart: the unmasked values (evaluate_q, agent.py:135-137; logging).
 * IRBPP_ERR_ARG unless 2 <= atoms <= 128, 1 <= s_rows <= 1024, n_env >= 1, row_stride >= atoms,
 * env_stride >= (s_rows-1)*row_stride + atoms, obs_stride >= 5*s_rows, q_stride >= s_rows.  NaN inputs are out of scope. */
int irbpp_categorical_act(const float* p_dev, int64_t env_stride, int64_t row_stride, const float* support_dev, int32_t atoms,
                          const float* obs_dev, int32_t obs_stride, int32_t s_rows, int32_t n_env, int64_t* action_dev,
                          float* q_out_dev, int64_t q_stride, void* stream);
/* replaces: Agent.learn between the two network calls and the loss (agent.py:88-115), one wave per sample, no atomics:
 * a_star[b] = argmax over rows of the same defined expected value of p_online (unmasked, agent.py:92);
 * pns_a = p_target[b][a_star[b]] (:97); Tz = returns + (nonterminals * gamma_n) * support clamped to [v_min, v_max]
 * (:100-101); b = (Tz - v_min) / delta_z with an IEEE division; l = floor(b), u = ceil(b) and the two l == u fix-ups in
 * the reference's order (:104-109); m[b][j] = the float32 sum of the l == j contributions pns_a[i] * (u_i - b_i) in
 * ascending i, continued with the u == j contributions pns_a[i] * (b_i - l_i) in ascending i -- the order of the two
 * sequential index_add_ calls (:114-115), so m is the same from run to run.  p_online_dev / p_target_dev float32
 * [batch][s_rows][atoms] strided as in irbpp_categorical_act; returns_dev, nonterminals_dev float32[batch]; gamma_n the
 * caller's discount ** n as float32; m_dev float32[batch][atoms]; a_star_dev int64[batch].  Same limits as
 * irbpp_categorical_act, and batch >= 1, v_max > v_min, delta_z > 0. */
int irbpp_categorical_target(const float* p_online_dev, int64_t online_env_stride, int64_t online_row_stride,
                             const float* p_target_dev, int64_t target_env_stride, int64_t target_row_stride, const float* returns_dev,
                             const float* nonterminals_dev, const float* support_dev, int32_t atoms, int32_t s_rows, int32_t batch,
                             float gamma_n, float v_min, float v_max, float delta_z, float* m_dev, int64_t* a_star_dev, void* stream);
/* replaces: the end of DQNBPP.forward (model.py:395-400: v + a - a.mean(1), softmax over the atoms) and all of Agent.act after
 * it (agent.py:51-58) in one launch from the network's logits: the [n_env][s_rows][atoms] probabilities never reach memory
 * unless p_out_dev asks for them.  v_dev float32 [n_env][atoms], rows v_stride floats apart; a_dev float32
 * [n_env][s_rows][atoms] strided as p_dev of irbpp_categorical_act; support, obs, action, q_out as there.  p_out_dev (may be
 * NULL) float32 [n_env][s_rows][atoms], contiguous.  The float32 arithmetic is defined (csrc/irbpp_dueling.hip: 16 interleaved
 * partial sums per column for the mean, x = (v + a) - mean, a maximum-subtracted softmax with the library's own exponential,
 * exactly 0 below -80, the denominator summed in ascending atoms, IEEE divisions, the expected value of
 * irbpp_categorical_act) and reproducible bit for bit whatever n_env, the strides and the block's size.  Logits must be
 * finite: a NaN or an infinity gives unspecified q_out / p_out values, the action is still a row index in [0, s_rows) and
 * nothing is accessed out of range.  IRBPP_ERR_ARG unless 2 <= atoms <= 128, 1 <= s_rows <= 1024, n_env >= 1,
 * v_stride >= atoms, row_stride >= atoms, env_stride >= (s_rows-1)*row_stride + atoms, obs_stride >= 5*s_rows,
 * q_stride >= s_rows. */
int irbpp_dueling_act(const float* v_dev, int64_t v_stride, const float* a_dev, int64_t env_stride, int64_t row_stride,
                      const float* support_dev, int32_t atoms, const float* obs_dev, int32_t obs_stride, int32_t s_rows,
                      int32_t n_env, int64_t* action_dev, float* q_out_dev, int64_t q_stride, float* p_out_dev, void* stream);
/* replaces: Agent.learn's no_grad block (agent.py:90-115) from the logits of the two networks: a_star from the online (v, a) by
 * the arithmetic of irbpp_dueling_act, unmasked; pns_a = row a_star of the target net's softmax by the same arithmetic (the
 * target block's mean and that one row); then the projection of irbpp_categorical_target operation for operation, no
 * atomics.  Blocks strided as in irbpp_dueling_act, the other arguments and limits as in irbpp_categorical_target.  The same
 * rule for non-finite logits: unspecified m, a_star in [0, s_rows). */
int irbpp_dueling_target(const float* v_online_dev, int64_t v_online_stride, const float* a_online_dev, int64_t online_env_stride,
                         int64_t online_row_stride, const float* v_target_dev, int64_t v_target_stride, const float* a_target_dev,
                         int64_t target_env_stride, int64_t target_row_stride, const float* returns_dev,
                         const float* nonterminals_dev, const float* support_dev, int32_t atoms, int32_t s_rows, int32_t batch,
                         float gamma_n, float v_min, float v_max, float delta_z, float* m_dev, int64_t* a_star_dev, void* stream);
/* replaces: the part of Agent.learn that carries the gradient, forward: the end of DQNBPP.forward with log=True (model.py:395-398:
 * v + a - a.mean(1), log_softmax over the atoms), log_ps[range(B), actions] and loss = -sum(m * log_ps_a, 1) (agent.py:85-86,
 * 117) in one launch from the logits; the [batch][s_rows][atoms] log-probabilities never exist.  v_dev, a_dev strided as in
 * irbpp_dueling_act; actions_dev int64[batch], an index in [-s_rows, 0) counting from the end; m_dev float32 [batch][atoms],
 * contiguous (irbpp_dueling_target's m).  loss_out_dev float32[batch]; g_out_dev float32 [batch][atoms]: d loss / d x of the
 * action's row, g = p * sum(m) - m, what irbpp_dueling_loss_backward starts from.  The float32 arithmetic is defined
 * (csrc/irbpp_dueling_loss.hip: the column means and the exponential of irbpp_dueling_act, the library's own logarithm of the
 * denominator, every sum in ascending atoms) and reproducible bit for bit.  An action outside [-s_rows, s_rows) accesses
 * nothing out of range and gives loss = NaN, g = 0.  Finite logits and a finite non-negative m are the contract.
 * IRBPP_ERR_ARG unless 2 <= atoms <= 128, 1 <= s_rows <= 1024, batch >= 1, v_stride >= atoms, row_stride >= atoms,
 * env_stride >= (s_rows-1)*row_stride + atoms. */
int irbpp_dueling_loss(const float* v_dev, int64_t v_stride, const float* a_dev, int64_t env_stride, int64_t row_stride,
                       const int64_t* actions_dev, const float* m_dev, int32_t atoms, int32_t s_rows, int32_t batch,
                       float* loss_out_dev, float* g_out_dev, void* stream);
/* replaces: autograd's way back through the lines above, one launch: with gw = grad_loss[b] * g[b] and c = gw / (float)s_rows,
 * grad_v_out_dev float32 [batch][atoms] = gw, and grad_a_out_dev float32 [batch][s_rows][atoms], dense and contiguous,
 * = gw - c in the action's row and -c in every other row.  Either output may be NULL (that side needs no gradient); with both
 * NULL nothing is launched.  g_dev, actions_dev as given to / written by irbpp_dueling_loss; grad_loss_dev float32[batch],
 * contiguous.  Same limits on atoms, s_rows and batch. */
int irbpp_dueling_loss_backward(const float* g_dev, const float* grad_loss_dev, const int64_t* actions_dev, int32_t atoms,
                                int32_t s_rows, int32_t batch, float* grad_v_out_dev, float* grad_a_out_dev, void* stream);

/* The four effective layers of the value and advantage streams (model.py:393-394: fc_h_v, fc_z_v, fc_h_a, fc_z_a), float32 on
 * the device, row-major [out][in] and contiguous: w_hv [hidden][embed], w_zv [atoms][hidden], w_ha [hidden][embed],
 * w_za [atoms][hidden], each bias [out].  In training mode they are what irbpp_noisy_weights writes; in eval mode the mu
 * tensors as they are. */
typedef struct { const float *w_hv, *b_hv, *w_zv, *b_zv, *w_ha, *b_ha, *w_za, *b_za;   /* effective, row-major [out][in] */
                 int32_t embed, hidden, atoms; } irbpp_stream_weights;
/* replaces: NoisyLinear.forward's weight_mu + weight_sigma * weight_epsilon and the same for the bias (model.py, training
 * mode), for one layer: w_out[j][k] = mu[j][k] + sigma[j][k] * eps[j][k] and b_out[j] = bias_mu[j] + bias_sigma[j] *
 * bias_eps[j], the multiply and the add rounded separately: torch's two elementwise ops, bit for bit.  All arrays float32 on
 * the device and contiguous: [out][in] and [out].  Call it after every reset_noise, once per layer.
 * IRBPP_ERR_ARG unless 1 <= out, in <= 256 and no pointer is NULL. */
int irbpp_noisy_weights(const float* mu, const float* sigma, const float* eps, const float* bias_mu, const float* bias_sigma,
                        const float* bias_eps, int32_t out, int32_t in, float* w_out, float* b_out, void* stream);
/* replaces: the last stage of DQNBPP.forward (model.py:393-400: the value stream fc_z_v(relu(fc_h_v(xGlobal))), the advantage
 * stream fc_z_a(relu(fc_h_a(x))), v + a - a.mean(1), softmax over the atoms) and all of Agent.act after it (agent.py:51-58) in
 * one launch from the embeddings: neither the [n_env][s_rows][hidden] hidden block nor the advantage logits reach memory
 * unless a_out_dev asks for them.  xg_dev float32 [n_env][embed], rows xg_stride floats apart; x_dev float32
 * [n_env][s_rows][embed], row r of env e at x_dev + e*env_stride + r*row_stride; support, obs, q_out as in
 * irbpp_dueling_act; action_dev int64[n_env], may be NULL when only logits are wanted (with q_out_dev NULL too nothing
 * after the logits is computed).  v_out_dev (may be NULL) float32 [n_env][atoms] and a_out_dev (may be NULL) float32
 * [n_env][s_rows][atoms], contiguous: the logits irbpp_dueling_target consumes.  The float32 arithmetic is defined
 * (csrc/irbpp_streams.hip): every output of a layer is one chain acc = b[j]; acc = fmaf(x[k], W[j][k], acc) for k ascending,
 * a single-rounding fused multiply-add, never split or re-associated; relu(s) = s > 0 ? s : +0; from (v, a) on the
 * arithmetic of irbpp_dueling_act.  Reproducible bit for bit whatever n_env, the strides and the block's size.  Where
 * s_rows * (atoms | 1) * 4 exceeds the 144 KB LDS tile of irbpp_dueling_act, a_out_dev is required as workspace (the logits
 * go to memory and a second launch takes irbpp_dueling_act's path over them: the same bits).  Inputs must be finite: a NaN
 * or an infinity gives unspecified values, the action is still a row index in [0, s_rows) and nothing is accessed out of
 * range.  IRBPP_ERR_ARG unless 1 <= embed, hidden <= 256, 2 <= atoms <= 128, 1 <= s_rows <= 1024, n_env >= 1,
 * xg_stride >= embed, row_stride >= embed, env_stride >= (s_rows-1)*row_stride + embed, obs_stride >= 5*s_rows,
 * q_stride >= s_rows, support_dev given with action_dev or q_out_dev, at least one output, and a_out_dev where the block
 * does not fit. */
int irbpp_streams_act(const irbpp_stream_weights* w, const float* xg_dev, int64_t xg_stride, const float* x_dev,
                      int64_t env_stride, int64_t row_stride, const float* support_dev, const float* obs_dev, int32_t obs_stride,
                      int32_t s_rows, int32_t n_env, int64_t* action_dev /* may be NULL when only logits are wanted */,
                      float* q_out_dev, int64_t q_stride, float* v_out_dev, float* a_out_dev, void* stream);

/* irbpp_streams_act with the advantage stream on the matrix cores (csrc/irbpp_streams_mfma.hip, csrc/irbpp_mfma_chain.h): the
 * same arguments, the same outputs and the same definition, and the bits are those of irbpp_streams_act -- the float32
 * matrix instruction of gfx950 rounds once per product and accumulates in k order, so with the accumulator started from the
 * bias and the k-steps issued ascending every output is the chain of the definition.  Same workspace rule above the 144 KB
 * tile (the second launch is irbpp_streams_act's own), same limits, and embed % 4 == 0 and hidden % 4 == 0 (k is never
 * padded): IRBPP_ERR_ARG otherwise, never another form in its place. */
int irbpp_streams_act_mfma(const irbpp_stream_weights* w, const float* xg_dev, int64_t xg_stride, const float* x_dev,
                           int64_t env_stride, int64_t row_stride, const float* support_dev, const float* obs_dev,
                           int32_t obs_stride, int32_t s_rows, int32_t n_env, int64_t* action_dev /* may be NULL */,
                           float* q_out_dev, int64_t q_stride, float* v_out_dev, float* a_out_dev, void* stream);

/* The noise of the four layers (NoisyLinear's weight_epsilon [out][in] and bias_epsilon [out] buffers), float32 on the device
 * and contiguous, named as in irbpp_stream_weights. */
typedef struct { const float *w_hv, *b_hv, *w_zv, *b_zv, *w_ha, *b_ha, *w_za, *b_za; } irbpp_stream_noise;
/* Where irbpp_streams_backward writes the gradients of the four layers' sixteen parameter tensors (hv = fc_h_v, zv = fc_z_v,
 * ha = fc_h_a, za = fc_z_a), float32 on the device, contiguous, each of its parameter's shape.  Any of them may be NULL: that
 * parameter needs no gradient. */
typedef struct { float *hv_weight_mu, *hv_weight_sigma, *hv_bias_mu, *hv_bias_sigma, *zv_weight_mu, *zv_weight_sigma, *zv_bias_mu,
                 *zv_bias_sigma, *ha_weight_mu, *ha_weight_sigma, *ha_bias_mu, *ha_bias_sigma, *za_weight_mu, *za_weight_sigma,
                 *za_bias_mu, *za_bias_sigma; } irbpp_stream_grads;
/* replaces: autograd's way back through the four noisy layers of the streams (model.py:393-394, NoisyLinear.forward :224-228)
 * in Agent.learn's online forward, from the gradients of the logits irbpp_streams_act wrote to v_out_dev and a_out_dev:
 * gv_dev float32 [batch][atoms] and ga_dev float32 [batch][s_rows][atoms], contiguous.  Either may be NULL: it counts as
 * zeros, nothing is launched for its stream and that stream's outputs are +0.  w, xg_dev, x_dev and their strides as given to
 * irbpp_streams_act (w the effective weights); eps the layers' noise, NULL in eval mode (the sigma outputs are then left
 * alone).  Outputs, written and not added to, each may be NULL: dx_dev float32 [batch][s_rows][embed] and dxg_dev float32
 * [batch][embed], contiguous, and the sixteen tensors of grads: weight_mu = dW, weight_sigma = dW * weight_epsilon,
 * bias_mu = db, bias_sigma = db * bias_epsilon.  Defined float32 arithmetic (csrc/irbpp_streams_grad.hip), reproducible bit
 * for bit: the pre-activations are the forward's chains again; per row e[j] is the chain over the atoms of g[t] W_z[t][j] from
 * +0, d[j] = e[j] where the pre-activation is > 0 and +0 elsewhere, dx[k] the chain over j of d[j] W_h[j][k]; the advantage
 * stream's weight gradients are per sample chains over the rows, summed over the samples in ascending order with plain adds,
 * the value stream's chains over the samples; single-rounding fused multiply-adds, never split or re-associated, no atomics.
 * The bits depend on the data and (batch, s_rows) alone.  workspace_dev: irbpp_streams_backward_workspace bytes, written
 * before it is read.  At most four launches on `stream`.  Finite inputs are the contract: a NaN or an infinity gives
 * unspecified values and touches nothing out of range.
 * IRBPP_ERR_ARG unless 1 <= embed, hidden <= 256, 2 <= atoms <= 128, 1 <= s_rows <= 1024, 1 <= batch <= 1024, the strides as
 * for irbpp_streams_act, and w, its eight arrays, grads, xg_dev, x_dev, workspace_dev and, where eps is given, its eight
 * arrays are not NULL. */
int irbpp_streams_backward(const irbpp_stream_weights* w, const irbpp_stream_noise* eps /* NULL: eval mode */, const float* xg_dev,
                           int64_t xg_stride, const float* x_dev, int64_t env_stride, int64_t row_stride,
                           const float* ga_dev /* may be NULL */, const float* gv_dev /* may be NULL */, int32_t s_rows,
                           int32_t batch, float* workspace_dev, float* dx_dev, float* dxg_dev, const irbpp_stream_grads* grads,
                           void* stream);
/* The bytes of irbpp_streams_backward's workspace: batch * (hidden*embed + atoms*hidden + hidden + atoms + 2*hidden) floats --
 * per sample the advantage stream's four partials and the value stream's hidden row and its gradient.  0 outside the limits. */
int64_t irbpp_streams_backward_workspace(int32_t embed, int32_t hidden, int32_t atoms, int32_t s_rows, int32_t batch);

/* The shape encoder (model.py: shapeEncoder = Linear(3, hidden) LeakyReLU Linear(hidden, feat) LeakyReLU), float32 on the
 * device, row-major and contiguous: w1 [hidden][3], b1 [hidden], w2 [feat][hidden], b2 [feat]; slope is the LeakyReLU's
 * negative_slope (0.01 in the reference), >= 0. */
typedef struct { const float *w1, *b1, *w2, *b2; int32_t hidden, feat; float slope; } irbpp_shape_encoder;
/* replaces: the shape branch of DQNBPP.forward without a gradient (model.py:328-335, :365-372): shapeArray[ids.cpu()] on the
 * host, the gather of the sampled points, the copy to the device, shapeEncoder per row and the max over the points.  Two
 * launches on `stream`, no atomics: the feature is computed once per shape that occurs in the ids, then gathered.
 * points_dev float32 [n_shapes][n_points][3], contiguous; indices_dev int32 [k], one index set for all rows, duplicates are
 * legal; ids_dev [m_rows], element m at ids_dev[m * ids_stride] (a stride in elements: the id column of an [N][obs_len]
 * observation block passes as it is): float32 when ids_are_float != 0, truncated toward zero as .long() does, else int64;
 * out_dev float32 [m_rows][feat], rows out_stride floats apart; partial_dev float32 [n_shapes][partial_chunks][feat], a
 * workspace (rows of shapes that do not occur in the ids are neither written nor read).
 * The float32 arithmetic is defined (csrc/irbpp_shapefeat.hip): for row m with u = ids[m] and p_j = points[u][indices[j]],
 *   h1_j[i] = leaky(fmaf(p_j[2], w1[i][2], fmaf(p_j[1], w1[i][1], fmaf(p_j[0], w1[i][0], b1[i])))),
 *   s_j[f]  = b2[f], then s_j[f] = fmaf(h1_j[i], w2[f][i], s_j[f]) for i ascending,  leaky(s) = s > 0 ? s : slope * s,
 *   out[m][f] = max_j leaky(s_j[f]),
 * single-rounding fused multiply-adds, never split or re-associated.  The max is sticky for NaN (any NaN term gives the quiet
 * NaN 0x7fc00000, as torch.max does; fmaxf would drop it) and puts +0 above -0; it is exact, so the result does not depend
 * on partial_chunks, m_rows or the strides.  An id outside [0, n_shapes) -- NaN and infinite float ids included -- gives a NaN
 * row (torch's indexing raises there); an index outside [0, n_points) counts as a NaN point, so every row comes out NaN.
 * Nothing out of range is read in either case.
 * IRBPP_ERR_ARG unless 1 <= hidden, feat <= 256, slope >= 0, 1 <= k <= 4096, 1 <= n_shapes <= 65535, n_points >= 1,
 * m_rows >= 1, ids_stride >= 1, out_stride >= feat, partial_chunks == irbpp_shape_features_chunks(n_shapes, k) and no
 * pointer is NULL. */
int irbpp_shape_features(const float* points_dev, int32_t n_shapes, int32_t n_points, const int32_t* indices_dev, int32_t k,
                         const void* ids_dev, int32_t ids_are_float, int32_t ids_stride, int32_t m_rows,
                         const irbpp_shape_encoder* enc, float* partial_dev, int32_t partial_chunks, float* out_dev,
                         int32_t out_stride, void* stream);
/* The number of chunks the k points are split into for this many shapes (small shape sets get more chunks, so that they
 * still fill the chip): what partial_dev must be sized by.  0 outside the limits above. */
int irbpp_shape_features_chunks(int32_t n_shapes, int32_t k);
/* replaces: the same shape branch in the forward that carries a gradient (Agent.learn's online forward: the gather of the
 * sampled points, shapeEncoder per row with two [m_rows][k][hidden | feat] activation blocks kept for autograd, the max).
 * irbpp_shape_features with a record: the same arguments, the same definition and the same bits in out_dev, and
 *   arg_dev int32 [n_shapes][feat]: for a shape u that occurs in the ids the smallest j in [0, k) at which s_j[f] (before the
 *   second leaky, compared as the max compares: -0 below +0, every NaN on top) is largest; -1 in every entry of a shape that
 *   does not occur.
 * Workspaces: partial_key_dev uint32 and partial_j_dev int32, each [n_shapes][partial_chunks][feat].  Two launches on
 * `stream`, no atomics.  IRBPP_ERR_ARG as for irbpp_shape_features, and if arg_dev or a workspace is NULL. */
int irbpp_shape_features_arg(const float* points_dev, int32_t n_shapes, int32_t n_points, const int32_t* indices_dev, int32_t k,
                             const void* ids_dev, int32_t ids_are_float, int32_t ids_stride, int32_t m_rows,
                             const irbpp_shape_encoder* enc, uint32_t* partial_key_dev, int32_t* partial_j_dev,
                             int32_t partial_chunks, float* out_dev, int32_t out_stride, int32_t* arg_dev, void* stream);
/* The backward of irbpp_shape_features_arg for the encoder's four arrays (the points and the ids carry no gradient), from
 * grad_out_dev float32 [m_rows][feat], contiguous, and arg_dev as that call left it for the same points, indices, ids and
 * encoder: d_w1_dev [hidden][3], d_b1_dev [hidden], d_w2_dev [feat][hidden], d_b2_dev [feat] are written, not added to.
 * Defined float32 arithmetic (csrc/irbpp_shapefeat_grad.hip), reproducible bit for bit: the rows of grad_out are summed per
 * shape in ascending m, each (shape, feature) passes its sum to the one point arg names, through the leaky's derivative at
 * the recomputed s (s > 0 ? 1 : slope), and every sum over shapes or features is a chain in ascending order from +0.  Rows
 * with an id outside [0, n_shapes) contribute nothing.  Two launches on `stream`, no atomics.
 * Workspaces, both 16-byte aligned: point_d2_dev float32 [n_shapes][feat][4], first_dev float32 [n_shapes][hidden][4] (rows of
 * shapes that do not occur are neither written nor used).
 * IRBPP_ERR_ARG outside irbpp_shape_features' limits, for a NULL pointer or a misaligned workspace. */
int irbpp_shape_features_backward(const float* points_dev, int32_t n_shapes, int32_t n_points, const int32_t* indices_dev, int32_t k,
                                  const void* ids_dev, int32_t ids_are_float, int32_t ids_stride, int32_t m_rows,
                                  const irbpp_shape_encoder* enc, const int32_t* arg_dev, const float* grad_out_dev,
                                  float* point_d2_dev, float* first_dev, float* d_w1_dev, float* d_b1_dev, float* d_w2_dev,
                                  float* d_b2_dev, void* stream);

/* The layers of the embedding stage (model.py: heightEncoder = Conv2d(1, c1, 4, 2, 1) LeakyReLU Conv2d(c1, c2, 4, 2, 1) LeakyReLU
 * Conv2d(c2, c3, 3, 1, 1) LeakyReLU; init_candidate_embed = Linear(4, cand_hidden) LeakyReLU Linear(cand_hidden, cand_embed);
 * project_layer = Linear(feat + c3 (map_len/4)^2 + cand_embed, proj_hidden) LeakyReLU Linear(proj_hidden, embed)), float32 on
 * the device, contiguous, in torch's layouts: convolution weights [out][in][ky][kx], linear weights [out][in].  map_len is the
 * heightmap's side L; slope the LeakyReLUs' negative_slope (0.01 in the reference), >= 0. */
typedef struct { const float *w_conv1, *b_conv1, *w_conv2, *b_conv2, *w_conv3, *b_conv3, *w_c1, *b_c1, *w_c2, *b_c2, *w_p1, *b_p1,
                 *w_p2, *b_p2;
                 int32_t map_len, c1, c2, c3, feat, cand_hidden, cand_embed, proj_hidden, embed; float slope; } irbpp_embed_weights;
/* replaces: the embedding stage of DQNBPP.forward without a gradient (model.py:318-326, :337-352, bufferSize == 1): the
 * heightmap CNN, init_candidate_embed per candidate row, the [n_env * s_rows][feat + M + cand_embed] concatenation, both layers
 * of project_layer, the boolean-mask zeroing of the invalid rows and the mean over the rows.  Two launches on `stream`, no
 * atomics: the part of every project_layer[0] chain that is the same for all rows of a bin (shape feature, map feature) runs
 * once per bin into base_dev, every row continues from there; neither the concatenation nor the hidden blocks reach memory.
 * obs_dev float32 [n_env][obs_stride]: obs[5r .. 5r+3] candidate r, obs[5r+4] its mask, obs[5 s_rows + 9 ..] the map_len x
 * map_len heightmap, row-major (the item id at obs[5 s_rows] is not read); shape_feat_dev float32 [n_env][feat], rows
 * feat_stride floats apart (irbpp_shape_features' out); base_dev float32 [n_env][proj_hidden], a workspace; x_dev float32
 * [n_env][s_rows][embed], row r of env e at x_dev + e*env_stride + r*row_stride; xg_dev float32 [n_env][embed], rows
 * xg_stride floats apart: what irbpp_streams_act takes as x_dev and xg_dev.
 * The float32 arithmetic is defined (csrc/irbpp_embed.hip): every output of a layer is one chain acc = b[j]; acc =
 * fmaf(x[k], W[j][k], acc) for k ascending, a single-rounding fused multiply-add, never split or re-associated; a
 * convolution's chain runs over its taps in ascending (c_in, ky, kx), a tap in the padding taking part with the input +0.0;
 * project_layer[0]'s chain runs over the shape feature, the map feature and the candidate embedding in that order, as over
 * the concatenation; leaky(s) = s > 0 ? s : slope * s.  A row is valid iff its mask == 1.0f exactly (a NaN mask is invalid);
 * an invalid row is +0.0 in every element of x, whatever its candidate holds.  xg is the mean over all s_rows rows of x in
 * irbpp_dueling_act's summation: 16 interleaved partial sums (part g: rows g, g+16, .. ascending from 0.0) added left to
 * right, divided by (float)s_rows.  Reproducible bit for bit whatever n_env and the strides; no index depends on data, so
 * nothing is accessed out of range whatever the values.
 * IRBPP_ERR_ARG unless map_len is a multiple of 4 in [8, 32], 1 <= c1 <= 16, 1 <= c2 <= 32, 1 <= c3 <= 4, 1 <= feat,
 * cand_embed, proj_hidden, embed <= 256, 1 <= cand_hidden <= 64, slope >= 0, 1 <= s_rows <= 1024, n_env >= 1,
 * obs_stride >= 5*s_rows + 9 + map_len^2, feat_stride >= feat, row_stride >= embed, env_stride >= (s_rows-1)*row_stride +
 * embed, xg_stride >= embed and no pointer is NULL. */
int irbpp_embed(const irbpp_embed_weights* w, const float* obs_dev, int64_t obs_stride, const float* shape_feat_dev,
                int64_t feat_stride, int32_t s_rows, int32_t n_env, float* base_dev /* workspace [n_env][proj_hidden] */,
                float* x_dev, int64_t env_stride, int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream);

/* irbpp_embed with the three per-row layers (init_candidate_embed[1], the candidate columns of project_layer[0],
 * project_layer[1]) on the matrix cores (csrc/irbpp_embed_mfma.hip, csrc/irbpp_mfma_chain.h): the same arguments, workspace,
 * outputs and definition, two launches on `stream` (irbpp_embed's own bin kernel, then the row kernel of this form).  The
 * float32 matrix instruction of gfx950 rounds once per product and accumulates in k order, so with the accumulator started
 * from the chain's start (the bias, base) and the k-steps issued ascending every output is the chain of the definition: x and
 * xg equal irbpp_embed's bit for bit wherever irbpp_embed's are not NaN, and are NaN where they are (a NaN's payload is not
 * part of the definition).  Same limits and status codes, and cand_hidden % 4 == 0, cand_embed % 4 == 0 and
 * proj_hidden % 4 == 0 (the k of the three products is never padded): IRBPP_ERR_ARG otherwise, never another form in its
 * place. */
int irbpp_embed_mfma(const irbpp_embed_weights* w, const float* obs_dev, int64_t obs_stride, const float* shape_feat_dev,
                     int64_t feat_stride, int32_t s_rows, int32_t n_env, float* base_dev /* workspace [n_env][proj_hidden] */,
                     float* x_dev, int64_t env_stride, int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream);

/* The layers of the order network's embedding stage (model.py, bufferSize > 1: heightEncoder as above; gat_project_layer =
 * Linear(feat + c3 (map_len/4)^2, proj_hidden) LeakyReLU Linear(proj_hidden, embed); embedder = GraphAttentionEncoder with
 * one head and one layer: W_query, W_key, W_val Linear(embed, embed) without a bias, W_out Linear(embed, embed), the
 * feed-forward pair Linear(embed, ff_hidden) ReLU Linear(ff_hidden, embed)), float32 on the device, contiguous, in torch's
 * layouts.  w_g1 keeps the reference's columns: [0 .. feat) the shape feature, [feat ..) the map feature. */
typedef struct { const float *w_conv1, *b_conv1, *w_conv2, *b_conv2, *w_conv3, *b_conv3,
                 *w_g1, *b_g1, *w_g2, *b_g2, *w_q, *w_k, *w_v, *w_o, *b_o, *w_f1, *b_f1, *w_f2, *b_f2;
                 int32_t map_len, c1, c2, c3, feat, proj_hidden, embed, ff_hidden; float slope; } irbpp_order_embed_weights;
/* replaces: the embedding stage of DQNBPP.forward without a gradient for bufferSize > 1 (model.py:355-383,
 * embed_k_buffer_shape_with_gat, with :26-171 and :284-294; the order network of trainer_hierarchical, trainer.py:266): the
 * heightmap CNN, the [n_env * k_slots][feat + M] concatenation, both layers of gat_project_layer, Q / K / V, the two batched
 * k x k matmuls, the softmax, the clone and masked assignment (the mask is all zeros on this path and does not enter), W_out,
 * the feed-forward pair, the two residual adds and the mean.  Two launches on `stream`, no atomics: the map part of every
 * gat_project_layer[0] chain runs once per bin into base_dev; then tiles of 64 / k_slots whole bins, one (bin, slot) row
 * per lane; Q, K, V, the compatibilities and every hidden block stay in LDS and registers.
 * obs_dev float32 [n_env][obs_stride]: obs[0 .. k_slots) the buffered item ids (not read), obs[k_slots ..] the map_len x
 * map_len heightmap, row-major; shape_feat_dev float32 [n_env * k_slots][feat], bin-major, (bin, slot) rows feat_stride
 * floats apart (irbpp_shape_features' out over the n_env * k_slots ids); base_dev float32 [n_env][proj_hidden], a
 * workspace; x_dev float32 [n_env][k_slots][embed], row i of env e at x_dev + e*env_stride + i*row_stride; xg_dev float32
 * [n_env][embed], rows xg_stride floats apart: what irbpp_streams_act takes as x_dev and xg_dev with s_rows = k_slots and
 * obs_dev = NULL.
 * The float32 arithmetic is defined (csrc/irbpp_order_embed.hip): every output of a layer is one chain acc = start; acc =
 * fmaf(x[c], W[j][c], acc) for c ascending, a single-rounding fused multiply-add, never split or re-associated; leaky(s) =
 * s > 0 ? s : slope * s, relu(s) = s > 0 ? s : +0; the CNN as in irbpp_embed.  gat_project_layer[0]'s chain starts from its
 * bias, runs over the map feature against columns [feat ..) FIRST (once per bin) and then over the slot's shape feature
 * against columns [0 .. feat): a fixed permutation of the concatenation's summation order.  h0 = gat_project_layer[1] (no
 * activation).  Q, K, V are chains from +0.0; c[i][j] = nf * (the chain from +0.0 of fmaf(Q[i][d], K[j][d], acc), d
 * ascending) with nf = (float)(1.0 / sqrt((double)embed)); m = max_j c[i][j], e[j] = exp(c[i][j] - m) by irbpp_dueling_act's
 * exp, den the e[j] added left to right from 0.0, a[i][j] = e[j] / den; hd[i][d] the chain from +0.0 of fmaf(a[i][j],
 * V[j][d], acc), j ascending; h1 = h0 + lin(W_out, hd); h2 = h1 + lin(ff2, relu(lin(ff1, h1))); x = h2 and xg the mean of
 * the k_slots rows in irbpp_dueling_act's summation (16 interleaved partial sums added left to right, divided by
 * (float)k_slots).  Reproducible bit for bit whatever n_env, the strides and the tiles; no index depends on data, so nothing
 * is accessed out of range whatever the values.  Inputs must be finite: a NaN gives unspecified values.
 * IRBPP_ERR_ARG unless map_len is a multiple of 4 in [8, 32], 1 <= c1 <= 16, 1 <= c2 <= 32, 1 <= c3 <= 4, 1 <= feat,
 * proj_hidden, embed, ff_hidden <= 256, slope >= 0, 2 <= k_slots <= 64, n_env >= 1, obs_stride >= k_slots + map_len^2,
 * feat_stride >= feat, row_stride >= embed, env_stride >= (k_slots-1)*row_stride + embed, xg_stride >= embed and no pointer
 * is NULL. */
int irbpp_order_embed(const irbpp_order_embed_weights* w, const float* obs_dev, int64_t obs_stride,
                      const float* shape_feat_dev, int64_t feat_stride /* between (bin, slot) rows */,
                      int32_t k_slots, int32_t n_env, float* base_dev /* workspace [n_env][proj_hidden] */,
                      float* x_dev, int64_t env_stride, int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream);

/* irbpp_order_embed with its eight linear layers (both of gat_project_layer, W_query, W_key, W_val, W_out and the
 * feed-forward pair) on the matrix cores (csrc/irbpp_order_embed_mfma.hip, csrc/irbpp_mfma_chain.h): the same arguments,
 * workspace, outputs and definition, two launches on `stream` (irbpp_order_embed's own bin kernel, then the row kernel of this
 * form); the k x k attention between the layers stays on the vector unit.  The float32 matrix instruction of gfx950 rounds
 * once per product and accumulates in k order, so with the accumulator started from the chain's start (base of the row's
 * bin, a bias, +0.0), the k-steps issued ascending and each residual added after its chain every output is the chain of the
 * definition: x and xg equal irbpp_order_embed's bit for bit wherever irbpp_order_embed's are not NaN.  Same limits and
 * status codes, and feat % 4 == 0, proj_hidden % 4 == 0, embed % 4 == 0 and ff_hidden % 4 == 0 (the k of the eight products
 * is never padded): IRBPP_ERR_ARG otherwise, never another form in its place. */
int irbpp_order_embed_mfma(const irbpp_order_embed_weights* w, const float* obs_dev, int64_t obs_stride,
                           const float* shape_feat_dev, int64_t feat_stride /* between (bin, slot) rows */,
                           int32_t k_slots, int32_t n_env, float* base_dev /* workspace [n_env][proj_hidden] */,
                           float* x_dev, int64_t env_stride, int64_t row_stride, float* xg_dev, int64_t xg_stride, void* stream);

/* One parameter tensor of the optimiser step: float32, contiguous, numel elements, 4-byte alignment is enough (16-byte
 * aligned bases take 16-byte accesses).  target may be NULL (nothing is copied for that tensor). */
typedef struct { float *param, *grad, *exp_avg, *exp_avg_sq, *target; int64_t numel; } irbpp_optim_tensor;
#define IRBPP_ADAM_WRITE_GRADS 1   /* store the clipped gradient back, as clip_grad_norm_ leaves it                          */
#define IRBPP_ADAM_ZERO_GRADS  2   /* store 0.0f in its place: the next step's zero_grad, with stable gradient pointers     */
#define IRBPP_ADAM_SYNC_TARGET 4   /* store the new parameter to `target` as well: update_target_net for the parameters      */
#define IRBPP_ADAM_CLIP_ONLY   8   /* no Adam: the gradients are scaled and written back, clip_grad_norm_ alone             */
/* step_size = (float)(lr / (1 - beta1^t)) and rsq = (float)sqrt(1 - beta2^t), computed in float64 for the 1-based step t;
 * one_minus_beta1/2 the float32 values the update multiplies by. */
typedef struct { float step_size, rsq, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, max_norm; int32_t flags; } irbpp_adam_hyper;
/* replaces: clip_grad_norm_(online_net.parameters(), norm_clip) and optimiser.step() of optim.Adam (agent.py:120-121, 44), with
 * IRBPP_ADAM_ZERO_GRADS the next online_net.zero_grad() and with IRBPP_ADAM_SYNC_TARGET update_target_net's copy of the
 * parameters (agent.py:127-128), in two launches on `stream` over all tensors at once.  tensors_dev: the n_tensors tensors
 * that take part; chunks_dev: int32 [n_chunks][2] = (tensor, first element), every tensor cut into chunks of 1024 elements
 * in ascending order, its last chunk short (numel < 2^31); partial_dev: workspace float64 [n_chunks].  The arithmetic is
 * defined (csrc/irbpp_optim.hip: the squares summed in float64 in one fixed order without atomics, total = (float)sqrt(sum),
 * coef = max_norm / (total + 1e-6f) where that is < 1 and else 1, torch's Adam update with two fmaf) and reproducible bit for
 * bit.  total_norm_dev float32[1] receives total.  A sum whose exponent field is all ones (an infinite or NaN gradient)
 * skips the step: no tensor is written, *skipped_dev goes up by one, total is +inf or the NaN 0x7fc00000.  `hyper` is host
 * memory, read at the call.  The tables are device data and are not checked: a wrong entry is an out-of-range access.
 * IRBPP_ERR_ARG, before anything is launched, if a pointer is NULL, n_tensors < 1, n_chunks < n_tensors, flags has an
 * unknown bit, WRITE_GRADS together with ZERO_GRADS, or CLIP_ONLY together with ZERO_GRADS or SYNC_TARGET. */
int irbpp_clipped_adam_step(const irbpp_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunks_dev, int32_t n_chunks,
                            double* partial_dev, const irbpp_adam_hyper* hyper /* host, read at the call */,
                            float* total_norm_dev, int64_t* skipped_dev, void* stream);

/* Tooling: when cycles_dev != NULL every later transition launch stores, per bin, one row
 * int64[num_bins][16]: shader-clock stamps 0 start, 1 action applied, 2 overlap test done,
 * 3 contour stage done, 4 observation written; 5..7 contour-stage detail; 8/9 the 100 MHz wall
 * clock at entry/exit; 10 = HW_ID | XCC_ID<<32 of the CU that ran the bin; 11..15 unused.
 * NULL switches it off. */
int irbpp_debug_phase_cycles(irbpp_env* env, int64_t* cycles_dev);

/* Tooling: time the transition kernel alone.  capacity > 0 creates a ring of that many HIP event
 * pairs; every later transition launch (reset / step / get_action_candidates) records the next
 * pair on its stream right around irbpp_env_kernel (the few-microsecond ordering kernel in front
 * of it stays outside the bracket).  capacity 0 frees the ring.
 * irbpp_debug_kernel_times waits for the recorded launches and writes the durations of the latest
 * min(max_count, recorded) of them in ms to ms_host, oldest first; *count says how many; the ring
 * is then empty again. */
/* Tooling: LDS bytes per workgroup of the transition kernel for this configuration and the names of the kernels a step over
 * all bins of this environment launches, " + "-separated, the transition kernel's build first (a string owned by the
 * environment, rewritten by the next call).  Valid after irbpp_load_shapes. */
int irbpp_debug_kernel_info(const irbpp_env* env, int32_t* lds_bytes, const char** kernel_name);
/* The overlap path irbpp_load_shapes chose for the data set: 1 block path (every footprint a union of uniform b x b
 * tiles: lattice data), 2 box path (every footprint a solid box), 3 generic cell lists, 4 mixed (the block path for the rotations
 * whose footprints are lattice footprints, cell lists for the others: BlockOut at eight rotations); IRBPP_ERR_STATE before the
 * shapes are loaded.  (vec_env.groups_for decides by it how many groups of bins to step a data set as.) */
int irbpp_overlap_path(const irbpp_env* env);
int irbpp_debug_kernel_timing(irbpp_env* env, int32_t capacity);
/* events around every `every`-th transition only (default 1): two event packets per step cost the stream ~5 % at
 * 0.15 ms per step, so bench.py samples every fourth step of its timed region */
int irbpp_debug_kernel_timing_every(irbpp_env* env, int32_t every);
int irbpp_debug_kernel_times(irbpp_env* env, float* ms_host, int32_t max_count, int32_t* count);
/* Tooling: shrink the capacity of the eight per-die lists of polygon rounds (trace kernel -> polygon kernel), so that a FULL
 * list -- trace waves that approximate their borders in place, empty entries below the cap, the polygon kernel's clamp -- can
 * be reached with a handful of bins.  1 <= cap <= the capacity irbpp_create computed ((num_bins / 8 + 64) * 16); the
 * allocation stays as it is and both kernels index the lists with the cap as their stride.  IRBPP_ERR_ARG outside that range
 * and on the wide path (which has no such lists); IRBPP_ERR_STATE once a transition has been launched: one stride for the
 * environment's whole life keeps every stale entry a well-formed record of an earlier observation (the memory starts zeroed,
 * which reads as empty records).  Results never depend on the cap. */
int irbpp_debug_round_cap(irbpp_env* env, int32_t cap);
/* Tooling: the eight lists' reservation totals of the last observing launch to out[0..7] on the host: every trace wave adds
 * its rounds to its die's counter whether they fit or not, so a total above the cap says that list was full.  The emit kernel
 * that ends an observation retires the counters, so they are copied on the stream right behind the trace kernel -- from the
 * FIRST call of this function on, which switches that copy on (and answers zeros, like every call before a launch).
 * Synchronises the stream.  IRBPP_ERR_ARG on the wide path. */
int irbpp_debug_round_counts(irbpp_env* env, int32_t out[8], void* stream);

/* Device-side error word raised by kernels (0 = none).  Synchronises the stream. */
int irbpp_device_error(irbpp_env* env, void* stream, int32_t* flags_out);

#define IRBPP_DEVERR_LEVEL_RANGE   1   /* a height level fell outside the level codes of the configuration */
#define IRBPP_DEVERR_TRACE_GUARD   2   /* border following exceeded its iteration guard      */
#define IRBPP_DEVERR_BAD_ITEM      4   /* item id outside the loaded shape table             */
#define IRBPP_DEVERR_BAD_BIN       8   /* irbpp_reset_bins, irbpp_save_bins / irbpp_load_bins / irbpp_copy_bins: bin index outside
                                          [0, num_bins); the bin (the pair) was skipped              */
#define IRBPP_DEVERR_CAPACITY     16   /* a die's candidate list overflowed (it holds twice the worst case of a fair
                                          share of the bins): results of that step are incomplete                */
#define IRBPP_DEVERR_BAD_ACTION   64   /* irbpp_step / irbpp_get_action_candidates: an action outside [-S, S) (order action: [-k, k)):
                                          the reference raises IndexError at binPhy.py:235 / :163; a negative index in
                                          range counts from the end, as there.  The step ran on a clamped index.
                                          irbpp_step_cells: a cell outside the action grid (no wrap-around)           */
#define IRBPP_DEVERR_STREAM_DRY   32   /* item_stream = 1: a bin fetched a ring slot it had consumed already and the host
                                          had not rewritten (irbpp_stream_write): its episode got no item there  */

#ifdef __cplusplus
}
#endif
#endif /* IRBPP_H */
