// irbpp_dueling.hip -- the dueling head fused in front of the distributional head: the end of DQNBPP.forward
// (model.py:395-400: q = v + a - a.mean(1), softmax over the atoms) and the consumers of irbpp_c51.hip in one launch each,
// from the network's logits.  The [N][S][atoms] probabilities exist only in LDS unless the caller asks for them.
//
// Defined float32 arithmetic (multiply and add separate, -ffp-contract=off; tests/test_dueling_cpu.py restates it in numpy and
// the kernels are held to it bit for bit).  For one environment, v[atoms], a[S][atoms], z[atoms]:
//   part[g][k] = 0.0f + a[g][k] + a[g+16][k] + a[g+32][k] + ...        g = 0..15, rows ascending (an empty part stays 0)
//   mean[k]    = ((..(part[0][k] + part[1][k]) + ..) + part[15][k]) / (float)S                         IEEE division
//   x[i][k]    = (v[k] + a[i][k]) - mean[k]
//   mx[i]      = max_k x[i][k];  t = x[i][k] - mx[i];  e[i][k] = dexp(t)
//   den[i]     = ((e[i][0] + e[i][1]) + ..) + e[i][atoms-1]            (>= 1: the maximum's e is dexp(0) = 1)
//   p[i][k]    = e[i][k] / den[i]                                                                       IEEE division
//   q[i]       = ((p[i][0] z[0] + p[i][1] z[1]) + ..), every product and sum rounded: the value of irbpp_c51.hip
// The order is a function of (S, atoms) alone: not of N, of strides, of the launch, or of whether the block stayed in LDS.
// Mask, first maximum and the all-masked index 0 are the rules of irbpp_head.h, where the mean, the combine, dexp and the
// projection of the target kernel are written (for irbpp_dueling_loss.hip too).  Finite logits are the contract: a NaN or an
// infinite logit gives unspecified values in q_out, p_out and m, but the action / a_star is still a row of the block and
// nothing is read or written out of range.
//
// Layout: one workgroup of 512 threads per environment.  The a block is staged once into LDS with coalesced dword loads
// (consecutive threads, consecutive addresses of a row), rows `atoms | 1` floats apart (odd pitch: thread-per-row reads
// fall on 32 different banks), wherever S rows fit DUELING_TILE_BYTES; the column sums and the rows are then read from
// LDS.  A larger block takes its column sums from global memory and stages 256 rows at a time (a second pass).
#include "irbpp_head.h"

namespace irbpp {

// nrows rows of the block (src: its row r0) into the tile
__device__ __forceinline__ void dueling_stage(const float* __restrict__ src, long long row_stride, int atoms, int nrows, float* tile) {
    const int pitch = atoms | 1;
    head_walk<DUELING_THREADS>(atoms, nrows, [&](int row, int k, int) { tile[row * pitch + k] = src[(size_t)row * row_stride + k]; });
}

// One row of the tile in place: a -> p; returns its expected value.  sv, smean, sz: LDS copies of v, mean and the support.
__device__ __forceinline__ float dueling_row(float* rw, const float* sv, const float* smean, const float* sz, int atoms) {
    const float mx = dueling_combine(rw, sv, smean, atoms);
    float den = dueling_dexp(rw[0] - mx);
    rw[0] = den;
    for (int k = 1; k < atoms; ++k) {
        const float e = dueling_dexp(rw[k] - mx);
        rw[k] = e;
        den = den + e;
    }
    const float p0 = rw[0] / den;
    rw[0] = p0;
    float s = p0 * sz[0];
    for (int k = 1; k < atoms; ++k) {
        const float p = rw[k] / den;
        rw[k] = p;
        s = s + p * sz[k];
    }
    return s;
}

// One workgroup: the masked arg-max over the s_rows rows of one environment's head, from its logits.  flags, q_out as in
// c51_wave_argmax; p_out (may be NULL) receives the [s_rows][atoms] probabilities, contiguous.  Every thread returns the index.
__device__ __forceinline__ int dueling_block_argmax(const float* __restrict__ v, const float* __restrict__ a, long long row_stride,
                                                    const float* __restrict__ z, int atoms, int s_rows,
                                                    const float* __restrict__ flags, float* __restrict__ q_out,
                                                    float* __restrict__ p_out, float* tile, DuelingShared& sh) {
    const int tid = threadIdx.x, pitch = atoms | 1;
    const int tile_rows = dueling_tile_rows(s_rows, atoms);
    const bool resident = tile_rows == s_rows;
    if (tid < atoms) {
        sh.v[tid] = v[tid];
        sh.z[tid] = z[tid];
    }
    if (resident) {
        dueling_stage(a, row_stride, atoms, s_rows, tile);
        __syncthreads();
        dueling_mean(tile, pitch, atoms, s_rows, sh.part, sh.mean);
    } else {
        dueling_mean(a, row_stride, atoms, s_rows, sh.part, sh.mean);
    }
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int r0 = 0; r0 < s_rows; r0 += tile_rows) {
        const int nrows = s_rows - r0 < tile_rows ? s_rows - r0 : tile_rows;
        if (!resident) {
            dueling_stage(a + (size_t)r0 * row_stride, row_stride, atoms, nrows, tile);
            __syncthreads();
        }
        for (int lr = tid; lr < nrows; lr += DUELING_THREADS) {
            const int i = r0 + lr;
            const float s = dueling_row(tile + lr * pitch, sh.v, sh.mean, sh.z, atoms);
            if (q_out) q_out[i] = s;
            const float val = head_masked(flags, i, s);
            if (head_better(val, i, best, bi)) { best = val; bi = i; }
        }
        __syncthreads();
        if (p_out) {
            float* dst = p_out + (size_t)r0 * atoms;
            head_walk<DUELING_THREADS>(atoms, nrows, [&](int row, int k, int e) { dst[e] = tile[row * pitch + k]; });
        }
        __syncthreads();                                 // the tile is rewritten by the next trip
    }
    head_wave_argmax(best, bi);
    if ((tid & 63) == 0) {
        sh.best[tid >> 6] = best;
        sh.bi[tid >> 6] = bi;
    }
    __syncthreads();
    best = sh.best[0];
    bi = sh.bi[0];
    for (int w = 1; w < DUELING_THREADS / 64; ++w) {
        const float ob = sh.best[w];
        const int oi = sh.bi[w];
        if (head_better(ob, oi, best, bi)) { best = ob; bi = oi; }
    }
    __syncthreads();                                     // sh is reused by the caller
    return head_index(bi, s_rows);
}

// DQNBPP.forward's combine + softmax (model.py:395-400) and Agent.act after it (agent.py:51-58), per environment.
extern "C" __global__ void __launch_bounds__(DUELING_THREADS)
irbpp_dueling_act_kernel(const float* __restrict__ v, long long v_stride, const float* __restrict__ a, long long env_stride,
                         long long row_stride, const float* __restrict__ support, int atoms, const float* __restrict__ obs,
                         int obs_stride, int s_rows, int64_t* __restrict__ action, float* __restrict__ q_out, long long q_stride,
                         float* __restrict__ p_out) {
    HIP_DYNAMIC_SHARED(float, dueling_tile)             // dueling_tile_rows() * (atoms | 1) floats
    __shared__ DuelingShared sh;
    const int env = blockIdx.x;
    const int bi = dueling_block_argmax(v + (size_t)env * v_stride, a + (size_t)env * env_stride, row_stride, support, atoms, s_rows,
                                        obs ? obs + (size_t)env * obs_stride : nullptr,
                                        q_out ? q_out + (size_t)env * q_stride : nullptr,
                                        p_out ? p_out + (size_t)env * s_rows * atoms : nullptr, dueling_tile, sh);
    if (threadIdx.x == 0) action[env] = bi;
}

// Agent.learn's no_grad block (agent.py:90-115) from the logits of the two networks, per sample: a* from the online (v, a),
// unmasked; pns_a = row a* of the target net's softmax by the same arithmetic (the target block's mean, read once from global
// memory, and that one row); then head_project's projection, the one irbpp_c51_target_kernel does.
extern "C" __global__ void __launch_bounds__(DUELING_THREADS)
irbpp_dueling_target_kernel(const float* __restrict__ v_online, long long von_stride, const float* __restrict__ a_online,
                            long long on_env_stride, long long on_row_stride, const float* __restrict__ v_target,
                            long long vtg_stride, const float* __restrict__ a_target, long long tg_env_stride,
                            long long tg_row_stride, const float* __restrict__ returns, const float* __restrict__ nonterminals,
                            const float* __restrict__ support, int atoms, int s_rows, float gamma_n, float v_min, float v_max,
                            float delta_z, float* __restrict__ m, int64_t* __restrict__ a_star) {
    HIP_DYNAMIC_SHARED(float, dueling_tile)
    __shared__ DuelingShared sh;
    __shared__ HeadProjection proj;
    const int smp = blockIdx.x, tid = threadIdx.x;
    const int best = dueling_block_argmax(v_online + (size_t)smp * von_stride, a_online + (size_t)smp * on_env_stride, on_row_stride,
                                          support, atoms, s_rows, nullptr, nullptr, nullptr, dueling_tile, sh);
    if (tid == 0) a_star[smp] = best;
    const float* at = a_target + (size_t)smp * tg_env_stride;
    dueling_mean(at, tg_row_stride, atoms, s_rows, sh.part, sh.mean);
    if (tid < atoms) {
        sh.v[tid] = v_target[(size_t)smp * vtg_stride + tid];
        dueling_tile[tid] = at[(size_t)best * tg_row_stride + tid];
    }
    __syncthreads();
    if (tid == 0) dueling_row(dueling_tile, sh.v, sh.mean, sh.z, atoms);       // the row is sequential in k by definition
    head_project<DUELING_THREADS>(dueling_tile, sh.z, returns[smp], nonterminals[smp] * gamma_n, v_min, v_max, delta_z, atoms,
                                  m + (size_t)smp * atoms, proj);               // opens with the barrier the row needs
}

}  // namespace irbpp
