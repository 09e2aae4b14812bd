// irbpp_streams.hip -- the last stage of DQNBPP.forward fused in front of the dueling head: the four NoisyLinear layers of the
// value and advantage streams (model.py:393-394), the combine + softmax (model.py:395-400) and Agent.act after it
// (agent.py:51-58) in one launch, from the embeddings.  Neither the [N][S][H] hidden block nor the [N][S][atoms] advantage
// logits reach memory unless the caller asks for the logits.  Included after irbpp_dueling.hip, whose dueling_row and
// dueling_block_argmax it calls (irbpp_capi.hip and tests/host/streams_host.cpp include them in that order).
//
// Defined float32 arithmetic (tests/test_streams_cpu.py restates it and the kernels are held to it bit for bit):
//   W[j][k]  = mu[j][k] + sigma[j][k] * eps[j][k], b[j] likewise: multiply and add separate (irbpp_noisy_weights_kernel;
//              torch's two elementwise ops).  In eval mode the caller passes mu as W.
//   lin(W, b, x)[j]: acc = b[j]; for k = 0 .. K-1 ascending: acc = fmaf(x[k], W[j][k], acc).  The one place in the library
//              where a fused multiply-add is part of the definition: it is written out (fmaf), the build still contracts
//              nothing (-ffp-contract=off), and a chain is never split or re-associated.
//   relu(s)  = s > 0 ? s : +0.0f
//   v        = lin(W_zv, b_zv, relu(lin(W_hv, b_hv, xg)))               per environment
//   a[s]     = lin(W_za, b_za, relu(lin(W_ha, b_ha, x[s])))             per row
//   from (v, a) on: irbpp_dueling_act's definition through the same functions (irbpp_head.h, irbpp_dueling.hip).
// The result is a function of the inputs alone: not of N, of strides, of which instantiation ran, or of whether the block
// stayed in LDS.  Non-finite inputs: unspecified values, an action in [0, S), nothing accessed out of range (no index
// depends on data).
//
// Layout: one workgroup of 512 threads per environment, one row of x per thread (two trips above 512 rows).  The weights
// are wave-uniform: every lane of a wave multiplies its own x[k] or h[j] by the same W element, so they are read through
// plain loads of __restrict__ kernel arguments with wave-uniform addresses (the scalar cache) and feed the FMA as a scalar
// operand; no LDS traffic for them.  Hidden units are made STREAMS_HBLOCK at a time and consumed at once by the atoms'
// accumulators, in ascending j: the hidden row never exists as a whole.  <128, 32> (E = 128, atoms <= 32: the acting loop)
// holds its x row in registers and reads each W_ha row contiguously; <0, 128> is the generic form for every other shape
// within the limits, x re-read per block of hidden units.  The a block goes to the dueling tile (pitch atoms | 1) and is
// finished there; a block that does not fit the tile is written to a_out and finished by irbpp_streams_finish_kernel
// through dueling_block_argmax, the path of irbpp_dueling_act_kernel.
#include "irbpp_head.h"

namespace irbpp {

constexpr int STREAMS_MAX_WIDTH = 256;                   // E and H
constexpr int STREAMS_HBLOCK = 16;                       // hidden units per block: 16 contiguous W_za elements per atom

struct alignas(16) StreamsVec4 { float f[4]; };

__device__ __forceinline__ float streams_relu(float s) { return s > 0.0f ? s : 0.0f; }

// W = mu + sigma * eps for one layer, [out][in] contiguous, and its bias
extern "C" __global__ void __launch_bounds__(256)
irbpp_noisy_weights_kernel(const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ eps,
                           const float* __restrict__ bias_mu, const float* __restrict__ bias_sigma,
                           const float* __restrict__ bias_eps, int out, int in, float* __restrict__ w_out,
                           float* __restrict__ b_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)out * in) w_out[i] = mu[i] + sigma[i] * eps[i];
    if (i < out) b_out[i] = bias_mu[i] + bias_sigma[i] * bias_eps[i];
}

// The value stream of one environment by the workgroup: hv (LDS, H floats) the hidden row, v_dst (LDS) the atoms logits.
// Ends with a barrier.
__device__ __forceinline__ void streams_value(const float* __restrict__ xg, const float* __restrict__ w_hv,
                                              const float* __restrict__ b_hv, const float* __restrict__ w_zv,
                                              const float* __restrict__ b_zv, int E, int H, int atoms, float* hv, float* v_dst) {
    const int tid = threadIdx.x;
    for (int j = tid; j < H; j += DUELING_THREADS) {
        const float* wr = w_hv + (size_t)j * E;
        float s = b_hv[j];
        for (int k = 0; k < E; ++k) s = fmaf(xg[k], wr[k], s);
        hv[j] = streams_relu(s);
    }
    __syncthreads();
    if (tid < atoms) {
        const float* wr = w_zv + (size_t)tid * H;
        float s = b_zv[tid];
        for (int j = 0; j < H; ++j) s = fmaf(hv[j], wr[j], s);
        v_dst[tid] = s;
    }
    __syncthreads();
}

// acc[m] continues its chain over the nj hidden units of the block at jb (FULL: nj == STREAMS_HBLOCK)
template <int AMAX, bool FULL>
__device__ __forceinline__ void streams_consume(const float (&h)[STREAMS_HBLOCK], const float* __restrict__ w_za, int H, int jb, int nj,
                                                int atoms, float (&acc)[AMAX]) {
#pragma unroll
    for (int m = 0; m < AMAX; ++m) {
        if (m < atoms) {
            const float* wz = w_za + (size_t)m * H + jb;
#pragma unroll
            for (int jj = 0; jj < STREAMS_HBLOCK; ++jj)
                if (FULL || jj < nj) acc[m] = fmaf(h[jj], wz[jj], acc[m]);
        }
    }
}

// One row of the advantage stream: xr its E embeddings -> acc[0 .. atoms) the logits (the rest of acc is unspecified).
// vec4: xr is 16-byte aligned and E a multiple of 4 (x and the rows of W_ha are then read four floats at a time).
template <int AMAX>
__device__ __forceinline__ void streams_advantage_row(const float* __restrict__ xr, bool vec4, const float* __restrict__ w_ha,
                                                      const float* __restrict__ b_ha, const float* __restrict__ w_za,
                                                      const float* __restrict__ b_za, int E, int H, int atoms, float (&acc)[AMAX]) {
#pragma unroll
    for (int m = 0; m < AMAX; ++m) acc[m] = m < atoms ? b_za[m] : 0.0f;
    const int e4 = vec4 ? E : 0;
    for (int jb = 0; jb < H; jb += STREAMS_HBLOCK) {
        const int nj = H - jb < STREAMS_HBLOCK ? H - jb : STREAMS_HBLOCK;
        float h[STREAMS_HBLOCK];
        const float* wr[STREAMS_HBLOCK];
#pragma unroll
        for (int jj = 0; jj < STREAMS_HBLOCK; ++jj) {
            const int j = jj < nj ? jb + jj : H - 1;     // past the end: a row that exists, its result unused
            wr[jj] = w_ha + (size_t)j * E;
            h[jj] = b_ha[j];
        }
        for (int k = 0; k < e4; k += 4) {
            const StreamsVec4 xk = *(const StreamsVec4*)(xr + k);
#pragma unroll
            for (int jj = 0; jj < STREAMS_HBLOCK; ++jj) {
                const StreamsVec4 w = *(const StreamsVec4*)(wr[jj] + k);
#pragma unroll
                for (int c = 0; c < 4; ++c) h[jj] = fmaf(xk.f[c], w.f[c], h[jj]);
            }
        }
        for (int k = e4; k < E; ++k) {
            const float xk = xr[k];
#pragma unroll
            for (int jj = 0; jj < STREAMS_HBLOCK; ++jj) h[jj] = fmaf(xk, wr[jj][k], h[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < STREAMS_HBLOCK; ++jj) h[jj] = streams_relu(h[jj]);
        if (nj == STREAMS_HBLOCK)
            streams_consume<AMAX, true>(h, w_za, H, jb, nj, atoms, acc);
        else
            streams_consume<AMAX, false>(h, w_za, H, jb, nj, atoms, acc);
    }
}

// the shape of a launch; x_vec4: every row of x starts on a 16-byte boundary and embed is a multiple of 4
struct StreamsArgs {
    long long xg_stride, env_stride, row_stride, q_stride;
    int embed, hidden, atoms, obs_stride, s_rows, x_vec4;
};

// The a block of one environment stands in the tile (pitch atoms | 1; a barrier has passed since it was written), sh.v and
// sh.z are set: the logits to a_out, then the resident form of dueling_block_argmax on the tile as it stands.  Shared with
// irbpp_streams_mfma.hip.
__device__ __forceinline__ void streams_tile_finish(float* tile, DuelingShared& sh, const float* __restrict__ flags, const StreamsArgs& g,
                                                    int64_t* __restrict__ action, float* __restrict__ q_out, float* __restrict__ a_out) {
    const int tid = threadIdx.x, atoms = g.atoms, s_rows = g.s_rows, pitch = atoms | 1;
    if (a_out) head_walk<DUELING_THREADS>(atoms, s_rows, [&](int row, int k, int e) { a_out[e] = tile[row * pitch + k]; });
    if (!action && !q_out) return;                       // only the logits were wanted
    dueling_mean(tile, pitch, atoms, s_rows, sh.part, sh.mean);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < s_rows; i += DUELING_THREADS) {
        const float s = dueling_row(tile + i * pitch, sh.v, sh.mean, sh.z, atoms);
        if (q_out) q_out[i] = s;
        const float val = head_masked(flags, i, s);
        if (head_better(val, i, best, bi)) { best = val; bi = i; }
    }
    head_wave_argmax(best, bi);
    if ((tid & 63) == 0) {
        sh.best[tid >> 6] = best;
        sh.bi[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0 && action) {
        best = sh.best[0];
        bi = sh.bi[0];
        for (int w = 1; w < DUELING_THREADS / 64; ++w) {
            const float ob = sh.best[w];
            const int oi = sh.bi[w];
            if (head_better(ob, oi, best, bi)) { best = ob; bi = oi; }
        }
        *action = head_index(bi, s_rows);
    }
}

// One workgroup: everything for one environment.  hv: LDS, STREAMS_MAX_WIDTH floats.
template <int AMAX>
__device__ __forceinline__ void streams_act_block(const float* __restrict__ w_hv, const float* __restrict__ b_hv,
                                                  const float* __restrict__ w_zv, const float* __restrict__ b_zv,
                                                  const float* __restrict__ w_ha, const float* __restrict__ b_ha,
                                                  const float* __restrict__ w_za, const float* __restrict__ b_za,
                                                  const float* __restrict__ xg, const float* __restrict__ x,
                                                  const float* __restrict__ z, const float* __restrict__ flags,
                                                  const StreamsArgs& g, int64_t* __restrict__ action, float* __restrict__ q_out,
                                                  float* __restrict__ v_out, float* __restrict__ a_out, float* tile,
                                                  DuelingShared& sh, float* hv) {
    const int tid = threadIdx.x, atoms = g.atoms, s_rows = g.s_rows, pitch = atoms | 1;
    const bool resident = dueling_tile_rows(s_rows, atoms) == s_rows;
    streams_value(xg, w_hv, b_hv, w_zv, b_zv, g.embed, g.hidden, atoms, hv, sh.v);
    if (tid < atoms) {
        if (z) sh.z[tid] = z[tid];
        if (v_out) v_out[tid] = sh.v[tid];
    }
    for (int row = tid; row < s_rows; row += DUELING_THREADS) {
        float acc[AMAX];
        streams_advantage_row<AMAX>(x + (size_t)row * g.row_stride, g.x_vec4 != 0, w_ha, b_ha, w_za, b_za, g.embed, g.hidden,
                                        atoms, acc);
        if (resident) {
            float* dst = tile + row * pitch;
#pragma unroll
            for (int m = 0; m < AMAX; ++m)
                if (m < atoms) dst[m] = acc[m];
        } else if (a_out) {                              // the workspace: finished by irbpp_streams_finish_kernel
            float* dst = a_out + (size_t)row * atoms;
#pragma unroll
            for (int m = 0; m < AMAX; ++m)
                if (m < atoms) dst[m] = acc[m];
        }
    }
    if (!resident) return;
    __syncthreads();
    streams_tile_finish(tile, sh, flags, g, action, q_out, a_out);
}

#define IRBPP_STREAMS_KERNEL(NAME, AMAX)                                                                                           \
    extern "C" __global__ void __launch_bounds__(DUELING_THREADS)                                                                  \
    NAME(const float* __restrict__ w_hv, const float* __restrict__ b_hv, const float* __restrict__ w_zv,                           \
         const float* __restrict__ b_zv, const float* __restrict__ w_ha, const float* __restrict__ b_ha,                           \
         const float* __restrict__ w_za, const float* __restrict__ b_za, const float* __restrict__ xg,                             \
         const float* __restrict__ x, const float* __restrict__ support, const float* __restrict__ obs,                            \
         int64_t* __restrict__ action, float* __restrict__ q_out, float* __restrict__ v_out, float* __restrict__ a_out,            \
         StreamsArgs g) {                                                                                                          \
        HIP_DYNAMIC_SHARED(float, dueling_tile)          /* the tile of irbpp_dueling.hip, by its name */                                  \
        __shared__ DuelingShared sh;                                                                                               \
        __shared__ float hv[STREAMS_MAX_WIDTH];                                                                                    \
        const size_t env = blockIdx.x;                                                                                             \
        streams_act_block<AMAX>(w_hv,     b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za, xg + env * g.xg_stride,                        \
                                    x + env * g.env_stride, support, obs ? obs + env * g.obs_stride : nullptr, g,                  \
                                    action ? action + env : nullptr, q_out ? q_out + env * g.q_stride : nullptr,                   \
                                    v_out ? v_out + env * g.atoms : nullptr,                                                       \
                                    a_out ? a_out + env * g.s_rows * g.atoms : nullptr, dueling_tile, sh, hv);                     \
    }

// DQNBPP.forward's streams, combine + softmax (model.py:393-400) and Agent.act after it (agent.py:51-58), per environment:
// the two instantiations give the same bits (irbpp_streams_act chooses by shape).
IRBPP_STREAMS_KERNEL(irbpp_streams_act_kernel, HEAD_MAX_ATOMS)
IRBPP_STREAMS_KERNEL(irbpp_streams_act_a32_kernel, 32)

// The second launch of a block that did not fit the tile: v once more (the same chains, so the same bits) and
// irbpp_dueling_act_kernel's path over the a block that the first launch left in the workspace.
extern "C" __global__ void __launch_bounds__(DUELING_THREADS)
irbpp_streams_finish_kernel(const float* __restrict__ w_hv, const float* __restrict__ b_hv, const float* __restrict__ w_zv,
                            const float* __restrict__ b_zv, const float* __restrict__ xg, const float* __restrict__ a,
                            const float* __restrict__ support, const float* __restrict__ obs, int64_t* __restrict__ action,
                            float* __restrict__ q_out, StreamsArgs g) {
    HIP_DYNAMIC_SHARED(float, dueling_tile)
    __shared__ DuelingShared sh;
    __shared__ float hv[STREAMS_MAX_WIDTH];
    __shared__ float sv[HEAD_MAX_ATOMS];
    const size_t env = blockIdx.x;
    streams_value(xg + env * g.xg_stride, w_hv, b_hv, w_zv, b_zv, g.embed, g.hidden, g.atoms, hv, sv);
    const int bi = dueling_block_argmax(sv, a + env * g.s_rows * g.atoms, g.atoms, support, g.atoms, g.s_rows,
                                        obs ? obs + env * g.obs_stride : nullptr, q_out ? q_out + env * g.q_stride : nullptr, nullptr,
                                        dueling_tile, sh);
    if (threadIdx.x == 0 && action) action[env] = bi;
}

}  // namespace irbpp
