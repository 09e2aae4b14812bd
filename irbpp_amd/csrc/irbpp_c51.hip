// irbpp_c51.hip -- the Rainbow head around the network: the distributional greedy action of Agent.act
// (agent.py:51-58) and the double-Q selection + categorical projection of Agent.learn (agent.py:88-115), one launch each
// instead of a string of torch kernels over the [N][S][atoms] probabilities.
//
// Defined arithmetic (what makes both kernels testable bit for bit): a row's expected value is the float32 sum, left to
// right over a = 0 .. atoms-1, of fl32(p[a] * z[a]) -- multiply and add separate (the library is built with
// -ffp-contract=off), z the caller's own torch.linspace support.  Only the loading is free: a wave stages 64 rows at a
// time through LDS with coalesced dword loads (consecutive lanes, consecutive addresses of the row-major block) and
// then sums lane-per-row from LDS; rows lie `atoms | 1` floats apart there, an odd pitch, so the 32 lanes of a
// ds_read_b32 group fall on 32 different banks.  p is read exactly once.  The arg-max rule and the categorical projection
// are those of irbpp_head.h.
#include "irbpp_head.h"

namespace irbpp {

// One wave (a 64-thread workgroup): arg-max over the s_rows rows of one [S][atoms] block of the defined expected value;
// the first maximum wins, and with every row at -inf index 0 does (head_better, head_index).  flags (may be NULL) is the
// env's observation row (head_masked).  q_out (may be NULL) receives the unmasked values.  tile: 64 * (atoms | 1) floats
// of LDS.  Every lane returns the index.
__device__ __forceinline__ int c51_wave_argmax(const float* __restrict__ p, long long row_stride, const float* __restrict__ z,
                                               int atoms, int s_rows, const float* __restrict__ flags,
                                               float* __restrict__ q_out, float* tile) {
    const int lane = threadIdx.x;
    const int pitch = atoms | 1;
    // head_walk<64>'s steps, kept in the form these two kernels were measured in: fixed trip count, unrolled, the guard inside
    const int q64 = 64 / atoms, r64 = 64 - q64 * atoms;
    const int row0 = lane / atoms, a0 = lane - row0 * atoms;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int r0 = 0; r0 < s_rows; r0 += 64) {
        const int nrows = s_rows - r0 < 64 ? s_rows - r0 : 64;
        const float* src = p + (size_t)r0 * row_stride;
        int row = row0, a = a0;
#pragma unroll 8
        for (int t = 0; t < atoms; ++t) {
            if (row < nrows) tile[row * pitch + a] = src[(size_t)row * row_stride + a];
            row += q64;
            a += r64;
            if (a >= atoms) { a -= atoms; ++row; }
        }
        __syncthreads();
        if (lane < nrows) {
            const int i = r0 + lane;
            const float* rw = tile + lane * pitch;
            float s = rw[0] * z[0];
            for (int k = 1; k < atoms; ++k) s = s + rw[k] * z[k];
            if (q_out) q_out[i] = s;
            const float v = head_masked(flags, i, s);
            if (head_better(v, i, best, bi)) { best = v; bi = i; }
        }
        __syncthreads();                                 // the tile is rewritten by the next trip
    }
    head_wave_argmax(best, bi);
    return head_index(bi, s_rows);
}

// Agent.act (agent.py:51-58) after the network: (q_map * support).sum(2), sum_q_map[(1 - mask).bool()] = -inf, argmax(1),
// the mask read from the observation as in irbpp_masked_argmax_kernel (obs == NULL: orderDQN.act(state, None),
// trainer.py:266).  One wave per env.
extern "C" __global__ void __launch_bounds__(64)
irbpp_c51_act_kernel(const float* __restrict__ p, long long env_stride, long long row_stride, const float* __restrict__ support,
                     int atoms, const float* __restrict__ obs, int obs_stride, int s_rows, int64_t* __restrict__ action,
                     float* __restrict__ q_out, long long q_stride) {
    HIP_DYNAMIC_SHARED(float, c51_tile)                 // 64 * (atoms | 1) floats
    const int env = blockIdx.x;
    const int bi = c51_wave_argmax(p + (size_t)env * env_stride, row_stride, support, atoms, s_rows,
                                   obs ? obs + (size_t)env * obs_stride : nullptr,
                                   q_out ? q_out + (size_t)env * q_stride : nullptr, c51_tile);
    if (threadIdx.x == 0) action[env] = bi;
}

// Agent.learn (agent.py:88-115) after the two network calls, one wave per sample: a* = argmax of the (unmasked, :92)
// expected value of p_online, pns_a = p_target[b][a*], and head_project's projection of it onto the support.
extern "C" __global__ void __launch_bounds__(64)
irbpp_c51_target_kernel(const float* __restrict__ p_online, long long on_env_stride, long long on_row_stride,
                        const float* __restrict__ p_target, long long tg_env_stride, long long tg_row_stride,
                        const float* __restrict__ returns, const float* __restrict__ nonterminals,
                        const float* __restrict__ support, int atoms, int s_rows, float gamma_n, float v_min, float v_max,
                        float delta_z, float* __restrict__ m, int64_t* __restrict__ a_star) {
    HIP_DYNAMIC_SHARED(float, c51_tile)                 // 64 * (atoms | 1) floats
    __shared__ HeadProjection proj;
    const int smp = blockIdx.x, lane = threadIdx.x;
    const int best = c51_wave_argmax(p_online + (size_t)smp * on_env_stride, on_row_stride, support, atoms, s_rows, nullptr,
                                     nullptr, c51_tile);
    if (lane == 0) a_star[smp] = best;
    const float* pa = p_target + (size_t)smp * tg_env_stride + (size_t)best * tg_row_stride;
    head_project<64>(pa, support, returns[smp], nonterminals[smp] * gamma_n, v_min, v_max, delta_z, atoms, m + (size_t)smp * atoms,
                     proj);
}

}  // namespace irbpp
