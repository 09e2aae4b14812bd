// irbpp_streams_mfma.hip -- irbpp_streams.hip's launch with the advantage stream on the matrix cores: the same definition
// (the header of irbpp_streams.hip), the same outputs, the same bits.  Included after irbpp_streams.hip, whose value stream,
// argument block, tile finish and second launch (irbpp_streams_finish_kernel) it uses as they are.
//
// The advantage stream is two products of irbpp_mfma_chain.h per tile of 32 rows of x, one wave per tile (tiles dealt round
// robin to the 8 waves of the environment's workgroup):
//   hT[j][r] : C = b_ha[j], A = W_ha (32 hidden units), B = xT, over k = 0 .. E-1 ascending; relu in registers
//   aT[m][r] : C = b_za[m], A = W_za (32 atoms),        B = hT, over j = 0 .. H-1 ascending across all blocks of 32 hidden units
// hT's column (the row of x) sits on the lane and its rows (hidden units) in registers, four at a time per lane half, so the
// hand-over to the second product exchanges every second operand with lane ^ 32 (mfma_acc_as_b): the order j = 0, 1, 2, ...
// is the definition's.  E and H are multiples of 4 and never padded; rows of x past S, hidden units past H inside the first
// product and atoms past `atoms` are computed from rows that exist and thrown away.  NB blocks of 32 atoms share one hT.
// The weights and x are read from memory (L1 / L2) four floats per lane at a time: a lane's A operand of a k-step is one
// element of its own weight row, so a 16-byte load feeds two instructions; DESIGN.md, "The noisy streams on the matrix
// cores", records what that costs and what was not tried.
#include "irbpp_mfma_chain.h"

namespace irbpp {

// StreamsArgs::x_vec4 as this file reads it: which operands may be loaded 16 bytes at a time
constexpr int STREAMS_MFMA_X16 = 1, STREAMS_MFMA_WHA16 = 2, STREAMS_MFMA_WZA16 = 4;

// 32 rows of x from row0 on: acc[nb] = aT[32 nb + i][row0 + col], nb < nblk
template <int NB>
__device__ __forceinline__ void streams_mfma_tile(const float* __restrict__ x, const float* __restrict__ w_ha,
                                                  const float* __restrict__ b_ha, const float* __restrict__ w_za,
                                                  const float* __restrict__ b_za, const StreamsArgs& g, int row0, int nblk,
                                                  MfmaAcc (&acc)[NB]) {
    const int lane = mfma_lane(), col = mfma_col(lane), half = mfma_half(lane);
    const int E = g.embed, H = g.hidden, atoms = g.atoms;
    const bool x16 = g.x_vec4 & STREAMS_MFMA_X16, wha16 = g.x_vec4 & STREAMS_MFMA_WHA16, wza16 = g.x_vec4 & STREAMS_MFMA_WZA16;
    const int row = row0 + col < g.s_rows ? row0 + col : g.s_rows - 1;
    const float* xr = x + (size_t)row * g.row_stride;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
        if (nb < nblk) mfma_chain_bias(acc[nb], b_za, nb * MFMA_TILE, atoms, half);
    for (int jb = 0; jb < H; jb += MFMA_TILE) {
        const int nj = H - jb < MFMA_TILE ? H - jb : MFMA_TILE;
        MfmaAcc h;
        mfma_chain_bias(h, b_ha, jb, H, half);
        const float* wr = w_ha + (size_t)(jb + col < H ? jb + col : H - 1) * E;
#pragma unroll 4
        for (int k = 0; k < E; k += 4) mfma_chain_k4(h, mfma_load4(wr + k, wha16), mfma_load4(xr + k, x16), half);
#pragma unroll
        for (int r = 0; r < MFMA_ACC; ++r) h.r[r] = streams_relu(h.r[r]);
        float hb[MFMA_ACC];
        mfma_acc_as_b(h, half, hb);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            if (nb < nblk) {
                const int m = nb * MFMA_TILE + col;
                mfma_chain_acc(acc[nb], w_za + (size_t)(m < atoms ? m : atoms - 1) * H + jb, wza16, hb, nj, half);
            }
        }
    }
}

// One workgroup: everything for one environment, as streams_act_block.
template <int NB>
__device__ __forceinline__ void streams_mfma_block(const float* __restrict__ w_hv, const float* __restrict__ b_hv,
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
    const int lane = mfma_lane(), col = mfma_col(lane), half = mfma_half(lane);
    const int nblk = (atoms + MFMA_TILE - 1) / MFMA_TILE;
    for (int row0 = (tid >> 6) * MFMA_TILE; row0 < s_rows; row0 += DUELING_THREADS / 64 * MFMA_TILE) {     // wave-uniform
        MfmaAcc acc[NB];
        streams_mfma_tile<NB>(x, w_ha, b_ha, w_za, b_za, g, row0, nblk, acc);
        const int row = row0 + col;
        if (row >= s_rows || (!resident && !a_out)) continue;
        float* dst = resident ? tile + row * pitch : a_out + (size_t)row * atoms;   // the workspace: irbpp_streams_finish_kernel
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
            for (int r = 0; r < MFMA_ACC; ++r) {
                const int m = nb * MFMA_TILE + mfma_acc_row(r, half);
                if (m < atoms) dst[m] = acc[nb].r[r];
            }
        }
    }
    if (!resident) return;
    __syncthreads();
    streams_tile_finish(tile, sh, flags, g, action, q_out, a_out);
}

#define IRBPP_STREAMS_MFMA_KERNEL(NAME, NB)                                                                                        \
    extern "C" __global__ void __launch_bounds__(DUELING_THREADS)                                                                  \
    NAME(const float* __restrict__ w_hv, const float* __restrict__ b_hv, const float* __restrict__ w_zv,                           \
         const float* __restrict__ b_zv, const float* __restrict__ w_ha, const float* __restrict__ b_ha,                           \
         const float* __restrict__ w_za, const float* __restrict__ b_za, const float* __restrict__ xg,                             \
         const float* __restrict__ x, const float* __restrict__ support, const float* __restrict__ obs,                            \
         int64_t* __restrict__ action, float* __restrict__ q_out, float* __restrict__ v_out, float* __restrict__ a_out,            \
         StreamsArgs g) {                                                                                                          \
        HIP_DYNAMIC_SHARED(float, dueling_tile)                                                                                    \
        __shared__ DuelingShared sh;                                                                                               \
        __shared__ float hv[STREAMS_MAX_WIDTH];                                                                                    \
        const size_t env = blockIdx.x;                                                                                             \
        streams_mfma_block<NB>(w_hv, b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za, xg + env * g.xg_stride, x + env * g.env_stride,     \
                               support, obs ? obs + env * g.obs_stride : nullptr, g, action ? action + env : nullptr,              \
                               q_out ? q_out + env * g.q_stride : nullptr, v_out ? v_out + env * g.atoms : nullptr,                \
                               a_out ? a_out + env * g.s_rows * g.atoms : nullptr, dueling_tile, sh, hv);                          \
    }

// the two instantiations give the same bits (irbpp_streams_act_mfma chooses by atoms): up to 128 atoms, and up to 32
IRBPP_STREAMS_MFMA_KERNEL(irbpp_streams_act_mfma_kernel, HEAD_MAX_ATOMS / MFMA_TILE)
IRBPP_STREAMS_MFMA_KERNEL(irbpp_streams_act_mfma_a32_kernel, 1)

}  // namespace irbpp
