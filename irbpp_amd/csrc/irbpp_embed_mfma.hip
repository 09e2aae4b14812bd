// irbpp_embed_mfma.hip -- irbpp_embed.hip's row launch with its three per-row layers on the matrix cores: the same definition
// (the header of irbpp_embed.hip), the same outputs, the same bits.  Included after irbpp_embed.hip, whose bin kernel (CNN and
// `base`), argument block and LDS regions it uses as they are.  e1, the running parts of the mean, the transposed stores and xg
// are irbpp_embed_rows_kernel's lines repeated: as functions shared by the two kernels they changed that kernel's compiled code
// (9535 -> 9608 instructions), and it is held to stay what it was.
//
// e2, h and x of a tile of 64 rows are each one product of irbpp_mfma_chain.h per (block of 32 output features, half of 32
// rows), the pairs dealt round robin to the 8 waves of the bin's workgroup:
//   e2T[j][r] : C = b_c2[j],    A = W_c2 (32 features),                      B = e1T, over k = 0 .. Hc-1 ascending
//   hT[j][r]  : C = base[n][j], A = W_p1[j][F+M ..) (32 features, ld F+M+Ec), B = e2T, over k = 0 .. Ec-1; leaky in registers
//   xT[j][r]  : C = b_p2[j],    A = W_p2 (32 features),                      B = hT,  over k = 0 .. P-1; the mask in registers
// A layer's input lies in LDS as [k][64 rows], as in irbpp_embed_rows_kernel, so a lane's B operand of a k-step is one dword
// at (k0 + half) * 64 + 32 * rowhalf + col (conflict-free), and its A operand one element of its own weight row, four
// consecutive floats per 16-byte load where the row is aligned.  The accumulators go back to the LDS region of the next layer,
// register g to feature f0 + mfma_acc_row(g, half): the hand-over is through LDS, one MfmaAcc at a time.  Hc, Ec and P are
// multiples of 4 and never padded; features past a layer's width and rows past S are computed from ones that exist and thrown
// away.  DESIGN.md, "The embedding stage on the matrix cores", records the figures and what was not tried.
#include "irbpp_mfma_chain.h"

// NaNs are part of this definition (an invalid row may hold any candidate), whatever the build's command line says
#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

// what becomes of a layer's accumulators on their way to LDS
constexpr int EMBED_MFMA_PLAIN = 0, EMBED_MFMA_LEAKY = 1, EMBED_MFMA_MASKED = 2;

// One layer of the tile: out[f * pitch + row] = the chain from start[f] over in[k * 64 + row] against w[f * ld + k], k < K
// ascending, f < width, row < 64; valid0 / valid1: the masks of the lane's rows col and 32 + col (EMBED_MFMA_MASKED)
template <int MODE>
__device__ __forceinline__ void embed_mfma_layer(const float* in, int K, const float* __restrict__ w, int ld,
                                                 const float* __restrict__ start, int width, float* out, int pitch, int wave,
                                                 float slope, bool valid0, bool valid1) {
    const int lane = mfma_lane(), col = mfma_col(lane), half = mfma_half(lane);
    const bool w16 = (uintptr_t)w % 16 == 0 && ld % 4 == 0;
    const int pairs = 2 * ((width + MFMA_TILE - 1) / MFMA_TILE);
    for (int p = wave; p < pairs; p += EMBED_ROW_WAVES) {                           // wave-uniform
        const int f0 = (p >> 1) * MFMA_TILE, row = (p & 1) * MFMA_TILE + col;
        MfmaAcc c;
        mfma_chain_bias(c, start, f0, width, half);
        const float* wr = w + (size_t)(f0 + col < width ? f0 + col : width - 1) * ld;
        const float* b = in + half * EMBED_TILE_ROWS + row;
#pragma unroll 4
        for (int k = 0; k < K; k += 4) {
            const MfmaVec4 a4 = mfma_load4(wr + k, w16);
            mfma_32x32x2(half ? a4.f[1] : a4.f[0], b[k * EMBED_TILE_ROWS], c);
            mfma_32x32x2(half ? a4.f[3] : a4.f[2], b[(k + 2) * EMBED_TILE_ROWS], c);
        }
        const bool valid = (p & 1) ? valid1 : valid0;
#pragma unroll
        for (int r = 0; r < MFMA_ACC; ++r) {
            const int f = f0 + mfma_acc_row(r, half);
            float v = c.r[r];
            if (MODE == EMBED_MFMA_LEAKY) v = front_leaky(v, slope);
            if (MODE == EMBED_MFMA_MASKED) v = valid ? v : 0.0f;
            if (f < width) out[f * pitch + row] = v;
        }
    }
}

// Workgroup n: x[n][0 .. S)[0 .. E) and xg[n][0 .. E) from the observation row and base[n], as irbpp_embed_rows_kernel
extern "C" __global__ void __launch_bounds__(EMBED_ROW_THREADS)
irbpp_embed_rows_mfma_kernel(const float* __restrict__ w_c1, const float* __restrict__ b_c1, const float* __restrict__ w_c2,
                             const float* __restrict__ b_c2, const float* __restrict__ w_p1, const float* __restrict__ w_p2,
                             const float* __restrict__ b_p2, const float* __restrict__ obs, const float* __restrict__ base,
                             float* __restrict__ x, float* __restrict__ xg, EmbedArgs g) {
    HIP_DYNAMIC_SHARED(float, embed_tile)
    const int tid = threadIdx.x, lane = tid & 63, wave = front_wave_uniform(tid >> 6);
    const size_t n = blockIdx.x;
    const int S = g.s_rows, Hc = g.cand_hidden, Ec = g.cand_embed, P = g.proj_hidden, E = g.embed;
    const int ld1 = g.feat + g.c3 * (g.map_len / 4) * (g.map_len / 4) + Ec;
    float* ra = embed_tile;                              // e2 [Ec][64], then the x tile [E][65]
    float* rb = ra + embed_region_a(Ec, E);              // e1 [Hc][64], then h [P][64]
    float* part = rb + embed_region_b(Hc, P);            // [16][E]
    const float* row_obs = obs + n * g.obs_stride;
    const float* base_n = base + n * P;
    const float* w_p1c = w_p1 + (ld1 - Ec);              // the candidate columns of W_p1
    float* x_n = x + n * g.env_stride;
    for (int j = tid; j < DUELING_PARTS * E; j += EMBED_ROW_THREADS) part[j] = 0.0f;
    for (int r0 = 0; r0 < S; r0 += EMBED_TILE_ROWS) {
        const int r = r0 + lane < S ? r0 + lane : S - 1;
        const float* cand = row_obs + 5 * r;
        const float c0 = cand[0], c1 = cand[1], c2 = cand[2], c3 = cand[3];
        // the products' lane holds rows col and 32 + col of the tile: their masks
        const int m0 = r0 + (lane & 31) < S ? r0 + (lane & 31) : S - 1, m1 = m0 + 32 < S ? m0 + 32 : S - 1;
        const bool valid0 = row_obs[5 * m0 + 4] == 1.0f, valid1 = row_obs[5 * m1 + 4] == 1.0f;
        __syncthreads();                                 // the tile before: h and the x tile have been read
        for (int i = wave; i < Hc; i += EMBED_ROW_WAVES) {   // e1, lane = row: K = 4 stays on the vector unit
            const float* wr = w_c1 + (size_t)i * 4;
            rb[i * EMBED_TILE_ROWS + lane] = front_leaky(fmaf(c3, wr[3], fmaf(c2, wr[2], fmaf(c1, wr[1], fmaf(c0, wr[0], b_c1[i])))), g.slope);
        }
        __syncthreads();
        embed_mfma_layer<EMBED_MFMA_PLAIN>(rb, Hc, w_c2, Hc, b_c2, Ec, ra, EMBED_TILE_ROWS, wave, g.slope, valid0, valid1);
        __syncthreads();                                 // e2 is whole, e1 has been read
        embed_mfma_layer<EMBED_MFMA_LEAKY>(ra, Ec, w_p1c, ld1, base_n, P, rb, EMBED_TILE_ROWS, wave, g.slope, valid0, valid1);
        __syncthreads();                                 // h is whole, e2 has been read
        embed_mfma_layer<EMBED_MFMA_MASKED>(rb, P, w_p2, P, b_p2, E, ra, EMBED_X_PITCH, wave, g.slope, valid0, valid1);
        __syncthreads();                                 // the x tile is whole
        const int rows = S - r0 < EMBED_TILE_ROWS ? S - r0 : EMBED_TILE_ROWS;
        // the mean's parts: thread j owns (g, e) for every tile, so the rows reach part g in ascending order
        for (int j = tid; j < DUELING_PARTS * E; j += EMBED_ROW_THREADS) {
            const int e = j / DUELING_PARTS, gp = j - e * DUELING_PARTS;
            float s = part[gp * E + e];
            for (int i = gp; i < rows; i += DUELING_PARTS) s = s + ra[e * EMBED_X_PITCH + i];
            part[gp * E + e] = s;
        }
        for (int i = wave; i < rows; i += EMBED_ROW_WAVES) {
            float* dst = x_n + (size_t)(r0 + i) * g.row_stride;
            for (int e = lane; e < E; e += 64) dst[e] = ra[e * EMBED_X_PITCH + i];
        }
    }
    __syncthreads();
    if (tid < E) {
        float s = part[tid];
        for (int gp = 1; gp < DUELING_PARTS; ++gp) s = s + part[gp * E + tid];
        xg[n * g.xg_stride + tid] = s / (float)S;
    }
}

}  // namespace irbpp

#pragma float_control(pop)
