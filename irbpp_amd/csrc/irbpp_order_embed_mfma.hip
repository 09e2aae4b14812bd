// irbpp_order_embed_mfma.hip -- irbpp_order_embed.hip's row launch with its eight linear layers on the matrix cores: the same
// definition (the header of irbpp_order_embed.hip), the same outputs, the same bits.  Included after irbpp_order_embed.hip,
// whose bin kernel (CNN and `base`), argument block, tiles of 64 / k whole bins and LDS regions it uses as they are.  The shape
// feature load, the compatibility chains, the softmax, hd, the transposed stores and xg are irbpp_order_rows_kernel's lines
// repeated, not shared: that kernel is held to stay what it was compiled to.
//
// g, h0, Q, K, V, W_out and the feed-forward pair of a tile of 64 rows are each one product of irbpp_mfma_chain.h per (block of
// 32 output features, half of 32 rows), pair p of a layer going to wave p % 8 in that wave's pass p / 8 (a layer of 256 features
// has 16 pairs: two passes):
//   gT[j][r]  : C = base[bin of r][j], A = W_g1[j][0 .. F) (ld F + M), B = shape features, over c = 0 .. F-1; leaky in registers
//   h0T       : C = b_g2,  A = W_g2, B = gT  over P;    kept in registers
//   QT, KT, VT: C = +0.0,  A = W_q, W_k, W_v, B = h0T over E  (Q and K ORDER_QK_BLOCK features at a time, as in the chain form)
//   h1T       : C = b_o,   A = W_o,  B = hdT over E;    h1 = h0 + C in registers, kept
//   ffT       : C = b_f1,  A = W_f1, B = h1T over E;    relu in registers
//   xT        : C = b_f2,  A = W_f2, B = ffT over Hf;   x = h1 + C in registers
// h0, W_out and ff2 are all E wide, so the same wave takes the same pairs in the same passes and the residuals' first terms
// never leave its registers; a residual is added after its chain, never into the chain's start.  A layer's input lies in LDS as
// [c][64 rows], so a lane's B operand of a k-step is one dword at (c0 + half) * 64 + 32 * rowhalf + col, and its A operand one
// element of its own weight row, four consecutive floats per 16-byte load where the row is aligned.  A lane past the tile's
// last row holds that row once more in every LDS column it owns (the shape features are loaded so, and `base` is taken from
// that row's bin), so the products' columns past the last row recompute it and are dropped at the end, as in the chain form.
// F, P, E and Hf are multiples of 4 and never padded; features past a layer's width take the last weight row and start that
// exist and are thrown away.  DESIGN.md, "The order network on the matrix cores", records the figures and what was not tried.
#include "irbpp_mfma_chain.h"

#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

// passes of a layer: pairs of the widest layer over the waves
constexpr int ORDER_MFMA_PASSES = 2 * (ORDER_MAX_WIDTH / MFMA_TILE) / EMBED_ROW_WAVES;
// what a chain starts from, what becomes of a layer's accumulators on their way to LDS, and the residual's part
constexpr int ORDER_MFMA_FROM_START = 0, ORDER_MFMA_FROM_ZERO = 1;
constexpr int ORDER_MFMA_PLAIN = 0, ORDER_MFMA_LEAKY = 1, ORDER_MFMA_RELU = 2;
constexpr int ORDER_MFMA_NO_RES = 0, ORDER_MFMA_KEEP = 1, ORDER_MFMA_ADD_KEEP = 2, ORDER_MFMA_ADD = 3;

// floats of dynamic LDS of the rows kernel of this form: the regions are the chain form's, and the residuals stay in registers
constexpr int order_rows_mfma_lds_floats(int feat, int proj_hidden, int embed, int ff_hidden, int k_slots) {
    return order_rows_lds_floats(feat, proj_hidden, embed, ff_hidden, k_slots);
}

// One layer of the tile: out[f * pitch + row] = act(the chain from its start over in[c * 64 + row] against w[f * ld + c]), c < K
// ascending, f < width, row < 64.  The start of feature f in the lane's column: start0[f] (rows 0 .. 31) or start1[f] (rows
// 32 .. 63), or +0.0.  res: the residual's first term per pass, by ORDER_MFMA_KEEP (res = v), _ADD_KEEP (v = res = res + v) or
// _ADD (v = res + v)
template <int FROM, int ACT, int RES>
__device__ __forceinline__ void order_mfma_layer(const float* in, int K, const float* __restrict__ w, int ld, const float* start0,
                                                 const float* start1, int width, float* out, int pitch, int wave, float slope,
                                                 MfmaAcc (&res)[ORDER_MFMA_PASSES]) {
    const int lane = mfma_lane(), col = mfma_col(lane), half = mfma_half(lane);
    const bool w16 = (uintptr_t)w % 16 == 0 && ld % 4 == 0;
    const int pairs = 2 * ((width + MFMA_TILE - 1) / MFMA_TILE);
#pragma unroll
    for (int t = 0; t < ORDER_MFMA_PASSES; ++t) {
        const int p = wave + t * EMBED_ROW_WAVES;                                   // wave-uniform
        if (p < pairs) {
            const int f0 = (p >> 1) * MFMA_TILE, row = (p & 1) * MFMA_TILE + col;
            MfmaAcc c;
            if (FROM == ORDER_MFMA_FROM_ZERO)
                mfma_chain_zero(c);
            else
                mfma_chain_col_start(c, (p & 1) ? start1 : start0, f0, width, half);
            const float* wr = w + (size_t)(f0 + col < width ? f0 + col : width - 1) * ld;
            const float* b = in + half * EMBED_TILE_ROWS + row;
#pragma unroll 4
            for (int k = 0; k < K; k += 4) {
                const MfmaVec4 a4 = mfma_load4(wr + k, w16);
                // the lane's own two of the four B rows, in both places of its half: mfma_chain_k4 picks by half
                const float b0 = b[k * EMBED_TILE_ROWS], b2 = b[(k + 2) * EMBED_TILE_ROWS];
                const MfmaVec4 b4 = {{b0, b0, b2, b2}};
                mfma_chain_k4(c, a4, b4, half);
            }
#pragma unroll
            for (int r = 0; r < MFMA_ACC; ++r) {
                const int f = f0 + mfma_acc_row(r, half);
                float v = c.r[r];
                if (ACT == ORDER_MFMA_LEAKY) v = front_leaky(v, slope);
                if (ACT == ORDER_MFMA_RELU) v = order_relu(v);
                if (RES == ORDER_MFMA_KEEP) res[t].r[r] = v;
                if (RES == ORDER_MFMA_ADD_KEEP) v = res[t].r[r] = res[t].r[r] + v;
                if (RES == ORDER_MFMA_ADD) v = res[t].r[r] + v;
                if (f < width) out[f * pitch + row] = v;
            }
        }
    }
}

// Workgroup t: the bins [t * (64 / k), ..) of the tile: x[n][0 .. k)[0 .. E) and xg[n][0 .. E) from shape_feat and base, as
// irbpp_order_rows_kernel
extern "C" __global__ void __launch_bounds__(EMBED_ROW_THREADS)
irbpp_order_rows_mfma_kernel(const float* __restrict__ w_g1, const float* __restrict__ w_g2, const float* __restrict__ b_g2,
                             const float* __restrict__ w_q, const float* __restrict__ w_k, const float* __restrict__ w_v,
                             const float* __restrict__ w_o, const float* __restrict__ b_o, const float* __restrict__ w_f1,
                             const float* __restrict__ b_f1, const float* __restrict__ w_f2, const float* __restrict__ b_f2,
                             const float* __restrict__ shape_feat, const float* __restrict__ base, float* __restrict__ x,
                             float* __restrict__ xg, OrderEmbedArgs g) {
    HIP_DYNAMIC_SHARED(float, order_tile)
    const int tid = threadIdx.x, lane = tid & 63, wave = front_wave_uniform(tid >> 6);
    const int k = g.k_slots, F = g.feat, P = g.proj_hidden, E = g.embed, Hf = g.ff_hidden;
    const int ld1 = F + g.c3 * (g.map_len / 4) * (g.map_len / 4);
    const int per_tile = order_tile_bins(k);
    const size_t bin0 = (size_t)blockIdx.x * per_tile;
    const int bins = (size_t)g.n_env - bin0 < (size_t)per_tile ? (int)((size_t)g.n_env - bin0) : per_tile;
    const int live = bins * k;                            // rows of the tile: 1 .. 64
    const int r = lane < live ? lane : live - 1;         // past the last row: that row once more, dropped at the end
    const int bin = r / k, key0 = bin * k;               // the lane's bin in the tile and the tile row of its slot 0
    float* ra = order_tile;                              // A
    float* rb = ra + order_region_a(F, E, Hf);           // B
    float* cb = rb + order_region_b(P, E);               // compatibilities, then attention weights [k][64]
    MfmaAcc res[ORDER_MFMA_PASSES];                      // h0, then h1: the residuals' first terms
    {
        const float* sf = shape_feat + (bin0 * k + r) * g.feat_stride;
        for (int c = wave; c < F; c += EMBED_ROW_WAVES) ra[c * EMBED_TILE_ROWS + lane] = sf[c];
    }
    __syncthreads();
    {
        // the products' lane holds rows col and 32 + col of the tile: the `base` of their bins
        const int c0 = lane & 31, r0 = c0 < live ? c0 : live - 1, r1 = c0 + 32 < live ? c0 + 32 : live - 1;
        order_mfma_layer<ORDER_MFMA_FROM_START, ORDER_MFMA_LEAKY, ORDER_MFMA_NO_RES>(
            ra, F, w_g1, ld1, base + (bin0 + r0 / k) * P, base + (bin0 + r1 / k) * P, P, rb, EMBED_TILE_ROWS, wave, g.slope, res);
    }
    __syncthreads();                                     // g is whole, the shape features have been read
    order_mfma_layer<ORDER_MFMA_FROM_START, ORDER_MFMA_PLAIN, ORDER_MFMA_KEEP>(rb, P, w_g2, P, b_g2, b_g2, E, ra, EMBED_TILE_ROWS, wave,
                                                                                g.slope, res);
    __syncthreads();                                     // h0 is whole, g has been read
    {
        float* qb = rb;
        float* kb = rb + order_qk_rows(E) * EMBED_TILE_ROWS;
        float cacc[ORDER_PAIRS];
#pragma unroll
        for (int t = 0; t < ORDER_PAIRS; ++t) cacc[t] = 0.0f;
        for (int d0 = 0; d0 < E; d0 += ORDER_QK_BLOCK) {
            const int nd = E - d0 < ORDER_QK_BLOCK ? E - d0 : ORDER_QK_BLOCK;
            order_mfma_layer<ORDER_MFMA_FROM_ZERO, ORDER_MFMA_PLAIN, ORDER_MFMA_NO_RES>(ra, E, w_q + (size_t)d0 * E, E, nullptr, nullptr, nd, qb,
                                                                                        EMBED_TILE_ROWS, wave, g.slope, res);
            order_mfma_layer<ORDER_MFMA_FROM_ZERO, ORDER_MFMA_PLAIN, ORDER_MFMA_NO_RES>(ra, E, w_k + (size_t)d0 * E, E, nullptr, nullptr, nd, kb,
                                                                                        EMBED_TILE_ROWS, wave, g.slope, res);
            __syncthreads();                             // this block of Q and K is whole
#pragma unroll
            for (int t = 0; t < ORDER_PAIRS; ++t) {
                const int j = wave + t * EMBED_ROW_WAVES;
                if (j < k) {
                    float a = cacc[t];
                    for (int d = 0; d < nd; ++d) a = fmaf(qb[d * EMBED_TILE_ROWS + lane], kb[d * EMBED_TILE_ROWS + key0 + j], a);
                    cacc[t] = a;
                }
            }
            __syncthreads();                             // and has been read
        }
#pragma unroll
        for (int t = 0; t < ORDER_PAIRS; ++t) {
            const int j = wave + t * EMBED_ROW_WAVES;
            if (j < k) cb[j * EMBED_TILE_ROWS + lane] = g.norm * cacc[t];
        }
    }
    order_mfma_layer<ORDER_MFMA_FROM_ZERO, ORDER_MFMA_PLAIN, ORDER_MFMA_NO_RES>(ra, E, w_v, E, nullptr, nullptr, E, rb, EMBED_TILE_ROWS, wave,
                                                                                g.slope, res);
    __syncthreads();                                     // V and the compatibilities are whole, h0 has been read
    if (wave == 0) {
        float mx = cb[lane];
        for (int j = 1; j < k; ++j) {
            const float v = cb[j * EMBED_TILE_ROWS + lane];
            mx = v > mx ? v : mx;
        }
        float den = 0.0f;
        for (int j = 0; j < k; ++j) {
            const float e = dueling_dexp(cb[j * EMBED_TILE_ROWS + lane] - mx);
            cb[j * EMBED_TILE_ROWS + lane] = e;
            den = den + e;
        }
        for (int j = 0; j < k; ++j) cb[j * EMBED_TILE_ROWS + lane] = cb[j * EMBED_TILE_ROWS + lane] / den;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < ORDER_PASSES; ++p) {                 // hd on the vector unit, lane = row: block-diagonal per bin
        const int f0 = p * ORDER_QK_BLOCK + wave * EMBED_FBLOCK, nf = order_block_count(E, f0);
        if (nf > 0) {
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = 0.0f;
            for (int j = 0; j < k; ++j) {
                const float a = cb[j * EMBED_TILE_ROWS + lane];
#pragma unroll
                for (int m = 0; m < EMBED_FBLOCK; ++m)   // past the wave's last feature: that feature once more, unused
                    acc[m] = fmaf(a, rb[(f0 + (m < nf ? m : nf - 1)) * EMBED_TILE_ROWS + key0 + j], acc[m]);
            }
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m)
                if (m < nf) ra[(f0 + m) * EMBED_TILE_ROWS + lane] = acc[m];
        }
    }
    __syncthreads();                                     // hd is whole, V has been read
    order_mfma_layer<ORDER_MFMA_FROM_START, ORDER_MFMA_PLAIN, ORDER_MFMA_ADD_KEEP>(ra, E, w_o, E, b_o, b_o, E, rb, EMBED_TILE_ROWS, wave,
                                                                                    g.slope, res);
    __syncthreads();                                     // h1 is whole, hd has been read
    order_mfma_layer<ORDER_MFMA_FROM_START, ORDER_MFMA_RELU, ORDER_MFMA_NO_RES>(rb, E, w_f1, E, b_f1, b_f1, Hf, ra, EMBED_TILE_ROWS, wave,
                                                                                 g.slope, res);
    __syncthreads();                                     // the hidden block is whole, h1 has been read
    order_mfma_layer<ORDER_MFMA_FROM_START, ORDER_MFMA_PLAIN, ORDER_MFMA_ADD>(ra, Hf, w_f2, Hf, b_f2, b_f2, E, rb, EMBED_X_PITCH, wave, g.slope,
                                                                               res);
    __syncthreads();                                     // the x tile is whole
    for (int i = wave; i < live; i += EMBED_ROW_WAVES) {
        const int b = i / k, s = i - b * k;
        float* dst = x + (bin0 + b) * g.env_stride + (size_t)s * g.row_stride;
        for (int e = lane; e < E; e += 64) dst[e] = rb[e * EMBED_X_PITCH + i];
    }
    for (int j = tid; j < bins * E; j += EMBED_ROW_THREADS) {
        const int b = j / E, e = j - b * E;
        const float* col = rb + e * EMBED_X_PITCH + b * k;
        float total = 0.0f;
        for (int gp = 0; gp < DUELING_PARTS; ++gp) {
            float s = 0.0f;
            for (int i = gp; i < k; i += DUELING_PARTS) s = s + col[i];
            total = gp == 0 ? s : total + s;
        }
        xg[(bin0 + b) * g.xg_stride + e] = total / (float)k;
    }
}

}  // namespace irbpp

#pragma float_control(pop)
