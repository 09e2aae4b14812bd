// irbpp_order_embed.hip -- the embedding stage of the order network, DQNBPP.forward without a gradient for bufferSize > 1
// (model.py:355-383, embed_k_buffer_shape_with_gat: the heightmap CNN, gat_project_layer per buffered item, one attention
// layer of one head with its feed-forward pair, the mean): from the observation and the k shape features of every bin to
// embeddings [N][k][E] and graph_embed [N][E].  Two launches, no atomics; Q, K, V, the compatibilities and every hidden
// block stay in LDS and registers.
//
// Defined float32 arithmetic (tests/test_order_embed_cpu.py restates it and the kernels are held to it bit for bit).
//   Every layer output is one chain: acc = start; acc = fmaf(x[c], W[j][c], acc) for c ascending, never split or
//   re-associated; lin(W, b, x)[j] starts from b[j].  leaky(s) = s > 0 ? s : slope * s, relu(s) = s > 0 ? s : +0.
//   Observation row of bin n: obs[0 .. k) the k buffered item ids (not read here), obs[k ..] the L x L heightmap, row-major.
//   shape_feat[n][i][0 .. F): irbpp_shape_features over the N k ids, bin-major.
//   map[0 .. M), M = C3 (L/4)^2: the heightmap CNN of irbpp_embed.hip's definition (embed_height_map, irbpp_front.h).
//   base[j]  = the chain from b_g1[j] over map[0 .. M) against W_g1[j][F .. F+M)                       per bin, j < P
//   g[i][j]  = leaky(the chain continued from base[j] over shape_feat[i][0 .. F) against W_g1[j][0 .. F))   per slot i < k
//   h0[i]    = lin(W_g2, b_g2, g[i])                                                                   E values
//   Q[i], K[i], V[i]: chains from +0.0 over h0[i] against W_q, W_k, W_v (no bias)
//   c[i][j]  = nf * (the chain from +0.0 of fmaf(Q[i][d], K[j][d], acc), d ascending), nf = (float)(1.0 / sqrt((double)E))
//   m = max_j c[i][j], e[j] = dueling_dexp(c[i][j] - m), den = the e[j] added left to right from 0.0, a[i][j] = e[j] / den
//   hd[i][d] = the chain from +0.0 of fmaf(a[i][j], V[j][d], acc), j ascending
//   h1[i]    = h0[i] + lin(W_o, b_o, hd[i])
//   h2[i]    = h1[i] + lin(W_f2, b_f2, relu(lin(W_f1, b_f1, h1[i])))
//   x[n][i]  = h2[i]; xg[n] = dueling_mean's sum of the k rows (part g < 16 takes rows g, g+16, .. ascending from 0.0, the
//              parts are added left to right), divided by (float)k.
// The reference multiplies gat_project_layer[0] by the concatenation (shape feature, map feature).  The map part is the one
// all k slots of a bin share and two thirds of the chain, so here it goes FIRST and runs once per bin: the definition is a
// fixed permutation of the concatenation's summation order, not the concatenation's own order.  The attention mask does not
// enter: the reference passes all zeros on this path.
// A function of the inputs alone: not of N, of strides or of the tiles.  No index depends on data: nothing out of range is
// read whatever the values.  Inputs must be finite (a NaN gives unspecified values).
//
// Layout.  irbpp_order_bin_kernel, one workgroup of EMBED_BIN_THREADS per bin: irbpp_front.h's heightmap encoder through
// zero-padded LDS tiles, thread j then runs base[j].  irbpp_order_rows_kernel, one workgroup of EMBED_ROW_THREADS per tile
// of 64 rows: a row is a (bin, slot) pair taken bin-major, a tile holds 64 / k whole bins (attention never crosses a
// tile), lane = row; a lane past the tile's last row recomputes that last row and is dropped.  A layer's inputs lie in LDS as
// [c][row]; the waves own blocks of EMBED_FBLOCK output features whose weights are wave-uniform __restrict__ loads
// (embed_chain), so one read of a weight serves the whole tile.  Two LDS regions take turns:
//   A: shape features [F][64] -> h0 [E][64] -> hd [E][64] -> the feed-forward hidden block [Hf][64]
//   B: g [P][64] -> Q and K, ORDER_QK_BLOCK features of each at a time -> V [E][64] -> h1 [E][64] -> the x tile [E][65]
// and the k compatibilities of every row lie in a third, [k][64].  h0 and h1 stay in the registers of the thread that
// computed them (the same thread owns the same features of the residual's other term).  The compatibility chains run over
// all E features in order: with E > ORDER_QK_BLOCK the Q and K blocks are produced and consumed in turn, the running chains
// in registers (row = lane, key slot = wave, wave + 8, ..).  The softmax of a row is its lane's of wave 0.
#include "irbpp_front.h"

#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

constexpr int ORDER_MAX_WIDTH = 256;                     // F, P, E, Hf
constexpr int ORDER_MAX_SLOTS = EMBED_TILE_ROWS;         // k: a bin fits a tile
constexpr int ORDER_QK_BLOCK = EMBED_ROW_WAVES * EMBED_FBLOCK;   // features of Q and of K in LDS at a time: one block per wave
constexpr int ORDER_PASSES = ORDER_MAX_WIDTH / ORDER_QK_BLOCK;   // blocks of E output features per wave
constexpr int ORDER_PAIRS = ORDER_MAX_SLOTS / EMBED_ROW_WAVES;   // key slots per thread

struct OrderEmbedArgs {
    long long obs_stride, feat_stride, env_stride, row_stride, xg_stride;
    int map_len, c1, c2, c3, feat, proj_hidden, embed, ff_hidden, k_slots, n_env;
    float slope, norm;
};

// floats of dynamic LDS of the rows kernel (constexpr: the host sizes the launch by it, as for the device)
constexpr int order_max(int a, int b) { return a > b ? a : b; }
constexpr int order_qk_rows(int embed) { return embed < ORDER_QK_BLOCK ? embed : ORDER_QK_BLOCK; }
constexpr int order_region_a(int feat, int embed, int ff_hidden) { return order_max(feat, order_max(embed, ff_hidden)) * EMBED_TILE_ROWS; }
constexpr int order_region_b(int proj_hidden, int embed) {
    return order_max(order_max(proj_hidden, 2 * order_qk_rows(embed)) * EMBED_TILE_ROWS, embed * EMBED_X_PITCH);
}
constexpr int order_rows_lds_floats(int feat, int proj_hidden, int embed, int ff_hidden, int k_slots) {
    return order_region_a(feat, embed, ff_hidden) + order_region_b(proj_hidden, embed) + k_slots * EMBED_TILE_ROWS;
}
// whole bins per tile, and tiles per call
constexpr int order_tile_bins(int k_slots) { return EMBED_TILE_ROWS / k_slots; }
constexpr int order_tiles(int n_env, int k_slots) { return (n_env + order_tile_bins(k_slots) - 1) / order_tile_bins(k_slots); }

__device__ __forceinline__ float order_relu(float s) { return s > 0.0f ? s : 0.0f; }

// Workgroup n: base[n][0 .. P)
extern "C" __global__ void __launch_bounds__(EMBED_BIN_THREADS)
irbpp_order_bin_kernel(const float* __restrict__ w_conv1, const float* __restrict__ b_conv1, const float* __restrict__ w_conv2,
                       const float* __restrict__ b_conv2, const float* __restrict__ w_conv3, const float* __restrict__ b_conv3,
                       const float* __restrict__ w_g1, const float* __restrict__ b_g1, const float* __restrict__ obs,
                       float* __restrict__ base, OrderEmbedArgs g) {
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x;
    const float* height = obs + n * g.obs_stride + g.k_slots;
    const float* map = embed_height_map(height, w_conv1, b_conv1, w_conv2, b_conv2, w_conv3, b_conv3, g.map_len, g.c1, g.c2, g.c3, g.slope);
    const int L4 = g.map_len / 4;
    const int F = g.feat, M = g.c3 * L4 * L4, ld = F + M;
    for (int j = tid; j < g.proj_hidden; j += EMBED_BIN_THREADS) {
        const float* wr = w_g1 + (size_t)j * ld + F;
        float acc = b_g1[j];
        for (int c = 0; c < M; ++c) acc = fmaf(map[c], wr[c], acc);
        base[n * g.proj_hidden + j] = acc;
    }
}

// the wave's block of output features in pass p: f0, and how many of them exist (<= 0: none)
__device__ __forceinline__ int order_block_count(int width, int f0) {
    return width - f0 < EMBED_FBLOCK ? width - f0 : EMBED_FBLOCK;
}

// Workgroup t: the bins [t * (64 / k), ..) of the tile: x[n][0 .. k)[0 .. E) and xg[n][0 .. E) from shape_feat and base
extern "C" __global__ void __launch_bounds__(EMBED_ROW_THREADS)
irbpp_order_rows_kernel(const float* __restrict__ w_g1, const float* __restrict__ w_g2, const float* __restrict__ b_g2,
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
    float res[ORDER_PASSES][EMBED_FBLOCK];               // h0, then h1: the residuals' first terms
    {
        const float* sf = shape_feat + (bin0 * k + r) * g.feat_stride;
        for (int c = wave; c < F; c += EMBED_ROW_WAVES) ra[c * EMBED_TILE_ROWS + lane] = sf[c];
    }
    __syncthreads();
    {
        const float* base_r = base + (bin0 + bin) * P;
        for (int f0 = wave * EMBED_FBLOCK; f0 < P; f0 += ORDER_QK_BLOCK) {
            const int nf = order_block_count(P, f0);
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = base_r[f0 + (m < nf ? m : nf - 1)];
            embed_chain(ra, lane, F, w_g1, ld1, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m)
                if (m < nf) rb[(f0 + m) * EMBED_TILE_ROWS + lane] = front_leaky(acc[m], g.slope);
        }
    }
    __syncthreads();                                     // g is whole, the shape features have been read
#pragma unroll
    for (int p = 0; p < ORDER_PASSES; ++p) {
        const int f0 = p * ORDER_QK_BLOCK + wave * EMBED_FBLOCK, nf = order_block_count(E, f0);
        if (nf > 0) {
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = b_g2[f0 + (m < nf ? m : nf - 1)];
            embed_chain(rb, lane, P, w_g2, P, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) {
                res[p][m] = acc[m];
                if (m < nf) ra[(f0 + m) * EMBED_TILE_ROWS + lane] = acc[m];
            }
        }
    }
    __syncthreads();                                     // h0 is whole, g has been read
    {
        float* qb = rb;
        float* kb = rb + order_qk_rows(E) * EMBED_TILE_ROWS;
        float cacc[ORDER_PAIRS];
#pragma unroll
        for (int t = 0; t < ORDER_PAIRS; ++t) cacc[t] = 0.0f;
        for (int d0 = 0; d0 < E; d0 += ORDER_QK_BLOCK) {
            const int nd = E - d0 < ORDER_QK_BLOCK ? E - d0 : ORDER_QK_BLOCK;
            const int l0 = wave * EMBED_FBLOCK, nf = order_block_count(nd, l0);
            if (nf > 0) {
                float acc[EMBED_FBLOCK];
#pragma unroll
                for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = 0.0f;
                embed_chain(ra, lane, E, w_q, E, d0 + l0, nf, acc);
#pragma unroll
                for (int m = 0; m < EMBED_FBLOCK; ++m)
                    if (m < nf) qb[(l0 + m) * EMBED_TILE_ROWS + lane] = acc[m];
#pragma unroll
                for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = 0.0f;
                embed_chain(ra, lane, E, w_k, E, d0 + l0, nf, acc);
#pragma unroll
                for (int m = 0; m < EMBED_FBLOCK; ++m)
                    if (m < nf) kb[(l0 + m) * EMBED_TILE_ROWS + lane] = acc[m];
            }
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
#pragma unroll
    for (int p = 0; p < ORDER_PASSES; ++p) {
        const int f0 = p * ORDER_QK_BLOCK + wave * EMBED_FBLOCK, nf = order_block_count(E, f0);
        if (nf > 0) {
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = 0.0f;
            embed_chain(ra, lane, E, w_v, E, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m)
                if (m < nf) rb[(f0 + m) * EMBED_TILE_ROWS + lane] = acc[m];
        }
    }
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
    for (int p = 0; p < ORDER_PASSES; ++p) {
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
#pragma unroll
    for (int p = 0; p < ORDER_PASSES; ++p) {
        const int f0 = p * ORDER_QK_BLOCK + wave * EMBED_FBLOCK, nf = order_block_count(E, f0);
        if (nf > 0) {
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = b_o[f0 + (m < nf ? m : nf - 1)];
            embed_chain(ra, lane, E, w_o, E, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) {
                res[p][m] = res[p][m] + acc[m];
                if (m < nf) rb[(f0 + m) * EMBED_TILE_ROWS + lane] = res[p][m];
            }
        }
    }
    __syncthreads();                                     // h1 is whole, hd has been read
    for (int f0 = wave * EMBED_FBLOCK; f0 < Hf; f0 += ORDER_QK_BLOCK) {
        const int nf = order_block_count(Hf, f0);
        float acc[EMBED_FBLOCK];
#pragma unroll
        for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = b_f1[f0 + (m < nf ? m : nf - 1)];
        embed_chain(rb, lane, E, w_f1, E, f0, nf, acc);
#pragma unroll
        for (int m = 0; m < EMBED_FBLOCK; ++m)
            if (m < nf) ra[(f0 + m) * EMBED_TILE_ROWS + lane] = order_relu(acc[m]);
    }
    __syncthreads();                                     // the hidden block is whole, h1 has been read
#pragma unroll
    for (int p = 0; p < ORDER_PASSES; ++p) {
        const int f0 = p * ORDER_QK_BLOCK + wave * EMBED_FBLOCK, nf = order_block_count(E, f0);
        if (nf > 0) {
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = b_f2[f0 + (m < nf ? m : nf - 1)];
            embed_chain(ra, lane, Hf, w_f2, Hf, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m)
                if (m < nf) rb[(f0 + m) * EMBED_X_PITCH + lane] = res[p][m] + acc[m];
        }
    }
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
