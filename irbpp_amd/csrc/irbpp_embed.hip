// irbpp_embed.hip -- the embedding stage of DQNBPP.forward without a gradient (model.py:318-326, :337-352, bufferSize == 1):
// from the observation and shape_feature to embeddings [N][S][E] and graph_embed [N][E].  The reference concatenates
// (shape_feature, map_feature, candidate embedding) per candidate row and multiplies every row by project_layer[0]; the first
// F + M of those inputs are the same for all S rows of a bin, so here that part of every chain is run once per bin (`base`)
// and every row continues it: two launches, no atomics, neither the concatenation nor the hidden blocks reach memory.
//
// Defined float32 arithmetic (tests/test_embed_cpu.py restates it and the kernels are held to it bit for bit).
//   lin(W, b, x)[j]: acc = b[j]; for k = 0 .. K-1 ascending: acc = fmaf(x[k], W[j][k], acc): written out, never split or
//                    re-associated.  leaky(s) = s > 0 ? s : slope * s.
//   Observation row of bin n: obs[5r .. 5r+3] candidate r, obs[5r+4] its mask, obs[5S+9 ..] the L x L heightmap, row-major.
//   conv1 (1 -> C1, 4x4, stride 2, pad 1) leaky, conv2 (C1 -> C2, 4x4, stride 2, pad 1) leaky, conv3 (C2 -> C3, 3x3, stride 1,
//   pad 1) leaky: every output one chain from its bias over the taps in ascending (c_in, ky, kx), a tap in the padding being
//   part of the chain with the input +0.0.  map[c (L/4)^2 + y (L/4) + x], M = C3 (L/4)^2 values.
//   base[j]  = the chain from b_p1[j] over shape_feature[n][0 .. F) against W_p1[j][0 .. F), then over map[0 .. M) against
//              W_p1[j][F .. F+M)                                                                    per bin, j < P
//   e1 = leaky(lin(W_c1, b_c1, cand_r)), e2 = lin(W_c2, b_c2, e1)                                   per row
//   h[j]     = leaky(the chain continued from base[j] over e2[0 .. Ec) against W_p1[j][F+M ..))
//   x_r      = lin(W_p2, b_p2, h) where mask == 1.0f exactly (a NaN mask is invalid), else +0.0 in every element
//   xg[e]    = dueling_mean's sum of the rows of x over all S: part g < 16 takes rows g, g+16, .. ascending from 0.0, the
//              parts are added left to right, divided by (float)S.
// A function of the inputs alone: not of N, of strides or of the tiles.  No index depends on data: nothing out of range is
// read whatever the values.
//
// Layout.  irbpp_embed_bin_kernel, one workgroup of EMBED_BIN_THREADS per bin: the heightmap goes to a zero-padded LDS tile,
// the three convolutions pass through zero-padded LDS tiles (embed_height_map, irbpp_front.h), thread j then runs base[j].
// irbpp_embed_rows_kernel, one workgroup of EMBED_ROW_THREADS per bin, walks the bin's tiles of 64 rows in order, lane = row:
// a layer's inputs lie in LDS as [k][row] (conflict-free dword reads), the waves own blocks of EMBED_FBLOCK output features
// whose weights are wave-uniform __restrict__ loads (scalar cache, SGPR operands of the FMA), EMBED_KBLOCK contiguous
// elements per feature at a time (embed_chain, irbpp_front.h).  e1 shares the LDS of h (dead before h is written), the x tile
// (pitch 65, read transposed for coalesced stores) that of e2.  A row past S in the last tile recomputes row S-1 and is
// dropped.  The 16 running parts of the mean stay in LDS across the tiles; x is written once and never read back.
#include "irbpp_front.h"

// NaNs are part of this definition (an invalid row may hold any candidate), whatever the build's command line says
#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

constexpr int EMBED_MAX_WIDTH = 256;                     // F, Ec, P, E
constexpr int EMBED_MAX_CAND_HIDDEN = 64;                // Hc

struct EmbedArgs {
    long long obs_stride, feat_stride, env_stride, row_stride, xg_stride;
    int map_len, c1, c2, c3, feat, cand_hidden, cand_embed, proj_hidden, embed, s_rows;
    float slope;
};

// floats of dynamic LDS of the rows kernel: region A (e2 [Ec][64], then the x tile [E][65]), region B (e1 [Hc][64], then
// h [P][64]), the parts of the mean [16][E] (constexpr: the host sizes the launch by it, as for the device)
constexpr int embed_region_a(int cand_embed, int embed) {
    return cand_embed * EMBED_TILE_ROWS > embed * EMBED_X_PITCH ? cand_embed * EMBED_TILE_ROWS : embed * EMBED_X_PITCH;
}
constexpr int embed_region_b(int cand_hidden, int proj_hidden) {
    return (cand_hidden > proj_hidden ? cand_hidden : proj_hidden) * EMBED_TILE_ROWS;
}
constexpr int embed_rows_lds_floats(int cand_hidden, int cand_embed, int proj_hidden, int embed) {
    return embed_region_a(cand_embed, embed) + embed_region_b(cand_hidden, proj_hidden) + DUELING_PARTS * embed;
}

// Workgroup n: base[n][0 .. P)
extern "C" __global__ void __launch_bounds__(EMBED_BIN_THREADS)
irbpp_embed_bin_kernel(const float* __restrict__ w_conv1, const float* __restrict__ b_conv1, const float* __restrict__ w_conv2,
                       const float* __restrict__ b_conv2, const float* __restrict__ w_conv3, const float* __restrict__ b_conv3,
                       const float* __restrict__ w_p1, const float* __restrict__ b_p1, const float* __restrict__ obs,
                       const float* __restrict__ shape_feat, float* __restrict__ base, EmbedArgs g) {
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x;
    const float* height = obs + n * g.obs_stride + 5 * g.s_rows + 9;
    const float* map = embed_height_map(height, w_conv1, b_conv1, w_conv2, b_conv2, w_conv3, b_conv3, g.map_len, g.c1, g.c2, g.c3, g.slope);
    const int L4 = g.map_len / 4;
    const int F = g.feat, M = g.c3 * L4 * L4, ld = F + M + g.cand_embed;
    const float* sf = shape_feat + n * g.feat_stride;
    for (int j = tid; j < g.proj_hidden; j += EMBED_BIN_THREADS) {
        const float* wr = w_p1 + (size_t)j * ld;
        float acc = b_p1[j];
        for (int k = 0; k < F; ++k) acc = fmaf(sf[k], wr[k], acc);
        for (int k = 0; k < M; ++k) acc = fmaf(map[k], wr[F + k], acc);
        base[n * g.proj_hidden + j] = acc;
    }
}

// Workgroup n: x[n][0 .. S)[0 .. E) and xg[n][0 .. E) from the observation row and base[n]
extern "C" __global__ void __launch_bounds__(EMBED_ROW_THREADS)
irbpp_embed_rows_kernel(const float* __restrict__ w_c1, const float* __restrict__ b_c1, const float* __restrict__ w_c2,
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
        const bool valid = cand[4] == 1.0f;
        __syncthreads();                                 // the tile before: h and the x tile have been read
        for (int i = wave; i < Hc; i += EMBED_ROW_WAVES) {
            const float* wr = w_c1 + (size_t)i * 4;
            rb[i * EMBED_TILE_ROWS + lane] = front_leaky(fmaf(c3, wr[3], fmaf(c2, wr[2], fmaf(c1, wr[1], fmaf(c0, wr[0], b_c1[i])))), g.slope);
        }
        __syncthreads();
        for (int f0 = wave * EMBED_FBLOCK; f0 < Ec; f0 += EMBED_ROW_WAVES * EMBED_FBLOCK) {
            const int nf = Ec - f0 < EMBED_FBLOCK ? Ec - f0 : EMBED_FBLOCK;
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = b_c2[f0 + (m < nf ? m : nf - 1)];
            embed_chain(rb, lane, Hc, w_c2, Hc, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m)
                if (m < nf) ra[(f0 + m) * EMBED_TILE_ROWS + lane] = acc[m];
        }
        __syncthreads();                                 // e2 is whole, e1 has been read
        for (int f0 = wave * EMBED_FBLOCK; f0 < P; f0 += EMBED_ROW_WAVES * EMBED_FBLOCK) {
            const int nf = P - f0 < EMBED_FBLOCK ? P - f0 : EMBED_FBLOCK;
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = base_n[f0 + (m < nf ? m : nf - 1)];
            embed_chain(ra, lane, Ec, w_p1c, ld1, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m)
                if (m < nf) rb[(f0 + m) * EMBED_TILE_ROWS + lane] = front_leaky(acc[m], g.slope);
        }
        __syncthreads();                                 // h is whole, e2 has been read
        for (int f0 = wave * EMBED_FBLOCK; f0 < E; f0 += EMBED_ROW_WAVES * EMBED_FBLOCK) {
            const int nf = E - f0 < EMBED_FBLOCK ? E - f0 : EMBED_FBLOCK;
            float acc[EMBED_FBLOCK];
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m) acc[m] = b_p2[f0 + (m < nf ? m : nf - 1)];
            embed_chain(rb, lane, P, w_p2, P, f0, nf, acc);
#pragma unroll
            for (int m = 0; m < EMBED_FBLOCK; ++m)
                if (m < nf) ra[(f0 + m) * EMBED_X_PITCH + lane] = valid ? acc[m] : 0.0f;
        }
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
