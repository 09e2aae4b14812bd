// Host harness (test infrastructure): the bin kernel of irbpp_amd/csrc/irbpp_order_embed.hip and the row kernel of
// irbpp_amd/csrc/irbpp_order_embed_mfma.hip run on the CPU, one workgroup at a time, by 512 threads in lockstep (lockstep.h),
// the matrix instruction replaced by mfma_shim.h: the kernels' own source is compiled, so the operand and accumulator lane
// maps, the pairs of (feature block, row half) dealt to the waves and their passes, the starts of the chains (`base` of the
// column's bin, a bias, +0.0), the residuals kept in registers, the hand-over of a layer through its LDS region, the padded
// features, the lanes past the tile's last row and the element loads of unaligned weight rows are what the CPU suite checks
// against the numpy definition.  The dynamic LDS is a heap block of exactly the bytes irbpp_order_embed_mfma asks for, and the
// instruction waits for its own wave only, as on the device (waves take different numbers of pairs).  host_order_embed_mfma
// repeats the launches of irbpp_order_embed_mfma (irbpp_capi.hip) and its refusal of widths that are no multiple of 4.
// With -DORDER_EMBED_MFMA_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the kernels over a few
// shapes with buffers exactly as large as the kernels may touch and prints a checksum.
#include <stdio.h>

#include "lockstep.h"
#include "mfma_shim.h"

#include "../../irbpp_amd/csrc/irbpp_order_embed.hip"
#include "../../irbpp_amd/csrc/irbpp_order_embed_mfma.hip"

// w: the 19 arrays in irbpp_order_embed_weights' order; sizes: map_len, c1, c2, c3, feat, proj_hidden, embed, ff_hidden.
// Returns the bytes of dynamic LDS of the rows kernel, -1 where irbpp_order_embed_mfma answers IRBPP_ERR_ARG for the widths.
extern "C" long long host_order_embed_mfma(const float* const* w, const int* sizes, float slope, const float* obs, long long obs_stride,
                                           const float* shape_feat, long long feat_stride, int k_slots, int n_env, float* base, float* x,
                                           long long env_stride, long long row_stride, float* xg, long long xg_stride) {
    if (sizes[4] % 4 || sizes[5] % 4 || sizes[6] % 4 || sizes[7] % 4) return -1;
    irbpp::OrderEmbedArgs g;
    g.obs_stride = obs_stride, g.feat_stride = feat_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.xg_stride = xg_stride;
    g.map_len = sizes[0], g.c1 = sizes[1], g.c2 = sizes[2], g.c3 = sizes[3], g.feat = sizes[4], g.proj_hidden = sizes[5];
    g.embed = sizes[6], g.ff_hidden = sizes[7], g.k_slots = k_slots, g.n_env = n_env, g.slope = slope;
    g.norm = (float)(1.0 / sqrt((double)g.embed));
    lockstep_launch(irbpp::EMBED_BIN_THREADS, n_env, 1,
                    [&] { irbpp::irbpp_order_bin_kernel(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], obs, base, g); });
    LockstepLaunch how;
    how.wave_shuffles = true;
    how.dynamic_lds = (long long)irbpp::order_rows_mfma_lds_floats(g.feat, g.proj_hidden, g.embed, g.ff_hidden, k_slots) * (long long)sizeof(float);
    lockstep_launch(irbpp::EMBED_ROW_THREADS, irbpp::order_tiles(n_env, k_slots), 1, [&] {
        irbpp::irbpp_order_rows_mfma_kernel(w[6], w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15], w[16], w[17], w[18], shape_feat, base, x, xg, g);
    }, how);
    return how.dynamic_lds;
}

#ifdef ORDER_EMBED_MFMA_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    // N, k, then the eight sizes; pad: what the strides add to the rows.  Every width 4; widths that are no multiple of 32 (and
    // once more with L = 12 and c3 = 1: feat + M = 21, so no weight row of gat_project_layer[0] is 16-byte aligned); the
    // reference's widths; the widest with a full tile
    const int cases[][11] = {{1, 2, 8, 3, 5, 2, 4, 4, 4, 4, 0},         {14, 5, 8, 3, 5, 2, 12, 36, 44, 20, 3},  {7, 10, 8, 3, 5, 2, 12, 36, 44, 20, 1},
                             {3, 33, 12, 3, 5, 1, 12, 36, 44, 20, 2},  {2, 10, 32, 16, 32, 4, 128, 256, 128, 128, 5},
                             {2, 64, 8, 3, 5, 2, 256, 256, 256, 256, 0}};
    uint32_t rng = 24680u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (const auto& cs : cases) {
        const int N = cs[0], k = cs[1], L = cs[2], c1 = cs[3], c2 = cs[4], c3 = cs[5], F = cs[6], P = cs[7], E = cs[8], Hf = cs[9];
        const int pad = cs[10], M = c3 * (L / 4) * (L / 4), obs_len = k + L * L;
        const size_t counts[19] = {(size_t)c1 * 16, (size_t)c1, (size_t)c2 * c1 * 16, (size_t)c2, (size_t)c3 * c2 * 9, (size_t)c3,
                                   (size_t)P * (F + M), (size_t)P, (size_t)E * P, (size_t)E, (size_t)E * E, (size_t)E * E, (size_t)E * E,
                                   (size_t)E * E, (size_t)E, (size_t)Hf * E, (size_t)Hf, (size_t)E * Hf, (size_t)E};
        std::vector<std::vector<float>> store(19);
        const float* w[19];
        for (int i = 0; i < 19; ++i) {
            store[i].resize(counts[i]);
            for (auto& f : store[i]) f = next() * 0.2f;
            w[i] = store[i].data();
        }
        const long long obs_stride = obs_len + pad, feat_stride = F + pad, row_stride = E + pad, env_stride = (long long)k * row_stride + pad;
        const long long xg_stride = E + pad;
        std::vector<float> obs((size_t)(N - 1) * obs_stride + obs_len), sf((size_t)(N * k - 1) * feat_stride + F), base((size_t)N * P);
        std::vector<float> x((size_t)(N - 1) * env_stride + (size_t)(k - 1) * row_stride + E), xg((size_t)(N - 1) * xg_stride + E);
        for (auto* t : {&obs, &sf}) for (auto& f : *t) f = next();
        const int sizes[8] = {L, c1, c2, c3, F, P, E, Hf};
        const long long lds = host_order_embed_mfma(w, sizes, 0.01f, obs.data(), obs_stride, sf.data(), feat_stride, k, N, base.data(),
                                                    x.data(), env_stride, row_stride, xg.data(), xg_stride);
        if (lds < 0) return 1;
        for (int n = 0; n < N; ++n)
            for (int r = 0; r < k; ++r)
                for (int e = 0; e < E; ++e) {
                    const float v = x[(size_t)n * env_stride + (size_t)r * row_stride + e];
                    if (v != v) return 2;
                    sum += v;
                }
        for (int n = 0; n < N; ++n)
            for (int e = 0; e < E; ++e) sum += xg[(size_t)n * xg_stride + e];
        printf("N %d k %d L %d widths %d %d %d %d %d %d %d lds %lld: checksum %.9g\n", N, k, L, c1, c2, c3, F, P, E, Hf, lds, sum);
    }
    return 0;
}
#endif
