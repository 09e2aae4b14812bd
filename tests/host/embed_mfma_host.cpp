// Host harness (test infrastructure): the bin kernel of irbpp_amd/csrc/irbpp_embed.hip and the row kernel of
// irbpp_amd/csrc/irbpp_embed_mfma.hip run on the CPU, one workgroup at a time, by 512 threads in lockstep (lockstep.h), the
// matrix instruction replaced by mfma_shim.h: the kernels' own source is compiled, so the operand and accumulator lane maps,
// the pairs of (feature block, row half) dealt to the waves, the hand-over of a layer through its LDS region, the padded
// features and rows and the element loads of unaligned weight rows are what the CPU suite checks against the numpy definition.
// The dynamic LDS is a heap block of exactly the bytes irbpp_embed_mfma asks for, and the instruction waits for its own wave
// only, as on the device (waves take different numbers of pairs).  host_embed_mfma repeats the launches of irbpp_embed_mfma
// (irbpp_capi.hip) and its refusal of widths that are no multiple of 4.
// With -DEMBED_MFMA_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the kernels over the test's
// four configurations with buffers exactly as large as the kernels may touch and prints a checksum.
#include <stdio.h>

#include "lockstep.h"
#include "mfma_shim.h"

#include "../../irbpp_amd/csrc/irbpp_embed.hip"
#include "../../irbpp_amd/csrc/irbpp_embed_mfma.hip"

// w: the 14 arrays in irbpp_embed_weights' order; sizes: map_len, c1, c2, c3, feat, cand_hidden, cand_embed, proj_hidden, embed.
// Returns the bytes of dynamic LDS of the rows kernel, -1 where irbpp_embed_mfma answers IRBPP_ERR_ARG for the widths.
extern "C" long long host_embed_mfma(const float* const* w, const int* sizes, float slope, const float* obs, long long obs_stride,
                                     const float* shape_feat, long long feat_stride, int s_rows, int n_env, float* base, float* x,
                                     long long env_stride, long long row_stride, float* xg, long long xg_stride) {
    if (sizes[5] % 4 || sizes[6] % 4 || sizes[7] % 4) return -1;
    irbpp::EmbedArgs g;
    g.obs_stride = obs_stride, g.feat_stride = feat_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.xg_stride = xg_stride;
    g.map_len = sizes[0], g.c1 = sizes[1], g.c2 = sizes[2], g.c3 = sizes[3], g.feat = sizes[4], g.cand_hidden = sizes[5];
    g.cand_embed = sizes[6], g.proj_hidden = sizes[7], g.embed = sizes[8], g.s_rows = s_rows, g.slope = slope;
    lockstep_launch(irbpp::EMBED_BIN_THREADS, n_env, 1,
                    [&] { irbpp::irbpp_embed_bin_kernel(w[0], w[1], w[2], w[3], w[4], w[5], w[10], w[11], obs, shape_feat, base, g); });
    LockstepLaunch how;
    how.wave_shuffles = true;
    how.dynamic_lds = (long long)irbpp::embed_rows_lds_floats(g.cand_hidden, g.cand_embed, g.proj_hidden, g.embed) * (long long)sizeof(float);
    lockstep_launch(irbpp::EMBED_ROW_THREADS, n_env, 1,
                    [&] { irbpp::irbpp_embed_rows_mfma_kernel(w[6], w[7], w[8], w[9], w[10], w[12], w[13], obs, base, x, xg, g); }, how);
    return how.dynamic_lds;
}

#ifdef EMBED_MFMA_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    // N, S, then the nine sizes; pad: what the strides add to the rows.  small4 (and once more with weight rows of
    // project_layer[0] that are not 16-byte aligned: feat + M = 49), blocks, the reference's widths, the widest
    const int cases[][12] = {{3, 17, 8, 3, 5, 2, 40, 12, 36, 44, 33, 3},         {2, 33, 8, 3, 5, 2, 41, 12, 36, 44, 33, 1},
                             {2, 65, 8, 3, 5, 2, 40, 36, 68, 100, 70, 1},        {1, 65, 32, 16, 32, 4, 128, 32, 128, 256, 128, 5},
                             {1, 65, 8, 3, 5, 2, 256, 64, 256, 256, 256, 0}};
    uint32_t rng = 54321u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (const auto& cs : cases) {
        const int N = cs[0], S = cs[1], L = cs[2], c1 = cs[3], c2 = cs[4], c3 = cs[5], F = cs[6], Hc = cs[7], Ec = cs[8], P = cs[9], E = cs[10];
        const int pad = cs[11], M = c3 * (L / 4) * (L / 4), obs_len = 5 * S + 9 + L * L;
        const size_t counts[14] = {(size_t)c1 * 16, (size_t)c1, (size_t)c2 * c1 * 16, (size_t)c2, (size_t)c3 * c2 * 9, (size_t)c3, (size_t)Hc * 4,
                                   (size_t)Hc,      (size_t)Ec * Hc, (size_t)Ec,      (size_t)P * (F + M + Ec), (size_t)P, (size_t)E * P, (size_t)E};
        std::vector<std::vector<float>> store(14);
        const float* w[14];
        for (int i = 0; i < 14; ++i) {
            store[i].resize(counts[i]);
            for (auto& f : store[i]) f = next() * 0.2f;
            w[i] = store[i].data();
        }
        const long long obs_stride = obs_len + pad, feat_stride = F + pad, row_stride = E + pad, env_stride = (long long)S * row_stride + pad;
        const long long xg_stride = E + pad;
        std::vector<float> obs((size_t)(N - 1) * obs_stride + obs_len), sf((size_t)(N - 1) * feat_stride + F), base((size_t)N * P);
        std::vector<float> x((size_t)(N - 1) * env_stride + (size_t)(S - 1) * row_stride + E), xg((size_t)(N - 1) * xg_stride + E);
        for (auto* t : {&obs, &sf}) for (auto& f : *t) f = next();
        for (int n = 0; n < N; ++n)
            for (int r = 0; r < S; ++r) obs[(size_t)n * obs_stride + 5 * r + 4] = (r + n) % 3 == 0 ? 0.0f : 1.0f;
        const int sizes[9] = {L, c1, c2, c3, F, Hc, Ec, P, E};
        const long long lds = host_embed_mfma(w, sizes, 0.01f, obs.data(), obs_stride, sf.data(), feat_stride, S, N, base.data(), x.data(),
                                              env_stride, row_stride, xg.data(), xg_stride);
        if (lds < 0) return 1;
        for (int n = 0; n < N; ++n)
            for (int r = 0; r < S; ++r)
                for (int e = 0; e < E; ++e) {
                    const float v = x[(size_t)n * env_stride + (size_t)r * row_stride + e];
                    if (v != v || (((r + n) % 3 == 0) && v != 0.0f)) return 2;
                    sum += v;
                }
        for (int n = 0; n < N; ++n)
            for (int e = 0; e < E; ++e) sum += xg[(size_t)n * xg_stride + e];
        printf("N %d S %d L %d widths %d %d %d %d %d %d %d %d lds %lld: checksum %.9g\n", N, S, L, c1, c2, c3, F, Hc, Ec, P, E, lds, sum);
    }
    return 0;
}
#endif
