// Host harness (test infrastructure): the kernels of irbpp_amd/csrc/irbpp_streams.hip run on the CPU, one workgroup at a
// time, by 512 threads in lockstep (lockstep.h, as dueling_host.cpp).  The kernels' own source is compiled, so the chains,
// the staging, both instantiations and both sides of the LDS threshold (the second launch included) are what the CPU suite
// checks against the numpy definition; fmaf is the C library's, a single rounding (build with -ffp-contract=off).
// host_streams_act repeats the decisions of irbpp_streams_act (irbpp_capi.hip) after its argument checks.
// With -DSTREAMS_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the kernels over a few shapes,
// either side of the threshold included, and prints a checksum.
#include <stdio.h>

#define LOCKSTEP_TILE_FLOATS (144 * 1024 / 4)
#include "lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_dueling.hip"
#include "../../irbpp_amd/csrc/irbpp_streams.hip"

static_assert(sizeof g_tile == irbpp::DUELING_TILE_BYTES, "the harness tile is the kernels' dynamic LDS");

extern "C" void host_noisy_weights(const float* mu, const float* sigma, const float* eps, const float* bmu, const float* bsigma,
                                   const float* beps, int out, int in, float* w_out, float* b_out) {
    run_grid<256>((out * in + 255) / 256, 1, [&] { irbpp::irbpp_noisy_weights_kernel(mu, sigma, eps, bmu, bsigma, beps, out, in, w_out, b_out); });
}

// w: w_hv, b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za; force_generic: the <128> instantiation where irbpp_streams_act
// would take <32>.  Returns -1 where irbpp_streams_act would answer IRBPP_ERR_ARG for want of the workspace.
extern "C" int host_streams_act(const float* const* w, int embed, int hidden, int atoms, const float* xg, long long xg_stride,
                                const float* x, long long env_stride, long long row_stride, const float* support, const float* obs,
                                int obs_stride, int s_rows, int n_env, int64_t* action, float* q_out, long long q_stride, float* v_out,
                                float* a_out, int force_generic) {
    const bool resident = irbpp::dueling_tile_rows(s_rows, atoms) == s_rows;
    if (!resident && !a_out) return -1;
    irbpp::StreamsArgs g;
    g.xg_stride = xg_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.q_stride = q_stride;
    g.embed = embed, g.hidden = hidden, g.atoms = atoms, g.obs_stride = obs_stride, g.s_rows = s_rows;
    g.x_vec4 = ((uintptr_t)x % 16 == 0 && (uintptr_t)w[4] % 16 == 0 && env_stride % 4 == 0 && row_stride % 4 == 0 && embed % 4 == 0) ? 1 : 0;
    run_grid<irbpp::DUELING_THREADS>(n_env, 1, [&] {
        if (atoms <= 32 && !force_generic)
            irbpp::irbpp_streams_act_a32_kernel(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], xg, x, support, obs, action, q_out, v_out,
                                                a_out, g);
        else
            irbpp::irbpp_streams_act_kernel(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], xg, x, support, obs, action, q_out, v_out,
                                            a_out, g);
    });
    if (resident || (!action && !q_out)) return 0;
    run_grid<irbpp::DUELING_THREADS>(n_env, 1, [&] {
        irbpp::irbpp_streams_finish_kernel(w[0], w[1], w[2], w[3], xg, a_out, support, obs, action, q_out, g);
    });
    return 0;
}

#ifdef STREAMS_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    const int shapes[][5] = {{1, 5, 3, 2, 2}, {65, 130, 67, 31, 1}, {500, 128, 128, 31, 1}, {129, 16, 17, 128, 1}, {600, 7, 33, 51, 1},
                             {300, 5, 3, 128, 2}};                              // S, E, H, atoms, n; the last: the workspace path
    uint32_t rng = 12345u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (const auto& sh : shapes) {
        const int s = sh[0], E = sh[1], H = sh[2], atoms = sh[3], n = sh[4];
        const size_t sizes[8] = {(size_t)H * E, (size_t)H, (size_t)atoms * H, (size_t)atoms, (size_t)H * E, (size_t)H, (size_t)atoms * H, (size_t)atoms};
        std::vector<float> mu[8], eff[8];
        const float* w[8];
        for (int i = 0; i < 8; ++i) {
            mu[i].resize(sizes[i]);
            eff[i].resize(sizes[i]);
            for (auto& f : mu[i]) f = next() * 0.3f;
        }
        for (int i = 0; i < 8; i += 2) {
            host_noisy_weights(mu[i].data(), mu[i].data(), mu[i].data(), mu[i + 1].data(), mu[i + 1].data(), mu[i + 1].data(),
                               (int)sizes[i + 1], (int)(sizes[i] / sizes[i + 1]), eff[i].data(), eff[i + 1].data());
            w[i] = eff[i].data();
            w[i + 1] = eff[i + 1].data();
        }
        std::vector<float> xg((size_t)n * E), x((size_t)n * s * E), z(atoms), obs((size_t)n * s * 5), q((size_t)n * s), v((size_t)n * atoms),
            a((size_t)n * s * atoms);
        std::vector<int64_t> act(n);
        for (auto* t : {&xg, &x}) for (auto& f : *t) f = next();
        for (int k = 0; k < atoms; ++k) z[k] = -1.0f + 9.0f * k / (atoms - 1);
        for (size_t i = 0; i < obs.size(); ++i) obs[i] = (i % 5 == 4 && (i / 5) % 3 == 0) ? 0.0f : 1.0f;
        for (int generic = 0; generic < 2; ++generic) {
            if (host_streams_act(w, E, H, atoms, xg.data(), E, x.data(), (long long)s * E, E, z.data(), obs.data(), s * 5, s, n, act.data(),
                                 q.data(), s, v.data(), a.data(), generic))
                return 1;
            const bool fits = irbpp::dueling_tile_rows(s, atoms) == s;
            if (host_streams_act(w, E, H, atoms, xg.data(), E, x.data(), (long long)s * E, E, z.data(), nullptr, 0, s, n, act.data(), nullptr,
                                 0, nullptr, fits ? nullptr : a.data(), generic))
                return 1;
            for (int e = 0; e < n; ++e) sum += (double)act[e];
            for (float f : q) sum += f;
            for (float f : v) sum += f;
            for (float f : a) sum += f;
        }
        printf("S %d E %d H %d atoms %d n %d tile rows %d: checksum %.9g\n", s, E, H, atoms, n, irbpp::dueling_tile_rows(s, atoms), sum);
    }
    return 0;
}
#endif
