// Host harness (test infrastructure): the kernels of irbpp_amd/csrc/irbpp_streams_mfma.hip run on the CPU, one workgroup at
// a time, by 512 threads in lockstep (lockstep.h), the matrix instruction replaced by mfma_shim.h: the kernels' own source is
// compiled, so the operand and accumulator lane maps, the hand-over between the two products, the padding rules, both
// instantiations and both sides of the LDS threshold (the second launch included) are what the CPU suite checks against the
// numpy definition.  The dynamic LDS is a heap block of exactly the bytes irbpp_streams_act_mfma asks for, and shuffles and
// the instruction wait for their own wave only, as on the device (waves take different numbers of row tiles).
// host_streams_act_mfma repeats the decisions of irbpp_streams_act_mfma (irbpp_capi.hip), its argument checks included.
// With -DSTREAMS_MFMA_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the kernels over a few
// shapes, either side of the threshold included, with buffers exactly as large as the kernels may touch, and prints a checksum.
#include <stdio.h>

#include "lockstep.h"
#include "mfma_shim.h"

#include "../../irbpp_amd/csrc/irbpp_dueling.hip"
#include "../../irbpp_amd/csrc/irbpp_streams.hip"
#include "../../irbpp_amd/csrc/irbpp_streams_mfma.hip"

// w: w_hv, b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za; force_generic: the 128-atom instantiation where irbpp_streams_act_mfma
// would take the 32-atom one.  Returns -1 where irbpp_streams_act_mfma answers IRBPP_ERR_ARG for the shape.
extern "C" int host_streams_act_mfma(const float* const* w, int embed, int hidden, int atoms, const float* xg, long long xg_stride,
                                     const float* x, long long env_stride, long long row_stride, const float* support,
                                     const float* obs, int obs_stride, int s_rows, int n_env, int64_t* action, float* q_out,
                                     long long q_stride, float* v_out, float* a_out, int force_generic) {
    using namespace irbpp;
    if (embed < 1 || embed > STREAMS_MAX_WIDTH || hidden < 1 || hidden > STREAMS_MAX_WIDTH || embed % 4 || hidden % 4) return -1;
    const bool resident = dueling_tile_rows(s_rows, atoms) == s_rows;
    if (!resident && !a_out) return -1;
    StreamsArgs g;
    g.xg_stride = xg_stride, g.env_stride = env_stride, g.row_stride = row_stride, g.q_stride = q_stride;
    g.embed = embed, g.hidden = hidden, g.atoms = atoms, g.obs_stride = obs_stride, g.s_rows = s_rows;
    g.x_vec4 = (((uintptr_t)x % 16 == 0 && env_stride % 4 == 0 && row_stride % 4 == 0) ? STREAMS_MFMA_X16 : 0) |
               ((uintptr_t)w[4] % 16 == 0 ? STREAMS_MFMA_WHA16 : 0) | ((uintptr_t)w[6] % 16 == 0 ? STREAMS_MFMA_WZA16 : 0);
    LockstepLaunch how;
    how.wave_shuffles = true;
    how.dynamic_lds = resident ? (long long)s_rows * (atoms | 1) * 4 : 0;
    lockstep_launch(DUELING_THREADS, n_env, 1, [&] {
        if (atoms <= MFMA_TILE && !force_generic)
            irbpp_streams_act_mfma_a32_kernel(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], xg, x, support, obs, action, q_out, v_out,
                                              a_out, g);
        else
            irbpp_streams_act_mfma_kernel(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], xg, x, support, obs, action, q_out, v_out, a_out,
                                          g);
    }, how);
    if (resident || (!action && !q_out)) return 0;
    how.dynamic_lds = (long long)dueling_tile_rows(s_rows, atoms) * (atoms | 1) * 4;
    lockstep_launch(DUELING_THREADS, n_env, 1, [&] {
        irbpp_streams_finish_kernel(w[0], w[1], w[2], w[3], xg, a_out, support, obs, action, q_out, g);
    }, how);
    return 0;
}

#ifdef STREAMS_MFMA_HOST_MAIN
int main() {
    const int shapes[][5] = {{1, 4, 4, 2, 1}, {33, 12, 36, 31, 2}, {70, 128, 128, 33, 1}, {130, 8, 40, 128, 1},
                             {300, 8, 4, 128, 2}};                              // S, E, H, atoms, n; the last: the workspace path
    uint32_t rng = 4321u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (const auto& sh : shapes) {
        const int s = sh[0], E = sh[1], H = sh[2], atoms = sh[3], n = sh[4];
        const size_t sizes[8] = {(size_t)H * E, (size_t)H, (size_t)atoms * H, (size_t)atoms, (size_t)H * E, (size_t)H, (size_t)atoms * H, (size_t)atoms};
        std::vector<float> eff[8];
        const float* w[8];
        for (int i = 0; i < 8; ++i) {
            eff[i].resize(sizes[i]);
            for (auto& f : eff[i]) f = next() * 0.3f;
            w[i] = eff[i].data();
        }
        std::vector<float> xg((size_t)n * E), x((size_t)n * s * E), z(atoms), obs((size_t)n * s * 5), q((size_t)n * s), v((size_t)n * atoms),
            a((size_t)n * s * atoms);
        std::vector<int64_t> act(n);
        for (auto* t : {&xg, &x}) for (auto& f : *t) f = next();
        for (int k = 0; k < atoms; ++k) z[k] = -1.0f + 9.0f * k / (atoms - 1);
        for (size_t i = 0; i < obs.size(); ++i) obs[i] = (i % 5 == 4 && (i / 5) % 3 == 0) ? 0.0f : 1.0f;
        for (int generic = 0; generic < 2; ++generic) {
            if (host_streams_act_mfma(w, E, H, atoms, xg.data(), E, x.data(), (long long)s * E, E, z.data(), obs.data(), s * 5, s, n,
                                      act.data(), q.data(), s, v.data(), a.data(), generic))
                return 1;
            const bool fits = irbpp::dueling_tile_rows(s, atoms) == s;
            if (host_streams_act_mfma(w, E, H, atoms, xg.data(), E, x.data(), (long long)s * E, E, z.data(), nullptr, 0, s, n, act.data(),
                                      nullptr, 0, nullptr, fits ? nullptr : a.data(), generic))
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
