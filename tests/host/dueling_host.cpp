// Host harness (test infrastructure): the two kernels of irbpp_amd/csrc/irbpp_dueling.hip run on the CPU, one workgroup at a
// time, by 512 threads in lockstep (the workgroup's size; lockstep.h: barriers, shuffles, __shared__ and the dynamic LDS
// tile).  The kernels' own source is compiled,
// so their staging, indexing, reductions and both forms (resident block / staged in chunks) are what the CPU suite checks
// against the numpy definition; float arithmetic is IEEE float32 on both sides (build with -ffp-contract=off).
// With -DDUELING_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs both kernels over a few shapes,
// either form included, and prints a checksum.
#include <stdio.h>

#define LOCKSTEP_TILE_FLOATS (144 * 1024 / 4)
#include "lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_dueling.hip"

static_assert(sizeof g_tile == irbpp::DUELING_TILE_BYTES, "the harness tile is the kernels' dynamic LDS");

extern "C" int host_dueling_tile_rows(int s_rows, int atoms) { return irbpp::dueling_tile_rows(s_rows, atoms); }

extern "C" void host_dueling_act(const float* v, long long v_stride, const float* a, long long env_stride, long long row_stride,
                                 const float* support, int atoms, const float* obs, int obs_stride, int s_rows, int n_env,
                                 int64_t* action, float* q_out, long long q_stride, float* p_out) {
    run_grid<irbpp::DUELING_THREADS>(n_env, 1, [&] {
        irbpp::irbpp_dueling_act_kernel(v, v_stride, a, env_stride, row_stride, support, atoms, obs, obs_stride, s_rows, action, q_out,
                                        q_stride, p_out);
    });
}

extern "C" void host_dueling_target(const float* v_on, long long von_stride, const float* a_on, long long on_env, long long on_row,
                                    const float* v_tg, long long vtg_stride, const float* a_tg, long long tg_env, long long tg_row,
                                    const float* returns, const float* nonterminals, const float* support, int atoms, int s_rows,
                                    int batch, float gamma_n, float v_min, float v_max, float delta_z, float* m, int64_t* a_star) {
    run_grid<irbpp::DUELING_THREADS>(batch, 1, [&] {
        irbpp::irbpp_dueling_target_kernel(v_on, von_stride, a_on, on_env, on_row, v_tg, vtg_stride, a_tg, tg_env, tg_row, returns,
                                           nonterminals, support, atoms, s_rows, gamma_n, v_min, v_max, delta_z, m, a_star);
    });
}

#ifdef DUELING_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    const int shapes[][3] = {{1, 2, 2}, {3, 2, 3}, {65, 31, 2}, {500, 31, 1}, {129, 128, 1}, {300, 128, 2}, {1024, 128, 1}};
    uint32_t rng = 12345u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 8.0f - 4.0f; };
    double sum = 0;
    for (const auto& sh : shapes) {
        const int s = sh[0], atoms = sh[1], n = sh[2];
        std::vector<float> v((size_t)n * atoms), a((size_t)n * s * atoms), v2(v.size()), a2(a.size()), z(atoms), obs((size_t)n * s * 5),
            q((size_t)n * s), p((size_t)n * s * atoms), ret(n), nt(n), m((size_t)n * atoms);
        std::vector<int64_t> act(n), star(n);
        for (auto* x : {&v, &a, &v2, &a2}) for (auto& f : *x) f = next();
        a[0] = 200.0f;                                   // most of that row's e are exactly 0
        for (int k = 0; k < atoms; ++k) z[k] = -1.0f + 9.0f * k / (atoms - 1);
        for (size_t i = 0; i < obs.size(); ++i) obs[i] = (i % 5 == 4 && (i / 5) % 3 == 0) ? 0.0f : 1.0f;
        for (int e = 0; e < n; ++e) { ret[e] = next() * 3; nt[e] = (float)(e & 1); }
        host_dueling_act(v.data(), atoms, a.data(), (long long)s * atoms, atoms, z.data(), atoms, obs.data(), s * 5, s, n, act.data(),
                         q.data(), s, p.data());
        host_dueling_act(v.data(), atoms, a.data(), (long long)s * atoms, atoms, z.data(), atoms, nullptr, 0, s, n, act.data(), nullptr,
                         0, nullptr);
        host_dueling_target(v.data(), atoms, a.data(), (long long)s * atoms, atoms, v2.data(), atoms, a2.data(), (long long)s * atoms,
                            atoms, ret.data(), nt.data(), z.data(), atoms, s, n, 0.97f, -1.0f, 8.0f, 9.0f / (atoms - 1), m.data(),
                            star.data());
        for (int e = 0; e < n; ++e) sum += (double)act[e] + (double)star[e];
        for (float f : q) sum += f;
        for (float f : p) sum += f;
        for (float f : m) sum += f;
        printf("S %d atoms %d n %d tile rows %d: checksum %.9g\n", s, atoms, n, irbpp::dueling_tile_rows(s, atoms), sum);
    }
    return 0;
}
#endif
