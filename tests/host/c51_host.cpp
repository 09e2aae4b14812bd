// Host harness (test infrastructure): the two kernels of irbpp_amd/csrc/irbpp_c51.hip run on the CPU, one workgroup at a
// time, by 64 threads in lockstep (lockstep.h: barriers, shuffles, __shared__ and the dynamic LDS tile).  The kernels'
// own source is compiled, so their indexing, staging and reduction are what the CPU suite checks against the numpy
// definition; float arithmetic is IEEE float32 on both sides (build with -ffp-contract=off).
#define LOCKSTEP_TILE_FLOATS (64 * 129)
#include "lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_c51.hip"

extern "C" void host_c51_act(const float* p, long long env_stride, long long row_stride, const float* support, int atoms,
                             const float* obs, int obs_stride, int s_rows, int n_env, int64_t* action, float* q_out,
                             long long q_stride) {
    run_grid<64>(n_env, 1, [&] {
        irbpp::irbpp_c51_act_kernel(p, env_stride, row_stride, support, atoms, obs, obs_stride, s_rows, action, q_out, q_stride);
    });
}

extern "C" void host_c51_target(const float* p_on, long long on_env, long long on_row, const float* p_tg, long long tg_env,
                                long long tg_row, const float* returns, const float* nonterminals, const float* support,
                                int atoms, int s_rows, int batch, float gamma_n, float v_min, float v_max, float delta_z, float* m,
                                int64_t* a_star) {
    run_grid<64>(batch, 1, [&] {
        irbpp::irbpp_c51_target_kernel(p_on, on_env, on_row, p_tg, tg_env, tg_row, returns, nonterminals, support, atoms, s_rows,
                                       gamma_n, v_min, v_max, delta_z, m, a_star);
    });
}
