// Host harness (test infrastructure): the kernels of irbpp_amd/csrc/irbpp_streams_grad.hip run on the CPU, one workgroup at a
// time, its threads in lockstep (lockstep.h).  The kernels' own source is compiled, so the staging trips, the 4 x 4 tiles that
// carry their chains through the workspace, the tails of the widths and the sums over the samples are what the CPU suite
// checks against the numpy definition; fmaf is the C library's (build with -ffp-contract=off).  host_streams_backward repeats
// the launches of irbpp_streams_backward (irbpp_capi.hip) after its argument checks; the rows kernel's dynamic LDS is a heap
// block of exactly the bytes the entry point asks for.
// With -DSTREAMS_GRAD_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the kernels over a few shapes
// with buffers exactly as large as the kernels may touch and prints a checksum.
#include <stdio.h>
#include <string.h>

#include "lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_streams_grad.hip"

extern "C" long long host_streams_backward_workspace(int E, int H, int A, int B) {
    return (long long)B * irbpp::streams_grad_sample_floats(E, H, A) * (long long)sizeof(float);
}

// w: w_hv, b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za (effective); eps: the same eight or NULL; out: the sixteen gradients in the
// order of irbpp_stream_grads (hv, zv, ha, za; weight_mu, weight_sigma, bias_mu, bias_sigma), each may be NULL
extern "C" void host_streams_backward(const float* const* w, const float* const* eps, int E, int H, int A, const float* xg,
                                      long long xg_stride, const float* x, long long env_stride, long long row_stride, const float* ga,
                                      const float* gv, int S, int B, float* ws, float* dx, float* dxg, float* const* out) {
    using namespace irbpp;
    StreamsGradArgs g;
    g.xg_stride = xg_stride, g.env_stride = env_stride, g.row_stride = row_stride;
    g.embed = E, g.hidden = H, g.atoms = A, g.s_rows = S, g.batch = B;
    g.w_ha_vec4 = (E % 4 == 0 && (uintptr_t)w[4] % 16 == 0) ? 1 : 0;
    g.w_za_vec4 = (H % 4 == 0 && (uintptr_t)w[6] % 16 == 0) ? 1 : 0;
    if (gv) {
        lockstep_launch(STREAMS_GRAD_VALUE_THREADS, B, 1, [&] { irbpp_streams_grad_value_kernel(w[0], w[1], w[2], xg, gv, ws, dxg, g); });
    } else if (dxg) {
        const long long n = (long long)B * E;
        lockstep_launch(256, (int)((n + 255) / 256), 1, [&] { irbpp_streams_grad_zero_kernel(dxg, n); });
    }
    if (ga) {
        LockstepLaunch how;
        how.dynamic_lds = (long long)streams_grad_lds_bytes(E, H, A);
        lockstep_launch(STREAMS_GRAD_THREADS, B, 1, [&] { irbpp_streams_grad_rows_kernel(w[4], w[5], w[6], x, ga, ws, dx, g); }, how);
    } else if (dx) {
        const long long n = (long long)B * S * E;
        lockstep_launch(256, (int)((n + 255) / 256), 1, [&] { irbpp_streams_grad_zero_kernel(dx, n); });
    }
    StreamsGradOut ov, oa;
    ov.h_w_mu = out[0], ov.h_w_sigma = out[1], ov.h_b_mu = out[2], ov.h_b_sigma = out[3];
    ov.z_w_mu = out[4], ov.z_w_sigma = out[5], ov.z_b_mu = out[6], ov.z_b_sigma = out[7];
    oa.h_w_mu = out[8], oa.h_w_sigma = out[9], oa.h_b_mu = out[10], oa.h_b_sigma = out[11];
    oa.z_w_mu = out[12], oa.z_w_sigma = out[13], oa.z_b_mu = out[14], oa.z_b_sigma = out[15];
    ov.h_w_eps = eps ? eps[0] : nullptr, ov.h_b_eps = eps ? eps[1] : nullptr, ov.z_w_eps = eps ? eps[2] : nullptr;
    ov.z_b_eps = eps ? eps[3] : nullptr;
    oa.h_w_eps = eps ? eps[4] : nullptr, oa.h_b_eps = eps ? eps[5] : nullptr, oa.z_w_eps = eps ? eps[6] : nullptr;
    oa.z_b_eps = eps ? eps[7] : nullptr;
    const long long elems = 2 * ((long long)H * E + (long long)A * H + H + A);
    lockstep_launch(256, (int)((elems + 255) / 256), 1,
                    [&] { irbpp_streams_grad_reduce_kernel(ws, xg, gv, oa, ov, ga ? 1 : 0, gv ? 1 : 0, g); });
}

#ifdef STREAMS_GRAD_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    const int cases[][5] = {{1, 1, 1, 1, 2}, {2, 3, 3, 5, 3}, {3, 7, 12, 36, 31}, {2, 65, 33, 17, 33}, {1, 33, 256, 256, 128}, {2, 70, 8, 8, 5}};
    uint32_t rng = 9876u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (const auto& cs : cases) {
        const int B = cs[0], S = cs[1], E = cs[2], H = cs[3], A = cs[4];
        const size_t sizes[8] = {(size_t)H * E, (size_t)H, (size_t)A * H, (size_t)A, (size_t)H * E, (size_t)H, (size_t)A * H, (size_t)A};
        std::vector<std::vector<float>> w(8), eps(8), out(16);
        const float* wp[8];
        const float* ep[8];
        float* op[16];
        for (int i = 0; i < 8; ++i) {
            w[i].resize(sizes[i]), eps[i].resize(sizes[i]);
            for (auto& f : w[i]) f = next() * 0.3f;
            for (auto& f : eps[i]) f = next();
            wp[i] = w[i].data(), ep[i] = eps[i].data();
        }
        for (int i = 0; i < 16; ++i) {                       // layer i / 4: its weight (mu, sigma), its bias (mu, sigma)
            out[i].resize(sizes[(i / 4) * 2 + (i % 4) / 2]);
            op[i] = out[i].data();
        }
        // x with a row stride wider than E: the last row ends the buffer
        const long long row_stride = E + 3, env_stride = (long long)S * row_stride + 5, xg_stride = E + 2;
        std::vector<float> x((size_t)(B - 1) * env_stride + (size_t)(S - 1) * row_stride + E), xg((size_t)(B - 1) * xg_stride + E);
        std::vector<float> ga((size_t)B * S * A), gv((size_t)B * A), dx((size_t)B * S * E), dxg((size_t)B * E);
        std::vector<float> ws((size_t)host_streams_backward_workspace(E, H, A, B) / sizeof(float));
        for (auto* t : {&x, &xg, &ga, &gv}) for (auto& f : *t) f = next();
        for (int mode = 0; mode < 4; ++mode) {               // both gradients, one of them, eval mode without dx
            const float* a = mode == 1 ? nullptr : ga.data();
            const float* v = mode == 2 ? nullptr : gv.data();
            host_streams_backward(wp, mode == 3 ? nullptr : ep, E, H, A, xg.data(), xg_stride, x.data(), env_stride, row_stride, a, v, S, B,
                                  ws.data(), mode == 3 ? nullptr : dx.data(), dxg.data(), op);
            for (auto* t : {&dx, &dxg})
                for (float f : *t) {
                    if (f != f) return 3;
                    sum += f;
                }
            for (auto& t : out)
                for (float f : t) {
                    if (f != f) return 4;
                    sum += f;
                }
        }
        printf("B %d S %d E %d H %d A %d: checksum %.9g\n", B, S, E, H, A, sum);
    }
    return 0;
}
#endif
