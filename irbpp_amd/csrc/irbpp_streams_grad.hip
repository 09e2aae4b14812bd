// irbpp_streams_grad.hip -- the backward of the four NoisyLinear layers of the value and advantage streams (model.py:393-394) for
// Agent.learn's online forward: from the gradients of the logits to the gradients of the embeddings and of the sixteen
// parameter tensors.  The forward is irbpp_streams.hip's, launched unchanged; nothing of that file is used here but the limits
// of irbpp_head.h.
//
// Defined float32 arithmetic (tests/test_streams_grad_cpu.py restates it and the kernels are held to it bit for bit).  With
// x [B][S][E], xg [B][E], the effective W, b of irbpp_streams.hip, ga [B][S][A], gv [B][A]:
//   pa[b][s][j] = lin(W_ha, b_ha, x[b][s])[j], ha = relu(pa); pv[b][j] = lin(W_hv, b_hv, xg[b])[j], hv = relu(pv)   (the forward's chains)
//   e[b][s][j]  = +0; for t ascending: e = fmaf(ga[b][s][t], W_za[t][j], e);   d[b][s][j] = pa[b][s][j] > 0 ? e : +0
//   dx[b][s][k] = +0; for j ascending: dx = fmaf(d[b][s][j], W_ha[j][k], dx)
//   P_za[b][t][j] = +0; for s ascending: fmaf(ga[b][s][t], ha[b][s][j], .);   P_ha[b][j][k] likewise with d[b][s][j], x[b][s][k]
//   Pb_za[b][t] = +0; for s ascending: += ga[b][s][t];   Pb_ha[b][j] likewise with d[b][s][j]                      (plain adds)
//   dW_za = +0; for b ascending: += P_za[b] (plain adds); dW_ha, db_za, db_ha likewise
//   e_v, d_v, dxg as e, d, dx with gv, W_zv, pv, W_hv;  dW_zv[t][j] = +0; for b ascending: fmaf(gv[b][t], hv[b][j], .);
//   dW_hv[j][k] likewise with d_v[b][j], xg[b][k];  db_zv[t] = sum_b gv[b][t], db_hv[j] = sum_b d_v[b][j]         (plain adds)
//   grad mu = dW (db); grad sigma = dW * eps (db * bias_eps), one rounding
// The side of the relu is read from the bits of pa (the library is built with -fno-honor-nans, under which a comparison need
// not reject a NaN).  Every chain is walked by one thread in the order written; nothing is split over lanes or re-associated;
// no atomics.  Which rows share a staging trip is no part of the result: a chain over s is carried from trip to trip through
// the workspace, a float32 store and load, which changes no bit.
//
// Layout.  irbpp_streams_grad_value_kernel: a workgroup per sample, thread j for the hidden unit (pv, e_v, d_v), then thread k
// for dxg; hv[b] and d_v[b] go to the workspace.  irbpp_streams_grad_rows_kernel: a workgroup of 512 threads per sample, its
// rows staged through LDS STREAMS_GRAD_ROWS at a time (x, ga, then ha and d beside them; row pitches a multiple of four floats
// plus four, so that the 16-byte reads of consecutive rows fall into different banks).  Thread (s, g) = (tid & 31, tid >> 5)
// walks, four hidden units at a time, their pa chains over k (x from LDS, four rows of W_ha) and their e chains over t (four
// contiguous W_za elements per t), then, four k at a time, the dx chains over j.  After a barrier the threads take 4 x 4 tiles
// of P_ha and P_za: per row two 16-byte LDS reads feed sixteen chains, which go on from the workspace's value (+0 in the first
// trip) and return there.  irbpp_streams_grad_reduce_kernel: a thread per parameter element -- the sums over b of the
// advantage stream's partials, the value stream's chains over b, the products with epsilon, all sixteen tensors.
#include "irbpp_head.h"

#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

constexpr int STREAMS_GRAD_MAX_WIDTH = 256;              // E and H: irbpp_streams.hip's STREAMS_MAX_WIDTH
constexpr int STREAMS_GRAD_MAX_BATCH = 1024;
constexpr int STREAMS_GRAD_THREADS = 512;
constexpr int STREAMS_GRAD_ROWS = 32;                    // rows per staging trip
constexpr int STREAMS_GRAD_VALUE_THREADS = 256;          // a thread per hidden unit, then per embedding

struct alignas(16) StreamsGradVec4 { float f[4]; };

struct StreamsGradArgs {
    long long xg_stride, env_stride, row_stride;
    int embed, hidden, atoms, s_rows, batch;
    int w_ha_vec4, w_za_vec4;                            // E (H) a multiple of 4 and the array on a 16-byte boundary
};

// the parameter gradients of one stream's two layers (NULL: not wanted) and the layers' epsilon (NULL: eval mode)
struct StreamsGradOut {
    float *h_w_mu, *h_w_sigma, *h_b_mu, *h_b_sigma, *z_w_mu, *z_w_sigma, *z_b_mu, *z_b_sigma;
    const float *h_w_eps, *h_b_eps, *z_w_eps, *z_b_eps;
};

// floats of workspace per sample: P_ha [H][E], P_za [A][H], Pb_ha [H], Pb_za [A], then hv [H] and d_v [H]
__host__ __device__ constexpr long long streams_grad_sample_floats(int E, int H, int A) {
    return (long long)H * E + (long long)A * H + H + A + 2LL * H;
}

__host__ __device__ constexpr int streams_grad_pitch(int n) { return ((n + 3) & ~3) + 4; }

// dynamic LDS of the rows kernel: x, ga, ha and d of STREAMS_GRAD_ROWS rows
__host__ __device__ constexpr size_t streams_grad_lds_bytes(int E, int H, int A) {
    return (size_t)STREAMS_GRAD_ROWS * (streams_grad_pitch(E) + streams_grad_pitch(A) + 2 * streams_grad_pitch(H)) * sizeof(float);
}

// s > 0, from the bits: (+0, +inf]
__device__ __forceinline__ bool streams_grad_positive(float s) {
    uint32_t b;
    memcpy(&b, &s, 4);
    return b - 1u < 0x7f800000u;
}

// w[c] = row[i0 + c] for c < 4: one 16-byte load where vec4 allows it, else element by element with the index held below n
// (an element past the end repeats the last one; its chain is never stored)
__device__ __forceinline__ StreamsGradVec4 streams_grad_load4(const float* __restrict__ row, int i0, int n, bool vec4) {
    StreamsGradVec4 w;
    if (vec4) {
        w = *(const StreamsGradVec4*)(row + i0);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) w.f[c] = row[i0 + c < n ? i0 + c : n - 1];
    }
    return w;
}

// The value stream of sample b: dxg[b] (may be NULL), and hv[b], d_v[b] into the workspace
extern "C" __global__ void __launch_bounds__(STREAMS_GRAD_VALUE_THREADS)
irbpp_streams_grad_value_kernel(const float* __restrict__ w_hv, const float* __restrict__ b_hv, const float* __restrict__ w_zv,
                                const float* __restrict__ xg, const float* __restrict__ gv, float* __restrict__ ws,
                                float* __restrict__ dxg, StreamsGradArgs g) {
    __shared__ float sx[STREAMS_GRAD_MAX_WIDTH], sd[STREAMS_GRAD_MAX_WIDTH], sg[HEAD_MAX_ATOMS];
    const int tid = threadIdx.x, E = g.embed, H = g.hidden, A = g.atoms;
    const size_t b = blockIdx.x;
    if (tid < E) sx[tid] = xg[b * g.xg_stride + tid];
    if (tid < A) sg[tid] = gv[b * A + tid];
    __syncthreads();
    float* wsb = ws + b * streams_grad_sample_floats(E, H, A) + (size_t)H * E + (size_t)A * H + H + A;
    if (tid < H) {
        const float* wr = w_hv + (size_t)tid * E;
        float pv = b_hv[tid];
        for (int k = 0; k < E; ++k) pv = fmaf(sx[k], wr[k], pv);
        float e = 0.0f;
        for (int t = 0; t < A; ++t) e = fmaf(sg[t], w_zv[(size_t)t * H + tid], e);
        const bool on = streams_grad_positive(pv);
        const float d = on ? e : 0.0f;
        sd[tid] = d;
        wsb[tid] = on ? pv : 0.0f;
        wsb[H + tid] = d;
    }
    __syncthreads();
    if (dxg && tid < E) {
        float acc = 0.0f;
        for (int j = 0; j < H; ++j) acc = fmaf(sd[j], w_hv[(size_t)j * E + tid], acc);
        dxg[b * E + tid] = acc;
    }
}

// The advantage stream of sample b: dx[b] (may be NULL) and the sample's four partials into the workspace
extern "C" __global__ void __launch_bounds__(STREAMS_GRAD_THREADS)
irbpp_streams_grad_rows_kernel(const float* __restrict__ w_ha, const float* __restrict__ b_ha, const float* __restrict__ w_za,
                               const float* __restrict__ x, const float* __restrict__ ga, float* __restrict__ ws,
                               float* __restrict__ dx, StreamsGradArgs g) {
    HIP_DYNAMIC_SHARED(float, streams_grad_lds)
    const int tid = threadIdx.x, E = g.embed, H = g.hidden, A = g.atoms, S = g.s_rows;
    const int px = streams_grad_pitch(E), ph = streams_grad_pitch(H), pg = streams_grad_pitch(A);
    float* xs = streams_grad_lds;                        // [ROWS][px]
    float* gs = xs + STREAMS_GRAD_ROWS * px;             // [ROWS][pg]
    float* hs = gs + STREAMS_GRAD_ROWS * pg;             // [ROWS][ph]: ha
    float* ds = hs + STREAMS_GRAD_ROWS * ph;             // [ROWS][ph]: d
    const size_t b = blockIdx.x;
    const float* xb = x + b * g.env_stride;
    const float* gb = ga + b * (size_t)S * A;
    float* p_ha = ws + b * streams_grad_sample_floats(E, H, A);
    float* p_za = p_ha + (size_t)H * E;
    float* pb_ha = p_za + (size_t)A * H;
    float* pb_za = pb_ha + H;
    const bool ha4 = g.w_ha_vec4 != 0, za4 = g.w_za_vec4 != 0;
    const int s = tid & (STREAMS_GRAD_ROWS - 1), grp = tid / STREAMS_GRAD_ROWS;
    constexpr int GROUPS = STREAMS_GRAD_THREADS / STREAMS_GRAD_ROWS;

    for (int i = tid; i < STREAMS_GRAD_ROWS * ph; i += STREAMS_GRAD_THREADS) hs[i] = 0.0f, ds[i] = 0.0f;   // the pitch's tail stays +0

    for (int s0 = 0; s0 < S; s0 += STREAMS_GRAD_ROWS) {
        const int nr = S - s0 < STREAMS_GRAD_ROWS ? S - s0 : STREAMS_GRAD_ROWS;
        for (int i = tid; i < nr * px; i += STREAMS_GRAD_THREADS) {
            const int r = i / px, k = i - r * px;
            xs[i] = k < E ? xb[(size_t)(s0 + r) * g.row_stride + k] : 0.0f;
        }
        for (int i = tid; i < nr * pg; i += STREAMS_GRAD_THREADS) {
            const int r = i / pg, k = i - r * pg;
            gs[i] = k < A ? gb[(size_t)(s0 + r) * A + k] : 0.0f;
        }
        __syncthreads();

        if (s < nr) {
            const float* xr = xs + s * px;
            const float* gr = gs + s * pg;
            const int e4 = ha4 ? E : 0;
            for (int j0 = grp * 4; j0 < H; j0 += GROUPS * 4) {
                const float* wr[4];
                float pa[4], e[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int j = j0 + c < H ? j0 + c : H - 1;       // past the end: a row that exists, its result unused
                    wr[c] = w_ha + (size_t)j * E;
                    pa[c] = b_ha[j];
                    e[c] = 0.0f;
                }
                for (int k = 0; k < e4; k += 4) {
                    const StreamsGradVec4 xk = *(const StreamsGradVec4*)(xr + k);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const StreamsGradVec4 w = *(const StreamsGradVec4*)(wr[c] + k);
#pragma unroll
                        for (int q = 0; q < 4; ++q) pa[c] = fmaf(xk.f[q], w.f[q], pa[c]);
                    }
                }
                for (int k = e4; k < E; ++k) {
                    const float xk = xr[k];
#pragma unroll
                    for (int c = 0; c < 4; ++c) pa[c] = fmaf(xk, wr[c][k], pa[c]);
                }
                for (int t = 0; t < A; ++t) {
                    const float gt = gr[t];
                    const StreamsGradVec4 w = streams_grad_load4(w_za + (size_t)t * H, j0, H, za4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) e[c] = fmaf(gt, w.f[c], e[c]);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (j0 + c < H) {
                        const bool on = streams_grad_positive(pa[c]);
                        hs[s * ph + j0 + c] = on ? pa[c] : 0.0f;
                        ds[s * ph + j0 + c] = on ? e[c] : 0.0f;
                    }
                }
            }
        }
        __syncthreads();

        if (dx && s < nr) {
            const float* dr = ds + s * ph;
            float* dst = dx + (b * S + s0 + s) * (size_t)E;
            for (int k0 = grp * 4; k0 < E; k0 += GROUPS * 4) {
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int j = 0; j < H; ++j) {
                    const float dj = dr[j];
                    const StreamsGradVec4 w = streams_grad_load4(w_ha + (size_t)j * E, k0, E, ha4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = fmaf(dj, w.f[c], acc[c]);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (k0 + c < E) dst[k0 + c] = acc[c];
            }
        }

        // the partials' chains over the trip's rows, 4 x 4 per thread: P_ha[j][k] from (d, x), P_za[t][j] from (ga, ha)
        const int jt_n = (H + 3) >> 2, kt_n = (E + 3) >> 2, tt_n = (A + 3) >> 2;
        const int n_ha = jt_n * kt_n, n_all = n_ha + tt_n * jt_n;
        for (int q = tid; q < n_all; q += STREAMS_GRAD_THREADS) {
            const bool first = q < n_ha;
            const int qq = first ? q : q - n_ha;
            const int cols_t = first ? kt_n : jt_n;
            const int r0 = (qq / cols_t) * 4, c0 = (qq - (qq / cols_t) * cols_t) * 4;
            const int n_r = first ? H : A, n_c = first ? E : H;
            const float* left = first ? ds : gs;
            const float* right = first ? xs : hs;
            const int pl = first ? ph : pg, pr = first ? px : ph;
            float* dst = first ? p_ha : p_za;
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[i][c] = (s0 > 0 && r0 + i < n_r && c0 + c < n_c) ? dst[(size_t)(r0 + i) * n_c + c0 + c] : 0.0f;
            for (int r = 0; r < nr; ++r) {
                const StreamsGradVec4 l = *(const StreamsGradVec4*)(left + r * pl + r0);
                const StreamsGradVec4 m = *(const StreamsGradVec4*)(right + r * pr + c0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(l.f[i], m.f[c], acc[i][c]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (r0 + i < n_r && c0 + c < n_c) dst[(size_t)(r0 + i) * n_c + c0 + c] = acc[i][c];
        }
        if (tid < H) {
            float acc = s0 > 0 ? pb_ha[tid] : 0.0f;
            for (int r = 0; r < nr; ++r) acc = acc + ds[r * ph + tid];
            pb_ha[tid] = acc;
        }
        if (tid >= STREAMS_GRAD_THREADS - A) {
            const int t = tid - (STREAMS_GRAD_THREADS - A);
            float acc = s0 > 0 ? pb_za[t] : 0.0f;
            for (int r = 0; r < nr; ++r) acc = acc + gs[r * pg + t];
            pb_za[t] = acc;
        }
        __syncthreads();
    }
}

// mu = v, sigma = v * eps, where wanted
__device__ __forceinline__ void streams_grad_emit(float v, long long i, float* __restrict__ mu, float* __restrict__ sigma,
                                                  const float* __restrict__ eps) {
    if (mu) mu[i] = v;
    if (sigma && eps) sigma[i] = v * eps[i];
}

// One thread per element of [H][E], [A][H], [H], [A] of the advantage stream, then of the value stream.  has_a / has_v: the
// stream's workspace was filled (else its gradients are +0).
extern "C" __global__ void __launch_bounds__(256)
irbpp_streams_grad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ xg, const float* __restrict__ gv,
                                 StreamsGradOut oa, StreamsGradOut ov, int has_a, int has_v, StreamsGradArgs g) {
    const int E = g.embed, H = g.hidden, A = g.atoms, B = g.batch;
    const long long n_h = (long long)H * E, n_z = (long long)A * H, per = n_h + n_z + H + A;
    const long long stride = streams_grad_sample_floats(E, H, A);
    long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < per) {                                       // the advantage stream: plain adds over b of the element's partial
        float acc = 0.0f;
        if (has_a)
            for (int b = 0; b < B; ++b) acc = acc + ws[b * stride + t];
        if (t < n_h)
            streams_grad_emit(acc, t, oa.h_w_mu, oa.h_w_sigma, oa.h_w_eps);
        else if (t < n_h + n_z)
            streams_grad_emit(acc, t - n_h, oa.z_w_mu, oa.z_w_sigma, oa.z_w_eps);
        else if (t < n_h + n_z + H)
            streams_grad_emit(acc, t - n_h - n_z, oa.h_b_mu, oa.h_b_sigma, oa.h_b_eps);
        else
            streams_grad_emit(acc, t - n_h - n_z - H, oa.z_b_mu, oa.z_b_sigma, oa.z_b_eps);
        return;
    }
    t -= per;
    if (t >= per) return;
    const float* hv = ws + per;                          // hv[b] at hv + b * stride, d_v[b] H floats further
    float acc = 0.0f;
    if (t < n_h) {
        const int j = (int)(t / E), k = (int)(t - (long long)j * E);
        if (has_v)
            for (int b = 0; b < B; ++b) acc = fmaf(hv[b * stride + H + j], xg[b * g.xg_stride + k], acc);
        streams_grad_emit(acc, t, ov.h_w_mu, ov.h_w_sigma, ov.h_w_eps);
    } else if (t < n_h + n_z) {
        const long long u = t - n_h;
        const int a = (int)(u / H), j = (int)(u - (long long)a * H);
        if (has_v)
            for (int b = 0; b < B; ++b) acc = fmaf(gv[(size_t)b * A + a], hv[b * stride + j], acc);
        streams_grad_emit(acc, u, ov.z_w_mu, ov.z_w_sigma, ov.z_w_eps);
    } else if (t < n_h + n_z + H) {
        const int j = (int)(t - n_h - n_z);
        if (has_v)
            for (int b = 0; b < B; ++b) acc = acc + hv[b * stride + H + j];
        streams_grad_emit(acc, j, ov.h_b_mu, ov.h_b_sigma, ov.h_b_eps);
    } else {
        const int a = (int)(t - n_h - n_z - H);
        if (has_v)
            for (int b = 0; b < B; ++b) acc = acc + gv[(size_t)b * A + a];
        streams_grad_emit(acc, a, ov.z_b_mu, ov.z_b_sigma, ov.z_b_eps);
    }
}

// n floats of +0: dx or dxg of a stream whose gradient is missing
extern "C" __global__ void __launch_bounds__(256) irbpp_streams_grad_zero_kernel(float* __restrict__ dst, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = 0.0f;
}

}  // namespace irbpp

#pragma float_control(pop)
