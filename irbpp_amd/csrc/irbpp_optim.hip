// irbpp_optim.hip -- the optimiser step of Agent.learn: clip_grad_norm_(online_net.parameters(), norm_clip) and
// optim.Adam's step (agent.py:120-121, 44), the next step's zero_grad and update_target_net's parameter copy (agent.py:127-128),
// in two launches over all parameter tensors at once.  No floating-point atomics, no grid-wide synchronisation: the second
// kernel's workgroups each add the first kernel's partial sums themselves, in one fixed order, and so hold the same bits.
//
// Defined arithmetic (tests/test_clipped_adam_cpu.py restates it in numpy and the kernels are held to it bit for bit).
// float32 unless stated; multiply and add separate (-ffp-contract=off) unless written fmaf; float32 denormals are kept.
// T tensors p_i with gradient g_i and moments m_i, v_i; hyper-parameters as irbpp_adam_hyper carries them.
//
// Chunks.  Every tensor is cut into chunks of 1024 elements, its last chunk short; chunk c is (tensor, first element).
//
// Norm, in float64 (the square of a float32 is exact there).  Thread t (0 .. 255) of chunk c takes the elements
// first + 4t + j, j = 0 .. 3, and adds their squares in ascending j:  s_t = ((q0 + q1) + q2) + q3, a position past the
// tensor's end giving q = +0.0.  A wave of 64 threads is reduced by the butterfly  s = s + s[lane ^ o]  for
// o = 1, 2, 4, 8, 16, 32 in this order (every lane then holds the wave's sum; IEEE addition is commutative, so the two
// partners of an exchange hold the same bits).  The four waves' sums are joined as  partial[c] = ((w0 + w1) + w2) + w3.
// The C partial sums are added in the same shape: thread t takes partial[t], partial[t + 256], partial[t + 512], .. in
// ascending order (+0.0 if it has none), then the same butterfly and the same join of four waves give `sum`.
//   nonfinite = the exponent field of sum is all ones (tested on the bits: the library is built with -fno-honor-nans)
//   total = (float)sqrt(sum);  if nonfinite, total is the bit pattern 0x7fc00000 where sum's mantissa field is not zero, else +inf
//   coef  = max_norm / (total + 1e-6f), replaced by 1.0f unless coef < 1.0f
// Non-finite norm: the step is skipped.  Parameters, moments, gradients and targets stay bit for bit as they were, total is
// written, and *skipped goes up by one.
//
// Update, per element (step_size = (float)(lr / (1 - beta1^t)) and rsq = (float)sqrt(1 - beta2^t) are computed by the host in
// float64 and rounded once; one_minus_beta1 and one_minus_beta2 are float32 values of the host's):
//   g = g * coef
//   m = fmaf(one_minus_beta1, g - m, m)
//   v = fmaf(g * g, one_minus_beta2, v * beta2)
//   d = sqrtf(v) / rsq + eps                 correctly rounded square root and division
//   p = fmaf(-step_size, m / d, p)
// Stores: p, m, v; with WRITE_GRADS the clipped g, with ZERO_GRADS 0.0f in its place, with neither the gradient is left as it
// was; with SYNC_TARGET the new p also to the tensor's target, where it has one.  CLIP_ONLY: g = g * coef is stored and
// nothing else is read or written (clip_grad_norm_ alone).
//
// Memory access: a thread whose four elements all exist takes them as one 16-byte load / store per array where every array's
// base of the tensor is 16-byte aligned (a chunk's first element is a multiple of 1024), and as dwords otherwise; the
// arithmetic per element is the same either way.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/irbpp.h"

namespace irbpp {

constexpr int OPTIM_THREADS = 256;
constexpr int OPTIM_PER_THREAD = 4;
constexpr int OPTIM_CHUNK = OPTIM_THREADS * OPTIM_PER_THREAD;     // 1024 elements

// The 256 threads' values to one: the butterfly within each wave, then ((w0 + w1) + w2) + w3 by every thread from LDS, so
// the whole workgroup returns the same bits.  Ends after a barrier; `waves` may be reused after the next one.
__device__ __forceinline__ double optim_block_sum(double s, double* waves) {
    for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) waves[tid >> 6] = s;
    __syncthreads();
    return ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

__device__ __forceinline__ bool optim_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ double optim_square(float x) { return (double)x * (double)x; }

// One 256-thread workgroup per chunk: partial[c] = the chunk's sum of squares in float64, by the order of the header.
extern "C" __global__ void __launch_bounds__(OPTIM_THREADS)
irbpp_grad_sumsq_kernel(const irbpp_optim_tensor* __restrict__ tensors, const int32_t* __restrict__ chunks,
                        double* __restrict__ partial) {
    __shared__ double waves[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const irbpp_optim_tensor t = tensors[chunks[2 * c]];
    const int64_t e0 = (int64_t)chunks[2 * c + 1] + OPTIM_PER_THREAD * tid;
    const float* g = t.grad + e0;
    double s;
    if (e0 + OPTIM_PER_THREAD <= t.numel && optim_aligned16(t.grad)) {
        const float4 x = *reinterpret_cast<const float4*>(g);
        s = ((optim_square(x.x) + optim_square(x.y)) + optim_square(x.z)) + optim_square(x.w);
    } else {
        double q[OPTIM_PER_THREAD];
        for (int j = 0; j < OPTIM_PER_THREAD; ++j) q[j] = e0 + j < t.numel ? optim_square(g[j]) : 0.0;
        s = ((q[0] + q[1]) + q[2]) + q[3];
    }
    s = optim_block_sum(s, waves);
    if (tid == 0) partial[c] = s;
}

struct OptimElement {
    float p, g, m, v;
};

// the update of the header for one element
__device__ __forceinline__ void optim_adam_element(OptimElement& e, float coef, const irbpp_adam_hyper& h) {
    e.g = e.g * coef;
    e.m = fmaf(h.one_minus_beta1, e.g - e.m, e.m);
    e.v = fmaf(e.g * e.g, h.one_minus_beta2, e.v * h.beta2);
    const float d = sqrtf(e.v) / h.rsq + h.eps;
    e.p = fmaf(-h.step_size, e.m / d, e.p);
}

// One workgroup per chunk: the C partial sums once more by every workgroup, coef, then the chunk's update.
extern "C" __global__ void __launch_bounds__(OPTIM_THREADS)
irbpp_clipped_adam_kernel(const irbpp_optim_tensor* __restrict__ tensors, const int32_t* __restrict__ chunks,
                          const double* __restrict__ partial, int n_chunks, irbpp_adam_hyper h, float* __restrict__ total_out,
                          long long* __restrict__ skipped) {
    __shared__ double waves[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n_chunks; i += OPTIM_THREADS) s = s + partial[i];
    const double sum = optim_block_sum(s, waves);
    uint64_t bits;
    memcpy(&bits, &sum, 8);
    const bool nonfinite = ((bits >> 52) & 0x7ffu) == 0x7ffu;
    float total = (float)sqrt(sum);
    if (nonfinite) {
        const uint32_t tb = (bits & 0x000fffffffffffffull) ? 0x7fc00000u : 0x7f800000u;
        memcpy(&total, &tb, 4);
    }
    if (c == 0 && tid == 0) {
        *total_out = total;
        if (nonfinite) *skipped = *skipped + 1;
    }
    if (nonfinite) return;
    float coef = h.max_norm / (total + 1e-6f);
    if (!(coef < 1.0f)) coef = 1.0f;

    const irbpp_optim_tensor t = tensors[chunks[2 * c]];
    const int64_t e0 = (int64_t)chunks[2 * c + 1] + OPTIM_PER_THREAD * tid;
    if (e0 >= t.numel) return;
    const bool clip_only = h.flags & IRBPP_ADAM_CLIP_ONLY;
    const bool write_g = h.flags & (IRBPP_ADAM_WRITE_GRADS | IRBPP_ADAM_CLIP_ONLY), zero_g = h.flags & IRBPP_ADAM_ZERO_GRADS;
    float* target = (h.flags & IRBPP_ADAM_SYNC_TARGET) && !clip_only ? t.target : nullptr;
    const bool full = e0 + OPTIM_PER_THREAD <= t.numel;
    if (clip_only) {
        if (full && optim_aligned16(t.grad)) {
            float4 g = *reinterpret_cast<const float4*>(t.grad + e0);
            g.x = g.x * coef, g.y = g.y * coef, g.z = g.z * coef, g.w = g.w * coef;
            *reinterpret_cast<float4*>(t.grad + e0) = g;
        } else {
            for (int j = 0; j < OPTIM_PER_THREAD; ++j)
                if (e0 + j < t.numel) t.grad[e0 + j] = t.grad[e0 + j] * coef;
        }
        return;
    }
    if (full && optim_aligned16(t.param) && optim_aligned16(t.grad) && optim_aligned16(t.exp_avg) && optim_aligned16(t.exp_avg_sq) &&
        optim_aligned16(target)) {
        const float4 p4 = *reinterpret_cast<const float4*>(t.param + e0), g4 = *reinterpret_cast<const float4*>(t.grad + e0);
        const float4 m4 = *reinterpret_cast<const float4*>(t.exp_avg + e0), v4 = *reinterpret_cast<const float4*>(t.exp_avg_sq + e0);
        OptimElement e[OPTIM_PER_THREAD] = {{p4.x, g4.x, m4.x, v4.x}, {p4.y, g4.y, m4.y, v4.y}, {p4.z, g4.z, m4.z, v4.z},
                                            {p4.w, g4.w, m4.w, v4.w}};
        for (int j = 0; j < OPTIM_PER_THREAD; ++j) optim_adam_element(e[j], coef, h);
        const float4 po = make_float4(e[0].p, e[1].p, e[2].p, e[3].p);
        *reinterpret_cast<float4*>(t.param + e0) = po;
        *reinterpret_cast<float4*>(t.exp_avg + e0) = make_float4(e[0].m, e[1].m, e[2].m, e[3].m);
        *reinterpret_cast<float4*>(t.exp_avg_sq + e0) = make_float4(e[0].v, e[1].v, e[2].v, e[3].v);
        if (zero_g) *reinterpret_cast<float4*>(t.grad + e0) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else if (write_g) *reinterpret_cast<float4*>(t.grad + e0) = make_float4(e[0].g, e[1].g, e[2].g, e[3].g);
        if (target) *reinterpret_cast<float4*>(target + e0) = po;
        return;
    }
    for (int j = 0; j < OPTIM_PER_THREAD; ++j) {
        const int64_t i = e0 + j;
        if (i >= t.numel) break;
        OptimElement e = {t.param[i], t.grad[i], t.exp_avg[i], t.exp_avg_sq[i]};
        optim_adam_element(e, coef, h);
        t.param[i] = e.p;
        t.exp_avg[i] = e.m;
        t.exp_avg_sq[i] = e.v;
        if (zero_g) t.grad[i] = 0.0f;
        else if (write_g) t.grad[i] = e.g;
        if (target) target[i] = e.p;
    }
}

}  // namespace irbpp
