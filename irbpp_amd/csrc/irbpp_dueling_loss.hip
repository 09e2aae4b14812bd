// irbpp_dueling_loss.hip -- the part of Agent.learn that carries the gradient, from the network's logits: the end of
// DQNBPP.forward with log=True (model.py:395-398: q = v + a - a.mean(1), log_softmax over the atoms), log_ps[range(B), actions]
// and loss = -sum(m * log_ps_a, 1) (agent.py:85-86, 117) in one launch, and autograd's way back through all of that in a
// second one.  Only row actions[b] of a sample's block enters the loss; the block is read for its column means alone.
// DuelingShared, dueling_mean, dueling_combine, dueling_dexp and the limits are those of irbpp_head.h.
//
// Defined float32 arithmetic (multiply and add separate, -ffp-contract=off; tests/test_dueling_loss_cpu.py restates it in
// numpy and the kernels are held to it bit for bit).  For one sample: v[atoms], a[S][atoms], the action row r, the target
// distribution m[atoms], the upstream gradient w:
//   mean[k] = dueling_mean of irbpp_head.h (16 interleaved partial sums, added left to right, / (float)S)
//   x[k]    = (v[k] + a[r][k]) - mean[k];   mx = max_k x[k];   t[k] = x[k] - mx;   e[k] = dueling_dexp(t[k])
//   den     = ((e[0] + e[1]) + ..) + e[atoms-1]                         in [1, atoms]: the maximum's e is dexp(0) = 1
//   L       = dlog(den);   lp[k] = t[k] - L
//   loss    = -(((m[0] lp[0]) + m[1] lp[1]) + ..)                       every product and sum rounded, ascending k
//   M       = ((m[0] + m[1]) + ..)
//   p[k]    = e[k] / den                                                IEEE division
//   g[k]    = p[k] M - m[k]                                             d loss / d x[k], sum(m) == 1 not assumed
// and backward
//   gw[k]   = w g[k];   grad_v[k] = gw[k];   c[k] = gw[k] / (float)S    IEEE division
//   grad_a[s][k] = gw[k] - c[k] for s == r, -c[k] for every other row.
// An action in [-S, 0) counts from the end, as torch indexing does.  One outside [-S, S) reads and writes nothing out of
// range: loss = NaN, g = 0 (so every gradient of that sample is zero).  Finite logits and a finite non-negative m are the
// contract.  The values are a function of (S, atoms) and the inputs alone: not of the batch, the strides or the grid.
#include "irbpp_head.h"

namespace irbpp {

constexpr int DUELING_LOSS_CHUNK_ROWS = 64;              // rows of grad_a one workgroup of the backward kernel writes

// log(d) for d in [1, 128] in plain float32 operations, the same bits on every IEEE machine: d = 2^n f with f in [1, 2) from
// the bits; f > sqrt(2) is halved (n + 1), so f lies in (0.7071, 1.4143] and |s| <= 0.1716 for s = (f - 1) / (f + 1) (f - 1
// is exact); log f = 2 s (1 + z/3 + z^2/5 + .. + z^5/11) with z = s s, the odd series through s^11 in Horner form (the
// first term left out: 2 atanh(s) 0.1716^12 / 13 < 5e-11 relative); then n LN2_HI + (log f + n LN2_LO) with the split constants
// of dueling_dexp (n LN2_HI is exact).  dlog(1) = 0 exactly; the result is finite and >= 0 on the interval (log f >= -0.3466
// only where n >= 1).  Measured error: profiles/dueling_loss/dlog_sweep.json.
__device__ __forceinline__ float dueling_dlog(float d) {
    uint32_t bits;
    memcpy(&bits, &d, 4);
    int n = (int)(bits >> 23) - 127;
    bits = (bits & 0x007fffffu) | 0x3f800000u;
    float f;
    memcpy(&f, &bits, 4);
    if (f > 1.4142135623730951f) {
        f = f * 0.5f;
        n += 1;
    }
    const float nf = (float)n;
    const float s = (f - 1.0f) / (f + 1.0f);
    const float z = s * s;
    float p = 9.0909090909090912e-02f;                   // 1/11
    p = p * z + 1.1111111111111111e-01f;                 // 1/9
    p = p * z + 1.4285714285714285e-01f;                 // 1/7
    p = p * z + 2.0000000000000001e-01f;                 // 1/5
    p = p * z + 3.3333333333333331e-01f;                 // 1/3
    const float s2 = s + s;
    const float lf = s2 + s2 * (z * p);
    return nf * 0.693145751953125f + (lf + nf * 1.4286068203094172e-06f);
}

// The action's row, sequential in k by definition.  rw: a[r] on entry, g on return; se: scratch for e; sv, smean, sm: LDS
// copies of v, mean and m.  Returns the loss.
__device__ __forceinline__ float dueling_loss_row(float* rw, float* se, const float* sv, const float* smean, const float* sm, int atoms) {
    const float mx = dueling_combine(rw, sv, smean, atoms);
    float den = 0.0f;
    for (int k = 0; k < atoms; ++k) {
        const float t = rw[k] - mx;
        const float e = dueling_dexp(t);
        rw[k] = t;
        se[k] = e;
        den = k ? den + e : e;
    }
    const float L = dueling_dlog(den);
    float loss = sm[0] * (rw[0] - L), M = sm[0];
    for (int k = 1; k < atoms; ++k) {
        loss = loss + sm[k] * (rw[k] - L);
        M = M + sm[k];
    }
    for (int k = 0; k < atoms; ++k) rw[k] = (se[k] / den) * M - sm[k];
    return -loss;
}

// One workgroup per sample: the column means straight from global memory (each element of a read once: the same bits for every
// S, no resident / staged distinction), row r, v and m into LDS, the row by one thread, g out coalesced.
extern "C" __global__ void __launch_bounds__(DUELING_THREADS)
irbpp_dueling_loss_kernel(const float* __restrict__ v, long long v_stride, const float* __restrict__ a, long long env_stride,
                          long long row_stride, const int64_t* __restrict__ actions, const float* __restrict__ m, int atoms,
                          int s_rows, float* __restrict__ loss, float* __restrict__ g) {
    __shared__ DuelingShared sh;                         // sh.z holds m
    __shared__ float srow[HEAD_MAX_ATOMS], se[HEAD_MAX_ATOMS];
    const int smp = blockIdx.x, tid = threadIdx.x;
    long long r = actions[smp];
    if (r < 0) r += s_rows;
    if (r < 0 || r >= s_rows) {                          // the whole workgroup: no barrier is left waiting
        if (tid < atoms) g[(size_t)smp * atoms + tid] = 0.0f;
        if (tid == 0) {
            const uint32_t nan_bits = 0x7fc00000u;
            memcpy(&loss[smp], &nan_bits, 4);
        }
        return;
    }
    const float* ab = a + (size_t)smp * env_stride;
    if (tid < atoms) {
        sh.v[tid] = v[(size_t)smp * v_stride + tid];
        sh.z[tid] = m[(size_t)smp * atoms + tid];
        srow[tid] = ab[(size_t)r * row_stride + tid];
    }
    dueling_mean(ab, row_stride, atoms, s_rows, sh.part, sh.mean);             // ends on a barrier
    if (tid == 0) loss[smp] = dueling_loss_row(srow, se, sh.v, sh.mean, sh.z, atoms);
    __syncthreads();
    if (tid < atoms) g[(size_t)smp * atoms + tid] = srow[tid];
}

// Workgroup (smp, chunk): gw and c of the sample once into LDS as the two values a grad_a element can take, then rows
// chunk * 64 .. of the dense grad_a[smp] with coalesced dword stores (head_walk).  Chunk 0 writes grad_v.  Either output may
// be NULL.
extern "C" __global__ void __launch_bounds__(DUELING_THREADS)
irbpp_dueling_loss_backward_kernel(const float* __restrict__ g, const float* __restrict__ grad_loss,
                                   const int64_t* __restrict__ actions, int atoms, int s_rows, float* __restrict__ grad_v,
                                   float* __restrict__ grad_a) {
    __shared__ float hit[HEAD_MAX_ATOMS], miss[HEAD_MAX_ATOMS];
    const int smp = blockIdx.x, r0 = blockIdx.y * DUELING_LOSS_CHUNK_ROWS, tid = threadIdx.x;
    if (tid < atoms) {
        const float gw = grad_loss[smp] * g[(size_t)smp * atoms + tid];
        const float c = gw / (float)s_rows;
        hit[tid] = gw - c;
        miss[tid] = -c;
        if (grad_v && blockIdx.y == 0) grad_v[(size_t)smp * atoms + tid] = gw;
    }
    if (!grad_a) return;
    __syncthreads();
    long long r = actions[smp];
    if (r < 0) r += s_rows;
    const int hit_row = (r >= r0 && r < r0 + DUELING_LOSS_CHUNK_ROWS) ? (int)(r - r0) : -1;
    const int nrows = s_rows - r0 < DUELING_LOSS_CHUNK_ROWS ? s_rows - r0 : DUELING_LOSS_CHUNK_ROWS;
    float* dst = grad_a + ((size_t)smp * s_rows + r0) * atoms;
    head_walk<DUELING_THREADS>(atoms, nrows, [&](int row, int k, int e) { dst[e] = row == hit_row ? hit[k] : miss[k]; });
}

}  // namespace irbpp
