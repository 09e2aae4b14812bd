// irbpp_mfma_chain.h -- the library's defined linear layer, acc = b[j]; acc = fmaf(x[k], W[j][k], acc) for k ascending, on the
// matrix cores.  v_mfma_f32_32x32x2_f32 (float32 in, float32 accumulate) computes, for every element of its 32 x 32 result,
// D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)): one rounding per product, nothing accumulated wider, subnormals kept.  A product
// "C (preloaded with the bias) += A B" whose k-steps are issued in ascending order is therefore the chain of the definition,
// bit for bit, as long as K itself is never padded (a zero product would turn a -0.0 accumulator into +0.0); padded rows and
// columns are computed and thrown away.  tests/test_gpu_streams_mfma.py holds the hardware to that claim.
//
// This is the one place that knows the lane maps of the instruction (wave of 64 lanes, lane l, col = l & 31, half = l >> 5):
//   A operand (32 x 2): one float per lane, A[row = col][k = half];   B operand (2 x 32): one float per lane, B[k = half][col]
//   C / D (32 x 32):    16 floats per lane, register g is D[row = (g & 3) + 8 (g >> 2) + 4 half][col]
// Written for reuse: irbpp_streams_mfma.hip is the first user, irbpp_embed_mfma.hip (the row part of the embedding stage, whose
// chains start from a bias or from `base` and hand over through LDS) the second; tests/test_gpu_embed_mfma.py holds it too.
// irbpp_order_embed_mfma.hip (the order network's eight layers: chains started from a `base` per column, from a bias and from
// +0.0) is the third, held by tests/test_gpu_order_embed_mfma.py.
// The instruction sits behind mfma_32x32x2 alone; a host build defines IRBPP_MFMA_CHAIN_SHIM and supplies
// lockstep_mfma_32x32x2(a, b, float c[16]) in its place (tests/host/mfma_shim.h).
#pragma once
#include <hip/hip_runtime.h>

namespace irbpp {

constexpr int MFMA_TILE = 32;                            // rows and columns of a result tile
constexpr int MFMA_ACC = 16;                             // accumulator registers per lane

struct MfmaAcc { float r[MFMA_ACC]; };
struct alignas(16) MfmaVec4 { float f[4]; };

__device__ __forceinline__ int mfma_lane() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ int mfma_col(int lane) { return lane & 31; }
__device__ __forceinline__ int mfma_half(int lane) { return lane >> 5; }
__device__ __forceinline__ int mfma_acc_row(int g, int half) { return (g & 3) + 8 * (g >> 2) + 4 * half; }

// c += A B for one k-step of two: a = A[col][k0 + half], b = B[k0 + half][col]; k0 before k0 + 1 in every element's chain
#ifdef IRBPP_MFMA_CHAIN_SHIM
__device__ __forceinline__ void mfma_32x32x2(float a, float b, MfmaAcc& c) { lockstep_mfma_32x32x2(a, b, c.r); }
#else
__device__ __forceinline__ void mfma_32x32x2(float a, float b, MfmaAcc& c) {
    typedef float v16 __attribute__((ext_vector_type(16)));
    v16 v;
#pragma unroll
    for (int g = 0; g < MFMA_ACC; ++g) v[g] = c.r[g];
    v = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, v, 0, 0, 0);
#pragma unroll
    for (int g = 0; g < MFMA_ACC; ++g) c.r[g] = v[g];
}
#endif

// four consecutive floats at p: one 16-byte load where the caller knows p to be aligned, else four loads
__device__ __forceinline__ MfmaVec4 mfma_load4(const float* __restrict__ p, bool aligned) {
    if (aligned) return *(const MfmaVec4*)p;
    MfmaVec4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) v.f[c] = p[c];
    return v;
}

// C = the bias: row i of the tile starts its chains from bias[row0 + i]; rows at or past `rows` take the last one that exists
// (their results are thrown away)
__device__ __forceinline__ void mfma_chain_bias(MfmaAcc& c, const float* __restrict__ bias, int row0, int rows, int half) {
#pragma unroll
    for (int g = 0; g < MFMA_ACC; ++g) {
        const int i = row0 + mfma_acc_row(g, half);
        c.r[g] = bias[i < rows ? i : rows - 1];
    }
}

// C = a start of its own per column (a lane holds one column of the tile): row i of the lane's column starts its chain from
// start_col[row0 + i], start_col the lane's own pointer; rows at or past `rows` take the last one that exists (thrown away)
__device__ __forceinline__ void mfma_chain_col_start(MfmaAcc& c, const float* start_col, int row0, int rows, int half) {
#pragma unroll
    for (int g = 0; g < MFMA_ACC; ++g) {
        const int i = row0 + mfma_acc_row(g, half);
        c.r[g] = start_col[i < rows ? i : rows - 1];
    }
}

// C = +0.0: chains without a bias
__device__ __forceinline__ void mfma_chain_zero(MfmaAcc& c) {
#pragma unroll
    for (int g = 0; g < MFMA_ACC; ++g) c.r[g] = 0.0f;
}

// four steps of k, ascending, as two instructions: a4 = A[col][k .. k + 3] and b4 = B[k .. k + 3][col], the same four in
// both lane halves; half 0 feeds k and k + 2, half 1 k + 1 and k + 3
__device__ __forceinline__ void mfma_chain_k4(MfmaAcc& c, const MfmaVec4& a4, const MfmaVec4& b4, int half) {
    mfma_32x32x2(half ? a4.f[1] : a4.f[0], half ? b4.f[1] : b4.f[0], c);
    mfma_32x32x2(half ? a4.f[3] : a4.f[2], half ? b4.f[3] : b4.f[2], c);
}

// A result tile X as the B operand of a following product that sums over X's ROW index, rows ascending: a lane half owns
// rows 0-3, 8-11, ... (half 0) or 4-7, 12-15, ... (half 1) of its column, and k-step s needs row 2 s in half 0 and row
// 2 s + 1 in half 1, so every second operand comes from the other half's lane of the same column (lane ^ 32).
// -> b[s], s = 0 .. 15: this lane's B operand of the step that covers rows 2 s and 2 s + 1 of X.
__device__ __forceinline__ void mfma_acc_as_b(const MfmaAcc& x, int half, float (&b)[MFMA_ACC]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {                            // rows 8 q .. 8 q + 7
        const float r0 = x.r[4 * q], r1 = x.r[4 * q + 1], r2 = x.r[4 * q + 2], r3 = x.r[4 * q + 3];
        const float o1 = __shfl_xor(half ? r0 : r1, 32);     // half 0 receives row 8 q + 4, half 1 row 8 q + 1
        const float o2 = __shfl_xor(half ? r2 : r3, 32);     // half 0 receives row 8 q + 6, half 1 row 8 q + 3
        b[4 * q] = half ? o1 : r0;                           // rows 8 q,     8 q + 1
        b[4 * q + 1] = half ? o2 : r2;                       //      8 q + 2, 8 q + 3
        b[4 * q + 2] = half ? r1 : o1;                       //      8 q + 4, 8 q + 5
        b[4 * q + 3] = half ? r3 : o2;                       //      8 q + 6, 8 q + 7
    }
}

// c += A X over the first `rows` rows of X (a multiple of 4, at most 32), ascending: b from mfma_acc_as_b, a_row = A[col]
// at the column of A that meets row 0 of X
__device__ __forceinline__ void mfma_chain_acc(MfmaAcc& c, const float* __restrict__ a_row, bool aligned, const float (&b)[MFMA_ACC],
                                               int rows, int half) {
#pragma unroll
    for (int t = 0; t < MFMA_TILE / 4; ++t) {
        if (4 * t < rows) {                                  // wave-uniform
            const MfmaVec4 a4 = mfma_load4(a_row + 4 * t, aligned);
            mfma_32x32x2(half ? a4.f[1] : a4.f[0], b[2 * t], c);
            mfma_32x32x2(half ? a4.f[3] : a4.f[2], b[2 * t + 1], c);
        }
    }
}

}  // namespace irbpp
