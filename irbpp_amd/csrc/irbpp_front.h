// irbpp_front.h -- what the kernels of the network's front share (irbpp_shapefeat.hip, irbpp_embed.hip, irbpp_order_embed.hip):
// leaky and the wave-uniform hint, the block chain (a wave's block of output features continued over a block of inputs
// against wave-uniform weights), the heightmap encoder and the row tile of the two rows kernels, each written once.  All of it
// is part of an arithmetic the tests pin bit for bit; the three files' own comments define that arithmetic.
#pragma once
#include "irbpp_head.h"

// NaNs are part of these definitions, whatever the build's command line says about them elsewhere
#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

__device__ __forceinline__ float front_leaky(float s, float slope) { return s > 0.0f ? s : slope * s; }

// v is the same in every lane of the wave: tell the compiler so
__device__ __forceinline__ int front_wave_uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

// ---- the block chain

// acc[m] continues its chain over the nj inputs of the block at kb (FULL: nj == KBLOCK): xk the lane's inputs, w the weights'
// first row, rows ld floats apart, the block's columns from w[.. + kb]; the wave owns the nf <= FBLOCK features from f0
template <int FBLOCK, int KBLOCK, bool FULL>
__device__ __forceinline__ void front_consume(const float (&xk)[KBLOCK], const float* __restrict__ w, int ld, int kb, int nj, int f0,
                                              int nf, float (&acc)[FBLOCK]) {
#pragma unroll
    for (int m = 0; m < FBLOCK; ++m) {
        // past the wave's last feature: that feature once more, its result unused (no branch between the chains, so that
        // the compiler may interleave them and batch the weight loads)
        const float* wz = w + (size_t)(f0 + (m < nf ? m : nf - 1)) * ld + kb;
#pragma unroll
        for (int jj = 0; jj < KBLOCK; ++jj)
            if (FULL || jj < nj) acc[m] = fmaf(xk[jj], wz[jj], acc[m]);
    }
}

// ---- the row tile of irbpp_embed_rows_kernel and irbpp_order_rows_kernel: lane = row, a layer's inputs in LDS as [k][row]

constexpr int EMBED_ROW_THREADS = 512;
constexpr int EMBED_ROW_WAVES = EMBED_ROW_THREADS / 64;
constexpr int EMBED_FBLOCK = 16;                         // output features per wave and block
constexpr int EMBED_KBLOCK = 16;                         // inputs per block: 16 contiguous weights per feature
constexpr int EMBED_TILE_ROWS = 64;
constexpr int EMBED_X_PITCH = EMBED_TILE_ROWS + 1;       // the x tile is read transposed

// acc[0 .. nf) continue their chains over the K inputs in[k * 64 + lane] (LDS) against w[(f0 + m) * ld + k]
__device__ __forceinline__ void embed_chain(const float* in, int lane, int K, const float* __restrict__ w, int ld, int f0, int nf,
                                            float (&acc)[EMBED_FBLOCK]) {
    for (int kb = 0; kb < K; kb += EMBED_KBLOCK) {
        const int nj = K - kb < EMBED_KBLOCK ? K - kb : EMBED_KBLOCK;
        float xk[EMBED_KBLOCK];
#pragma unroll
        for (int jj = 0; jj < EMBED_KBLOCK; ++jj)        // past the end: an input that exists, its product unused
            xk[jj] = in[(jj < nj ? kb + jj : K - 1) * EMBED_TILE_ROWS + lane];
        if (nj == EMBED_KBLOCK)
            front_consume<EMBED_FBLOCK, EMBED_KBLOCK, true>(xk, w, ld, kb, nj, f0, nf, acc);
        else
            front_consume<EMBED_FBLOCK, EMBED_KBLOCK, false>(xk, w, ld, kb, nj, f0, nf, acc);
    }
}

// ---- the heightmap encoder (irbpp_embed.hip defines its arithmetic), by a workgroup of EMBED_BIN_THREADS

constexpr int EMBED_MAX_MAP = 32;                        // L
constexpr int EMBED_MAX_C1 = 16, EMBED_MAX_C2 = 32, EMBED_MAX_C3 = 4;
constexpr int EMBED_BIN_THREADS = 256;

// One convolution by the workgroup: src [cin][sp][sp] a zero-padded LDS tile (sp = stride * n_out + ksize - stride), out element
// (c, y, x) = leaky(the chain from b[c] over (ci, ky, kx) ascending) -> dst[c * dst_plane + (y + dst_pad) * dst_pitch + x + dst_pad].
template <int KSIZE, int STRIDE>
__device__ __forceinline__ void embed_conv(const float* src, int cin, int sp, const float* __restrict__ w, const float* __restrict__ b,
                                           int cout, int n_out, float slope, float* dst, int dst_plane, int dst_pitch, int dst_pad) {
    const int plane = n_out * n_out;
    for (int o = threadIdx.x; o < cout * plane; o += EMBED_BIN_THREADS) {
        const int c = o / plane, rem = o - c * plane, y = rem / n_out, x = rem - y * n_out;
        const float* wr = w + (size_t)c * cin * KSIZE * KSIZE;
        const float* sr = src + (STRIDE * y) * sp + STRIDE * x;
        float acc = b[c];
        for (int ci = 0; ci < cin; ++ci) {
#pragma unroll
            for (int ky = 0; ky < KSIZE; ++ky)
#pragma unroll
                for (int kx = 0; kx < KSIZE; ++kx)
                    acc = fmaf(sr[(ci * sp + ky) * sp + kx], wr[(ci * KSIZE + ky) * KSIZE + kx], acc);
        }
        dst[c * dst_plane + (y + dst_pad) * dst_pitch + x + dst_pad] = front_leaky(acc, slope);
    }
}

// The L x L heightmap at `height` (row-major, global memory) through the three convolutions: the heightmap goes to a
// zero-padded LDS tile, conv1 and conv2 write zero-padded LDS tiles (one output per thread and trip).  Returns map[0 .. M),
// M = c3 (L/4)^2, in LDS, whole for every thread of the workgroup (the last barrier is inside).
__device__ __forceinline__ const float* embed_height_map(const float* height, const float* w_conv1, const float* b_conv1,
                                                         const float* w_conv2, const float* b_conv2, const float* w_conv3,
                                                         const float* b_conv3, int map_len, int c1, int c2, int c3, float slope) {
    __shared__ float hm[(EMBED_MAX_MAP + 2) * (EMBED_MAX_MAP + 2)];
    __shared__ float a1[EMBED_MAX_C1 * (EMBED_MAX_MAP / 2 + 2) * (EMBED_MAX_MAP / 2 + 2)];
    __shared__ float a2[EMBED_MAX_C2 * (EMBED_MAX_MAP / 4 + 2) * (EMBED_MAX_MAP / 4 + 2)];
    __shared__ float map[EMBED_MAX_C3 * (EMBED_MAX_MAP / 4) * (EMBED_MAX_MAP / 4)];
    const int tid = threadIdx.x;
    const int L = map_len, L2 = L / 2, L4 = L / 4, p0 = L + 2, p1 = L2 + 2, p2 = L4 + 2;
    for (int i = tid; i < p0 * p0; i += EMBED_BIN_THREADS) {
        const int y = i / p0 - 1, x = i - (y + 1) * p0 - 1;
        hm[i] = ((unsigned)y < (unsigned)L && (unsigned)x < (unsigned)L) ? height[y * L + x] : 0.0f;
    }
    for (int i = tid; i < c1 * p1 * p1; i += EMBED_BIN_THREADS) a1[i] = 0.0f;
    for (int i = tid; i < c2 * p2 * p2; i += EMBED_BIN_THREADS) a2[i] = 0.0f;
    __syncthreads();
    embed_conv<4, 2>(hm, 1, p0, w_conv1, b_conv1, c1, L2, slope, a1, p1 * p1, p1, 1);
    __syncthreads();
    embed_conv<4, 2>(a1, c1, p1, w_conv2, b_conv2, c2, L4, slope, a2, p2 * p2, p2, 1);
    __syncthreads();
    embed_conv<3, 1>(a2, c2, p2, w_conv3, b_conv3, c3, L4, slope, map, L4 * L4, L4, 0);
    __syncthreads();
    return map;
}

}  // namespace irbpp

#pragma float_control(pop)
