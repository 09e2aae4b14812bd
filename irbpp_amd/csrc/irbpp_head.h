// irbpp_head.h -- what the kernels of the Rainbow head share (irbpp_c51.hip, irbpp_dueling.hip, irbpp_dueling_loss.hip): the
// limits, the arg-max rule, the stepped walk over a row-major block, the categorical projection and the dueling arithmetic,
// each written once.  All of it is part of an arithmetic the tests pin bit for bit (multiply and add separate: the library is
// built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace irbpp {

constexpr int HEAD_MAX_ATOMS = 128;
constexpr int HEAD_MAX_ROWS = 1024;

// ---- the arg-max rule: the first maximum wins, and with every row at -inf index 0 does (irbpp_masked_argmax_kernel's rules)

__device__ __forceinline__ bool head_better(float v, int i, float best, int bi) { return v > best || (v == best && i < bi); }

// flags (may be NULL) is the env's observation row: row i counts as -inf when flags[5*i+4] == 0
__device__ __forceinline__ float head_masked(const float* flags, int i, float s) {
    return (flags && flags[i * 5 + 4] == 0.0f) ? -INFINITY : s;
}

// the 64-lane butterfly: every lane of a wave ends with the wave's (best, bi)
__device__ __forceinline__ void head_wave_argmax(float& best, int& bi) {
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (head_better(ob, oi, best, bi)) { best = ob; bi = oi; }
    }
}

// (NaN values, out of scope, match nothing and leave bi at its start, 0x7fffffff: still a row of the block)
__device__ __forceinline__ int head_index(int bi, int s_rows) { return bi < s_rows ? bi : 0; }

// ---- the walk: nrows rows of atoms floats taken by THREADS threads with coalesced dword accesses.  Element
// e = tid + THREADS t of the chunk is (row, k) = (e / atoms, e % atoms): stepped, not divided.  f(row, k, e) per element.
template <int THREADS, typename F>
__device__ __forceinline__ void head_walk(int atoms, int nrows, F f) {
    const int tid = threadIdx.x;
    const int q = THREADS / atoms, r = THREADS - q * atoms;
    int row = tid / atoms, k = tid - row * atoms, e = tid;
    while (row < nrows) {
        f(row, k, e);
        e += THREADS;
        row += q;
        k += r;
        if (k >= atoms) { k -= atoms; ++row; }
    }
}

// ---- the categorical projection of Agent.learn (agent.py:96-115), for one sample, by a workgroup of THREADS threads:
// Tz = R + (nonterminal * gamma^n) z clamped to [Vmin, Vmax] (g is nonterminal * gamma^n), b = (Tz - Vmin) / delta_z (IEEE
// division), l = floor b, u = ceil b with the two l == u fix-ups in the reference's order (:108-109), and the two index_add_
// calls (:114-115) without atomics: l, u and the two weights of every atom go to LDS and thread j sums, in ascending i, first
// the l == j contributions pa[i] (u_i - b_i) and then the u == j contributions pa[i] (b_i - l_i) -- the order in which the
// reference's two sequential scatters reach m[j].  An l or u outside [0, atoms) (a delta_z that is not (Vmax - Vmin) /
// (atoms - 1)) matches no thread: nothing is written out of range.  pa (the target net's row a*) and z may lie in LDS: the
// first barrier makes what the caller wrote there visible, the second one proj.
struct HeadProjection {
    int sl[HEAD_MAX_ATOMS], su[HEAD_MAX_ATOMS];
    float swl[HEAD_MAX_ATOMS], swu[HEAD_MAX_ATOMS];
};

template <int THREADS>
__device__ __forceinline__ void head_project(const float* pa, const float* z, float ret, float g, float v_min, float v_max,
                                             float delta_z, int atoms, float* __restrict__ m_row, HeadProjection& proj) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int i = tid; i < atoms; i += THREADS) {
        float tz = ret + g * z[i];
        tz = fminf(fmaxf(tz, v_min), v_max);
        const float b = (tz - v_min) / delta_z;
        int l = (int)floorf(b), u = (int)ceilf(b);
        if (u > 0 && l == u) l -= 1;                     // l[(u > 0) * (l == u)] -= 1
        if (l < atoms - 1 && l == u) u += 1;             // u[(l < (atoms - 1)) * (l == u)] += 1
        const float pi = pa[i];
        proj.sl[i] = l;
        proj.su[i] = u;
        proj.swl[i] = pi * ((float)u - b);
        proj.swu[i] = pi * (b - (float)l);
    }
    __syncthreads();
    for (int j = tid; j < atoms; j += THREADS) {
        float acc = 0.0f;
        for (int i = 0; i < atoms; ++i)
            if (proj.sl[i] == j) acc = acc + proj.swl[i];
        for (int i = 0; i < atoms; ++i)
            if (proj.su[i] == j) acc = acc + proj.swu[i];
        m_row[j] = acc;
    }
}

// ---- the dueling arithmetic (defined in the file comment of irbpp_dueling.hip)

constexpr int DUELING_THREADS = 512;
constexpr int DUELING_PARTS = 16;                        // interleaved partial column sums: part of the arithmetic
constexpr int DUELING_CHUNK_ROWS = 256;                  // rows per staging trip of a block that does not fit
constexpr int DUELING_TILE_BYTES = 144 * 1024;           // dynamic LDS for the tile; 10.6 KB of static LDS go on top

// rows of the block the tile holds at a time: all S of them (resident) or DUELING_CHUNK_ROWS (constexpr: for the host, which
// sizes the launch by it, as for the device)
constexpr int dueling_tile_rows(int s_rows, int atoms) {
    return (long long)s_rows * (atoms | 1) * 4 <= DUELING_TILE_BYTES ? s_rows : DUELING_CHUNK_ROWS;
}

struct DuelingShared {
    float part[DUELING_PARTS][HEAD_MAX_ATOMS];
    float mean[HEAD_MAX_ATOMS], v[HEAD_MAX_ATOMS], z[HEAD_MAX_ATOMS];
    float best[DUELING_THREADS / 64];
    int bi[DUELING_THREADS / 64];
};

// exp(t) for t <= 0 in plain float32 operations, the same bits on every IEEE machine: exactly 0.0f for t < -80
// (exp(-80) = 1.8e-35; above the cut-off neither e nor e / den with den <= 128 is subnormal), else n = floor(t log2(e) + 1/2),
// r = (t - n LN2_HI) - n LN2_LO (Cody-Waite; n LN2_HI is exact for |n| <= 127, |r| <= 0.347), the degree-7 Taylor
// polynomial in Horner form, and 2^n through the exponent bits.  Measured error: profiles/dueling_head/README.md.
__device__ __forceinline__ float dueling_dexp(float t) {
    if (t < -80.0f) return 0.0f;
    const float n = floorf(t * 1.4426950408889634f + 0.5f);
    const float r = (t - n * 0.693145751953125f) - n * 1.4286068203094172e-06f;      // LN2_HI = 45426 / 65536
    float p = 1.9841269841269841e-04f;                   // 1/5040
    p = p * r + 1.3888888888888889e-03f;                 // 1/720
    p = p * r + 8.3333333333333332e-03f;                 // 1/120
    p = p * r + 4.1666666666666664e-02f;                 // 1/24
    p = p * r + 1.6666666666666666e-01f;                 // 1/6
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const uint32_t bits = (uint32_t)((int)n + 127) << 23;
    float scale;
    memcpy(&scale, &bits, 4);
    return p * scale;
}

// mean[k] of the s_rows rows at src (row pitch `stride` floats: the tile or global memory, the same bits either way):
// thread j < 16 atoms sums part[j / atoms][j % atoms], then thread k < atoms adds the 16 parts left to right and divides
template <typename Stride>
__device__ __forceinline__ void dueling_mean(const float* src, Stride stride, int atoms, int s_rows, float (*part)[HEAD_MAX_ATOMS],
                                             float* mean) {
    const int tid = threadIdx.x;
    for (int j = tid; j < DUELING_PARTS * atoms; j += DUELING_THREADS) {
        const int g = j / atoms, k = j - g * atoms;
        float s = 0.0f;
        for (int i = g; i < s_rows; i += DUELING_PARTS) s = s + src[(size_t)i * stride + k];
        part[g][k] = s;
    }
    __syncthreads();
    if (tid < atoms) {
        float s = part[0][tid];
        for (int g = 1; g < DUELING_PARTS; ++g) s = s + part[g][tid];
        mean[tid] = s / (float)s_rows;
    }
    __syncthreads();
}

// One row in place: a -> x = (v + a) - mean; returns mx = max_k x[k].  sv, smean: LDS copies of v and mean.
__device__ __forceinline__ float dueling_combine(float* rw, const float* sv, const float* smean, int atoms) {
    float mx = (sv[0] + rw[0]) - smean[0];
    rw[0] = mx;
    for (int k = 1; k < atoms; ++k) {
        const float x = (sv[k] + rw[k]) - smean[k];
        rw[k] = x;
        mx = x > mx ? x : mx;
    }
    return mx;
}

}  // namespace irbpp
