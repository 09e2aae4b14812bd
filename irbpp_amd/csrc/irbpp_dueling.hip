// irbpp_dueling.hip -- the dueling head fused in front of the distributional head: the end of DQNBPP.forward
// (model.py:395-400: q = v + a - a.mean(1), softmax over the atoms) and the consumers of irbpp_c51.hip in one launch each,
// from the network's logits.  The [N][S][atoms] probabilities exist only in LDS unless the caller asks for them.
//
// Defined float32 arithmetic (multiply and add separate, -ffp-contract=off; tests/test_dueling_cpu.py restates it in numpy and
// the kernels are held to it bit for bit).  For one environment, v[atoms], a[S][atoms], z[atoms]:
//   part[g][k] = 0.0f + a[g][k] + a[g+16][k] + a[g+32][k] + ...        g = 0..15, rows ascending (an empty part stays 0)
//   mean[k]    = ((..(part[0][k] + part[1][k]) + ..) + part[15][k]) / (float)S                         IEEE division
//   x[i][k]    = (v[k] + a[i][k]) - mean[k]
//   mx[i]      = max_k x[i][k];  t = x[i][k] - mx[i];  e[i][k] = dexp(t)
//   den[i]     = ((e[i][0] + e[i][1]) + ..) + e[i][atoms-1]            (>= 1: the maximum's e is dexp(0) = 1)
//   p[i][k]    = e[i][k] / den[i]                                                                       IEEE division
//   q[i]       = ((p[i][0] z[0] + p[i][1] z[1]) + ..), every product and sum rounded: the value of irbpp_c51.hip
// The order is a function of (S, atoms) alone: not of N, of strides, of the launch, or of whether the block stayed in LDS.
// Mask, first maximum and the all-masked index 0 are the rules of c51_wave_argmax.  Finite logits are the contract: a NaN or
// an infinite logit gives unspecified values in q_out, p_out and m, but the action / a_star is still a row of the block and
// nothing is read or written out of range.
//
// Layout: one workgroup of 512 threads per environment.  The a block is staged once into LDS with coalesced dword loads
// (consecutive threads, consecutive addresses of a row), rows `atoms | 1` floats apart (odd pitch: thread-per-row reads
// fall on 32 different banks), wherever S rows fit DUELING_TILE_BYTES; the column sums and the rows are then read from
// LDS.  A larger block takes its column sums from global memory and stages 256 rows at a time (a second pass).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace irbpp {

constexpr int DUELING_MAX_ATOMS = 128;
constexpr int DUELING_MAX_ROWS = 1024;
constexpr int DUELING_THREADS = 512;
constexpr int DUELING_PARTS = 16;                        // interleaved partial column sums: part of the arithmetic
constexpr int DUELING_CHUNK_ROWS = 256;                  // rows per staging trip of a block that does not fit
constexpr int DUELING_TILE_BYTES = 144 * 1024;           // dynamic LDS for the tile; 10.6 KB of static LDS go on top

// rows of the block the tile holds at a time: all S of them (resident) or DUELING_CHUNK_ROWS
__host__ __device__ inline int dueling_tile_rows(int s_rows, int atoms) {
    return (long long)s_rows * (atoms | 1) * 4 <= DUELING_TILE_BYTES ? s_rows : DUELING_CHUNK_ROWS;
}

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

// nrows rows of the block (src: its row r0) into the tile, element e = tid + 512 t of the chunk being (row, k) =
// (e / atoms, e % atoms): stepped, not divided
__device__ __forceinline__ void dueling_stage(const float* __restrict__ src, long long row_stride, int atoms, int nrows, float* tile) {
    const int tid = threadIdx.x, pitch = atoms | 1;
    const int q = DUELING_THREADS / atoms, r = DUELING_THREADS - q * atoms;
    int row = tid / atoms, k = tid - row * atoms;
    while (row < nrows) {
        tile[row * pitch + k] = src[(size_t)row * row_stride + k];
        row += q;
        k += r;
        if (k >= atoms) { k -= atoms; ++row; }
    }
}

// mean[k] of the s_rows rows at src (row pitch `stride` floats: the tile or global memory, the same bits either way):
// thread j < 16 atoms sums part[j / atoms][j % atoms], then thread k < atoms adds the 16 parts left to right and divides
template <typename Stride>
__device__ __forceinline__ void dueling_mean(const float* src, Stride stride, int atoms, int s_rows, float (*part)[DUELING_MAX_ATOMS],
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

// One row of the tile in place: a -> p; returns its expected value.  sv, smean, sz: LDS copies of v, mean and the support.
__device__ __forceinline__ float dueling_row(float* rw, const float* sv, const float* smean, const float* sz, int atoms) {
    float mx = (sv[0] + rw[0]) - smean[0];
    rw[0] = mx;
    for (int k = 1; k < atoms; ++k) {
        const float x = (sv[k] + rw[k]) - smean[k];
        rw[k] = x;
        mx = x > mx ? x : mx;
    }
    float den = dueling_dexp(rw[0] - mx);
    rw[0] = den;
    for (int k = 1; k < atoms; ++k) {
        const float e = dueling_dexp(rw[k] - mx);
        rw[k] = e;
        den = den + e;
    }
    const float p0 = rw[0] / den;
    rw[0] = p0;
    float s = p0 * sz[0];
    for (int k = 1; k < atoms; ++k) {
        const float p = rw[k] / den;
        rw[k] = p;
        s = s + p * sz[k];
    }
    return s;
}

struct DuelingShared {
    float part[DUELING_PARTS][DUELING_MAX_ATOMS];
    float mean[DUELING_MAX_ATOMS], v[DUELING_MAX_ATOMS], z[DUELING_MAX_ATOMS];
    float best[DUELING_THREADS / 64];
    int bi[DUELING_THREADS / 64];
};

// One workgroup: the masked arg-max over the s_rows rows of one environment's head, from its logits.  flags, q_out as in
// c51_wave_argmax; p_out (may be NULL) receives the [s_rows][atoms] probabilities, contiguous.  Every thread returns the index.
__device__ __forceinline__ int dueling_block_argmax(const float* __restrict__ v, const float* __restrict__ a, long long row_stride,
                                                    const float* __restrict__ z, int atoms, int s_rows,
                                                    const float* __restrict__ flags, float* __restrict__ q_out,
                                                    float* __restrict__ p_out, float* tile, DuelingShared& sh) {
    const int tid = threadIdx.x, pitch = atoms | 1;
    const int tile_rows = dueling_tile_rows(s_rows, atoms);
    const bool resident = tile_rows == s_rows;
    if (tid < atoms) {
        sh.v[tid] = v[tid];
        sh.z[tid] = z[tid];
    }
    if (resident) {
        dueling_stage(a, row_stride, atoms, s_rows, tile);
        __syncthreads();
        dueling_mean(tile, pitch, atoms, s_rows, sh.part, sh.mean);
    } else {
        dueling_mean(a, row_stride, atoms, s_rows, sh.part, sh.mean);
    }
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int r0 = 0; r0 < s_rows; r0 += tile_rows) {
        const int nrows = s_rows - r0 < tile_rows ? s_rows - r0 : tile_rows;
        if (!resident) {
            dueling_stage(a + (size_t)r0 * row_stride, row_stride, atoms, nrows, tile);
            __syncthreads();
        }
        for (int lr = tid; lr < nrows; lr += DUELING_THREADS) {
            const int i = r0 + lr;
            const float s = dueling_row(tile + lr * pitch, sh.v, sh.mean, sh.z, atoms);
            if (q_out) q_out[i] = s;
            const float val = (flags && flags[i * 5 + 4] == 0.0f) ? -INFINITY : s;
            if (val > best || (val == best && i < bi)) { best = val; bi = i; }
        }
        __syncthreads();
        if (p_out) {
            float* dst = p_out + (size_t)r0 * atoms;
            const int q = DUELING_THREADS / atoms, r = DUELING_THREADS - q * atoms;
            int row = tid / atoms, k = tid - row * atoms, e = tid;
            while (row < nrows) {
                dst[e] = tile[row * pitch + k];
                e += DUELING_THREADS;
                row += q;
                k += r;
                if (k >= atoms) { k -= atoms; ++row; }
            }
        }
        __syncthreads();                                 // the tile is rewritten by the next trip
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if ((tid & 63) == 0) {
        sh.best[tid >> 6] = best;
        sh.bi[tid >> 6] = bi;
    }
    __syncthreads();
    best = sh.best[0];
    bi = sh.bi[0];
    for (int w = 1; w < DUELING_THREADS / 64; ++w) {
        const float ob = sh.best[w];
        const int oi = sh.bi[w];
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    __syncthreads();                                     // sh is reused by the caller
    return bi < s_rows ? bi : 0;                         // (NaN values, out of scope, match nothing: still a row of the block)
}

// DQNBPP.forward's combine + softmax (model.py:395-400) and Agent.act after it (agent.py:51-58), per environment.
extern "C" __global__ void __launch_bounds__(DUELING_THREADS)
irbpp_dueling_act_kernel(const float* __restrict__ v, long long v_stride, const float* __restrict__ a, long long env_stride,
                         long long row_stride, const float* __restrict__ support, int atoms, const float* __restrict__ obs,
                         int obs_stride, int s_rows, int64_t* __restrict__ action, float* __restrict__ q_out, long long q_stride,
                         float* __restrict__ p_out) {
    HIP_DYNAMIC_SHARED(float, dueling_tile)             // dueling_tile_rows() * (atoms | 1) floats
    __shared__ DuelingShared sh;
    const int env = blockIdx.x;
    const int bi = dueling_block_argmax(v + (size_t)env * v_stride, a + (size_t)env * env_stride, row_stride, support, atoms, s_rows,
                                        obs ? obs + (size_t)env * obs_stride : nullptr,
                                        q_out ? q_out + (size_t)env * q_stride : nullptr,
                                        p_out ? p_out + (size_t)env * s_rows * atoms : nullptr, dueling_tile, sh);
    if (threadIdx.x == 0) action[env] = bi;
}

// Agent.learn's no_grad block (agent.py:90-115) from the logits of the two networks, per sample: a* from the online (v, a),
// unmasked; pns_a = row a* of the target net's softmax by the same arithmetic (the target block's mean, read once from global
// memory, and that one row); then the projection of irbpp_c51_target_kernel operation for operation: Tz, b, l, u, the two
// fix-ups, and the scatter in the order of the two index_add_ calls without atomics.
extern "C" __global__ void __launch_bounds__(DUELING_THREADS)
irbpp_dueling_target_kernel(const float* __restrict__ v_online, long long von_stride, const float* __restrict__ a_online,
                            long long on_env_stride, long long on_row_stride, const float* __restrict__ v_target,
                            long long vtg_stride, const float* __restrict__ a_target, long long tg_env_stride,
                            long long tg_row_stride, const float* __restrict__ returns, const float* __restrict__ nonterminals,
                            const float* __restrict__ support, int atoms, int s_rows, float gamma_n, float v_min, float v_max,
                            float delta_z, float* __restrict__ m, int64_t* __restrict__ a_star) {
    HIP_DYNAMIC_SHARED(float, dueling_tile)
    __shared__ DuelingShared sh;
    __shared__ int sl[DUELING_MAX_ATOMS], su[DUELING_MAX_ATOMS];
    __shared__ float swl[DUELING_MAX_ATOMS], swu[DUELING_MAX_ATOMS];
    const int smp = blockIdx.x, tid = threadIdx.x;
    const int best = dueling_block_argmax(v_online + (size_t)smp * von_stride, a_online + (size_t)smp * on_env_stride, on_row_stride,
                                          support, atoms, s_rows, nullptr, nullptr, nullptr, dueling_tile, sh);
    if (tid == 0) a_star[smp] = best;
    const float* at = a_target + (size_t)smp * tg_env_stride;
    dueling_mean(at, tg_row_stride, atoms, s_rows, sh.part, sh.mean);
    if (tid < atoms) {
        sh.v[tid] = v_target[(size_t)smp * vtg_stride + tid];
        dueling_tile[tid] = at[(size_t)best * tg_row_stride + tid];
    }
    __syncthreads();
    if (tid == 0) dueling_row(dueling_tile, sh.v, sh.mean, sh.z, atoms);       // the row is sequential in k by definition
    __syncthreads();
    const float ret = returns[smp];
    const float g = nonterminals[smp] * gamma_n;
    for (int i = tid; i < atoms; i += DUELING_THREADS) {
        float tz = ret + g * sh.z[i];
        tz = fminf(fmaxf(tz, v_min), v_max);
        const float b = (tz - v_min) / delta_z;
        int l = (int)floorf(b), u = (int)ceilf(b);
        if (u > 0 && l == u) l -= 1;                     // l[(u > 0) * (l == u)] -= 1
        if (l < atoms - 1 && l == u) u += 1;             // u[(l < (atoms - 1)) * (l == u)] += 1
        const float pi = dueling_tile[i];
        sl[i] = l;
        su[i] = u;
        swl[i] = pi * ((float)u - b);
        swu[i] = pi * (b - (float)l);
    }
    __syncthreads();
    for (int j = tid; j < atoms; j += DUELING_THREADS) {
        float acc = 0.0f;
        for (int i = 0; i < atoms; ++i)
            if (sl[i] == j) acc = acc + swl[i];
        for (int i = 0; i < atoms; ++i)
            if (su[i] == j) acc = acc + swu[i];
        m[(size_t)smp * atoms + j] = acc;
    }
}

}  // namespace irbpp
