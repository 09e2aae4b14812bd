// irbpp_shapefeat.hip -- the shape branch of DQNBPP.forward without a gradient (model.py:328-335, :365-372 for bufferSize > 1):
// from the observation's item-id column to shape_feature, on the device.  The reference gathers samplePointsNum points of
// every row's shape on the host, copies them over and runs Linear(3, H1) LeakyReLU Linear(H1, F) LeakyReLU and a max over the
// points per row.  The feature depends on the item id and the index set alone, so here it is computed once per shape that
// occurs in the ids and gathered: two launches, no atomics.
//
// Defined float32 arithmetic (tests/test_shape_features_cpu.py restates it and the kernels are held to it bit for bit).
// points [n_shapes][P][3], indices int32 [k], ids [M], W1 [H1][3], b1 [H1], W2 [F][H1], b2 [F], slope.  For row m, u = ids[m]:
//   p_j      = points[u][indices[j]][:]                                              j < k, duplicates are legal
//   h1_j[i]  = leaky(fmaf(p_j[2], W1[i][2], fmaf(p_j[1], W1[i][1], fmaf(p_j[0], W1[i][0], b1[i]))))
//   s_j[f]   = b2[f]; for i = 0 .. H1-1 ascending: s_j[f] = fmaf(h1_j[i], W2[f][i], s_j[f])
//   leaky(s) = s > 0 ? s : slope * s                                                 (torch's float32 bits)
//   out[m][f] = max_j leaky(s_j[f])    with a sticky NaN (any NaN term: NaN, the quiet NaN 0x7fc00000) and +0 above -0.
// The max is taken on keys (shape_key: an order-preserving map of the float's bits to uint32 with every NaN on top), so it is
// exact and associative: the split of the points over lanes, trips, chunks and the two kernels cannot change a bit.
// An id outside [0, n_shapes) (a float32 id is truncated toward zero first, as .long() does; NaN and infinities are outside)
// gives a NaN row; an index outside [0, P) counts as a NaN point, so every row comes out NaN; nothing out of range is read.
// The fused multiply-adds are written out and never split or re-associated (the build keeps -ffp-contract=off).
//
// Layout.  irbpp_shape_partial_kernel, grid (n_shapes, C), one wave per block of SHAPE_FBLOCK output features: the workgroup
// first scans the ids for its shape and leaves if it does not occur (its rows of `partial` are then never written, and never
// read).  A lane owns one point at a time (chunk_points / 64 trips), the weights are wave-uniform __restrict__ loads (scalar
// cache, SGPR operands of the FMA), hidden units are made SHAPE_HBLOCK at a time from the point (three FMAs and a select each)
// and consumed at once by the wave's accumulators in ascending i, as irbpp_streams.hip does; per trip the wave reduces each
// feature's keys once (lane m keeps feature m's running maximum).  A lane without a point brings the key 0, which no value
// has.  irbpp_shape_gather_kernel: out[m][f] = max_c partial[ids[m]][c][f].
#include "irbpp_front.h"

// NaNs are part of this definition, whatever the build's command line says about them elsewhere
#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

constexpr int SHAPE_MAX_WIDTH = 256;                     // H1 and F
constexpr int SHAPE_MAX_POINTS = 4096;                   // k
constexpr int SHAPE_MAX_SHAPES = 65535;
constexpr int SHAPE_FBLOCK = 32;                         // output features per wave
constexpr int SHAPE_THREADS_MAX = 64 * (SHAPE_MAX_WIDTH / SHAPE_FBLOCK);   // one wave per block of features
constexpr int SHAPE_HBLOCK = 16;                         // hidden units per block: 16 contiguous W2 elements per feature
constexpr int SHAPE_TARGET_GROUPS = 2048;                // workgroups wanted before chunks grow beyond one wave of points
constexpr uint32_t SHAPE_NAN_BITS = 0x7fc00000u;
constexpr uint32_t SHAPE_NAN_KEY = 0xffffffffu;

// points per chunk for this many shapes and points: a multiple of 64; the number of chunks is ceil(k / chunk_points), so no
// chunk is empty (constexpr: the host sizes the launch and the workspace by it)
constexpr int shape_chunk_points(int n_shapes, int k) {
    const int waves = (k + 63) / 64;
    const int want = SHAPE_TARGET_GROUPS / n_shapes < 1 ? 1 : SHAPE_TARGET_GROUPS / n_shapes;
    const int chunks = want < waves ? want : waves;
    return 64 * (((k + chunks - 1) / chunks + 63) / 64);
}
constexpr int shape_chunks(int n_shapes, int k) {
    return (k + shape_chunk_points(n_shapes, k) - 1) / shape_chunk_points(n_shapes, k);
}

constexpr int shape_threads(int feat) { return 64 * ((feat + SHAPE_FBLOCK - 1) / SHAPE_FBLOCK); }

// float -> key: a < b as floats <=> key(a) < key(b) as uint32, -0 below +0, every NaN the largest key; no value maps to 0
__device__ __forceinline__ uint32_t shape_key(float s) {
    uint32_t b;
    memcpy(&b, &s, 4);
    if ((b & 0x7fffffffu) > 0x7f800000u) return SHAPE_NAN_KEY;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ uint32_t shape_key_bits(uint32_t key) {       // the float's bits again
    if (key == SHAPE_NAN_KEY) return SHAPE_NAN_BITS;
    return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
}

// ids[m] as a shape index, -1 for one outside [0, n_shapes)
__device__ __forceinline__ int shape_id(const void* __restrict__ ids, int ids_are_float, long long ids_stride, long long m,
                                        int n_shapes) {
    if (ids_are_float) {
        const float v = ((const float*)ids)[m * ids_stride];
        return (v > -1.0f && v < (float)n_shapes) ? (int)v : -1;         // a NaN fails both comparisons
    }
    const long long v = ((const long long*)ids)[m * ids_stride];
    return (v >= 0 && v < n_shapes) ? (int)v : -1;
}

struct ShapeArgs {
    long long ids_stride, m_rows, out_stride;
    int n_shapes, n_points, k, ids_are_float, hidden, feat, chunk_points, chunks;
    float slope;
};

// one point -> acc[0 .. nf): s[f0 + m] before the second leaky
__device__ __forceinline__ void shape_point(float p0, float p1, float p2, const float* __restrict__ w1, const float* __restrict__ b1,
                                            const float* __restrict__ w2, const float* __restrict__ b2, int H1, float slope, int f0,
                                            int nf, float (&acc)[SHAPE_FBLOCK]) {
#pragma unroll
    for (int m = 0; m < SHAPE_FBLOCK; ++m) acc[m] = m < nf ? b2[f0 + m] : 0.0f;
    for (int ib = 0; ib < H1; ib += SHAPE_HBLOCK) {
        const int nj = H1 - ib < SHAPE_HBLOCK ? H1 - ib : SHAPE_HBLOCK;
        float h[SHAPE_HBLOCK];
#pragma unroll
        for (int jj = 0; jj < SHAPE_HBLOCK; ++jj) {
            const int i = jj < nj ? ib + jj : H1 - 1;        // past the end: a unit that exists, its result unused
            const float* wr = w1 + (size_t)i * 3;
            h[jj] = front_leaky(fmaf(p2, wr[2], fmaf(p1, wr[1], fmaf(p0, wr[0], b1[i]))), slope);
        }
        if (nj == SHAPE_HBLOCK)
            front_consume<SHAPE_FBLOCK, SHAPE_HBLOCK, true>(h, w2, H1, ib, nj, f0, nf, acc);
        else
            front_consume<SHAPE_FBLOCK, SHAPE_HBLOCK, false>(h, w2, H1, ib, nj, f0, nf, acc);
    }
}

// Workgroup (u, c) of shape_threads(F) threads: partial[u][c][f] = max over the chunk's points of h2[f], if u occurs in ids
extern "C" __global__ void __launch_bounds__(SHAPE_THREADS_MAX)
irbpp_shape_partial_kernel(const float* __restrict__ points, const int32_t* __restrict__ indices, const void* __restrict__ ids,
                           const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                           const float* __restrict__ b2, float* __restrict__ partial, ShapeArgs g) {
    __shared__ int32_t occurs[SHAPE_THREADS_MAX / 64];   // per wave: one of its lanes met an id equal to u
    const int tid = threadIdx.x, lane = tid & 63, u = blockIdx.x, c = blockIdx.y;
    const int threads = shape_threads(g.feat);
    int mine = 0;
    for (long long m = tid; m < g.m_rows; m += threads) mine |= shape_id(ids, g.ids_are_float, g.ids_stride, m, g.n_shapes) == u;
    for (int o = 32; o > 0; o >>= 1) mine |= __shfl_xor(mine, o);
    if (lane == 0) occurs[tid >> 6] = mine;
    __syncthreads();
    mine = 0;
    for (int w = 0; w < threads / 64; ++w) mine |= occurs[w];
    if (!mine) return;                                   // the whole workgroup

    const int f0 = front_wave_uniform(tid >> 6) * SHAPE_FBLOCK;         // in SGPRs: the weights' addresses are scalar
    const int nf = g.feat - f0 < SHAPE_FBLOCK ? g.feat - f0 : SHAPE_FBLOCK;
    const int j0 = c * g.chunk_points;
    const int j1 = j0 + g.chunk_points < g.k ? j0 + g.chunk_points : g.k;
    const float* pu = points + (size_t)u * g.n_points * 3;
    uint32_t mine_key = 0u;                               // lane m: the running maximum of feature f0 + m
    for (int jb = j0; jb < j1; jb += 64) {               // wave-uniform trips
        // a lane past j1 computes the chunk's last point along with the others (no divergence around the chains) and
        // brings the key 0, which no value has, to the reduction
        const bool has = jb + lane < j1;
        const int idx = indices[has ? jb + lane : j1 - 1];
        float p0, p1, p2;
        if ((uint32_t)idx < (uint32_t)g.n_points) {
            const float* p = pu + (size_t)idx * 3;
            p0 = p[0], p1 = p[1], p2 = p[2];
        } else {                                         // a NaN point: it reaches every feature through the chains
            const uint32_t nan_bits = SHAPE_NAN_BITS;
            memcpy(&p0, &nan_bits, 4);
            p1 = p0, p2 = p0;
        }
        float acc[SHAPE_FBLOCK];
        shape_point(p0, p1, p2, w1, b1, w2, b2, g.hidden, g.slope, f0, nf, acc);
        // one wave reduction per feature and trip
#pragma unroll
        for (int m = 0; m < SHAPE_FBLOCK; ++m) {
            if (m < nf) {
                uint32_t key = has ? shape_key(acc[m]) : 0u;
                for (int o = 32; o > 0; o >>= 1) {
                    const uint32_t other = (uint32_t)__shfl_xor((int)key, o);
                    key = other > key ? other : key;
                }
                if (lane == m && key > mine_key) mine_key = key;
            }
        }
    }
    // leaky is monotone and maps NaN to NaN: applied once, to the maximum
    if (lane < nf) {
        const uint32_t bits = shape_key_bits(mine_key);
        float s;
        memcpy(&s, &bits, 4);
        const uint32_t out_bits = shape_key_bits(shape_key(front_leaky(s, g.slope)));
        memcpy(&partial[((size_t)u * g.chunks + c) * g.feat + f0 + lane], &out_bits, 4);
    }
}

// out[m][f] = max_c partial[ids[m]][c][f]; a NaN row for an id outside [0, n_shapes).  One thread per element.
extern "C" __global__ void __launch_bounds__(256)
irbpp_shape_gather_kernel(const float* __restrict__ partial, const void* __restrict__ ids, float* __restrict__ out, ShapeArgs g) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= g.m_rows * g.feat) return;
    const long long m = e / g.feat;
    const int f = (int)(e - m * g.feat);
    const int u = shape_id(ids, g.ids_are_float, g.ids_stride, m, g.n_shapes);
    uint32_t key = SHAPE_NAN_KEY;
    if (u >= 0) {
        const float* src = partial + (size_t)u * g.chunks * g.feat + f;
        key = 0u;
        for (int c = 0; c < g.chunks; ++c) {
            const uint32_t other = shape_key(src[(size_t)c * g.feat]);
            key = other > key ? other : key;
        }
    }
    const uint32_t bits = shape_key_bits(key);
    memcpy(&out[m * g.out_stride + f], &bits, 4);
}

}  // namespace irbpp

#pragma float_control(pop)
