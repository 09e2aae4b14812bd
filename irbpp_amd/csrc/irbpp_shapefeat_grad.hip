// irbpp_shapefeat_grad.hip -- the shape branch of DQNBPP.forward with a gradient (model.py:328-335, :365-372 for bufferSize > 1
// in Agent.learn's online forward): the forward of irbpp_shapefeat.hip with a record of where each maximum sits, and the
// backward routed through that record, once per shape that occurs in the ids.  Included after irbpp_shapefeat.hip, whose
// shape_key, shape_id, shape_point, ShapeArgs and shape_chunk_points it uses; that file's two kernels are not touched.
//
// Defined float32 arithmetic (tests/test_shape_grad_cpu.py restates it and the kernels are held to it bit for bit).
// Forward: irbpp_shapefeat.hip's definition, the same bits as irbpp_shape_features, and per shape u that occurs in the ids
//   arg[u][f] = the smallest j in [0, k) with shape_key(s_j[f]) == max_j shape_key(s_j[f])        (s_j[f]: before the second leaky;
//   the NaN key counts like any other; the indices are drawn with replacement, so exact ties are ordinary)
// and arg[u][*] = -1 for a shape that does not occur.
// Backward, from g[m][f] (float32, contiguous); only w1, b1, w2, b2 carry a gradient:
//   G[u][f]   = +0; for m ascending with shape_id(ids[m]) == u: G[u][f] += g[m][f]                (a bad id's row adds nothing)
//   per occurring u and f: j = arg[u][f], p = points[u][indices[j]] (an index outside [0, P): a NaN point),
//     s1[i] = fmaf(p[2], w1[i][2], fmaf(p[1], w1[i][1], fmaf(p[0], w1[i][0], b1[i]))), h1[i] = leaky(s1[i]),
//     s2 = b2[f]; for i ascending: s2 = fmaf(h1[i], w2[f][i], s2)                                   (the forward's own chains)
//     d2[u][f] = s2 > 0 ? G[u][f] : slope * G[u][f]
//   db2[f] = +0; dW2[f][i] = +0; for occurring u ascending: db2[f] += d2[u][f]; dW2[f][i] = fmaf(d2[u][f], h1_{u,f}[i], dW2[f][i])
//   per occurring u: P1[u][i][c] = +0, Pb[u][i] = +0; for f ascending:
//     e = d2[u][f] * w2[f][i]; ds1 = s1_{u,f}[i] > 0 ? e : slope * e; P1[u][i][c] = fmaf(ds1, p_{u,f}[c], P1[u][i][c]); Pb[u][i] += ds1
//   dW1[i][c] = +0; db1[i] = +0; for occurring u ascending: dW1[i][c] += P1[u][i][c]; db1[i] += Pb[u][i]
// Every chain is walked by one thread in the order written: nothing is split over lanes or re-associated, there are no atomics,
// and the build keeps -ffp-contract=off.  NaNs go through the arithmetic as they come.
//
// Layout.  Forward: irbpp_shape_partial_arg_kernel is irbpp_shape_partial_kernel with the pair (key, j) as its running maximum
// (after the wave's maximum of a trip's keys, the lowest lane that holds it is the smallest j of the trip; a later trip or
// chunk replaces an earlier one only with a greater key) and leaves the key before the second leaky, so that chunks compare
// what the record is defined on; workgroup (u, 0) of a shape that does not occur writes j = -1 into its row of the j workspace.
// irbpp_shape_gather_arg_kernel: one thread per out[m][f] (the maximum over the chunks, then the leaky once) and one per
// arg[u][f].  Backward: irbpp_shape_backward_shape_kernel, a workgroup per shape, scans the ids 64 at a time (every wave on its
// own: the mask of matching rows is wave-uniform, and the rows are added in ascending order), leaves if u does not occur; thread
// f walks its s2 chain (w1 and b1 at wave-uniform addresses, its own row of w2) and puts (p, d2) into LDS and into pd[u][f];
// then thread i walks the f chain of P1 and Pb, recomputing s1 from the point in LDS (three FMAs) with w2[f][i] coalesced over
// i: no row of ds1 is ever stored.  irbpp_shape_backward_reduce_kernel: a thread per dW2[f][i] (h1 again from pd's point), per
// db2[f] and per (i, c) of dW1 / db1, each over u ascending; arg[u][.] >= 0 says that u occurs.
#include "irbpp_front.h"

#pragma float_control(push)
#pragma float_control(precise, on)
#pragma clang fp contract(off)

namespace irbpp {

constexpr int SHAPE_GRAD_THREADS = SHAPE_MAX_WIDTH;      // a thread per feature, then a thread per hidden unit

struct alignas(16) ShapeQuad { float x, y, z, w; };     // (p[0], p[1], p[2], d2) of one (u, f); (P1[0], P1[1], P1[2], Pb) of one (u, i)

struct ShapeGradArgs {
    long long ids_stride, m_rows;
    int n_shapes, n_points, k, ids_are_float, hidden, feat;
    float slope;
};

// the lanes of the wave for which pred holds, lane 0 in bit 0
__device__ __forceinline__ unsigned long long shape_ballot(bool pred, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return __ballot(pred);
#else
    long long m = pred ? (long long)(1ull << lane) : 0;
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o);
    return (unsigned long long)m;
#endif
}

// s > 0 read from the bits: the library is built with -fno-honor-nans, under which a comparison need not reject a NaN, and the
// derivative of the leaky at a NaN is part of the definition (the slope's side, as `s > 0 ? 1 : slope` says)
__device__ __forceinline__ bool shape_positive(float s) {
    uint32_t b;
    memcpy(&b, &s, 4);
    return b - 1u < 0x7f800000u;                         // (+0, +inf]
}

// points[u][idx], a NaN point for an index outside [0, n_points)
__device__ __forceinline__ void shape_load_point(const float* __restrict__ points, int u, int idx, int n_points, float& p0, float& p1,
                                                 float& p2) {
    if ((uint32_t)idx < (uint32_t)n_points) {
        const float* p = points + ((size_t)u * n_points + idx) * 3;
        p0 = p[0], p1 = p[1], p2 = p[2];
    } else {
        const uint32_t nan_bits = SHAPE_NAN_BITS;
        memcpy(&p0, &nan_bits, 4);
        p1 = p0, p2 = p0;
    }
}

// Workgroup (u, c) of shape_threads(F) threads: pkey[u][c][f] = the largest key of s_j[f] over the chunk's points, pj[u][c][f]
// the smallest j that has it, if u occurs in ids; else pj[u][0][f] = -1 (by workgroup (u, 0))
extern "C" __global__ void __launch_bounds__(SHAPE_THREADS_MAX)
irbpp_shape_partial_arg_kernel(const float* __restrict__ points, const int32_t* __restrict__ indices, const void* __restrict__ ids,
                               const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                               const float* __restrict__ b2, uint32_t* __restrict__ pkey, int32_t* __restrict__ pj, ShapeArgs g) {
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
    if (!mine) {                                         // the whole workgroup
        if (c == 0 && tid < g.feat) pj[(size_t)u * g.chunks * g.feat + tid] = -1;
        return;
    }

    const int f0 = front_wave_uniform(tid >> 6) * SHAPE_FBLOCK;
    const int nf = g.feat - f0 < SHAPE_FBLOCK ? g.feat - f0 : SHAPE_FBLOCK;
    const int j0 = c * g.chunk_points;
    const int j1 = j0 + g.chunk_points < g.k ? j0 + g.chunk_points : g.k;
    uint32_t mine_key = 0u;                               // lane m: the running maximum of feature f0 + m ...
    int mine_j = 0;                                       // ... and the first position that reached it
    for (int jb = j0; jb < j1; jb += 64) {               // wave-uniform trips, j ascending
        const bool has = jb + lane < j1;                 // a lane past j1: the key 0, which no value has
        float p0, p1, p2;
        shape_load_point(points, u, indices[has ? jb + lane : j1 - 1], g.n_points, p0, p1, p2);
        float acc[SHAPE_FBLOCK];
        shape_point(p0, p1, p2, w1, b1, w2, b2, g.hidden, g.slope, f0, nf, acc);
#pragma unroll
        for (int m = 0; m < SHAPE_FBLOCK; ++m) {
            if (m < nf) {
                const uint32_t own = has ? shape_key(acc[m]) : 0u;
                uint32_t key = own;
                for (int o = 32; o > 0; o >>= 1) {
                    const uint32_t other = (uint32_t)__shfl_xor((int)key, o);
                    key = other > key ? other : key;
                }
                // lane jb's point is in the trip, so key > 0 and some lane holds it: the lowest one is the smallest j
                const int first = __builtin_ctzll(shape_ballot(own == key, lane));
                if (lane == m && key > mine_key) mine_key = key, mine_j = jb + first;
            }
        }
    }
    if (lane < nf) {
        const size_t o = ((size_t)u * g.chunks + c) * g.feat + f0 + lane;
        pkey[o] = mine_key;
        pj[o] = mine_j;
    }
}

// Thread e < M F: out[m][f] = leaky(max_c pkey[ids[m]][c][f]), a NaN row for an id outside [0, n_shapes).  Thread M F + u F + f:
// arg[u][f] = the j of the first chunk with the largest key, -1 if u does not occur.
extern "C" __global__ void __launch_bounds__(256)
irbpp_shape_gather_arg_kernel(const uint32_t* __restrict__ pkey, const int32_t* __restrict__ pj, const void* __restrict__ ids,
                              float* __restrict__ out, int32_t* __restrict__ arg, ShapeArgs g) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rows = g.m_rows * g.feat;
    if (e < rows) {
        const long long m = e / g.feat;
        const int f = (int)(e - m * g.feat);
        const int u = shape_id(ids, g.ids_are_float, g.ids_stride, m, g.n_shapes);
        uint32_t key = SHAPE_NAN_KEY;
        if (u >= 0) {
            const uint32_t* src = pkey + (size_t)u * g.chunks * g.feat + f;
            key = 0u;
            for (int c = 0; c < g.chunks; ++c) {
                const uint32_t other = src[(size_t)c * g.feat];
                key = other > key ? other : key;
            }
        }
        // leaky is monotone and maps NaN to NaN: applied once, to the maximum
        const uint32_t bits = shape_key_bits(key);
        float s;
        memcpy(&s, &bits, 4);
        const uint32_t out_bits = shape_key_bits(shape_key(front_leaky(s, g.slope)));
        memcpy(&out[m * g.out_stride + f], &out_bits, 4);
        return;
    }
    const long long t = e - rows;
    if (t >= (long long)g.n_shapes * g.feat) return;
    const int u = (int)(t / g.feat), f = (int)(t - (long long)u * g.feat);
    const size_t base = (size_t)u * g.chunks * g.feat + f;
    int j = pj[base];
    if (j >= 0) {                                        // u occurs: every chunk's entry was written
        uint32_t key = pkey[base];
        for (int c = 1; c < g.chunks; ++c) {             // later chunks hold greater j: only a greater key replaces
            const uint32_t other = pkey[base + (size_t)c * g.feat];
            if (other > key) key = other, j = pj[base + (size_t)c * g.feat];
        }
    }
    arg[t] = j;
}

// Workgroup u of SHAPE_GRAD_THREADS threads, if u occurs in ids: pd[u][f] = (p_{u,f}, d2[u][f]), p1[u][i] = (P1[u][i][:], Pb[u][i])
extern "C" __global__ void __launch_bounds__(SHAPE_GRAD_THREADS)
irbpp_shape_backward_shape_kernel(const float* __restrict__ points, const int32_t* __restrict__ indices, const void* __restrict__ ids,
                                  const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                  const float* __restrict__ b2, const int32_t* __restrict__ arg, const float* __restrict__ grad_out,
                                  ShapeQuad* __restrict__ pd, ShapeQuad* __restrict__ p1, ShapeGradArgs g) {
    __shared__ ShapeQuad sp[SHAPE_MAX_WIDTH];
    const int tid = threadIdx.x, lane = tid & 63, u = blockIdx.x;
    // G[u][tid]: every wave scans all ids, 64 at a time, and adds the matching rows in ascending order
    float G = 0.0f;
    int occurs = 0;
    for (long long mb = 0; mb < g.m_rows; mb += 64) {
        const long long m = mb + lane;
        const bool is = m < g.m_rows && shape_id(ids, g.ids_are_float, g.ids_stride, m, g.n_shapes) == u;
        unsigned long long rows = shape_ballot(is, lane);
        occurs |= rows != 0;
        while (rows) {                                   // wave-uniform
            const int b = __builtin_ctzll(rows);
            rows &= rows - 1;
            if (tid < g.feat) G += grad_out[(size_t)(mb + b) * g.feat + tid];
        }
    }
    if (!front_wave_uniform(occurs)) return;             // the whole workgroup: every wave saw the same ids

    if (tid < g.feat) {                                  // thread f: the point of its maximum, its s2 chain again, d2
        const int j = arg[(size_t)u * g.feat + tid];
        float p0, p1v, p2;
        shape_load_point(points, u, (uint32_t)j < (uint32_t)g.k ? indices[j] : -1, g.n_points, p0, p1v, p2);
        const float* wz = w2 + (size_t)tid * g.hidden;
        float s2 = b2[tid];
        for (int i = 0; i < g.hidden; ++i) {
            const float* wr = w1 + (size_t)i * 3;
            const float h = front_leaky(fmaf(p2, wr[2], fmaf(p1v, wr[1], fmaf(p0, wr[0], b1[i]))), g.slope);
            s2 = fmaf(h, wz[i], s2);
        }
        ShapeQuad q;
        q.x = p0, q.y = p1v, q.z = p2, q.w = shape_positive(s2) ? G : g.slope * G;
        sp[tid] = q;
        pd[(size_t)u * g.feat + tid] = q;
    }
    __syncthreads();
    if (tid < g.hidden) {                                // thread i: the chains over f of P1[u][i][:] and Pb[u][i]
        const float w10 = w1[tid * 3], w11 = w1[tid * 3 + 1], w12 = w1[tid * 3 + 2], bias = b1[tid];
        ShapeQuad a;
        a.x = 0.0f, a.y = 0.0f, a.z = 0.0f, a.w = 0.0f;
        for (int f = 0; f < g.feat; ++f) {
            const ShapeQuad q = sp[f];
            const float s1 = fmaf(q.z, w12, fmaf(q.y, w11, fmaf(q.x, w10, bias)));
            const float e = q.w * w2[(size_t)f * g.hidden + tid];
            const float ds1 = shape_positive(s1) ? e : g.slope * e;
            a.x = fmaf(ds1, q.x, a.x);
            a.y = fmaf(ds1, q.y, a.y);
            a.z = fmaf(ds1, q.z, a.z);
            a.w += ds1;
        }
        p1[(size_t)u * g.hidden + tid] = a;
    }
}

// One thread per element of dW2 [F][H1], then of db2 [F], then per (i, c) of dW1 [H1][3] (c < 3) and db1 [H1] (c == 3): its sum
// over the shapes that occur, u ascending
extern "C" __global__ void __launch_bounds__(256)
irbpp_shape_backward_reduce_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const int32_t* __restrict__ arg,
                                   const ShapeQuad* __restrict__ pd, const ShapeQuad* __restrict__ p1, float* __restrict__ d_w1,
                                   float* __restrict__ d_b1, float* __restrict__ d_w2, float* __restrict__ d_b2, ShapeGradArgs g) {
    long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n_w2 = (long long)g.feat * g.hidden;
    if (t < n_w2) {
        const int f = (int)(t / g.hidden), i = (int)(t - (long long)f * g.hidden);
        const float w10 = w1[i * 3], w11 = w1[i * 3 + 1], w12 = w1[i * 3 + 2], bias = b1[i];
        float acc = 0.0f;
        for (int u = 0; u < g.n_shapes; ++u) {
            const size_t o = (size_t)u * g.feat + f;
            if (arg[o] < 0) continue;                    // u does not occur: its row of pd was never written
            const ShapeQuad q = pd[o];
            const float h = front_leaky(fmaf(q.z, w12, fmaf(q.y, w11, fmaf(q.x, w10, bias))), g.slope);
            acc = fmaf(q.w, h, acc);
        }
        d_w2[t] = acc;
        return;
    }
    t -= n_w2;
    if (t < g.feat) {
        float acc = 0.0f;
        for (int u = 0; u < g.n_shapes; ++u) {
            const size_t o = (size_t)u * g.feat + t;
            if (arg[o] >= 0) acc += pd[o].w;
        }
        d_b2[t] = acc;
        return;
    }
    t -= g.feat;
    if (t < 4LL * g.hidden) {
        const int i = (int)(t >> 2), c = (int)(t & 3);
        float acc = 0.0f;
        for (int u = 0; u < g.n_shapes; ++u) {
            if (arg[(size_t)u * g.feat] < 0) continue;
            const ShapeQuad q = p1[(size_t)u * g.hidden + i];
            acc += c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
        }
        if (c < 3)
            d_w1[i * 3 + c] = acc;
        else
            d_b1[i] = acc;
    }
}

}  // namespace irbpp

#pragma float_control(pop)
