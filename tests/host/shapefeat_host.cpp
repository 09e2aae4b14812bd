// Host harness (test infrastructure): the two kernels of irbpp_amd/csrc/irbpp_shapefeat.hip run on the CPU, one workgroup at a
// time, its threads in lockstep (lockstep.h; shuffles wait for their own wave, since the waves of a workgroup reduce different
// numbers of features).  The kernels' own source is compiled, so the chains, the blocks of features and hidden units, the
// trips and chunks, the keys of the max and the id rules are what the CPU suite checks against the numpy definition; fmaf is
// the C library's, a single rounding (build with -ffp-contract=off).  host_shape_features repeats the launches of
// irbpp_shape_features (irbpp_capi.hip) after its argument checks; chunk_points > 0 forces another split of the points than
// the library would choose (the bits must not depend on it).
// With -DSHAPEFEAT_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the kernels over a few shapes
// with buffers exactly as large as the kernels may touch and prints a checksum.
#include <stdio.h>

#include "lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_shapefeat.hip"

extern "C" int host_shape_chunks(int n_shapes, int k) { return irbpp::shape_chunks(n_shapes, k); }

// w: w1, b1, w2, b2.  Returns the number of chunks used (partial: float32 [n_shapes][chunks][feat]).
extern "C" int host_shape_features(const float* points, int n_shapes, int n_points, const int32_t* indices, int k, const void* ids,
                                   int ids_are_float, long long ids_stride, long long m_rows, const float* const* w, int hidden, int feat,
                                   float slope, float* partial, int chunk_points, float* out, long long out_stride) {
    irbpp::ShapeArgs g;
    g.ids_stride = ids_stride, g.m_rows = m_rows, g.out_stride = out_stride;
    g.n_shapes = n_shapes, g.n_points = n_points, g.k = k, g.ids_are_float = ids_are_float, g.hidden = hidden, g.feat = feat;
    g.chunk_points = chunk_points > 0 ? chunk_points : irbpp::shape_chunk_points(n_shapes, k);
    g.chunks = (k + g.chunk_points - 1) / g.chunk_points;
    g.slope = slope;
    LockstepLaunch how;
    how.wave_shuffles = true;
    const int threads = irbpp::shape_threads(feat);
    lockstep_launch(threads, n_shapes, g.chunks, [&] { irbpp::irbpp_shape_partial_kernel(points, indices, ids, w[0], w[1], w[2], w[3], partial, g); },
                    how);
    lockstep_launch(256, (int)((m_rows * feat + 255) / 256), 1, [&] { irbpp::irbpp_shape_gather_kernel(partial, ids, out, g); }, how);
    return g.chunks;
}

#ifdef SHAPEFEAT_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    const int cases[][7] = {{1, 1, 1, 5, 3, 1, 0},      {3, 50, 65, 130, 67, 5, 0},  {7, 40, 200, 128, 128, 9, 0},
                            {2, 9, 100, 16, 256, 4, 64}, {300, 4, 150, 5, 3, 6, 0}};   // n_shapes, P, k, H1, F, M, forced chunk_points
    uint32_t rng = 12345u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (const auto& cs : cases) {
        const int n_shapes = cs[0], P = cs[1], k = cs[2], H1 = cs[3], F = cs[4], M = cs[5], forced = cs[6];
        std::vector<float> points((size_t)n_shapes * P * 3), w1((size_t)H1 * 3), b1(H1), w2((size_t)F * H1), b2(F);
        for (auto* t : {&points, &w1, &b1, &w2, &b2}) for (auto& f : *t) f = next();
        std::vector<int32_t> indices(k);
        for (int j = 0; j < k; ++j) indices[j] = (int32_t)((next() * 0.5f + 0.5f) * (P - 1));
        indices[0] = P - 1;
        const float* w[4] = {w1.data(), b1.data(), w2.data(), b2.data()};
        const int cp = forced ? forced : irbpp::shape_chunk_points(n_shapes, k);
        const int chunks = (k + cp - 1) / cp;
        std::vector<float> partial((size_t)n_shapes * chunks * F), out((size_t)M * F);
        for (int as_float = 0; as_float < 2; ++as_float) {
            const int stride = 1 + as_float * 2;                 // the last element of a strided column ends the buffer
            std::vector<long long> ids_i((size_t)(M - 1) * stride + 1);
            std::vector<float> ids_f((size_t)(M - 1) * stride + 1);
            for (int m = 0; m < M; ++m) {
                const int id = m == 1 ? -1 : m == 2 ? n_shapes : (m * 5) % n_shapes;      // a bad id on either side
                ids_i[(size_t)m * stride] = id;
                ids_f[(size_t)m * stride] = (float)id + (id >= 0 ? 0.75f : 0.0f);
            }
            const void* ids = as_float ? (const void*)ids_f.data() : (const void*)ids_i.data();
            if (host_shape_features(points.data(), n_shapes, P, indices.data(), k, ids, as_float, stride, M, w, H1, F, 0.01f, partial.data(),
                                    forced, out.data(), F) != chunks)
                return 1;
            for (int m = 0; m < M; ++m)
                for (int f = 0; f < F; ++f) {
                    const float v = out[(size_t)m * F + f];
                    if ((v != v) != (m == 1 || m == 2)) return 2;
                    if (v == v) sum += v;
                }
        }
        printf("n_shapes %d P %d k %d H1 %d F %d M %d chunks %d: checksum %.9g\n", n_shapes, P, k, H1, F, M, chunks, sum);
    }
    return 0;
}
#endif
