// Host harness (test infrastructure): the four kernels of irbpp_amd/csrc/irbpp_shapefeat_grad.hip run on the CPU, one workgroup
// at a time, its threads in lockstep (lockstep.h; shuffles wait for their own wave; the wave's ballot is an OR over shuffles,
// shape_ballot's host branch).  The kernels' own source is compiled, so the running (key, j) maximum over trips and chunks, the
// ordered sum of the gradient rows, the recomputed chains and the chains over f and u are what the CPU suite checks against the
// numpy definition; fmaf is the C library's (build with -ffp-contract=off).  host_shape_features_arg and
// host_shape_features_backward repeat the launches of the two entry points (irbpp_capi.hip) after their argument checks;
// chunk_points > 0 forces another split of the points than the library would choose (no bit may depend on it).
// With -DSHAPE_GRAD_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the kernels over a few shapes
// with buffers exactly as large as the kernels may touch and prints a checksum.
#include <stdio.h>
#include <string.h>

#include "lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_shapefeat.hip"
#include "../../irbpp_amd/csrc/irbpp_shapefeat_grad.hip"

extern "C" int host_shape_grad_chunks(int n_shapes, int k) { return irbpp::shape_chunks(n_shapes, k); }

// w: w1, b1, w2, b2.  pkey, pj: [n_shapes][chunks][feat]; arg int32 [n_shapes][feat].  Returns the number of chunks used.
extern "C" int host_shape_features_arg(const float* points, int n_shapes, int n_points, const int32_t* indices, int k, const void* ids,
                                       int ids_are_float, long long ids_stride, long long m_rows, const float* const* w, int hidden,
                                       int feat, float slope, uint32_t* pkey, int32_t* pj, int chunk_points, float* out,
                                       long long out_stride, int32_t* arg) {
    irbpp::ShapeArgs g;
    g.ids_stride = ids_stride, g.m_rows = m_rows, g.out_stride = out_stride;
    g.n_shapes = n_shapes, g.n_points = n_points, g.k = k, g.ids_are_float = ids_are_float, g.hidden = hidden, g.feat = feat;
    g.chunk_points = chunk_points > 0 ? chunk_points : irbpp::shape_chunk_points(n_shapes, k);
    g.chunks = (k + g.chunk_points - 1) / g.chunk_points;
    g.slope = slope;
    LockstepLaunch how;
    how.wave_shuffles = true;
    lockstep_launch(irbpp::shape_threads(feat), n_shapes, g.chunks,
                    [&] { irbpp::irbpp_shape_partial_arg_kernel(points, indices, ids, w[0], w[1], w[2], w[3], pkey, pj, g); }, how);
    const long long elems = (m_rows + n_shapes) * feat;
    lockstep_launch(256, (int)((elems + 255) / 256), 1, [&] { irbpp::irbpp_shape_gather_arg_kernel(pkey, pj, ids, out, arg, g); }, how);
    return g.chunks;
}

// grad_out [m_rows][feat]; pd [n_shapes][feat][4], first [n_shapes][hidden][4], both 16-byte aligned; d: d_w1, d_b1, d_w2, d_b2
extern "C" void host_shape_features_backward(const float* points, int n_shapes, int n_points, const int32_t* indices, int k,
                                             const void* ids, int ids_are_float, long long ids_stride, long long m_rows,
                                             const float* const* w, int hidden, int feat, float slope, const int32_t* arg,
                                             const float* grad_out, float* pd, float* first, float* const* d) {
    irbpp::ShapeGradArgs g;
    g.ids_stride = ids_stride, g.m_rows = m_rows, g.n_shapes = n_shapes, g.n_points = n_points, g.k = k;
    g.ids_are_float = ids_are_float, g.hidden = hidden, g.feat = feat, g.slope = slope;
    LockstepLaunch how;
    how.wave_shuffles = true;
    lockstep_launch(irbpp::SHAPE_GRAD_THREADS, n_shapes, 1, [&] {
        irbpp::irbpp_shape_backward_shape_kernel(points, indices, ids, w[0], w[1], w[2], w[3], arg, grad_out, (irbpp::ShapeQuad*)pd,
                                                 (irbpp::ShapeQuad*)first, g);
    }, how);
    const long long elems = (long long)feat * hidden + feat + 4LL * hidden;
    lockstep_launch(256, (int)((elems + 255) / 256), 1, [&] {
        irbpp::irbpp_shape_backward_reduce_kernel(w[0], w[1], arg, (const irbpp::ShapeQuad*)pd, (const irbpp::ShapeQuad*)first, d[0], d[1],
                                                  d[2], d[3], g);
    }, how);
}

#ifdef SHAPE_GRAD_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    const int cases[][7] = {{1, 1, 1, 1, 1, 1, 0},      {3, 50, 65, 17, 33, 7, 0},  {5, 40, 130, 128, 128, 9, 0},
                            {2, 9, 100, 16, 256, 4, 64}, {2, 9, 70, 256, 5, 70, 0}, {300, 4, 150, 5, 3, 6, 0}};   // n_shapes, P, k, H1, F, M, forced chunk_points
    uint32_t rng = 4321u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (const auto& cs : cases) {
        const int n_shapes = cs[0], P = cs[1], k = cs[2], H1 = cs[3], F = cs[4], M = cs[5], forced = cs[6];
        std::vector<float> points((size_t)n_shapes * P * 3), w1((size_t)H1 * 3), b1(H1), w2((size_t)F * H1), b2(F), grad((size_t)M * F);
        for (auto* t : {&points, &w1, &b1, &w2, &b2, &grad}) for (auto& f : *t) f = next();
        std::vector<int32_t> indices(k);
        for (int j = 0; j < k; ++j) indices[j] = (int32_t)((next() * 0.5f + 0.5f) * (P - 1));
        indices[0] = P - 1;
        const float* w[4] = {w1.data(), b1.data(), w2.data(), b2.data()};
        const int cp = forced ? forced : irbpp::shape_chunk_points(n_shapes, k);
        const int chunks = (k + cp - 1) / cp;
        std::vector<uint32_t> pkey((size_t)n_shapes * chunks * F);
        std::vector<int32_t> pj((size_t)n_shapes * chunks * F), arg((size_t)n_shapes * F);
        std::vector<float> out((size_t)M * F), pd((size_t)n_shapes * F * 4), first((size_t)n_shapes * H1 * 4);
        std::vector<float> d_w1((size_t)H1 * 3), d_b1(H1), d_w2((size_t)F * H1), d_b2(F);
        float* d[4] = {d_w1.data(), d_b1.data(), d_w2.data(), d_b2.data()};
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
            if (host_shape_features_arg(points.data(), n_shapes, P, indices.data(), k, ids, as_float, stride, M, w, H1, F, 0.01f, pkey.data(),
                                        pj.data(), forced, out.data(), F, arg.data()) != chunks)
                return 1;
            for (size_t e = 0; e < arg.size(); ++e)
                if (arg[e] < -1 || arg[e] >= k) return 2;
            host_shape_features_backward(points.data(), n_shapes, P, indices.data(), k, ids, as_float, stride, M, w, H1, F, 0.01f, arg.data(),
                                         grad.data(), pd.data(), first.data(), d);
            for (auto* t : {&d_w1, &d_b1, &d_w2, &d_b2})
                for (float v : *t) {
                    if (v != v) return 3;
                    sum += v;
                }
        }
        printf("n_shapes %d P %d k %d H1 %d F %d M %d chunks %d: checksum %.9g\n", n_shapes, P, k, H1, F, M, chunks, sum);
    }
    return 0;
}
#endif
