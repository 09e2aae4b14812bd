// Host harness (test infrastructure): the two kernels of irbpp_amd/csrc/irbpp_dueling_loss.hip run on the CPU, one workgroup at
// a time, by 512 threads in lockstep (the workgroup's size; lockstep.h: barriers, __shared__, and a blockIdx of the two
// dimensions the backward kernel's grid has).  The kernels' own source is compiled, so their indexing, the column
// means, the row loop and the stepped stores are what the CPU suite checks against the numpy definition; float arithmetic is
// IEEE float32 on both sides (build with -ffp-contract=off).
// With -DDUELING_LOSS_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs both kernels over a few
// shapes in buffers of exactly the size they may touch and prints a checksum.
#include <stdio.h>

#include "lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_dueling_loss.hip"

extern "C" int host_dueling_loss_chunk_rows() { return irbpp::DUELING_LOSS_CHUNK_ROWS; }

extern "C" float host_dueling_dlog(float d) { return irbpp::dueling_dlog(d); }

extern "C" void host_dueling_loss(const float* v, long long v_stride, const float* a, long long env_stride, long long row_stride,
                                  const int64_t* actions, const float* m, int atoms, int s_rows, int batch, float* loss, float* g) {
    run_grid<irbpp::DUELING_THREADS>(batch, 1, [&] {
        irbpp::irbpp_dueling_loss_kernel(v, v_stride, a, env_stride, row_stride, actions, m, atoms, s_rows, loss, g);
    });
}

// the grid of irbpp_dueling_loss_backward: (batch, chunks of rows), one chunk when grad_a is not asked for
extern "C" void host_dueling_loss_backward(const float* g, const float* grad_loss, const int64_t* actions, int atoms, int s_rows,
                                           int batch, float* grad_v, float* grad_a) {
    const int chunks = grad_a ? (s_rows + irbpp::DUELING_LOSS_CHUNK_ROWS - 1) / irbpp::DUELING_LOSS_CHUNK_ROWS : 1;
    run_grid<irbpp::DUELING_THREADS>(batch, chunks, [&] {
        irbpp::irbpp_dueling_loss_backward_kernel(g, grad_loss, actions, atoms, s_rows, grad_v, grad_a);
    });
}

#ifdef DUELING_LOSS_HOST_MAIN
// Buffers are exactly as large as the kernels may touch, so a sanitizer sees any access beyond them.
int main() {
    const int shapes[][3] = {{1, 2, 2}, {3, 2, 3}, {17, 31, 5}, {65, 31, 2}, {500, 31, 2}, {33, 51, 1}, {1024, 128, 1}};
    uint32_t rng = 12345u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 8.0f - 4.0f; };
    double sum = 0;
    for (const auto& sh : shapes) {
        const int s = sh[0], atoms = sh[1], n = sh[2];
        std::vector<float> v((size_t)n * atoms), a((size_t)n * s * atoms), m((size_t)n * atoms), w(n), loss(n), g((size_t)n * atoms),
            gv((size_t)n * atoms), ga((size_t)n * s * atoms);
        std::vector<int64_t> act(n);
        for (auto* x : {&v, &a}) for (auto& f : *x) f = next();
        for (auto& f : m) f = fabsf(next()) / (4.0f * atoms);
        for (auto& f : w) f = fabsf(next());
        a[0] = 200.0f;                                   // most of row 0's e are exactly 0
        const int64_t picks[] = {0, s - 1, -1, (int64_t)s};                    // first, last, from the end, out of range
        for (int e = 0; e < n; ++e) act[e] = picks[e % 4];
        if (n == 1) act[0] = s / 2;
        host_dueling_loss(v.data(), atoms, a.data(), (long long)s * atoms, atoms, act.data(), m.data(), atoms, s, n, loss.data(),
                          g.data());
        host_dueling_loss_backward(g.data(), w.data(), act.data(), atoms, s, n, gv.data(), ga.data());
        host_dueling_loss_backward(g.data(), w.data(), act.data(), atoms, s, n, gv.data(), nullptr);
        host_dueling_loss_backward(g.data(), w.data(), act.data(), atoms, s, n, nullptr, ga.data());
        for (float f : loss) sum += f == f ? f : 1.0;
        for (float f : g) sum += f;
        for (float f : gv) sum += f;
        for (float f : ga) sum += f;
        printf("S %d atoms %d n %d: checksum %.9g\n", s, atoms, n, sum);
    }
    return 0;
}
#endif
