// Host harness (test infrastructure): the two kernels of irbpp_amd/csrc/irbpp_optim.hip run on the CPU, one workgroup at a time,
// by 256 threads in lockstep (lockstep.h, optim_lockstep.h: barriers, __shared__, the double shuffle, float4).  The kernels'
// own source is compiled, so their chunk indexing, the order of the float64 additions, the 16-byte / dword choice and the
// flags are what the CPU suite checks against the numpy definition; float arithmetic is IEEE on both sides (build with
// -ffp-contract=off).
// With -DOPTIM_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs the step over a few tensor sets in
// buffers of exactly the size the kernels may touch and prints a checksum.
#include <stdio.h>
#include <string.h>

#include "optim_lockstep.h"

#include "../../irbpp_amd/csrc/irbpp_optim.hip"

extern "C" int host_optim_chunk() { return irbpp::OPTIM_CHUNK; }

// irbpp_clipped_adam_step's two launches (the tables are host memory here); returns its argument check's verdict
extern "C" int host_clipped_adam_step(const irbpp_optim_tensor* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                                      double* partial, const irbpp_adam_hyper* hyper, float* total, long long* skipped) {
    if (!tensors || !chunks || !partial || !hyper || !total || !skipped || n_tensors < 1 || n_chunks < n_tensors) return -1;
    run_grid<irbpp::OPTIM_THREADS>(n_chunks, 1, [&] { irbpp::irbpp_grad_sumsq_kernel(tensors, chunks, partial); });
    run_grid<irbpp::OPTIM_THREADS>(n_chunks, 1, [&] {
        irbpp::irbpp_clipped_adam_kernel(tensors, chunks, partial, n_chunks, *hyper, total, skipped);
    });
    return 0;
}

#ifdef OPTIM_HOST_MAIN
// Buffers are exactly as large as the kernels may touch (every tensor a heap block of its own, the odd ones one float into
// a larger block), so a sanitizer sees any access beyond them.
int main() {
    const int sizes[] = {1, 3, 1023, 1024, 1025, 4099, 2500};
    const int T = sizeof(sizes) / sizeof(sizes[0]);
    uint32_t rng = 12345u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    double sum = 0;
    for (int flags : {1, 2, 1 | 4, 8}) {
        std::vector<std::vector<float>> store;
        std::vector<irbpp_optim_tensor> tensors;
        std::vector<int32_t> chunks;
        for (int i = 0; i < T; ++i) {
            const int n = sizes[i], off = i == T - 1 ? 1 : 0;                 // the last tensor: 4-byte aligned only
            float* ptr[5];
            for (int a = 0; a < 5; ++a) {
                store.emplace_back((size_t)n + off);
                for (auto& f : store.back()) f = a == 3 ? fabsf(next()) : next();
                ptr[a] = store.back().data() + off;
            }
            tensors.push_back({ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], n});
            for (int first = 0; first < n; first += irbpp::OPTIM_CHUNK) chunks.push_back(i), chunks.push_back(first);
        }
        std::vector<double> partial(chunks.size() / 2);
        const irbpp_adam_hyper h = {1e-2f, 0.0316f, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 1.0f, flags};
        float total = 0;
        long long skipped = 0;
        if (host_clipped_adam_step(tensors.data(), T, chunks.data(), (int)partial.size(), partial.data(), &h, &total, &skipped)) return 1;
        for (const auto& v : store) for (float f : v) sum += f;
        printf("flags %d: total %.9g skipped %lld checksum %.9g\n", flags, total, skipped, sum);
    }
    return 0;
}
#endif
