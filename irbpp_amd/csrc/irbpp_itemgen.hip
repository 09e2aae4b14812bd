// irbpp_itemgen.hip -- the device item generator: the streams of irbpp_itemgen.h drawn on the GPU, a wave per stream
// (irbpp_itemgen_device.h), so that the item rings of stream mode are refilled without the host: no cursor read-back, no
// synchronisation, no upload.  irbpp_itemgen_dev_draw serves parity tests and tooling, irbpp_stream_refill (irbpp_capi.hip)
// the rings; both advance the same per-stream state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../include/irbpp.h"
#include "irbpp_device.h"
#include "irbpp_itemgen_device.h"

namespace irbpp {

constexpr int ITEMGEN_WAVES = 4;       // streams per workgroup

// per stream, in device memory
struct ItemGenStreams {
    uint32_t* key;          // [n_streams][624]
    int32_t* pos;           // [n_streams] next key word (624: regenerate first)
    long long* delivered;   // [n_streams] items written so far
};

__device__ __forceinline__ void itemgen_load(int lane, uint32_t* k, const uint32_t* key) {
    for (int i = lane; i < MT_N; i += 64) k[i] = key[i];
    IRBPP_ITEMGEN_SYNC();
}
__device__ __forceinline__ void itemgen_store(int lane, const uint32_t* k, uint32_t* key) {
    IRBPP_ITEMGEN_SYNC();
    for (int i = lane; i < MT_N; i += 64) key[i] = k[i];
}

struct DrawSink {
    int32_t* out;
    __device__ __forceinline__ void operator()(int j, int32_t id) const { out[j] = id; }
};
struct RingSink {           // ring slot (first + j) mod len; ids below -1 become -1 as in irbpp_stream_write (-3 is the bins' mark)
    int32_t* row;
    uint32_t first, len;
    __device__ __forceinline__ void operator()(int j, int32_t id) const { row[(first + (uint32_t)j) % len] = id < -1 ? -1 : id; }
};

}  // namespace irbpp

extern "C" __global__ void __launch_bounds__(256)
irbpp_itemgen_seed_kernel(irbpp::ItemGenStreams st, const uint32_t* seeds, int n_streams) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_streams) return;
    irbpp::mt_seed_serial(st.key + (size_t)s * irbpp::MT_N, seeds[s]);
    st.pos[s] = irbpp::MT_N;
    st.delivered[s] = 0;
}

extern "C" __global__ void __launch_bounds__(64 * irbpp::ITEMGEN_WAVES)
irbpp_itemgen_draw_kernel(irbpp::ItemGenStreams st, irbpp::ItemGenTables G, int n_streams, int count, int32_t* out) {
    using namespace irbpp;
    __shared__ uint32_t keys[ITEMGEN_WAVES][MT_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * ITEMGEN_WAVES + wave;
    if (s >= n_streams) return;                      // (no workgroup barrier anywhere: the waves are on their own)
    uint32_t* k = keys[wave];
    uint32_t* key = st.key + (size_t)s * MT_N;
    itemgen_load(lane, k, key);
    DrawSink sink{out + (size_t)s * count};
    const int pos = itemgen_draw_wave(lane, k, st.pos[s], G, count, sink);
    itemgen_store(lane, k, key);
    if (lane == 0) {
        st.pos[s] = pos;
        st.delivered[s] += count;
    }
}

// Bin b is fed by stream first_stream + b: with c its cursor and w what the stream has delivered, the c + len - w slots the
// bin has consumed since are rewritten.  c > w: the bin went past what it was given -- the sticky error word, as at the fetch.
extern "C" __global__ void __launch_bounds__(64 * irbpp::ITEMGEN_WAVES)
irbpp_stream_refill_kernel(irbpp::ItemGenStreams st, irbpp::ItemGenTables G, const irbpp::BinState* bs, int32_t* seq, int N,
                           int seq_len, int first_stream, int32_t* err) {
    using namespace irbpp;
    __shared__ uint32_t keys[ITEMGEN_WAVES][MT_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * ITEMGEN_WAVES + wave;
    if (b >= N) return;
    const int s = first_stream + b;
    const long long w = st.delivered[s];
    const long long c = bs[b].cursor;
    if (c > w) {
        if (lane == 0) atomicOr(err, IRBPP_DEVERR_STREAM_DRY);
        return;
    }
    const int count = (int)(c + seq_len - w);
    if (count <= 0) return;
    uint32_t* k = keys[wave];
    uint32_t* key = st.key + (size_t)s * MT_N;
    itemgen_load(lane, k, key);
    RingSink sink{seq + (size_t)b * seq_len, (uint32_t)(w % seq_len), (uint32_t)seq_len};
    const int pos = itemgen_draw_wave(lane, k, st.pos[s], G, count, sink);
    itemgen_store(lane, k, key);
    if (lane == 0) {
        st.pos[s] = pos;
        st.delivered[s] = w + count;
    }
}

struct irbpp_itemgen_dev {
    int device = 0, n_streams = 0;
    irbpp::ItemGenStreams st{};
    irbpp::ItemGenTables G{};
    uint32_t* seeds = nullptr;
    void* tables[3] = {nullptr, nullptr, nullptr};
};

namespace irbpp {

inline int itemgen_launch_refill(irbpp_itemgen_dev* gen, const BinState* bs, int32_t* seq, int N, int seq_len, int first_stream,
                                 int32_t* err, hipStream_t stream) {
    hipLaunchKernelGGL(irbpp_stream_refill_kernel, dim3((unsigned)((N + ITEMGEN_WAVES - 1) / ITEMGEN_WAVES)),
                       dim3(64 * ITEMGEN_WAVES), 0, stream, gen->st, gen->G, bs, seq, N, seq_len, first_stream, err);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

}  // namespace irbpp

extern "C" {

int irbpp_itemgen_dev_destroy(irbpp_itemgen_dev* g) {
    if (!g) return IRBPP_OK;
    hipSetDevice(g->device);
    hipDeviceSynchronize();                          // a draw or a refill may still be running on some stream
    hipFree(g->st.key);
    hipFree(g->st.pos);
    hipFree(g->st.delivered);
    hipFree(g->seeds);
    for (void* p : g->tables) hipFree(p);
    delete g;
    return IRBPP_OK;
}

int irbpp_itemgen_dev_create(int32_t device, int32_t n_streams, const uint32_t* seeds_host, int32_t n_groups,
                             const int32_t* group_offsets, const int32_t* members, int32_t n_members, void* stream,
                             irbpp_itemgen_dev** out) {
    if (!out || !members || n_members < 1 || n_groups < 0 || (n_groups > 0 && !group_offsets)) return IRBPP_ERR_ARG;
    if (n_streams < 1 || !seeds_host || device < 0) return IRBPP_ERR_ARG;
    if (n_groups > 0) {
        if (group_offsets[0] != 0 || group_offsets[n_groups] != n_members) return IRBPP_ERR_ARG;
        for (int i = 0; i < n_groups; ++i)
            if (group_offsets[i + 1] <= group_offsets[i]) return IRBPP_ERR_ARG;     // np.random.choice of an empty list raises
    }
    if (hipSetDevice(device) != hipSuccess) return IRBPP_ERR_HIP;
    irbpp_itemgen_dev* g = new (std::nothrow) irbpp_itemgen_dev();
    if (!g) return IRBPP_ERR_NOMEM;
    g->device = device;
    g->n_streams = n_streams;
    const size_t n = (size_t)n_streams;
    uint32_t* masks_host = n_groups > 0 ? new (std::nothrow) uint32_t[n_groups] : nullptr;
    bool ok = n_groups == 0 || masks_host != nullptr;
    ok = ok && hipMalloc((void**)&g->st.key, n * irbpp::MT_N * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc((void**)&g->st.pos, n * sizeof(int32_t)) == hipSuccess;
    ok = ok && hipMalloc((void**)&g->st.delivered, n * sizeof(long long)) == hipSuccess;
    ok = ok && hipMalloc((void**)&g->seeds, n * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc(&g->tables[0], (size_t)n_members * sizeof(int32_t)) == hipSuccess;
    if (n_groups > 0) {
        ok = ok && hipMalloc(&g->tables[1], (size_t)(n_groups + 1) * sizeof(int32_t)) == hipSuccess;
        ok = ok && hipMalloc(&g->tables[2], (size_t)n_groups * sizeof(uint32_t)) == hipSuccess;
    }
    if (!ok) {
        delete[] masks_host;
        irbpp_itemgen_dev_destroy(g);
        return IRBPP_ERR_NOMEM;
    }
    ok = hipMemcpy(g->seeds, seeds_host, n * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(g->tables[0], members, (size_t)n_members * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (n_groups > 0) {
        for (int i = 0; i < n_groups; ++i) masks_host[i] = irbpp::randint_mask((uint32_t)(group_offsets[i + 1] - group_offsets[i]) - 1u);
        ok = ok && hipMemcpy(g->tables[1], group_offsets, (size_t)(n_groups + 1) * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(g->tables[2], masks_host, (size_t)n_groups * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    }
    delete[] masks_host;
    if (ok) {
        g->G.n_groups = n_groups;
        g->G.n_members = n_members;
        g->G.members = (const int32_t*)g->tables[0];
        g->G.offsets = (const int32_t*)g->tables[1];
        g->G.group_mask = (const uint32_t*)g->tables[2];
        g->G.mask0 = irbpp::randint_mask((uint32_t)(n_groups > 0 ? n_groups : n_members) - 1u);
        // init_genrand on the device, a thread per stream: the upload is the seeds, not 2.5 KB of key words per stream
        hipLaunchKernelGGL(irbpp_itemgen_seed_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           g->st, g->seeds, n_streams);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) {
        irbpp_itemgen_dev_destroy(g);
        return IRBPP_ERR_HIP;
    }
    *out = g;
    return IRBPP_OK;
}

int irbpp_itemgen_dev_draw(irbpp_itemgen_dev* g, int32_t count, int32_t* out_dev, void* stream) {
    if (!g || count < 0 || (count > 0 && !out_dev)) return IRBPP_ERR_ARG;
    if (count == 0) return IRBPP_OK;
    hipLaunchKernelGGL(irbpp_itemgen_draw_kernel, dim3((unsigned)((g->n_streams + irbpp::ITEMGEN_WAVES - 1) / irbpp::ITEMGEN_WAVES)),
                       dim3(64 * irbpp::ITEMGEN_WAVES), 0, (hipStream_t)stream, g->st, g->G, g->n_streams, count, out_dev);
    return hipGetLastError() == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

int irbpp_itemgen_dev_delivered(irbpp_itemgen_dev* g, int64_t* out_dev, void* stream) {
    if (!g || !out_dev) return IRBPP_ERR_ARG;
    return hipMemcpyAsync(out_dev, g->st.delivered, (size_t)g->n_streams * sizeof(int64_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream) == hipSuccess ? IRBPP_OK : IRBPP_ERR_HIP;
}

}  // extern "C"
