// irbpp_metrics.hip -- the trainer's logged episode metrics on the device (trainer.py:145-147, 168-178, 215-222): the three
// deque(maxlen=W) of finished episodes' round(r, 6) / ratio / counter, kept as a window per environment and updated by one
// small launch behind every step, plus the merge of several such windows (groups of bins, ranks) into the rows the trainer
// logs -- (T, n, mean r, max r, min r, mean ratio, mean counter) -- bit for bit, read back every few hundred steps instead of a
// host round trip per step.  Buffers are the caller's (irbpp_episode_window, include/irbpp.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "irbpp_metrics.h"

namespace irbpp {

constexpr int WINDOW_MAX = 1024;
constexpr int WINDOW_PARTS_MAX = 64;
constexpr int WINDOW_UPDATE_THREADS = 1024;

// The window of one environment after one step.  One workgroup: thread t owns a contiguous segment of the N done flags (in bin
// order); a workgroup scan of the per-thread counts gives every finished bin its rank j among the F finished this step.  Only
// the last m = min(F, W) can survive in the window: rank j >= F - m is appended to the ring at (head + fill + j - (F - m)) % W,
// over the oldest entries, which are exactly the ones the deque would drop.  Then the window, oldest first, goes to snapshot
// row T % H with (T, fill) beside it, and the state advances.  state = {steps recorded, fill, ring head, unused}.
extern "C" __global__ void __launch_bounds__(WINDOW_UPDATE_THREADS)
irbpp_window_update_kernel(const uint8_t* __restrict__ done, const double* __restrict__ ep_reward, const double* __restrict__ ratio,
                           const int32_t* __restrict__ counter, int n, int global_offset, irbpp_episode_entry* __restrict__ ring,
                           irbpp_episode_entry* __restrict__ snap, int32_t* __restrict__ rows, int32_t* __restrict__ state, int W,
                           int H) {
    __shared__ int wave_total[WINDOW_UPDATE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int T = state[0] + 1, fill = state[1], head = state[2];
    const int seg = (n + WINDOW_UPDATE_THREADS - 1) / WINDOW_UPDATE_THREADS;
    const int lo = min(n, tid * seg), hi = min(n, lo + seg);
    int c = 0;
    for (int b = lo; b < hi; ++b) c += done[b] != 0;
    int incl = c;                                            // inclusive scan: in the wave, then across the waves
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_total[wid] = incl;
    __syncthreads();
    int before = 0, F = 0;
    for (int w = 0; w < WINDOW_UPDATE_THREADS / 64; ++w) {
        const int v = wave_total[w];
        before += w < wid ? v : 0;
        F += v;
    }
    const int m = min(F, W);
    const int first_kept = F - m;
    int j = before + incl - c;                               // rank of this segment's first finished bin
    if (c > 0 && j + c > first_kept) {
        for (int b = lo; b < hi; ++b) {
            if (!done[b]) continue;
            if (j >= first_kept) {
                irbpp_episode_entry e;
                e.key = ((int64_t)T << 32) | (int64_t)(uint32_t)(global_offset + b);
                e.r = py_round6(ep_reward[b]);
                e.ratio = ratio[b];
                e.counter = counter[b];
                e.reserved = 0;
                ring[(head + fill + (j - first_kept)) % W] = e;
            }
            ++j;
        }
    }
    __syncthreads();                                         // the appended entries are visible to the whole workgroup
    const int fill2 = min(fill + m, W);
    const int head2 = (head + fill + m - fill2) % W;
    const int row = T % H;
    irbpp_episode_entry* out = snap + (size_t)row * W;
    for (int i = tid; i < fill2; i += WINDOW_UPDATE_THREADS) out[i] = ring[(head2 + i) % W];
    if (tid == 0) {
        rows[2 * row] = T;
        rows[2 * row + 1] = fill2;
        state[0] = T;
        state[1] = fill2;
        state[2] = head2;
    }
}

struct WindowParts {
    const irbpp_episode_entry* snap[WINDOW_PARTS_MAX];
    const int32_t* rows[WINDOW_PARTS_MAX];
    const int32_t* state[WINDOW_PARTS_MAX];
    int P, W, H;
};

// One wave per step t = first + blockIdx.x: the global window at t is the newest min(W, sum of fills) entries of the union of
// the parts' snapshots at t (tail_merge; with one part the snapshot itself), staged in LDS oldest first, then the statistics
// the trainer logs: np.mean as np_sum / n, max and min exact.  out row = (t, n, mean r, max r, min r, mean ratio, mean counter),
// NaN where n == 0 (the trainer logs nothing).  A step some part has not recorded yet gets n = -2, a step whose snapshot row
// has been overwritten since (more than H steps ago) n = -1, both with NaN values: never a row of the wrong step.
extern "C" __global__ void __launch_bounds__(64)
irbpp_window_metrics_kernel(const WindowParts parts, int first, double* __restrict__ out) {
    extern __shared__ double lds_window[];                  // [3][W]: r, ratio, counter
    double* wr = lds_window;
    double* wq = lds_window + parts.W;
    double* wc = lds_window + 2 * parts.W;
    const int lane = threadIdx.x;
    const int t = first + blockIdx.x;
    const int P = parts.P, W = parts.W, row = t % parts.H;
    double* o = out + (size_t)blockIdx.x * 7;
    const bool mine = lane < P;
    const int recorded = mine ? parts.state[lane][0] : t;
    const int row_step = mine ? parts.rows[lane][2 * row] : t;
    const int fill = mine ? min(max(parts.rows[lane][2 * row + 1], 0), W) : 0;
    const bool not_yet = metrics_ballot(recorded < t) != 0;
    const bool lost = metrics_ballot(row_step != t) != 0;
    int total = fill;
    for (int s = 32; s > 0; s >>= 1) total += __shfl_xor(total, s);
    const int n = min(W, total);
    if (lane == 0) {
        o[0] = (double)t;
        o[1] = not_yet ? -2.0 : lost ? -1.0 : (double)n;
    }
    if (not_yet || lost || n == 0) {
        if (lane >= 2 && lane < 7) o[lane] = NAN;
        return;
    }
    const irbpp_episode_entry* mysnap = mine ? parts.snap[lane] + (size_t)row * W : nullptr;
    if (P == 1) {
        const irbpp_episode_entry* only = parts.snap[0] + (size_t)row * W;
        for (int i = lane; i < n; i += 64) {
            const irbpp_episode_entry e = only[i];
            wr[i] = e.r; wq[i] = e.ratio; wc[i] = (double)e.counter;
        }
    } else {
        tail_merge(lane, P, fill, n, [&](int i) { return mysnap[i].key; },
                   [&](int i, int slot) { const irbpp_episode_entry e = mysnap[i]; wr[slot] = e.r; wq[slot] = e.ratio; wc[slot] = (double)e.counter; });
    }
    __syncthreads();
    if (lane == 0) {
        double hi = wr[0], lo = wr[0];
        for (int i = 1; i < n; ++i) { hi = fmax(hi, wr[i]); lo = fmin(lo, wr[i]); }
        o[2] = np_sum(wr, n) / (double)n;
        o[3] = hi;
        o[4] = lo;
        o[5] = np_sum(wq, n) / (double)n;
        o[6] = np_sum(wc, n) / (double)n;
    }
}

}  // namespace irbpp
