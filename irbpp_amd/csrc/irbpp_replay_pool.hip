// irbpp_replay_pool.hip -- the N per-env replay memories of irbpp_replay.hip sampled as ONE prioritised memory: a learning
// batch of B transitions stratified over the pooled priority mass whatever N is (B < N included, which the per-env calls
// -- B >= 1 draws from every env -- cannot express), and the B priorities written back to whichever memories they came from.
// The reference has no counterpart: its batch is the concatenation of the per-worker batches (agent.py:69-84).  What it
// fixes stays as it is: float32 throughout, node = left + right, descent by `v <= left ? left : (v - left, right)`
// (memory.py:72-86), the validity test of memory.py:175, the weights of memory.py:199-202, _get_transition_new.
//
// The pooled tree is a top tree over the N row roots (an implicit heap over P leaves, P the power of two >= N, padding 0)
// with each env's own tree hanging below its leaf.  The top tree is rebuilt in LDS by every sample launch and never stored.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace irbpp {

constexpr int POOL_MAX_DRAWS = 1024;                     // draws of one sample launch, triples of one update launch
constexpr uint32_t POOL_RNG_ENV = 0xFFFFFFFFu;            // uniform01's env field for pooled draws: no env has this number

// One workgroup of 256 threads.  LDS: the top tree, 2*top_leaves - 1 floats (at least 8: the reductions' scratch), dynamic.
// values == nullptr: draw j is j * segment + u * segment, redrawn up to max_tries times while invalid; otherwise values[j] is
// the position itself and is looked up once.  failed[0] |= 1 if some draw stayed invalid.
extern "C" __global__ void __launch_bounds__(256)
irbpp_replay_pool_sample_kernel(const float* __restrict__ tree, const int64_t* __restrict__ index, const uint8_t* __restrict__ full,
                                int n_env, int cap, int top_leaves, int b, int n_step, const float* __restrict__ values, uint64_t seed,
                                int max_tries, float beta, int64_t* __restrict__ env_out, float* __restrict__ prob,
                                int64_t* __restrict__ data_idx, int64_t* __restrict__ tree_idx, float* __restrict__ weight,
                                int32_t* __restrict__ failed) {
    HIP_DYNAMIC_SHARED(float, top)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = 2 * cap - 1, top_len = 2 * top_leaves - 1;
    // filled: the integer sum over envs of (capacity if full else index), converted once
    long long part = 0;
    for (int e = tid; e < n_env; e += 256) part += full[e] ? (long long)cap : (long long)index[e];
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    long long* scratch = (long long*)top;
    if (lane == 0) scratch[wave] = part;
    __syncthreads();
    const float filled = (float)(scratch[0] + scratch[1] + scratch[2] + scratch[3]);
    __syncthreads();
    // top tree: leaves from the row roots, then one level per barrier
    for (int e = tid; e < top_leaves; e += 256) top[top_leaves - 1 + e] = e < n_env ? tree[(size_t)e * len] : 0.0f;
    __syncthreads();
    for (int width = top_leaves >> 1; width >= 1; width >>= 1) {
        const int lo = width - 1;
        for (int i = lo + tid; i < lo + width; i += 256) top[i] = top[2 * i + 1] + top[2 * i + 2];
        __syncthreads();
    }
    const float p_total = top[0];
    const float segment = p_total / (float)b;
    float wmax = 0.0f;
    for (int j = tid; j < b; j += 256) {
        const float lo = (float)j * segment;
        const int tries = values ? 1 : max_tries;
        float p = 0.0f;
        int env = 0, idx = cap - 1;
        bool ok = false;
        for (int attempt = 0; attempt < tries && !ok; ++attempt) {
            float v = values ? values[j] : lo + uniform01(seed, POOL_RNG_ENV, (uint32_t)j, (uint32_t)attempt) * segment;
            int t = 0;
            for (;;) {
                const int left = 2 * t + 1;
                if (left >= top_len) break;
                const float lv = top[left];
                if (v <= lv) t = left;
                else { v = v - lv; t = left + 1; }
            }
            env = t - (top_leaves - 1);
            if (env >= n_env) {                                   // a padding leaf: no memory below it
                env = n_env - 1; idx = cap - 1; p = 0.0f;
                continue;
            }
            const float* row = tree + (size_t)env * len;          // the same walk carries on in env's own tree, in global memory
            idx = 0;
            for (;;) {
                const int left = 2 * idx + 1;
                if (left >= len) break;
                const float lv = row[left];
                if (v <= lv) idx = left;
                else { v = v - lv; idx = left + 1; }
            }
            p = row[idx];
            const int w = (int)index[env];
            const int d = idx - (cap - 1);
            int a = (w - d) % cap, c = (d - w) % cap;             // Python's % : non-negative
            if (a < 0) a += cap;
            if (c < 0) c += cap;
            ok = a > n_step && c >= 1 && p != 0.0f;               // memory.py:175
        }
        if (!ok) atomicOr(failed, 1);
        env_out[j] = env;
        prob[j] = p;
        data_idx[j] = idx - (cap - 1);
        tree_idx[j] = idx;
        const float probs = p / p_total;                          // memory.py:199-201 on the pooled memory
        const float wj = powf(filled * probs, -beta);
        weight[j] = wj;
        wmax = fmaxf(wmax, wj);
    }
    for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));
    __syncthreads();                                              // every walk through the top tree is over: its LDS is scratch again
    if (lane == 0) top[wave] = wmax;
    __syncthreads();
    wmax = fmaxf(fmaxf(top[0], top[1]), fmaxf(top[2], top[3]));
    for (int j = tid; j < b; j += 256) weight[j] = weight[j] / wmax;       // (this thread's own stores, read back)
}

// irbpp_replay_gather_kernel's inner body with (env, data_idx) read per row: one workgroup per sampled row.  A row whose env
// is outside [0, n_env) is written as zeros.
extern "C" __global__ void __launch_bounds__(256)
irbpp_replay_pool_gather_kernel(const float* __restrict__ states, const int64_t* __restrict__ actions, const float* __restrict__ rewards,
                                const uint8_t* __restrict__ nonterminals, const float* __restrict__ scaling, int n_env, int cap,
                                int obs_len, int n_step, const int64_t* __restrict__ env_idx, const int64_t* __restrict__ data_idx,
                                float* __restrict__ out_state, int64_t* __restrict__ out_action, float* __restrict__ out_return,
                                float* __restrict__ out_next, float* __restrict__ out_nonterminal) {
    const size_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t e64 = env_idx[row];
    float* o0 = out_state + row * obs_len;
    float* o1 = out_next + row * obs_len;
    if (e64 < 0 || e64 >= n_env) {
        for (int i = tid; i < obs_len; i += 256) { o0[i] = 0.0f; o1[i] = 0.0f; }
        if (tid == 0) { out_action[row] = 0; out_return[row] = 0.0f; out_nonterminal[row] = 0.0f; }
        return;
    }
    const size_t env = (size_t)e64;
    int d0 = (int)(data_idx[row] % cap);
    if (d0 < 0) d0 += cap;
    // alive chain (wave-uniform scalar work, repeated by every thread: n_step is tiny)
    bool alive = true;
    float ret = 0.0f;
    int pos = d0;
    for (int t = 0; t < n_step; ++t) {
        const float r = alive ? rewards[env * cap + pos] : 0.0f;
        ret = ret + r * scaling[t];
        alive = alive && nonterminals[env * cap + pos] != 0;
        pos = pos + 1 == cap ? 0 : pos + 1;
    }
    const int dn = pos;                                           // (d0 + n_step) % cap
    const float* s0 = states + (env * cap + d0) * obs_len;
    const float* sn = states + (env * cap + dn) * obs_len;
    for (int i = tid; i < obs_len; i += 256) {
        o0[i] = s0[i];
        o1[i] = alive ? sn[i] : 0.0f;
    }
    if (tid == 0) {
        out_action[row] = actions[env * cap + d0];
        out_return[row] = ret;
        out_nonterminal[row] = (alive && nonterminals[env * cap + dn] != 0) ? 1.0f : 0.0f;
    }
}

// SegmentTree.update (memory.py:55-58) for b triples (env, tree index, priority) in list order, touching only the listed
// leaves and their ancestors.  One workgroup, thread t owns triple t (b <= blockDim.x <= 1024).  A triple is live if no later
// one names the same leaf; the last triple of each env folds that env's maximum, so no two threads write one max[env].
extern "C" __global__ void __launch_bounds__(1024)
irbpp_replay_pool_update_kernel(float* tree, float* __restrict__ maxp, int n_env, int cap, const int64_t* __restrict__ env_idx,
                                const int64_t* __restrict__ tree_idx, const float* __restrict__ prio, int b) {
    __shared__ int s_env[POOL_MAX_DRAWS];
    __shared__ int s_ti[POOL_MAX_DRAWS];
    __shared__ float s_pr[POOL_MAX_DRAWS];
    const int t = threadIdx.x;
    const int len = 2 * cap - 1;
    int env = -1, ti = 0;
    float pr = 0.0f;
    if (t < b) {
        const int64_t e64 = env_idx[t], t64 = tree_idx[t];
        if (e64 >= 0 && e64 < n_env && t64 >= cap - 1 && t64 < len) {      // otherwise ignored: not a leaf of a row
            env = (int)e64;
            ti = (int)t64;
            pr = prio[t];
        }
    }
    s_env[t] = env; s_ti[t] = ti; s_pr[t] = pr;
    __syncthreads();
    bool live = env >= 0, last_of_env = env >= 0;
    float m = pr;
    if (env >= 0) {
        for (int k = 0; k < b; ++k) {                                      // (every thread reads the same word: an LDS broadcast)
            if (s_env[k] != env) continue;
            m = fmaxf(m, s_pr[k]);                                         // overwritten duplicates included (self.max = max(value, self.max))
            if (k > t) {
                last_of_env = false;
                if (s_ti[k] == ti) live = false;
            }
        }
    }
    float* row = tree + (size_t)(env >= 0 ? env : 0) * len;
    if (last_of_env) maxp[env] = fmaxf(maxp[env], m);
    if (live) row[ti] = pr;
    __syncthreads();                                                       // the leaves are in place for the whole workgroup
    // ancestors by actual depth floor(log2(idx + 1)), deepest level first: leaves of a capacity that is no power of two sit
    // at two depths.  Readers of a round read depth d, writers write depth d - 1; threads that meet write the same sum.
    int node = ti;
    int depth = live ? 31 - __clz(node + 1) : 0;
    const int deepest = 31 - __clz(len);                                   // depth of the last leaf, 2*cap - 2
    for (int d = deepest; d >= 1; --d) {
        if (live && depth == d) {
            node = (node - 1) >> 1;
            row[node] = row[2 * node + 1] + row[2 * node + 2];
            depth = d - 1;
        }
        __syncthreads();
    }
}

}  // namespace irbpp
