// Host harness (test infrastructure): the nine kernels of irbpp_amd/csrc/irbpp_replay.hip and irbpp_replay_pool.hip run on the
// CPU, one workgroup at a time, by as many threads in lockstep as the launch has (lockstep.h: 256, 64 for the per-env update,
// (count + 63) / 64 * 64 up to 1024 for the pooled update).  The kernels' own source is compiled, so the walks, the validity
// test, the ring wraps, the LDS staging and the generator are what the CPU suite checks against oracle/replay.py and the numpy
// models; powf is the C library's (build with -ffp-contract=off: the n-step chain is then f32(ret + f32(r * s))).
// Every host_* entry point has the signature of the irbpp_* function of irbpp_capi.hip it mirrors (the stream is ignored) and
// repeats what that function does after its argument checks: the same refusals answer -1 (IRBPP_ERR_ARG), and grid, block
// and dynamic LDS bytes are the C API's -- the dynamic LDS as a heap block of exactly that size (LockstepLaunch::dynamic_lds).
// With -DREPLAY_HOST_MAIN the file is a program of its own (for a sanitizer build): it runs all nine kernels over a few shapes
// on heap blocks of exactly the size a launch may touch, and prints checksums.
#include <stdio.h>

#include "lockstep.h"

#include "../../include/irbpp.h"
#include "../../irbpp_amd/csrc/irbpp_replay.hip"
#include "../../irbpp_amd/csrc/irbpp_replay_pool.hip"          // (after irbpp_replay.hip: it uses its uniform01)

using namespace irbpp;

static LockstepLaunch with_lds(size_t bytes) {
    LockstepLaunch how;
    how.dynamic_lds = (long long)bytes;
    return how;
}

extern "C" float host_uniform01(uint64_t seed, uint32_t env, uint32_t j, uint32_t attempt) { return uniform01(seed, env, j, attempt); }

// irbpp_sumtree_find
extern "C" int host_sumtree_find(const float* tree_dev, int32_t n_env, int32_t capacity, const float* values_dev, int32_t draws,
                                 float* prob_dev, int64_t* data_idx_dev, int64_t* tree_idx_dev, void*) {
    if (!tree_dev || !values_dev || !prob_dev || !data_idx_dev || !tree_idx_dev || n_env < 1 || capacity < 1 || draws < 1)
        return IRBPP_ERR_ARG;
    const int n = n_env * draws;
    lockstep_launch(256, (n + 255) / 256, 1, [&] {
        irbpp_sumtree_find_kernel(tree_dev, n_env, capacity, values_dev, draws, prob_dev, data_idx_dev, tree_idx_dev);
    });
    return IRBPP_OK;
}

// irbpp_sumtree_sample
extern "C" int host_sumtree_sample(const float* tree_dev, const int64_t* index_dev, int32_t n_env, int32_t capacity, int32_t draws,
                                   int32_t n_step, uint64_t seed, int32_t max_tries, float* prob_dev, int64_t* data_idx_dev,
                                   int64_t* tree_idx_dev, int32_t* failed_dev, void*) {
    if (!tree_dev || !index_dev || !prob_dev || !data_idx_dev || !tree_idx_dev || !failed_dev || n_env < 1 || capacity < 1 ||
        draws < 1 || n_step < 0 || max_tries < 1)
        return IRBPP_ERR_ARG;
    const int n = n_env * draws;
    lockstep_launch(256, (n + 255) / 256, 1, [&] {
        irbpp_sumtree_sample_kernel(tree_dev, index_dev, n_env, capacity, draws, n_step, seed, max_tries, prob_dev, data_idx_dev,
                                    tree_idx_dev, failed_dev);
    });
    return IRBPP_OK;
}

// irbpp_sumtree_update
extern "C" int host_sumtree_update(float* tree_dev, float* max_dev, int32_t n_env, int32_t capacity, const int64_t* tree_idx_dev,
                                   const float* priority_dev, int32_t leaves, const uint8_t* env_mask_dev, void*) {
    if (!tree_dev || !max_dev || !tree_idx_dev || !priority_dev || n_env < 1 || capacity < 1 || leaves < 1) return IRBPP_ERR_ARG;
    if (2 * capacity - 1 > SUMTREE_LDS) return IRBPP_ERR_ARG;
    lockstep_launch(64, n_env, 1, [&] {
        irbpp_sumtree_update_kernel(tree_dev, max_dev, capacity, tree_idx_dev, priority_dev, leaves, env_mask_dev);
    }, with_lds((size_t)(2 * capacity - 1) * sizeof(float)));
    return IRBPP_OK;
}

// irbpp_masked_argmax (waves of the last workgroup return before the others shuffle: per-wave shuffles)
extern "C" int host_masked_argmax(const float* q_dev, int32_t q_stride, const float* obs_dev, int32_t obs_stride, int32_t selected,
                                  int32_t n_env, int64_t* action_dev, void*) {
    if (!q_dev || !obs_dev || !action_dev || n_env < 1 || selected < 1 || q_stride < selected || obs_stride < 5 * selected)
        return IRBPP_ERR_ARG;
    LockstepLaunch how;
    how.wave_shuffles = true;
    lockstep_launch(256, (n_env + 3) / 4, 1, [&] {
        irbpp_masked_argmax_kernel(q_dev, q_stride, obs_dev, obs_stride, selected, n_env, action_dev);
    }, how);
    return IRBPP_OK;
}

// irbpp_replay_gather
extern "C" int host_replay_gather(const irbpp_replay_view* v, int32_t draws, float beta, const int64_t* data_idx_dev, const float* prob_dev,
                                  float* state_dev, int64_t* action_dev, float* return_dev, float* next_state_dev,
                                  float* nonterminal_dev, float* weight_dev, void*) {
    if (!v || !v->states_dev || !v->actions_dev || !v->rewards_dev || !v->nonterminals_dev || !v->tree_dev || !v->index_dev ||
        !v->full_dev || !v->scaling_dev || v->n_env < 1 || v->capacity < 1 || v->obs_len < 1 || v->n_step < 1 || draws < 1 ||
        draws > 256 || !data_idx_dev || !prob_dev || !state_dev || !action_dev || !return_dev || !next_state_dev ||
        !nonterminal_dev || !weight_dev)
        return IRBPP_ERR_ARG;
    lockstep_launch(256, v->n_env, 1, [&] {
        irbpp_replay_gather_kernel(v->states_dev, v->actions_dev, v->rewards_dev, v->nonterminals_dev, v->tree_dev, v->index_dev,
                                   v->full_dev, v->scaling_dev, v->capacity, v->obs_len, v->n_step, draws, beta, data_idx_dev, prob_dev,
                                   state_dev, action_dev, return_dev, next_state_dev, nonterminal_dev, weight_dev);
    });
    return IRBPP_OK;
}

// irbpp_replay_append
extern "C" int host_replay_append(const irbpp_replay_store* m, const float* state_dev, int64_t state_stride, const void* action_dev,
                                  int32_t action_bytes, const void* reward_dev, int32_t reward_bytes, const uint8_t* terminal_dev,
                                  const uint8_t* valid_dev, void*) {
    if (!m || !m->states_dev || !m->actions_dev || !m->rewards_dev || !m->nonterminals_dev || !m->timesteps_dev || !m->tree_dev ||
        !m->max_dev || !m->index_dev || !m->full_dev || !m->t_dev || m->n_env < 1 || m->capacity < 1 || m->obs_len < 1 ||
        !state_dev || state_stride < m->obs_len || !action_dev || (action_bytes != 4 && action_bytes != 8) || !reward_dev ||
        (reward_bytes != 4 && reward_bytes != 8) || !terminal_dev)
        return IRBPP_ERR_ARG;
    lockstep_launch(256, m->n_env, 1, [&] {
        irbpp_replay_append_kernel(m->states_dev, m->actions_dev, m->rewards_dev, m->nonterminals_dev, m->timesteps_dev, m->tree_dev,
                                   m->max_dev, m->index_dev, m->full_dev, m->t_dev, m->capacity, m->obs_len, state_dev,
                                   (long long)state_stride, action_dev, action_bytes, reward_dev, reward_bytes, terminal_dev, valid_dev);
    });
    return IRBPP_OK;
}

// replay_view_ok of irbpp_capi.hip
static bool replay_view_ok(const irbpp_replay_view* v) {
    return v && v->states_dev && v->actions_dev && v->rewards_dev && v->nonterminals_dev && v->tree_dev && v->index_dev &&
           v->full_dev && v->scaling_dev && v->n_env >= 1 && v->capacity >= 1 && v->capacity <= (1 << 30) && v->obs_len >= 1 &&
           v->n_step >= 1;
}

// irbpp_replay_pool_sample
extern "C" int host_replay_pool_sample(const irbpp_replay_view* v, int32_t draws, const float* values_dev, uint64_t seed,
                                       int32_t max_tries, float beta, int64_t* env_dev, float* prob_dev, int64_t* data_idx_dev,
                                       int64_t* tree_idx_dev, float* weight_dev, int32_t* failed_dev, void*) {
    if (!replay_view_ok(v) || draws < 1 || draws > POOL_MAX_DRAWS || max_tries < 1 || !env_dev || !prob_dev || !data_idx_dev ||
        !tree_idx_dev || !weight_dev || !failed_dev)
        return IRBPP_ERR_ARG;
    if (v->n_env > SUMTREE_LDS / 2) return IRBPP_ERR_ARG;
    int top_leaves = 1;
    while (top_leaves < v->n_env) top_leaves <<= 1;
    const int floats = 2 * top_leaves - 1 < 8 ? 8 : 2 * top_leaves - 1;
    lockstep_launch(256, 1, 1, [&] {
        irbpp_replay_pool_sample_kernel(v->tree_dev, v->index_dev, v->full_dev, v->n_env, v->capacity, top_leaves, draws, v->n_step,
                                        values_dev, seed, max_tries, beta, env_dev, prob_dev, data_idx_dev, tree_idx_dev, weight_dev,
                                        failed_dev);
    }, with_lds((size_t)floats * sizeof(float)));
    return IRBPP_OK;
}

// irbpp_replay_pool_gather
extern "C" int host_replay_pool_gather(const irbpp_replay_view* v, int32_t draws, const int64_t* env_dev, const int64_t* data_idx_dev,
                                       float* state_dev, int64_t* action_dev, float* return_dev, float* next_state_dev,
                                       float* nonterminal_dev, void*) {
    if (!replay_view_ok(v) || draws < 1 || !env_dev || !data_idx_dev || !state_dev || !action_dev || !return_dev ||
        !next_state_dev || !nonterminal_dev)
        return IRBPP_ERR_ARG;
    lockstep_launch(256, draws, 1, [&] {
        irbpp_replay_pool_gather_kernel(v->states_dev, v->actions_dev, v->rewards_dev, v->nonterminals_dev, v->scaling_dev, v->n_env,
                                        v->capacity, v->obs_len, v->n_step, env_dev, data_idx_dev, state_dev, action_dev, return_dev,
                                        next_state_dev, nonterminal_dev);
    });
    return IRBPP_OK;
}

// irbpp_replay_pool_update
extern "C" int host_replay_pool_update(float* tree_dev, float* max_dev, int32_t n_env, int32_t capacity, const int64_t* env_dev,
                                       const int64_t* tree_idx_dev, const float* priority_dev, int32_t count, void*) {
    if (!tree_dev || !max_dev || !env_dev || !tree_idx_dev || !priority_dev || n_env < 1 || capacity < 1 || capacity > (1 << 30) ||
        count < 1 || count > POOL_MAX_DRAWS)
        return IRBPP_ERR_ARG;
    lockstep_launch((count + 63) / 64 * 64, 1, 1, [&] {
        irbpp_replay_pool_update_kernel(tree_dev, max_dev, n_env, capacity, env_dev, tree_idx_dev, priority_dev, count);
    });
    return IRBPP_OK;
}

#ifdef REPLAY_HOST_MAIN
// Every buffer is a heap block of exactly the size a launch may touch, so a sanitizer sees any access beyond it.
template <typename T>
static double sum_of(const std::vector<T>& a) {
    double s = 0;
    for (const T& x : a) s += (double)x;
    return s;
}

int main() {
    // n_env, capacity, obs_len, n_step, draws: capacity 1; capacity 11 (leaves at two depths) with 3 envs under a top tree of 4
    // leaves; the smallest ring that has a sibling, 255 draws; a power of two with the per-env gather's 256 draws; a top tree
    // wider than a wave with draws in the draw loop's second trip
    const int shapes[][5] = {{1, 1, 1, 1, 1}, {3, 11, 300, 3, 5}, {5, 2, 1, 1, 255}, {2, 64, 7, 3, 256}, {65, 11, 1, 3, 257}};
    uint32_t rng = 2463534242u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) * (1.0f / 16777216.0f); };
    for (const auto& sh : shapes) {
        const int n = sh[0], cap = sh[1], obs_len = sh[2], n_step = sh[3], b = sh[4], len = 2 * cap - 1;
        const int pb = b < 256 ? b : 256;                                    // the per-env gather takes at most 256 draws
        std::vector<float> states((size_t)n * cap * obs_len, 0.0f), rewards((size_t)n * cap, 0.0f), tree((size_t)n * len, 0.0f), maxp(n, 1.0f);
        std::vector<int64_t> actions((size_t)n * cap, 0), index(n, 0);
        std::vector<uint8_t> nonterm((size_t)n * cap, 0), full(n, 0);
        std::vector<int32_t> timesteps((size_t)n * cap, 0), tcount(n, 0);
        std::vector<float> scaling(n_step);
        for (int t = 0; t < n_step; ++t) scaling[t] = powf(0.99f, (float)t);
        const irbpp_replay_store store = {states.data(), actions.data(), rewards.data(), nonterm.data(), timesteps.data(), tree.data(),
                                          maxp.data(), index.data(), full.data(), tcount.data(), n, cap, obs_len};
        const irbpp_replay_view view = {states.data(), actions.data(), rewards.data(), nonterm.data(), tree.data(), index.data(),
                                        full.data(), scaling.data(), n, cap, obs_len, n_step};
        // appends through one wrap and three slots on: strided rows, both action and reward widths, a valid mask, terminals
        const long long stride = obs_len + 3;
        for (int t = 0; t < cap + 3; ++t) {
            std::vector<float> state((size_t)(n - 1) * stride + obs_len);
            for (auto& f : state) f = next() * 0.3f;
            std::vector<int32_t> a4(n);
            std::vector<int64_t> a8(n);
            std::vector<float> r4(n);
            std::vector<double> r8(n);
            std::vector<uint8_t> term(n), valid(n);
            for (int e = 0; e < n; ++e) {
                a4[e] = (int32_t)(next() * 500.0f), a8[e] = a4[e], r4[e] = next(), r8[e] = r4[e];
                term[e] = next() < 0.2f, valid[e] = (t % 3 == 1 && n > 1) ? e % 2 : 1;
            }
            if (host_replay_append(&store, state.data(), stride, t % 2 ? (const void*)a4.data() : (const void*)a8.data(), t % 2 ? 4 : 8,
                                   t % 4 < 2 ? (const void*)r4.data() : (const void*)r8.data(), t % 4 < 2 ? 4 : 8, term.data(),
                                   t % 3 == 1 ? valid.data() : nullptr, nullptr))
                return 1;
        }
        // per-env update: first leaf, last leaf, a duplicate, and indices that are no leaf of the row (the last internal node, past
        // the row, negative, beyond 2^32); env 1 masked out
        {
            const int k = 8;
            std::vector<int64_t> ti((size_t)n * k);
            std::vector<float> pr((size_t)n * k);
            std::vector<uint8_t> mask(n, 1);
            if (n > 1) mask[1] = 0;
            for (int e = 0; e < n; ++e) {
                const int64_t row[k] = {cap - 1, 2 * cap - 2, cap - 2, 2 * cap - 1, -1, ((int64_t)1 << 32) + cap - 1, cap - 1 + (int64_t)(next() * cap), cap - 1};
                for (int j = 0; j < k; ++j) ti[(size_t)e * k + j] = row[j], pr[(size_t)e * k + j] = 0.05f + 2.0f * next();
            }
            if (host_sumtree_update(tree.data(), maxp.data(), n, cap, ti.data(), pr.data(), k, mask.data(), nullptr)) return 1;
        }
        // find: 0, the total, the float above it, values in between
        std::vector<float> values((size_t)n * pb), prob((size_t)n * pb);
        std::vector<int64_t> data_idx((size_t)n * pb), tree_idx((size_t)n * pb);
        for (int e = 0; e < n; ++e) {
            const float total = tree[(size_t)e * len];
            for (int j = 0; j < pb; ++j) values[(size_t)e * pb + j] = j == 0 ? 0.0f : j == 1 ? total : j == 2 ? nextafterf(total, INFINITY) : next() * total;
        }
        if (host_sumtree_find(tree.data(), n, cap, values.data(), pb, prob.data(), data_idx.data(), tree_idx.data(), nullptr)) return 1;
        double sum = sum_of(prob) + sum_of(data_idx) + sum_of(tree_idx);
        // per-env gather of what find returned
        {
            std::vector<float> o_state((size_t)n * pb * obs_len), o_next((size_t)n * pb * obs_len), o_ret((size_t)n * pb), o_nt((size_t)n * pb), o_w((size_t)n * pb);
            std::vector<int64_t> o_act((size_t)n * pb);
            if (host_replay_gather(&view, pb, 0.4f, data_idx.data(), prob.data(), o_state.data(), o_act.data(), o_ret.data(), o_next.data(),
                                   o_nt.data(), o_w.data(), nullptr))
                return 1;
            sum += sum_of(o_state) + sum_of(o_next) + sum_of(o_ret) + sum_of(o_nt) + sum_of(o_act);
        }
        // per-env sample drawn on the "device"
        std::vector<int32_t> failed(1, 0);
        if (host_sumtree_sample(tree.data(), index.data(), n, cap, pb, n_step, 0x8000000000000005ull, 16, prob.data(), data_idx.data(),
                                tree_idx.data(), failed.data(), nullptr))
            return 1;
        sum += sum_of(prob) + sum_of(data_idx) + sum_of(tree_idx) + failed[0];
        // pooled sample: drawn, then supplied values with one past the pooled total (3 envs: the padding leaf of 4)
        std::vector<int64_t> p_env(b), p_data(b), p_tree(b);
        std::vector<float> p_prob(b), p_w(b), p_values(b);
        if (host_replay_pool_sample(&view, b, nullptr, 7, 16, 0.4f, p_env.data(), p_prob.data(), p_data.data(), p_tree.data(), p_w.data(),
                                    failed.data(), nullptr))
            return 1;
        sum += sum_of(p_env) + sum_of(p_prob) + sum_of(p_data) + sum_of(p_tree) + failed[0];
        float pooled = 0.0f;
        for (int e = 0; e < n; ++e) pooled += tree[(size_t)e * len];
        for (int j = 0; j < b; ++j) p_values[j] = next() * pooled;
        p_values[b - 1] = pooled * 1.5f;
        if (host_replay_pool_sample(&view, b, p_values.data(), 0, 1, 0.4f, p_env.data(), p_prob.data(), p_data.data(), p_tree.data(),
                                    p_w.data(), failed.data(), nullptr))
            return 1;
        sum += sum_of(p_env) + sum_of(p_prob) + sum_of(p_data) + sum_of(p_tree) + failed[0];
        // pooled gather of those rows, one env below and one past the range, a negative data index
        {
            p_env[0] = -1;
            if (b > 1) p_env[b - 1] = n;
            if (b > 2) p_data[1] = -3;
            std::vector<float> o_state((size_t)b * obs_len), o_next((size_t)b * obs_len), o_ret(b), o_nt(b);
            std::vector<int64_t> o_act(b);
            if (host_replay_pool_gather(&view, b, p_env.data(), p_data.data(), o_state.data(), o_act.data(), o_ret.data(), o_next.data(),
                                        o_nt.data(), nullptr))
                return 1;
            sum += sum_of(o_state) + sum_of(o_next) + sum_of(o_ret) + sum_of(o_nt) + sum_of(o_act);
        }
        // pooled update: the sampled leaves (duplicates among them) and triples that are to be ignored
        {
            for (int j = 0; j < b; ++j) p_prob[j] = 0.05f + 2.0f * next();
            if (b > 3) p_tree[2] = cap - 2, p_tree[3] = 2 * cap - 1;
            if (host_replay_pool_update(tree.data(), maxp.data(), n, cap, p_env.data(), p_tree.data(), p_prob.data(), b, nullptr)) return 1;
            sum += sum_of(tree) + sum_of(maxp);
        }
        // masked arg-max over obs_len + 60 candidates: q and the observations as strided rows that end with the last env's
        {
            const int s = obs_len + 60, q_stride = s + 3, obs_stride = 5 * s + 2;
            std::vector<float> q((size_t)(n - 1) * q_stride + s), obs((size_t)(n - 1) * obs_stride + 5 * s);
            for (auto& f : q) f = next();
            for (auto& f : obs) f = next() < 0.5f ? 0.0f : 1.0f;
            std::vector<int64_t> act(n);
            if (host_masked_argmax(q.data(), q_stride, obs.data(), obs_stride, s, n, act.data(), nullptr)) return 1;
            sum += sum_of(act);
        }
        sum += sum_of(states) + sum_of(actions) + sum_of(rewards) + sum_of(nonterm) + sum_of(timesteps) + sum_of(index) + sum_of(full) + sum_of(tcount);
        printf("n_env %d capacity %d obs_len %d n_step %d draws %d: checksum %.9g\n", n, cap, obs_len, n_step, b, sum);
    }
    return 0;
}
#endif
