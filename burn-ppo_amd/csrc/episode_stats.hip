// episode_stats.hip — a rollout's finished episodes as the reference's episode/* scalars need
// them (main.rs:1134-1217, compute_avg_points env.rs:208-261) and its last 100 episodes in the
// reference's push order (main.rs:842-875), computed from the device's episode records, so the
// pipelined loop (bppo_train_steps) has them for every iteration without a record crossing PCIe.
//
// Statistics: one pass, per-thread bppo_episode_stats merged up a fixed tree (lanes, waves, then
// the blocks' partials in the last kernel).  No float atomics; only the f64 return sums depend
// on the order of the records in their slots.
//
// Tail: the 100 records with the largest key step * N + env_index.  The fused CartPole rollout
// fills its slots in no time order and a whole batch of envs can finish at one step, so the tail
// is selected exactly: a radix select of the 100th-largest key over 11-bit digits from the top
// (ep_key_digits(T N) <= 3 of them), one histogram pass per digit (LDS bins, flushed with
// integer atomics, whose order cannot change a count), every block of the next pass re-reading
// the bins to pick the digit; a compaction pass then moves the records at or above that key
// into 100 slots and one block rank-sorts them.  Each pass is O(kept), the number of passes
// depends on T N alone, nothing waits on another block.
#include <algorithm>
#include <cstring>
#include <vector>
#include "bppo_internal.h"

namespace bppo {

struct EpsArgs {
    const EpisodeRec *eps;
    const int32_t *count;        // the rollout's finished episodes (device)
    int cap;                     // records kept at most
    int P, N, nd;                // seated players, envs, key digits
    bppo_episode_stats *part;    // [EPS_BLOCKS]
    int32_t *sel;                // [EPS_SEL_WORDS], zero before the first pass
    EpisodeRec *cand;            // [BPPO_EPISODE_TAIL]
};

__device__ __forceinline__ bppo_episode_stats eps_shfl_down(const bppo_episode_stats &s, int off) {
    bppo_episode_stats o;
    o.episodes = __shfl_down(s.episodes, off, 64);
    o.kept = __shfl_down(s.kept, off, 64);
    o.length_min = __shfl_down(s.length_min, off, 64);
    o.length_max = __shfl_down(s.length_max, off, 64);
    o.length_sum = (int64_t)__shfl_down((long long)s.length_sum, off, 64);
    o.with_outcome = __shfl_down(s.with_outcome, off, 64);
    o.draws = __shfl_down(s.draws, off, 64);
    for (int p = 0; p < BPPO_MAX_PLAYERS; p++) {
        o.return_sum[p] = __shfl_down(s.return_sum[p], off, 64);
        o.return_min[p] = __shfl_down(s.return_min[p], off, 64);
        o.return_max[p] = __shfl_down(s.return_max[p], off, 64);
        o.outcome_games[p] = __shfl_down(s.outcome_games[p], off, 64);
        o.points2_sum[p] = (int64_t)__shfl_down((long long)s.points2_sum[p], off, 64);
    }
    return o;
}

// the block's threads merged in thread order up a fixed tree; the result is thread 0's
__device__ __forceinline__ void eps_block_merge(bppo_episode_stats &s, bppo_episode_stats *sh /*[EPS_THREADS / 64]*/) {
    for (int off = 32; off > 0; off >>= 1) {
        const bppo_episode_stats o = eps_shfl_down(s, off);
        if ((int)(threadIdx.x & 63) + off < 64) epstats_merge(s, o);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < EPS_THREADS / 64; w++) epstats_merge(s, sh[w]);
}

// bins: one digit's histogram of the keys still in play.  The digit holding the want-th largest
// of them (1 <= want <= their count), and want becomes its rank within that digit's keys.
// Whole block; sh [EPS_THREADS + 2].
__device__ __forceinline__ uint32_t eps_pick_digit(const int32_t *bins, int &want, int *sh) {
    constexpr int PER = EPS_BINS / EPS_THREADS;
    const int t = threadIdx.x;
    int loc[PER], sum = 0;
    for (int i = 0; i < PER; i++) {            // thread t: bins 2047 - 8 t downwards
        loc[i] = bins[EPS_BINS - 1 - (t * PER + i)];
        sum += loc[i];
    }
    sh[t] = sum;
    __syncthreads();
    for (int off = 1; off < EPS_THREADS; off <<= 1) {
        const int v = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    const int incl = sh[t], excl = incl - sum;
    if (t == 0) { sh[EPS_THREADS] = 0; sh[EPS_THREADS + 1] = 1; }   // (never read when the precondition holds)
    __syncthreads();
    if (excl < want && want <= incl) {         // one thread
        int acc = excl;
        for (int i = 0; i < PER; i++) {
            if (acc + loc[i] >= want) { sh[EPS_THREADS] = EPS_BINS - 1 - (t * PER + i); sh[EPS_THREADS + 1] = want - acc; break; }
            acc += loc[i];
        }
    }
    __syncthreads();
    const uint32_t digit = (uint32_t)sh[EPS_THREADS];
    want = sh[EPS_THREADS + 1];
    __syncthreads();
    return digit;
}

// the first d digits of the BPPO_EPISODE_TAIL-th largest key, from the histograms of passes 0..d-1
__device__ __forceinline__ uint64_t eps_prefix(const int32_t *sel, int d, int *sh) {
    uint64_t prefix = 0;
    int want = BPPO_EPISODE_TAIL;
    for (int j = 0; j < d; j++) prefix = (prefix << EPS_DIGIT_BITS) | eps_pick_digit(sel + j * EPS_BINS, want, sh);
    return prefix;
}

// pass d of the select: digit d of every kept record whose first d digits are the picked ones;
// STATS (pass 0): the statistics of every kept record as well
template <bool STATS>
__global__ void __launch_bounds__(EPS_THREADS) k_eps_hist(EpsArgs a, int d) {
    __shared__ int hist[EPS_BINS];
    __shared__ int pick[EPS_THREADS + 2];
    __shared__ bppo_episode_stats shs[EPS_THREADS / 64];
    const int kept = min(*a.count, a.cap);
    const bool select = kept > BPPO_EPISODE_TAIL;      // otherwise every record is in the tail
    if (!STATS && !select) return;
    for (int i = threadIdx.x; i < EPS_BINS; i += EPS_THREADS) hist[i] = 0;
    uint64_t prefix = 0;
    if (!STATS) prefix = eps_prefix(a.sel, d, pick);    // (syncs: hist is zero past here)
    else __syncthreads();
    const int shift = EPS_DIGIT_BITS * (a.nd - d);      // bits below the first d digits
    bppo_episode_stats s;
    if (STATS) epstats_identity(s);
    for (int i = blockIdx.x * EPS_THREADS + threadIdx.x; i < kept; i += EPS_BLOCKS * EPS_THREADS) {
        const EpisodeRec &r = a.eps[i];
        const uint64_t key = ep_key(r.step, r.env_index, a.N);
        if (STATS) {
            float tot[BPPO_MAX_PLAYERS];
            for (int p = 0; p < BPPO_MAX_PLAYERS; p++) tot[p] = r.total_reward[p];
            epstats_add(s, tot, r.length, (uint32_t)r.pad, a.P);
        }
        if (select && (STATS || (key >> shift) == prefix)) atomicAdd(&hist[ep_digit(key, d, a.nd)], 1);
    }
    __syncthreads();
    if (select)
        for (int i = threadIdx.x; i < EPS_BINS; i += EPS_THREADS)
            if (hist[i]) atomicAdd(&a.sel[d * EPS_BINS + i], hist[i]);
    if (STATS) {
        eps_block_merge(s, shs);
        if (threadIdx.x == 0) a.part[blockIdx.x] = s;
    }
}

// the records at or above the picked key into the candidate slots: min(100, kept) of them
__global__ void __launch_bounds__(EPS_THREADS) k_eps_compact(EpsArgs a) {
    __shared__ int pick[EPS_THREADS + 2];
    const int kept = min(*a.count, a.cap);
    uint64_t thr = 0;
    if (kept > BPPO_EPISODE_TAIL) thr = eps_prefix(a.sel, a.nd, pick);
    int32_t *counter = a.sel + EPS_MAX_DIGITS * EPS_BINS;
    // whole waves go round together: wave_episode_slot is a ballot
    for (int base = blockIdx.x * EPS_THREADS; base < kept; base += EPS_BLOCKS * EPS_THREADS) {
        const int i = base + (int)threadIdx.x;
        bool take = false;
        if (i < kept) take = ep_key(a.eps[i].step, a.eps[i].env_index, a.N) >= thr;
        const int slot = wave_episode_slot(take, counter);
        if (take && slot < BPPO_EPISODE_TAIL) a.cand[slot] = a.eps[i];
    }
}

// one block: the blocks' partials merged in block order, the candidates ordered by key; both
// written in the pinned slot's layout (bppo_internal.h ROLL_*)
__global__ void __launch_bounds__(EPS_THREADS) k_eps_final(EpsArgs a, double *slot) {
    static_assert(EPS_BLOCKS == EPS_THREADS && BPPO_EPISODE_TAIL <= EPS_THREADS, "one partial, one candidate per thread");
    __shared__ bppo_episode_stats shs[EPS_THREADS / 64];
    __shared__ uint64_t keys[BPPO_EPISODE_TAIL];
    const int t = threadIdx.x;
    const int count = *a.count;
    const int n_tail = min(min(count, a.cap), BPPO_EPISODE_TAIL);
    EpisodeRec r;
    if (t < n_tail) { r = a.cand[t]; keys[t] = ep_key(r.step, r.env_index, a.N); }
    bppo_episode_stats s = a.part[t];
    eps_block_merge(s, shs);              // (syncs: keys are visible)
    if (t == 0) {
        s.episodes = count;
        *reinterpret_cast<bppo_episode_stats *>(slot + ROLL_STATS_OFF) = s;
        *reinterpret_cast<int32_t *>(slot + ROLL_NTAIL_OFF) = n_tail;
    }
    if (t < n_tail) {
        int rank = 0;
        for (int j = 0; j < n_tail; j++) rank += keys[j] < keys[t] || (keys[j] == keys[t] && j < t);
        bppo_episode_tail o;
        float tot[BPPO_MAX_PLAYERS];
        for (int p = 0; p < BPPO_MAX_PLAYERS; p++) tot[p] = r.total_reward[p];
        eptail_fill(o, tot, r.length, r.env_index, r.step, (uint32_t)r.pad);
        reinterpret_cast<bppo_episode_tail *>(slot + ROLL_TAIL_OFF)[rank] = o;
    }
}

static hipError_t episode_stats_enqueue(hipStream_t st, const EpsArgs &a, double *d_slot) {
    hipError_t e = hipMemsetAsync(a.sel, 0, sizeof(int32_t) * EPS_SEL_WORDS, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_eps_hist<true>, dim3(EPS_BLOCKS), dim3(EPS_THREADS), 0, st, a, 0);
    for (int d = 1; d < a.nd; d++)
        hipLaunchKernelGGL(k_eps_hist<false>, dim3(EPS_BLOCKS), dim3(EPS_THREADS), 0, st, a, d);
    hipLaunchKernelGGL(k_eps_compact, dim3(EPS_BLOCKS), dim3(EPS_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_eps_final, dim3(1), dim3(EPS_THREADS), 0, st, a, d_slot);
    return hipGetLastError();
}

bppo_status episode_stats_alloc(bppo_ctx *c) {
    if (c->d_ep_part) return BPPO_OK;
    BPPO_HIP(c, c->mem.alloc(&c->d_ep_part, (size_t)EPS_BLOCKS));
    BPPO_HIP(c, c->mem.alloc(&c->d_ep_sel, (size_t)EPS_SEL_WORDS));
    BPPO_HIP(c, c->mem.alloc(&c->d_ep_cand, (size_t)BPPO_EPISODE_TAIL));
    return BPPO_OK;
}

bppo_status launch_episode_stats(bppo_ctx *c, double *d_slot) {
    EpsArgs a;
    a.eps = c->d_eps; a.count = c->d_ep_count; a.cap = c->eps_cap;
    a.P = c->Pa; a.N = c->N; a.nd = ep_key_digits((uint64_t)c->T * (uint64_t)c->N);
    a.part = c->d_ep_part; a.sel = c->d_ep_sel; a.cand = c->d_ep_cand;
    if (a.nd > EPS_MAX_DIGITS) { c->err = "episode statistics: num_steps * num_envs above 2^33"; return BPPO_ERR_UNSUPPORTED; }
    const hipError_t e = episode_stats_enqueue(c->stream, a, d_slot);
    return e == hipSuccess ? BPPO_OK : hip_fail(c, e, __func__);
}

// the host build: a loop over the records in their order and a sort
static void episode_stats_host(const std::vector<EpisodeRec> &recs, int P, int N, bppo_episode_stats *out,
                               bppo_episode_tail *tail, int32_t *n_tail) {
    bppo_episode_stats s;
    epstats_identity(s);
    for (const EpisodeRec &r : recs) epstats_add(s, r.total_reward, r.length, (uint32_t)r.pad, P);
    s.episodes = (int32_t)recs.size();
    *out = s;
    std::vector<const EpisodeRec *> order;
    for (const EpisodeRec &r : recs) order.push_back(&r);
    std::sort(order.begin(), order.end(), [N](const EpisodeRec *x, const EpisodeRec *y) {
        return ep_key(x->step, x->env_index, N) < ep_key(y->step, y->env_index, N); });
    const size_t m = std::min<size_t>(order.size(), BPPO_EPISODE_TAIL);
    for (size_t i = 0; i < m; i++) {
        const EpisodeRec &r = *order[order.size() - m + i];
        eptail_fill(tail[i], r.total_reward, r.length, r.env_index, r.step, (uint32_t)r.pad);
    }
    *n_tail = (int32_t)m;
}

}  // namespace bppo

using namespace bppo;

extern "C" bppo_status bppo_debug_episode_stats(int32_t device, int32_t n, const bppo_episode *eps,
                                                const int32_t *outcome_words, int32_t P, int32_t N, int32_t T,
                                                bppo_episode_stats *out, bppo_episode_tail *tail, int32_t *n_tail) {
    if (n < 0 || P < 1 || P > BPPO_MAX_PLAYERS || N < 1 || T < 1 || (n > 0 && !eps) || !out || !tail || !n_tail)
        return BPPO_ERR_ARG;
    if (ep_key_digits((uint64_t)T * (uint64_t)N) > EPS_MAX_DIGITS) return BPPO_ERR_ARG;
    std::vector<EpisodeRec> recs((size_t)n);
    std::vector<uint64_t> keys((size_t)n);
    for (int i = 0; i < n; i++) {
        if (eps[i].step < 0 || eps[i].step >= T || eps[i].env_index < 0 || eps[i].env_index >= N) return BPPO_ERR_ARG;
        std::copy(eps[i].total_reward, eps[i].total_reward + BPPO_MAX_PLAYERS, recs[i].total_reward);
        recs[i].length = eps[i].length; recs[i].env_index = eps[i].env_index; recs[i].step = eps[i].step;
        recs[i].pad = outcome_words ? outcome_words[i] : 0;
        keys[i] = ep_key(eps[i].step, eps[i].env_index, N);
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return BPPO_ERR_ARG;
    if (!device) {
        episode_stats_host(recs, P, N, out, tail, n_tail);
        return BPPO_OK;
    }
    DeviceMem buf;   // this call's buffers, freed when it ends
    EpsArgs a;
    EpisodeRec *d_eps = nullptr;
    int32_t *d_count = nullptr;
    double *d_slot = nullptr;
    if (buf.alloc(&d_eps, (size_t)n) != hipSuccess || buf.alloc(&d_count, 1) != hipSuccess ||
        buf.alloc(&a.part, (size_t)EPS_BLOCKS) != hipSuccess || buf.alloc(&a.sel, (size_t)EPS_SEL_WORDS) != hipSuccess ||
        buf.alloc(&a.cand, (size_t)BPPO_EPISODE_TAIL) != hipSuccess || buf.alloc(&d_slot, (size_t)ROLL_HOST_WORDS) != hipSuccess)
        return BPPO_ERR_HIP;
    if ((n > 0 && hipMemcpy(d_eps, recs.data(), sizeof(EpisodeRec) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(d_count, &n, 4, hipMemcpyHostToDevice) != hipSuccess)
        return BPPO_ERR_HIP;
    a.eps = d_eps; a.count = d_count; a.cap = n; a.P = P; a.N = N;
    a.nd = ep_key_digits((uint64_t)T * (uint64_t)N);
    std::vector<double> slot((size_t)ROLL_HOST_WORDS);
    if (episode_stats_enqueue(nullptr, a, d_slot) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(slot.data(), d_slot, sizeof(double) * slot.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return BPPO_ERR_HIP;
    std::memcpy(out, slot.data() + ROLL_STATS_OFF, sizeof *out);
    std::memcpy(n_tail, slot.data() + ROLL_NTAIL_OFF, 4);
    if (*n_tail < 0 || *n_tail > BPPO_EPISODE_TAIL) return BPPO_ERR_HIP;
    std::memcpy(tail, slot.data() + ROLL_TAIL_OFF, sizeof(bppo_episode_tail) * (size_t)*n_tail);
    return BPPO_OK;
}

extern "C" size_t bppo_episode_stats_size(void) { return sizeof(bppo_episode_stats); }
extern "C" size_t bppo_episode_tail_size(void) { return sizeof(bppo_episode_tail); }
