// eval.hip — stats-mode evaluation on the device: run_stats_mode_env
// (eval.rs:1621-1877), the engine of `eval --num-games` and of the tournament
// pods (tournament.rs:1843).  The same machine as the opponent-pool rollout
// (opponents.hip) with a temperature sampler, envs that can be frozen, game
// outcomes captured before the auto-reset, and the games cap + freeze rule.
//
// One loop (evaluate_run) plays n_pods independent matchups (pods) of E envs each: pod k owns
// envs [k E, (k + 1) E), its own RNG key and position, games counter and freeze state; only
// the forward pass is shared, one model's rows from every pod being contiguous (DESIGN.md
// section 7d).  bppo_evaluate_pods is that loop; bppo_evaluate is its one-pod case.
//
// Per loop iteration, on the context's stream:
//   observe          rows, masks, player to move (k_wide_observe)
//   k_eval_group     one block per pod: each active env's mover model seat_model[perm[player]]
//                    (eval.rs:1697-1704), its temperature (eval.rs:1766), its rank among the
//                    pod's rows of that model and, if it draws, its draw index: the pod's
//                    slots ascending, within a slot the non-frozen envs in ascending index
//                    (eval.rs:1685-1769); the (model, pod) row counts
//   k_eval_scan      the counts scanned model-major, pod-minor: each env's row, the header
//   one host read    {unfinished pods, error flags, group bases}: bounds the forward's
//                    grids and ends the loop (eval.rs:1670-1674)
//   forward          models_step_forward (model_set.hip), the opponent-pool rollout's too: rows
//                    sorted model-major; all models at once, one obs normalizer launch
//                    (eval.rs:1727-1734) and one GEMM launch per layer over every model's row
//                    range, read from the header on the device; logits
//                    selected back; a random model's rows see zero logits (eval.rs:1749-1752).
//                    Nets with conv layers: one model after the other (wide_forward_actor)
//   k_eval_sample    sample_with_temperature per row at the pod's word position + draw index
//   env step         k_wide_step with the frozen mask, the outcome sink and per-env seeds
//   k_eval_finish    one block per pod: games recorded in env order up to the cap, seat ->
//                    checkpoint remap, permutation rotation, move counts, freeze rule, RNG
//                    position (eval.rs:1774-1869)
// The RNG positions live on the device (as in the opponent-pool rollout).
//
// A pod's slots are the host-built table slot_model, the one thing the two entry points
// differ in: bppo_evaluate lists the seated models in ascending model index (the reference's
// draw order), bppo_evaluate_pods by first appearance among the pod's seats (run_pod's
// de-duplication).
#include <algorithm>
#include <cstring>
#include <vector>
#include "bppo_internal.h"
#include "bppo_envs.h"
#include "bppo_wide.h"
#include "bppo_eval.h"
#include "bppo_gemm.h"
#include "bppo_scan.h"

namespace bppo {

constexpr int EV_MAX_MODELS = 64;
constexpr int EV_SINGLE_MAX_MODELS = 15;  // bppo_evaluate's documented limit (bppo.h)
constexpr int EV_MAX_PODS = 1024;
constexpr int EV_POD_THREADS = 1024;      // at most; a pod's block is its envs rounded up to whole waves
constexpr int EV_SCAN_THREADS = 1024;
constexpr int EV_ERR_ZERO_SUM = 16;   // d_err bit: the sampler's sum == 0.0 exit (bppo_eval.h temp_draws)

// the step's small record, read by the host once per iteration; its size is independent of n_pods
struct EvalHdr {
    int32_t unfinished;                  // pods with games < num_games and an active env
    int32_t err;                         // the context's error flags so far
    int32_t gbase[EV_MAX_MODELS + 2];    // group g (0 frozen, 1 + model) owns rows [gbase[g], gbase[g + 1])
};

struct EvalState {
    int n_pods, E, P, K, nperm, num_games, cap;
    bppo_eval::TempSched temp;
    const int32_t *perm_tab;             // [nperm][P]: perm[player] = checkpoint
    const int32_t *seat_model;           // [n_pods][P] checkpoint -> model
    const int32_t *slot_model;           // [n_pods][P] slot -> model, -1 past the pod's last slot
    int32_t *perm_idx, *moves;           // [N]
    uint8_t *frozen;                     // [N]
    int32_t *group, *gpos, *didx;        // [N] 0 frozen / 1 + model; row; draw index from the pod's RNG position or -1
    int32_t *lrank;                      // [N] rank among the pod's rows of its group
    float *tempv;                        // [N]
    int32_t *counts, *offs;              // [K + 1][n_pods] rows of (group, pod); their exclusive scan
    int32_t *games, *active, *ndraw;     // [n_pods]
    uint64_t *rngpos;                    // [n_pods]
    EvalHdr *hdr;
    const int32_t *err;
};

struct EvalSampleArgs {
    int N;
    const float *logits;         // [N][A], env order
    const uint8_t *mask;         // [N][A]
    const int32_t *group;        // 0: frozen (writes nothing); 1 + model (null: every row model 0)
    const int32_t *didx;         // draw index or -1
    const float *temp;           // [N]
    uint64_t random_models;      // bit k: model k is the random player (zero logits)
    int pod_envs;                // env e belongs to pod e / pod_envs
    const Key8 *pod_key;         // [pods]
    const uint64_t *pod_rngpos;  // [pods] the step's first word position
    uint64_t stream;             // ChaCha stream id: 0 in the evaluation loop
    int32_t *act;
    int32_t *used;               // [N] whether the row drew (may be null)
    int32_t *err;
};

// one row per lane; the row's word computed once; the sequential chains in registers
template <int A>
__global__ void __launch_bounds__(64) k_eval_sample(EvalSampleArgs g) {
    __shared__ MathLds T;
    T.load();
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.N) return;
    const int grp = g.group ? g.group[e] : 1;
    if (grp == 0) return;                                   // frozen: never sampled again
    const bool rnd = (g.random_models >> (grp - 1)) & 1ull;
    float x[A];
    uint8_t mk[A];
#pragma unroll
    for (int a = 0; a < A; a++) { mk[a] = g.mask[(size_t)e * A + a]; x[a] = g.logits[(size_t)e * A + a]; }
    int first = -1;
#pragma unroll
    for (int a = 0; a < A; a++) {
        const bool ok = mk[a] != 0;
        if (ok && first < 0) first = a;
        x[a] = ok ? (rnd ? 0.0f : x[a]) : -INFINITY;        // eval.rs:230-238, :1749-1752
    }
    const int di = g.didx[e];
    const int pod = e / g.pod_envs;
    uint32_t word = 0;
    if (di >= 0) word = chacha12_word(g.pod_key[pod], g.stream, g.pod_rngpos[pod] + (uint64_t)di);
    int used = 0;
    const int a = bppo_eval::sample_with_temperature<A>(x, first < 0 ? 0 : first, g.temp[e], word, &used, T);
    if (used != (di >= 0)) atomicOr(g.err, EV_ERR_ZERO_SUM);
    g.act[e] = a;
    if (g.used) g.used[e] = used;
}

static hipError_t eval_sample(int A, hipStream_t st, const EvalSampleArgs &g) {
    const dim3 grid((g.N + 63) / 64), block(64);
    if (A == C4_ACT) hipLaunchKernelGGL(k_eval_sample<C4_ACT>, grid, block, 0, st, g);
    else if (A == LD_ACT) hipLaunchKernelGGL(k_eval_sample<LD_ACT>, grid, block, 0, st, g);
    else if (A == SK_ACT) hipLaunchKernelGGL(k_eval_sample<SK_ACT>, grid, block, 0, st, g);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// rewards_to_placements (eval.rs:276-306) on n <= 6 rewards: a stable sort by reward
// descending (incomparable pairs equal), then tie groups within 1e-6 of the group's first
__device__ __forceinline__ void rewards_to_placements(const float *r, int n, int32_t *pl) {
    int idx[BPPO_MAX_PLAYERS];
    for (int i = 0; i < n; i++) idx[i] = i;
    for (int i = 1; i < n; i++) {                 // insertion sort: stable
        const int k = idx[i];
        int j = i - 1;
        while (j >= 0 && r[k] > r[idx[j]]) { idx[j + 1] = idx[j]; j--; }
        idx[j + 1] = k;
    }
    int cur = 1, i = 0;
    while (i < n) {
        const float cr = r[idx[i]];
        int tied = 0;
        while (i + tied < n && fabsf(__fsub_rn(r[idx[i + tied]], cr)) < 1e-6f) tied++;
        if (tied == 0) tied = 1;                  // a NaN reward ties with nothing, itself included
        for (int j = 0; j < tied; j++) pl[idx[i + j]] = cur;
        cur += tied;
        i += tied;
    }
}

// a finished game as recorded: seat -> checkpoint remap under the env's permutation
// perm[player] = checkpoint (eval.rs:1798-1825)
__device__ __forceinline__ bppo_eval_game game_record(const int32_t *perm, int P, const EvalOutcome &o, int env_index,
                                                      int pi, int step) {
    bppo_eval_game rec;
    for (int c = 0; c < BPPO_MAX_PLAYERS; c++) { rec.total_reward[c] = 0.0f; rec.placement[c] = 0; }
    for (int c = 0; c < P; c++) {                     // checkpoint c sat on seat p (:1798-1821)
        int p = 0;
        for (int q = 0; q < P; q++) p = perm[q] == c ? q : p;
        rec.total_reward[c] = o.total_reward[p];
        rec.placement[c] = o.placement[p];
    }
    if (!o.has_outcome) rewards_to_placements(rec.total_reward, P, rec.placement);   // :1822-1825
    rec.length = o.length; rec.env_index = env_index; rec.perm_index = pi; rec.step = step;
    return rec;
}

// One block per pod.  The draw order: the pod's slots ascending (slot_model; a pod's slots
// name distinct models, so an env's group tells its slot), within a slot its envs ascending:
// thread t owns envs [t per, (t + 1) per) of the pod, so any E is covered in env order.
__global__ void __launch_bounds__(EV_POD_THREADS) k_eval_group(EvalState s, const int32_t *players) {
    __shared__ uint64_t wsum[EV_POD_THREADS / 64];
    const int pod = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int per = (s.E + nt - 1) / nt;
    const int j0 = min(s.E, tid * per), j1 = min(s.E, j0 + per);
    const size_t b = (size_t)pod * s.E;
    const int32_t *sm = s.seat_model + (size_t)pod * s.P;
    for (int g = tid; g <= s.K; g += nt) s.counts[(size_t)g * s.n_pods + pod] = 0;
    for (int j = tid; j < s.E; j += nt) {    // each env by itself: consecutive threads, consecutive envs
        const size_t e = b + j;
        int g = 0;
        float temp = 0.0f;
        int draws = 0;
        if (!s.frozen[e]) {
            const int cp = s.perm_tab[(size_t)s.perm_idx[e] * s.P + players[e]];   // eval.rs:1700-1701
            g = 1 + sm[cp];                                                         // :1704
            temp = bppo_eval::get_temp(s.temp, s.moves[e]);                         // :1766
            draws = bppo_eval::temp_draws(temp) ? 1 : 0;
        }
        s.group[e] = g;
        s.tempv[e] = temp;
        s.didx[e] = draws - 1;       // 0: draws (index below), -1: no draw
    }
    __syncthreads();                 // group, didx of the thread's own run
    uint32_t dbase = 0;              // draws of the slots before sl (the same in every thread)
    for (int sl = 0; sl <= s.P; sl++) {
        const int g = sl == 0 ? 0 : 1 + s.slot_model[(size_t)pod * s.P + sl - 1];
        if (sl > 0 && g == 0) break;                          // past the pod's last slot (block-uniform)
        uint32_t nr = 0, nd = 0;
        for (int j = j0; j < j1; j++)
            if (s.group[b + j] == g) { nr++; nd += s.didx[b + j] >= 0; }
        uint64_t tot;
        const uint64_t ex = block_scan_excl((uint64_t)nr | ((uint64_t)nd << 32), wsum, &tot);
        uint32_t r = (uint32_t)ex, d = dbase + (uint32_t)(ex >> 32);
        for (int j = j0; j < j1; j++)
            if (s.group[b + j] == g) {
                s.lrank[b + j] = (int32_t)r++;
                if (s.didx[b + j] >= 0) s.didx[b + j] = (int32_t)d++;
            }
        if (tid == 0) s.counts[(size_t)g * s.n_pods + pod] = (int32_t)(uint32_t)tot;
        dbase += (uint32_t)(tot >> 32);
    }
    if (tid == 0) s.ndraw[pod] = (int32_t)dbase;
}

// One block: the (group, pod) row counts scanned group-major, pod-minor, so a model's rows
// from all pods are contiguous with the pods ascending; each env's global row; the header.
__global__ void __launch_bounds__(EV_SCAN_THREADS) k_eval_scan(EvalState s) {
    __shared__ uint64_t wsum[EV_SCAN_THREADS / 64];
    __shared__ int unfinished;
    const int tid = threadIdx.x;
    const int n = (s.K + 1) * s.n_pods;
    const int per = (n + EV_SCAN_THREADS - 1) / EV_SCAN_THREADS;
    const int i0 = min(n, tid * per), i1 = min(n, i0 + per);
    if (tid == 0) unfinished = 0;
    uint32_t sum = 0;
    for (int i = i0; i < i1; i++) sum += (uint32_t)s.counts[i];
    uint64_t tot;
    uint32_t r = (uint32_t)block_scan_excl((uint64_t)sum, wsum, &tot);
    for (int i = i0; i < i1; i++) { s.offs[i] = (int32_t)r; r += (uint32_t)s.counts[i]; }
    for (int k = tid; k < s.n_pods; k += EV_SCAN_THREADS)
        if (s.games[k] < s.num_games && s.active[k] > 0) atomicAdd(&unfinished, 1);
    __syncthreads();                 // offs, unfinished
    for (int g = tid; g <= s.K; g += EV_SCAN_THREADS) s.hdr->gbase[g] = s.offs[(size_t)g * s.n_pods];
    const int N = s.n_pods * s.E;
    for (int e = tid; e < N; e += EV_SCAN_THREADS)
        s.gpos[e] = s.offs[(size_t)s.group[e] * s.n_pods + e / s.E] + s.lrank[e];
    if (tid == 0) {
        s.hdr->gbase[s.K + 1] = (int32_t)(uint32_t)tot;
        s.hdr->unfinished = unfinished;
        s.hdr->err = *s.err;
    }
}

// After the env step (eval.rs:1774-1869).  One block per pod against the pod's own counters,
// thread t owning envs [t per, (t + 1) per) of the pod; games go to games[pod cap + ...] with
// env_index the index within the pod
__global__ void __launch_bounds__(EV_POD_THREADS) k_eval_finish(EvalState s, int step, const uint8_t *done,
                                                                 const EvalOutcome *sink, bppo_eval_game *games) {
    __shared__ uint64_t wsum[EV_POD_THREADS / 64];
    const int pod = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    if (s.active[pod] == 0) return;                  // a finished pod: every env frozen (block-uniform)
    const int per = (s.E + nt - 1) / nt;
    const int j0 = min(s.E, tid * per), j1 = min(s.E, j0 + per);
    const size_t b = (size_t)pod * s.E;
    const int g0 = s.games[pod];
    uint32_t nd = 0, na = 0;
    for (int j = j0; j < j1; j++) { nd += done[b + j] != 0; na += s.frozen[b + j] == 0; }
    uint64_t tot;
    const uint64_t ex = block_scan_excl((uint64_t)nd | ((uint64_t)na << 32), wsum, &tot);   // (games / active read above: barrier inside)
    const int ND = (int)(uint32_t)tot, ACT = (int)(tot >> 32);
    const int nrec = min(ND, max(0, s.num_games - g0));                                    // :1783-1789
    const int g1 = g0 + nrec;
    const int remaining = max(0, s.num_games - g1);                                        // :1841-1869
    const int to_freeze = ACT > remaining ? ACT - remaining : 0;
    const int f1 = min(to_freeze, ND), f2 = to_freeze - f1;
    int k = (int)(uint32_t)ex;
    uint32_t alive = 0;
    for (int j = j0; j < j1; j++) {
        const size_t e = b + j;
        int mv = s.moves[e] + 1;                                    // every env, frozen included (:1775-1777)
        if (done[e]) {
            if (k < nrec) {
                const int pi = s.perm_idx[e];
                const bppo_eval_game rec = game_record(s.perm_tab + (size_t)pi * s.P, s.P, sink[e], j, pi, step);
                if (g0 + k < s.cap) games[(size_t)pod * s.cap + g0 + k] = rec;
                mv = 0;                                              // :1830
                s.perm_idx[e] = (pi + 1) % s.nperm;                  // :1831
            }
            if (k < f1) s.frozen[e] = 1;
            k++;
        }
        s.moves[e] = mv;
        alive += s.frozen[e] == 0;
    }
    if (f2 > 0) {                                                   // the same in every thread
        uint64_t t2;
        int r = (int)(uint32_t)block_scan_excl((uint64_t)alive, wsum, &t2);
        for (int j = j0; j < j1; j++)
            if (!s.frozen[b + j]) {
                if (r < f2) s.frozen[b + j] = 1;
                r++;
            }
    }
    if (tid == 0) {
        s.games[pod] = g1;
        s.active[pod] = ACT - to_freeze;
        s.rngpos[pod] += (uint64_t)s.ndraw[pod];                   // the step's draws
    }
}

__global__ void k_eval_init(EvalState s, uint64_t pos) {
    const int N = s.n_pods * s.E;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < N; e += gridDim.x * blockDim.x) {
        s.perm_idx[e] = (e % s.E) % s.nperm;  // eval.rs:1662, per pod
        s.moves[e] = 0;
        s.frozen[e] = 0;
        if (e < s.n_pods) {
            s.games[e] = 0;
            s.active[e] = s.E;
            s.ndraw[e] = 0;
            s.rngpos[e] = pos;
        }
    }
}

// generate_permutations / heap_permute (eval.rs:1591-1612), exactly as written
static void heap_permute(int32_t *arr, int k, int n, std::vector<int32_t> &out) {
    if (k == 1) { out.insert(out.end(), arr, arr + n); return; }
    heap_permute(arr, k - 1, n, out);
    for (int i = 0; i < k - 1; i++) {
        if (k % 2 == 0) std::swap(arr[i], arr[k - 1]);
        else std::swap(arr[0], arr[k - 1]);
        heap_permute(arr, k - 1, n, out);
    }
}
static std::vector<int32_t> generate_permutations(int n) {
    std::vector<int32_t> out;
    int32_t arr[BPPO_MAX_PLAYERS];
    for (int i = 0; i < n; i++) arr[i] = i;
    heap_permute(arr, n, n, out);
    return out;
}

struct HostMath {
    float expf(float v) const { return bppo_math::expf_glibc(v); }
};

template <int A>
static void sample_rows_host(int B, const float *logits, const uint8_t *masks, const float *temps, const Key8 &key,
                             uint64_t stream, uint64_t pos, int32_t *actions, int32_t *used_out) {
    const HostMath T;
    for (int b = 0; b < B; b++) {
        float x[A];
        int first = -1;
        for (int a = 0; a < A; a++) {
            const bool ok = masks[(size_t)b * A + a] != 0;
            if (ok && first < 0) first = a;
            x[a] = ok ? logits[(size_t)b * A + a] : -INFINITY;
        }
        uint32_t blk[16];
        chacha12_block(key, pos >> 4, stream, blk);
        int used = 0;
        actions[b] = bppo_eval::sample_with_temperature<A>(x, first < 0 ? 0 : first, temps[b], blk[pos & 15], &used, T);
        pos += (uint64_t)used;
        if (used_out) used_out[b] = used;
    }
}

}  // namespace bppo

using namespace bppo;

extern "C" size_t bppo_eval_config_size(void) { return sizeof(bppo_eval_config); }
extern "C" size_t bppo_eval_game_size(void) { return sizeof(bppo_eval_game); }

extern "C" bppo_status bppo_debug_eval_perms(int32_t n, int32_t *out) {
    if (!out || n < 1 || n > BPPO_MAX_PLAYERS) return BPPO_ERR_ARG;
    const std::vector<int32_t> t = generate_permutations(n);
    std::memcpy(out, t.data(), sizeof(int32_t) * t.size());
    return BPPO_OK;
}

extern "C" bppo_status bppo_debug_eval_sample(int32_t device, int32_t A, int32_t B, const float *logits,
                                              const uint8_t *masks, const float *temps, uint64_t seed,
                                              uint64_t stream, uint64_t word_pos, int32_t *actions,
                                              int32_t *draws_used) {
    if (!logits || !masks || !temps || !actions || B <= 0 || (A != C4_ACT && A != LD_ACT && A != SK_ACT))
        return BPPO_ERR_ARG;
    const Key8 key = seed_key(seed);
    if (!device) {
        if (A == C4_ACT) sample_rows_host<C4_ACT>(B, logits, masks, temps, key, stream, word_pos, actions, draws_used);
        else if (A == LD_ACT) sample_rows_host<LD_ACT>(B, logits, masks, temps, key, stream, word_pos, actions, draws_used);
        else sample_rows_host<SK_ACT>(B, logits, masks, temps, key, stream, word_pos, actions, draws_used);
        return BPPO_OK;
    }
    // the rows' draw indices in row order, as k_eval_group's second prefix gives them
    std::vector<int32_t> didx((size_t)B);
    int32_t nd = 0;
    for (int b = 0; b < B; b++) didx[b] = bppo_eval::temp_draws(temps[b]) ? nd++ : -1;
    const size_t nA = (size_t)B * A;
    DeviceMem buf;   // this call's buffers, freed when it ends
    float *d_l = nullptr, *d_t = nullptr;
    uint8_t *d_m = nullptr;
    int32_t *d_di = nullptr, *d_a = nullptr, *d_u = nullptr, *d_e = nullptr;
    Key8 *d_key = nullptr;
    uint64_t *d_pos = nullptr;
    int32_t err = 0;
    if (buf.alloc(&d_l, nA) != hipSuccess || buf.alloc(&d_m, nA) != hipSuccess || buf.alloc(&d_t, (size_t)B) != hipSuccess ||
        buf.alloc(&d_di, (size_t)B) != hipSuccess || buf.alloc(&d_a, (size_t)B) != hipSuccess ||
        buf.alloc(&d_u, (size_t)B) != hipSuccess || buf.alloc(&d_e, 1) != hipSuccess ||
        buf.alloc(&d_key, 1) != hipSuccess || buf.alloc(&d_pos, 1) != hipSuccess)
        return BPPO_ERR_HIP;
    if (hipMemcpy(d_l, logits, nA * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_m, masks, nA, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_t, temps, 4ull * B, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_di, didx.data(), 4ull * B, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_key, &key, sizeof(Key8), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_pos, &word_pos, 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_e, 0, 4) != hipSuccess)
        return BPPO_ERR_HIP;
    EvalSampleArgs g;                       // one pod of B rows, all of model 0
    g.N = B; g.logits = d_l; g.mask = d_m; g.group = nullptr; g.didx = d_di; g.temp = d_t; g.random_models = 0;
    g.pod_envs = B; g.pod_key = d_key; g.pod_rngpos = d_pos; g.stream = stream; g.act = d_a; g.used = d_u; g.err = d_e;
    if (eval_sample(A, nullptr, g) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(actions, d_a, 4ull * B, hipMemcpyDeviceToHost) != hipSuccess ||
        (draws_used && hipMemcpy(draws_used, d_u, 4ull * B, hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy(&err, d_e, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return BPPO_ERR_HIP;
    return (err & EV_ERR_ZERO_SUM) ? BPPO_ERR_NONFINITE : BPPO_OK;
}

static uint64_t random_mask(const int32_t *is_random, int K) {
    uint64_t m = 0;
    for (int k = 0; k < K; k++)
        if (is_random && is_random[k]) m |= 1ull << k;
    return m;
}

// One pod's slots from its P seats: slot_model (-1 on entry) = the distinct seated models in
// first-appearance order, or in ascending model index.
static void pod_slots(const int32_t *seat_model, int P, bool ascending, int32_t *slot_model) {
    int n = 0;
    for (int p = 0; p < P; p++)
        if (std::find(slot_model, slot_model + n, seat_model[p]) == slot_model + n) slot_model[n++] = seat_model[p];
    if (ascending) std::sort(slot_model, slot_model + n);
}

// The evaluation loop behind both entry points, which have checked their arguments: n_pods
// matchups of E envs on the context's n_pods * E envs.  slot_model [n_pods][P]: each pod's
// draw order (EvalState); who: the prefix of the error messages.
static bppo_status evaluate_run(bppo_ctx *c, const std::string &who, const bppo_eval_config *cfg, int K,
                                const float *params, const double *norm_mean, const double *norm_m2,
                                const double *norm_count, uint64_t random_models, int n_pods, int E,
                                const uint64_t *pod_seeds, const int32_t *pod_seat_model,
                                const std::vector<int32_t> &slot_model, bppo_eval_game *games, int cap_per_pod,
                                int32_t *n_games, uint64_t *rng_word_pos) {
    const int P = c->Pa, N = c->N, A = c->A, L = c->L;
    drop_prefetch(c);
    if (!c->gae_done) c->collected = 0;       // a rollout not yet bootstrapped would read the evaluation's envs
    for (int k = 0; k < n_pods; k++) n_games[k] = 0;

    // per pod: StdRng(pod_seeds[k]), whose first u64 seeds its envs (bppo_eval.h pod_key)
    std::vector<Key8> keys((size_t)n_pods);
    std::vector<uint64_t> env_seed((size_t)N);
    for (int k = 0; k < n_pods; k++) {
        uint64_t base_seed;
        keys[k] = bppo_eval::pod_key(pod_seeds[k], &base_seed);
        for (int j = 0; j < E; j++) env_seed[(size_t)k * E + j] = base_seed + (uint64_t)j;
    }

    const std::vector<int32_t> perms = generate_permutations(P);
    const int nperm = (int)(perms.size() / (size_t)P);

    DeviceMem buf;   // this call's buffers, freed when it ends
    EvalState s{};
    int32_t *d_perm_tab = nullptr, *d_seat_model = nullptr, *d_slot_model = nullptr;
    float *d_oxc = nullptr, *d_ologits = nullptr;
    ModelSet mod;
    EvalOutcome *d_sink = nullptr;
    bppo_eval_game *d_games = nullptr;
    Key8 *d_keys = nullptr;
    uint64_t *d_env_seed = nullptr;
    const int cap = std::min(cap_per_pod, cfg->num_games);
    const size_t ncount = (size_t)(K + 1) * n_pods;
    BPPO_HIP(c, buf.alloc(&d_perm_tab, perms.size()));
    BPPO_HIP(c, buf.alloc(&d_seat_model, (size_t)n_pods * P));
    BPPO_HIP(c, buf.alloc(&d_slot_model, (size_t)n_pods * P));
    BPPO_HIP(c, buf.alloc(&d_keys, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&d_env_seed, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.perm_idx, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.moves, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.frozen, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.group, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.gpos, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.didx, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.lrank, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.tempv, (size_t)N));
    BPPO_HIP(c, buf.alloc(&s.counts, ncount));
    BPPO_HIP(c, buf.alloc(&s.offs, ncount));
    BPPO_HIP(c, buf.alloc(&s.games, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&s.active, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&s.ndraw, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&s.rngpos, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&s.hdr, 1));
    BPPO_HIP(c, buf.alloc(&d_oxc, (size_t)N * L));
    BPPO_HIP(c, buf.alloc(&d_ologits, (size_t)N * A));
    BPPO_HIP(c, buf.alloc(&d_sink, (size_t)N));
    BPPO_HIP(c, buf.alloc(&d_games, (size_t)n_pods * cap));
    EvalHdr *h_hdr = nullptr;
    BPPO_HIP(c, buf.alloc_pinned(&h_hdr, 1));
    s.n_pods = n_pods; s.E = E; s.P = P; s.K = K; s.nperm = nperm; s.num_games = cfg->num_games; s.cap = cap;
    s.temp = bppo_eval::TempSched{cfg->temp_initial, cfg->temp_final, cfg->temp_cutoff, cfg->temp_decay};
    s.perm_tab = d_perm_tab; s.seat_model = d_seat_model; s.slot_model = d_slot_model;
    s.err = c->d_err;

    // models: uploads ordered on the context's stream, drained before the host arrays may go
    TRY(mod.upload(c, buf, K, params, norm_mean, norm_m2, norm_count, random_models));
    BPPO_HIP(c, hipMemcpyAsync(d_perm_tab, perms.data(), sizeof(int32_t) * perms.size(), hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemcpyAsync(d_seat_model, pod_seat_model, sizeof(int32_t) * (size_t)n_pods * P, hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemcpyAsync(d_slot_model, slot_model.data(), sizeof(int32_t) * slot_model.size(), hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemcpyAsync(d_keys, keys.data(), sizeof(Key8) * keys.size(), hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemcpyAsync(d_env_seed, env_seed.data(), sizeof(uint64_t) * env_seed.size(), hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemsetAsync(c->d_err, 0, 4, c->stream));
    BPPO_HIP(c, hipMemsetAsync(c->d_ep_count, 0, 4, c->stream));
    hipLaunchKernelGGL(k_eval_init, dim3(std::min((N + 255) / 256, 1024)), dim3(256), 0, c->stream, s, (uint64_t)2);
    TRY(launch_check(c, "k_eval_init"));
    // per pod VecEnv::new (env j of pod k = E::new(base_k + j) and a reset), then set_all_num_players
    // resets every env again (env.rs:281-302, 313-326); E::new's reward shaping is the zero schedule
    // (liars_dice.rs:461-463, skull.rs:1062-1065); Skull is seated with the context's player_count
    BPPO_HIP(c, wide_env_reset(c->cfg.env_kind, c->stream, N, 0, P, c->d_wstate, c->d_env_pos, c->d_ep_ret, c->d_ep_len,
                               d_env_seed));
    BPPO_HIP(c, wide_env_reset_again(c->cfg.env_kind, c->stream, N, 0, c->d_wstate, c->d_env_pos, d_env_seed));

    // a pod's block: its envs rounded up to whole waves, 1,024 threads at most (a thread then owns a run of envs)
    const int pod_threads = std::min(EV_POD_THREADS, (E + 63) / 64 * 64);
    auto observe_group = [&]() -> bppo_status {
        BPPO_HIP(c, wide_env_observe(c->cfg.env_kind, c->G > 0, c->stream, N, c->d_wstate, c->d_bxc, c->d_bmask,
                                     c->d_bplayers));
        hipLaunchKernelGGL(k_eval_group, dim3(n_pods), dim3(pod_threads), 0, c->stream, s, c->d_bplayers);
        TRY(launch_check(c, "k_eval_group"));
        hipLaunchKernelGGL(k_eval_scan, dim3(1), dim3(EV_SCAN_THREADS), 0, c->stream, s);
        TRY(launch_check(c, "k_eval_scan"));
        BPPO_HIP(c, hipMemcpyAsync(h_hdr, s.hdr, sizeof(EvalHdr), hipMemcpyDeviceToHost, c->stream));
        BPPO_HIP(c, hipStreamSynchronize(c->stream));
        return BPPO_OK;
    };
    TRY(observe_group());
    bppo_status st = BPPO_OK;
    for (int step = 0;; step++) {
        const EvalHdr &h = *h_hdr;
        if (h.unfinished == 0) break;              // every pod: num_games games or no active env (eval.rs:1670-1674)
        if (step >= cfg->max_steps) { c->err = who + ": max_steps exceeded before every pod had played num_games games"; st = BPPO_ERR_ARG; break; }
        TRY(models_step_forward(c, mod, s.group, s.gpos, h.gbase, s.hdr->gbase, c->d_bxc, d_oxc, d_ologits,
                                c->d_logits));
        EvalSampleArgs g;
        g.N = N; g.logits = c->d_logits; g.mask = c->d_bmask; g.group = s.group; g.didx = s.didx; g.temp = s.tempv;
        g.random_models = random_models; g.pod_envs = E; g.pod_key = d_keys; g.pod_rngpos = s.rngpos; g.stream = 0;
        g.act = c->d_act_in; g.used = nullptr; g.err = c->d_err;
        BPPO_HIP(c, eval_sample(A, c->stream, g));
        WideStepArgs w;
        w.N = N; w.t = step; w.state = c->d_wstate; w.env_pos = c->d_env_pos; w.seed_base = 0;
        w.actions = c->d_act_in; w.shaping = 0.0f;
        w.all_r = nullptr; w.rew_act = nullptr; w.done_f = nullptr; w.done_u8 = c->d_scr_d;
        w.ep_ret = c->d_ep_ret; w.ep_len = c->d_ep_len; w.eps = c->d_eps; w.ep_count = c->d_ep_count;
        w.eps_cap = 0; w.err = c->d_err;
        w.frozen = s.frozen; w.sink = d_sink; w.env_seed = d_env_seed;
        BPPO_HIP(c, wide_env_step(c->cfg.env_kind, c->stream, w));
        hipLaunchKernelGGL(k_eval_finish, dim3(n_pods), dim3(pod_threads), 0, c->stream, s, step, c->d_scr_d, d_sink,
                           d_games);
        TRY(launch_check(c, "k_eval_finish"));
        TRY(observe_group());
    }
    // results, also after a max_steps error: every pod's game count and RNG position, then its
    // games; the episode counter back to zero
    BPPO_HIP(c, hipMemcpyAsync(n_games, s.games, sizeof(int32_t) * (size_t)n_pods, hipMemcpyDeviceToHost, c->stream));
    if (rng_word_pos)
        BPPO_HIP(c, hipMemcpyAsync(rng_word_pos, s.rngpos, sizeof(uint64_t) * (size_t)n_pods, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, hipMemsetAsync(c->d_ep_count, 0, 4, c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    BPPO_HIP(c, bppo_eval::fetch_pod_games(c->stream, d_games, n_pods, cap, n_games, games, cap_per_pod));
    if (st != BPPO_OK) return st;
    const int32_t err = h_hdr->err;
    if (err & 8) { c->err = who + ": an action outside the env's action mask"; return BPPO_ERR_ARG; }
    if (err & EV_ERR_ZERO_SUM) { c->err = who + ": the sampler's softmax sum was zero"; return BPPO_ERR_NONFINITE; }
    return BPPO_OK;
}

// One pod of all the context's envs, seeded with cfg->seed, drawing over the seated models in
// ascending model index (eval.rs:1685-1769).
extern "C" bppo_status bppo_evaluate(bppo_ctx *c, const bppo_eval_config *cfg, int32_t n_models, const float *params,
                                     const double *norm_mean, const double *norm_m2, const double *norm_count,
                                     const int32_t *is_random, const int32_t *seat_model, int32_t n_checkpoints,
                                     bppo_eval_game *games, int32_t cap, int32_t *n_games, uint64_t *rng_word_pos) {
    if (!c) return BPPO_ERR_ARG;
    if (!c->wide || c->cfg.env_kind == BPPO_ENV_CARTPOLE) {
        c->err = "evaluate: multi-player envs only (no stats mode for CartPole)";
        return BPPO_ERR_UNSUPPORTED;
    }
    if (!cfg || !seat_model || !n_games || (cap > 0 && !games) || cap < 0) { c->err = "evaluate: NULL argument"; return BPPO_ERR_ARG; }
    if (cfg->num_games < 0 || cfg->max_steps < 0) { c->err = "evaluate: num_games and max_steps must not be negative"; return BPPO_ERR_ARG; }
    if (n_models < 1 || n_models > EV_SINGLE_MAX_MODELS) { c->err = "evaluate: 1..15 models"; return BPPO_ERR_ARG; }
    const int P = c->Pa, K = n_models;
    // the reference's permutations are over 0..num_players and a further checkpoint panics
    // (eval.rs:1801-1804), fewer fail its assert (:1640-1643)
    if (n_checkpoints != P) { c->err = "evaluate: n_checkpoints must equal the seated player count"; return BPPO_ERR_ARG; }
    const uint64_t random_models = random_mask(is_random, K);
    for (int p = 0; p < P; p++)
        if (seat_model[p] < 0 || seat_model[p] >= K) { c->err = "evaluate: seat_model names a model out of range"; return BPPO_ERR_ARG; }
    if (random_models != (1ull << K) - 1ull && !params) { c->err = "evaluate: model parameters required"; return BPPO_ERR_ARG; }
    std::vector<int32_t> slot_model((size_t)P, -1);
    pod_slots(seat_model, P, true, slot_model.data());
    const uint64_t seed = cfg->seed;
    return evaluate_run(c, "evaluate", cfg, K, params, norm_mean, norm_m2, norm_count, random_models, 1, c->N, &seed,
                        seat_model, slot_model, games, cap, n_games, rng_word_pos);
}

// The pods draw over their models in first-appearance order of their seats (run_pod's
// de-duplication, tournament.rs:1811-1838).
extern "C" bppo_status bppo_evaluate_pods(bppo_ctx *c, const bppo_eval_config *cfg, int32_t n_models, const float *params,
                                          const double *norm_mean, const double *norm_m2, const double *norm_count,
                                          const int32_t *is_random, int32_t n_pods, int32_t envs_per_pod,
                                          const uint64_t *pod_seeds, const int32_t *pod_seat_model,
                                          bppo_eval_game *games, int32_t cap_per_pod, int32_t *n_games,
                                          uint64_t *rng_word_pos) {
    if (!c) return BPPO_ERR_ARG;
    if (!c->wide || c->cfg.env_kind == BPPO_ENV_CARTPOLE) {
        c->err = "evaluate_pods: multi-player envs only (no stats mode for CartPole)";
        return BPPO_ERR_UNSUPPORTED;
    }
    if (!cfg || !pod_seeds || !pod_seat_model || !n_games || (cap_per_pod > 0 && !games) || cap_per_pod < 0) {
        c->err = "evaluate_pods: NULL argument";
        return BPPO_ERR_ARG;
    }
    if (cfg->num_games < 0 || cfg->max_steps < 0) { c->err = "evaluate_pods: num_games and max_steps must not be negative"; return BPPO_ERR_ARG; }
    if (n_models < 1 || n_models > EV_MAX_MODELS) { c->err = "evaluate_pods: 1..64 models"; return BPPO_ERR_ARG; }
    if (n_pods < 1 || n_pods > EV_MAX_PODS) { c->err = "evaluate_pods: 1..1024 pods"; return BPPO_ERR_ARG; }
    const int P = c->Pa, K = n_models, E = envs_per_pod;
    if (E < 1 || (int64_t)n_pods * E != (int64_t)c->N) {
        c->err = "evaluate_pods: n_pods * envs_per_pod must equal the context's num_envs";
        return BPPO_ERR_ARG;
    }
    const uint64_t random_models = random_mask(is_random, K);
    for (int i = 0; i < n_pods * P; i++)
        if (pod_seat_model[i] < 0 || pod_seat_model[i] >= K) { c->err = "evaluate_pods: pod_seat_model names a model out of range"; return BPPO_ERR_ARG; }
    const uint64_t all_models = K == 64 ? ~0ull : (1ull << K) - 1ull;
    if (random_models != all_models && !params) { c->err = "evaluate_pods: model parameters required"; return BPPO_ERR_ARG; }
    std::vector<int32_t> slot_model((size_t)n_pods * P, -1);
    for (int k = 0; k < n_pods; k++)
        pod_slots(pod_seat_model + (size_t)k * P, P, false, &slot_model[(size_t)k * P]);
    return evaluate_run(c, "evaluate_pods", cfg, K, params, norm_mean, norm_m2, norm_count, random_models, n_pods, E,
                        pod_seeds, pod_seat_model, slot_model, games, cap_per_pod, n_games, rng_word_pos);
}

// Parity hook of the grouped forward: model k's rows are [gbase[k], gbase[k + 1]) of xc
// [gbase[n_models]][L] (rows before gbase[0] belong to nobody, as the frozen group's); logits
// [gbase[n_models]][A], a random model's rows and those before gbase[0] zero.  mode 0: one
// model after the other (launch_obs_norm_rows_on + wide_forward_actor); mode 1: the grouped
// launches.  The context gives the net shape, the stream and the hidden buffers d_hbuf, which
// are overwritten: a rollout not yet bootstrapped is dropped, as evaluate_run drops it; the
// context's parameters are not read.
extern "C" bppo_status bppo_debug_forward_groups(bppo_ctx *c, int32_t mode, int32_t n_models, const float *params,
                                                 const double *norm_mean, const double *norm_m2,
                                                 const double *norm_count, const int32_t *is_random,
                                                 const int32_t *gbase, const float *xc, float *logits) {
    if (!c) return BPPO_ERR_ARG;
    if (!c->wide || c->cfg.env_kind == BPPO_ENV_CARTPOLE) { c->err = "debug_forward_groups: multi-player envs only"; return BPPO_ERR_UNSUPPORTED; }
    if (mode != 0 && mode != 1) { c->err = "debug_forward_groups: mode 0 or 1"; return BPPO_ERR_ARG; }
    if (mode == 1 && c->net.n_conv) { c->err = "debug_forward_groups: nets with conv layers have no grouped forward"; return BPPO_ERR_UNSUPPORTED; }
    if (!gbase || !xc || !logits) { c->err = "debug_forward_groups: NULL argument"; return BPPO_ERR_ARG; }
    if (n_models < 1 || n_models > EV_MAX_MODELS) { c->err = "debug_forward_groups: 1..64 models"; return BPPO_ERR_ARG; }
    const int K = n_models, A = c->A, L = c->L;
    std::vector<int32_t> gb((size_t)K + 2, 0);
    for (int k = 0; k <= K; k++) {
        if (gbase[k] < gb[k]) { c->err = "debug_forward_groups: gbase must start at >= 0 and not decrease"; return BPPO_ERR_ARG; }
        gb[k + 1] = gbase[k];
    }
    const int rows = gb[K + 1];
    if (rows > c->rows_max) { c->err = "debug_forward_groups: more rows than the context's buffers hold"; return BPPO_ERR_ARG; }
    const uint64_t random_models = random_mask(is_random, K);
    const uint64_t all_models = K == 64 ? ~0ull : (1ull << K) - 1ull;
    if (random_models != all_models && !params) { c->err = "debug_forward_groups: model parameters required"; return BPPO_ERR_ARG; }
    if (rows == 0) return BPPO_OK;
    drop_prefetch(c);
    if (!c->gae_done) c->collected = 0;       // the hidden buffers are the rollout's
    DeviceMem buf;   // this call's buffers, freed when it ends
    ModelSet mod;
    int32_t *d_gb = nullptr;
    float *d_x = nullptr, *d_l = nullptr;
    BPPO_HIP(c, buf.alloc(&d_gb, gb.size()));
    BPPO_HIP(c, buf.alloc(&d_x, (size_t)rows * L));
    BPPO_HIP(c, buf.alloc(&d_l, (size_t)rows * A));
    TRY(mod.upload(c, buf, K, params, norm_mean, norm_m2, norm_count, random_models));
    BPPO_HIP(c, hipMemcpyAsync(d_gb, gb.data(), sizeof(int32_t) * gb.size(), hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemcpyAsync(d_x, xc, sizeof(float) * (size_t)rows * L, hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemsetAsync(d_l, 0, sizeof(float) * (size_t)rows * A, c->stream));
    TRY(forward_models(c, mod, gb.data(), d_gb, d_x, d_l, mode == 1));
    BPPO_HIP(c, hipMemcpyAsync(logits, d_l, sizeof(float) * (size_t)rows * A, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    return BPPO_OK;
}
