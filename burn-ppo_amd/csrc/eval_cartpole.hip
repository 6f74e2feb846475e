// eval_cartpole.hip — single-player stats-mode evaluation on the device:
// run_stats_mode_env::<CartPole> (eval.rs:1621-1877) with num_players = 1, whose summary is
// EvalStats::print_single_player_summary (eval.rs:416-469).  One checkpoint, one permutation,
// no action mask, no game_outcome: the envs of an evaluation are coupled only by three
// ordered counts per step (who draws a random word, which finished episodes are recorded,
// who is frozen), and all three are block-level scans.  So one thread block plays a whole
// evaluation (a pod), every env's state private to a thread, as k_cartpole_rollout plays a
// rollout; many independent evaluations (every checkpoint of a run, one checkpoint under
// many seeds) are the blocks of one launch.
//
// Per loop iteration of a pod (k_cartpole_eval), while games < num_games and an env is
// active (eval.rs:1670-1674):
//   pre-pass    per active env the temperature of its move count (eval.rs:1766) and whether
//               it draws; one scan: the env's word is rngpos + its rank among the pod's
//               drawing active envs, in env order (eval.rs:1685-1769 with one model)
//   body        obs -> ObsNormalizer::normalize_batch (eval.rs:1727-1734) -> cp_forward ->
//               sample_with_temperature, no mask (eval.rs:223-272) -> CartPole step, episode
//               total and length, auto-reset from the env's own stream (env.rs:400-487)
//   finish      k_eval_finish's two scans: the finished episodes recorded in env order up to
//               num_games, move counts, the freeze rule (eval.rs:1774-1869)
// A launch runs at most steps_per_launch iterations of every unfinished pod and leaves a
// per-pod header; the host reads the headers and relaunches.  Every kernel is a counted loop:
// nothing spins, no grid-wide barrier, no blocks that must be resident together.
#include <algorithm>
#include <cstring>
#include <vector>
#include "bppo_internal.h"
#include "bppo_eval.h"
#include "bppo_scan.h"

namespace bppo {

constexpr int CE_THREADS = 256;       // H = 64 tanh: parameters + the tanh stage are 83 KB of LDS at this width
constexpr int CE_MAX_PODS = 1024, CE_MAX_ENVS = 16384;
constexpr int CE_ERR_ZERO_SUM = 16;   // header err bit: the sampler's sum == 0.0 exit (bppo_eval.h temp_draws)
// default steps_per_launch: CE_LAUNCH_ENV_STEPS / (envs per thread).  Measured: an
// iteration of the 64 x 2 net takes 75-90 us per env a thread owns, so 256 env-steps per thread
// keep a launch near 20 ms whatever the pod size, and the header read (tens of us) stays under 1%
constexpr int CE_LAUNCH_ENV_STEPS = 256, CE_LAUNCH_MAX_STEPS = 256;

// one env of a pod between iterations and launches (global scratch of the call, L2-resident)
struct CpEvalEnv {
    float x, x_dot, theta, theta_dot;
    int32_t steps;
    float total;            // episode_rewards / episode_lengths of VecEnv (env.rs:413-431)
    int32_t length;
    int32_t moves;          // move_counts (eval.rs:1663)
    uint64_t env_pos;       // word position of the env's own StdRng
    int32_t frozen;         // terminal (eval.rs:1664)
    float fin_total;        // the episode finished this iteration, until the finish pass takes it
    int32_t fin_length;     // 0: none
    int32_t pad;
};
static_assert(sizeof(CpEvalEnv) == 56, "CpEvalEnv layout");

// a pod between launches; the host reads every pod's after each launch
struct CpEvalHdr {
    int32_t games, active, steps, err;
    uint64_t rngpos;
};

struct CpEvalArgs {
    int E, num_games, cap, max_steps, launch_steps, n_params;
    bppo_eval::TempSched temp;
    const float *params;        // [n_pods][n_params]
    const double *on;           // [n_pods][11] mean, M2, count (count 0: raw obs)
    const Key8 *key;            // [n_pods] the pod's StdRng key
    const uint64_t *base_seed;  // [n_pods] its first u64
    CpEvalEnv *env;             // [n_pods][E]
    CpEvalHdr *hdr;             // [n_pods]
    bppo_eval_game *games;      // [n_pods][cap]
};

// per pod StdRng words 0 and 1 seed the envs: env j = CartPole::new(base + j), which resets
// once (cartpole.rs:104), VecEnv::new resets again (env.rs:289-293) and set_all_num_players
// a third time (env.rs:313-326): three resets from the env's own stream before the first
// move; the pod's sampling draws follow from word 2 (eval.rs:1646-1648)
__global__ void __launch_bounds__(256) k_cartpole_eval_init(int n_pods, int E, const uint64_t *base_seed,
                                                            CpEvalEnv *env, CpEvalHdr *hdr) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < (size_t)n_pods) hdr[i] = CpEvalHdr{0, E, 0, 0, 2};
    if (i >= (size_t)n_pods * E) return;
    const int pod = (int)(i / E), j = (int)(i - (size_t)pod * E);
    WordCursor c;
    c.init(seed_key(base_seed[pod] + (uint64_t)j), 0, 0);
    CartPoleState s;
    cartpole_reset(s, c);
    cartpole_reset(s, c);
    cartpole_reset(s, c);
    CpEvalEnv ev;
    ev.x = s.x; ev.x_dot = s.x_dot; ev.theta = s.theta; ev.theta_dot = s.theta_dot; ev.steps = s.steps;
    ev.total = 0.0f; ev.length = 0; ev.moves = 0; ev.env_pos = c.pos; ev.frozen = 0;
    ev.fin_total = 0.0f; ev.fin_length = 0; ev.pad = 0;
    env[i] = ev;
}

// One block per pod; thread t owns the pod's envs [t per, (t + 1) per), so every scan below is
// in env order and the results do not depend on the block size.
template <int H, int NL, int ACT>
__global__ void __launch_bounds__(CE_THREADS) k_cartpole_eval(CpEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sP[];
    __shared__ MathLds T;
    __shared__ ObsNorm5 nz;
    __shared__ uint64_t wsum[CE_THREADS / 64];
    const int pod = blockIdx.x, tid = threadIdx.x;
    const CpEvalHdr h0 = a.hdr[pod];
    // a finished pod's block returns at once (block-uniform)
    if (h0.games >= a.num_games || h0.active == 0 || h0.steps >= a.max_steps) return;
    constexpr CpOffsets O = cp_offsets<H, NL>();
    const float *__restrict__ P = a.params + (size_t)pod * a.n_params;
    for (int i = tid; i < O.n; i += CE_THREADS) sP[i] = P[i];
    if (tid == 0) nz.load(a.on + (size_t)pod * 11, 1);       // eval.rs:1727-1734; count < 2: raw obs
    T.load();                                                 // (barrier: sP, nz, T)
    const int per = (a.E + CE_THREADS - 1) / CE_THREADS;
    const int j0 = min(a.E, tid * per), j1 = min(a.E, j0 + per);
    CpEvalEnv *__restrict__ env = a.env + (size_t)pod * a.E;
    const Key8 key = a.key[pod];
    const uint64_t base = a.base_seed[pod];
    // the pod's counters: the same in every thread (each scan's total is)
    int games = h0.games, active = h0.active, step = h0.steps;
    uint64_t rngpos = h0.rngpos;
    int bad = 0;
#pragma unroll 1
    for (int it = 0; it < a.launch_steps; it++) {
        if (games >= a.num_games || active == 0 || step >= a.max_steps) break;   // eval.rs:1670-1674
        // ---- who draws: temp = TempSchedule::get_temp(move_count) (eval.rs:1766); a draw is
        // consumed iff temp != 0 (eval.rs:240-272)
        uint32_t nd = 0;
        for (int j = j0; j < j1; j++)
            if (!env[j].frozen) nd += bppo_eval::temp_draws(bppo_eval::get_temp(a.temp, env[j].moves)) ? 1u : 0u;
        uint64_t tot;
        uint32_t d = (uint32_t)block_scan_excl((uint64_t)nd, wsum, &tot);
        const uint32_t ndraw = (uint32_t)tot;
        // ---- the env's move and step
        uint32_t ndone = 0, nact = 0;
#pragma unroll 1
        for (int j = j0; j < j1; j++) {
            CpEvalEnv ev = env[j];
            if (ev.frozen) continue;                         // a terminal env is not stepped (env.rs:407-411)
            nact++;
            CartPoleState s;
            s.x = ev.x; s.x_dot = ev.x_dot; s.theta = ev.theta; s.theta_dot = ev.theta_dot; s.steps = ev.steps;
            float raw[5], x[5];
            cartpole_obs(s, raw);
            nz.apply(raw, x);
            float lg[2], v;
            int zero = 0;
            asm volatile("" : "+v"(zero));                   // keep weight reads inside the step loop (no LICM spill)
            cp_forward<H, NL, ACT>(sP + zero, x, lg, v, sP + cp_stage_ofs<H, NL>() + tid, CE_THREADS);
            const float temp = bppo_eval::get_temp(a.temp, ev.moves);
            const bool draws = bppo_eval::temp_draws(temp);
            uint32_t word = 0;
            if (draws) word = chacha12_word(key, 0, rngpos + (uint64_t)d++);
            int used = 0;
            const int act = bppo_eval::sample_with_temperature<2>(lg, 0, temp, word, &used, T);   // mask None
            bad |= used != (draws ? 1 : 0);
            float r;
            const bool done = cartpole_step(s, act, r);
            ev.total = __fadd_rn(ev.total, r);               // env.rs:413-431
            ev.length += 1;
            if (done) {                                      // env.rs:433-467: completed episode, auto-reset
                ev.fin_total = ev.total;
                ev.fin_length = ev.length;
                WordCursor ec;
                ec.init(seed_key(base + (uint64_t)j), 0, ev.env_pos);
                cartpole_reset(s, ec);
                ev.env_pos = ec.pos;
                ev.total = 0.0f;
                ev.length = 0;
                ndone++;
            }
            ev.x = s.x; ev.x_dot = s.x_dot; ev.theta = s.theta; ev.theta_dot = s.theta_dot; ev.steps = s.steps;
            env[j] = ev;
        }
        // ---- records, move counts, the freeze rule (eval.rs:1774-1869), as k_eval_finish
        const uint64_t ex = block_scan_excl((uint64_t)ndone | ((uint64_t)nact << 32), wsum, &tot);
        const int ND = (int)(uint32_t)tot, ACTV = (int)(tot >> 32);
        const int nrec = min(ND, max(0, a.num_games - games));                   // :1783-1789
        const int g1 = games + nrec;
        const int remaining = max(0, a.num_games - g1);                          // :1841-1869
        const int to_freeze = ACTV > remaining ? ACTV - remaining : 0;
        const int f1 = min(to_freeze, ND), f2 = to_freeze - f1;                  // just-finished envs first
        int k = (int)(uint32_t)ex;
        uint32_t alive = 0;
        for (int j = j0; j < j1; j++) {
            int mv = env[j].moves + 1;                       // every env, frozen ones included (:1775-1777)
            int fz = env[j].frozen;
            const int fl = env[j].fin_length;
            if (fl) {
                if (k < nrec) {
                    // rewards_to_placements of one reward: place 1 (eval.rs:276-306, :1822-1825)
                    bppo_eval_game rec;
                    for (int c = 0; c < BPPO_MAX_PLAYERS; c++) { rec.total_reward[c] = 0.0f; rec.placement[c] = 0; }
                    rec.total_reward[0] = env[j].fin_total;
                    rec.placement[0] = 1;
                    rec.length = fl; rec.env_index = j; rec.perm_index = 0; rec.step = step;
                    if (games + k < a.cap) a.games[(size_t)pod * a.cap + games + k] = rec;
                    mv = 0;                                  // :1830; a dropped episode leaves the count alone
                }
                if (k < f1) fz = 1;
                k++;
                env[j].fin_length = 0;
            }
            env[j].moves = mv;
            env[j].frozen = fz;
            alive += fz == 0;
        }
        if (f2 > 0) {                                        // then active envs from index 0 (the same in every thread)
            uint64_t t2;
            int r = (int)(uint32_t)block_scan_excl((uint64_t)alive, wsum, &t2);
            for (int j = j0; j < j1; j++)
                if (!env[j].frozen) {
                    if (r < f2) env[j].frozen = 1;
                    r++;
                }
        }
        games = g1;
        active = ACTV - to_freeze;
        rngpos += (uint64_t)ndraw;
        step++;
    }
    const int anybad = __syncthreads_or(bad);
    if (tid == 0) {
        CpEvalHdr h;
        h.games = games; h.active = active; h.steps = step; h.err = h0.err | (anybad ? CE_ERR_ZERO_SUM : 0);
        h.rngpos = rngpos;
        a.hdr[pod] = h;
    }
}

static bppo_status launch_cartpole_eval(bppo_ctx *c, int n_pods, const CpEvalArgs &a) {
    const int h = c->cfg.hidden_size, nl = c->cfg.num_hidden;
    const dim3 grid(n_pods), blk(CE_THREADS);
#define L(H_, NL_, A_) \
    hipLaunchKernelGGL((k_cartpole_eval<H_, NL_, A_>), grid, blk, (cp_lds<H_, NL_>(A_, CE_THREADS)), c->stream, a)
#define D(H_, NL_)                                                            \
    if (h == H_ && nl == NL_) {                                               \
        if (c->cfg.relu) L(H_, NL_, ACT_RELU); else L(H_, NL_, ACT_TANH);     \
        return launch_check(c, "k_cartpole_eval");                            \
    }
    D(16, 1) D(16, 2) D(32, 1) D(32, 2) D(64, 1) D(64, 2)
#undef D
#undef L
    c->err = "evaluate_episodes: no fused kernel for this net";
    return BPPO_ERR_UNSUPPORTED;
}

}  // namespace bppo

using namespace bppo;

extern "C" bppo_status bppo_evaluate_episodes(bppo_ctx *c, const bppo_eval_config *cfg, int32_t n_pods,
                                              int32_t envs_per_pod, const float *params, const double *norm_mean,
                                              const double *norm_m2, const double *norm_count,
                                              const uint64_t *pod_seeds, int32_t steps_per_launch,
                                              bppo_eval_game *games, int32_t cap_per_pod, int32_t *n_games,
                                              uint64_t *rng_word_pos, int32_t *loop_steps) {
    if (!c) return BPPO_ERR_ARG;
    if (c->cfg.env_kind != BPPO_ENV_CARTPOLE) {
        c->err = "evaluate_episodes: CartPole contexts only (multi-player envs: bppo_evaluate / bppo_evaluate_pods)";
        return BPPO_ERR_UNSUPPORTED;
    }
    if (c->wide) {
        c->err = "evaluate_episodes: only the fused CartPole nets, hidden {16, 32, 64} x {1, 2} layers without "
                 "split_networks (this context's net runs on the GEMM path)";
        return BPPO_ERR_UNSUPPORTED;
    }
    if (!cfg || !params || !pod_seeds || !n_games || (cap_per_pod > 0 && !games) || cap_per_pod < 0) {
        c->err = "evaluate_episodes: NULL argument";
        return BPPO_ERR_ARG;
    }
    if (cfg->num_games < 0 || cfg->max_steps < 0) { c->err = "evaluate_episodes: num_games and max_steps must not be negative"; return BPPO_ERR_ARG; }
    if (n_pods < 1 || n_pods > CE_MAX_PODS) { c->err = "evaluate_episodes: n_pods must be 1..1024"; return BPPO_ERR_ARG; }
    if (envs_per_pod < 1 || envs_per_pod > CE_MAX_ENVS) { c->err = "evaluate_episodes: envs_per_pod must be 1..16384"; return BPPO_ERR_ARG; }
    if (steps_per_launch < 0) { c->err = "evaluate_episodes: steps_per_launch must not be negative"; return BPPO_ERR_ARG; }
    const int E = envs_per_pod;
    const size_t np = c->net.n_params, N = (size_t)n_pods * E;
    const int per = (E + CE_THREADS - 1) / CE_THREADS;
    const int launch_steps = steps_per_launch > 0 ? steps_per_launch
                                                  : std::max(1, std::min(CE_LAUNCH_MAX_STEPS, CE_LAUNCH_ENV_STEPS / per));
    const int cap = std::min(cap_per_pod, cfg->num_games);

    // per pod: StdRng(pod_seeds[k]) and its first u64, which seeds the pod's envs (bppo_eval.h pod_key)
    std::vector<Key8> keys((size_t)n_pods);
    std::vector<uint64_t> base_seed((size_t)n_pods);
    for (int k = 0; k < n_pods; k++) keys[k] = bppo_eval::pod_key(pod_seeds[k], &base_seed[k]);

    DeviceMem buf;   // this call's buffers, freed when it ends
    CpEvalArgs a{};
    ModelSet mod;    // pod k plays model k: blocks of 2 D + 1 = 11 doubles (CpEvalArgs::on)
    Key8 *d_keys = nullptr;
    uint64_t *d_base = nullptr;
    BPPO_HIP(c, buf.alloc(&d_keys, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&d_base, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&a.env, N));
    BPPO_HIP(c, buf.alloc(&a.hdr, (size_t)n_pods));
    BPPO_HIP(c, buf.alloc(&a.games, (size_t)n_pods * cap));
    CpEvalHdr *h_hdr = nullptr;
    BPPO_HIP(c, buf.alloc_pinned(&h_hdr, (size_t)n_pods));
    a.E = E; a.num_games = cfg->num_games; a.cap = cap; a.max_steps = cfg->max_steps; a.launch_steps = launch_steps;
    a.n_params = (int)np;
    a.temp = bppo_eval::TempSched{cfg->temp_initial, cfg->temp_final, cfg->temp_cutoff, cfg->temp_decay};
    // uploads ordered on the context's stream; the first header read below drains them
    // before the host arrays may go
    TRY(mod.upload(c, buf, n_pods, params, norm_mean, norm_m2, norm_count, 0, false));
    a.params = mod.d_params; a.on = mod.d_on; a.key = d_keys; a.base_seed = d_base;
    BPPO_HIP(c, hipMemcpyAsync(d_keys, keys.data(), sizeof(Key8) * keys.size(), hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemcpyAsync(d_base, base_seed.data(), sizeof(uint64_t) * base_seed.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_cartpole_eval_init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, n_pods, E,
                       (const uint64_t *)d_base, a.env, a.hdr);
    TRY(launch_check(c, "k_cartpole_eval_init"));
    auto read_headers = [&]() -> bppo_status {
        BPPO_HIP(c, hipMemcpyAsync(h_hdr, a.hdr, sizeof(CpEvalHdr) * (size_t)n_pods, hipMemcpyDeviceToHost, c->stream));
        BPPO_HIP(c, hipStreamSynchronize(c->stream));
        return BPPO_OK;
    };
    auto unfinished = [&](int k) { return h_hdr[k].games < cfg->num_games && h_hdr[k].active > 0; };
    TRY(read_headers());
    for (;;) {
        bool more = false;
        for (int k = 0; k < n_pods; k++) more = more || (unfinished(k) && h_hdr[k].steps < cfg->max_steps);
        if (!more) break;
        TRY(launch_cartpole_eval(c, n_pods, a));
        TRY(read_headers());
    }
    // results, also after a max_steps error
    bool over = false;
    int32_t err = 0;
    for (int k = 0; k < n_pods; k++) {
        const CpEvalHdr &h = h_hdr[k];
        n_games[k] = h.games;
        if (rng_word_pos) rng_word_pos[k] = h.rngpos;
        if (loop_steps) loop_steps[k] = h.steps;
        over = over || unfinished(k);
        err |= h.err;
    }
    BPPO_HIP(c, bppo_eval::fetch_pod_games(c->stream, a.games, n_pods, cap, n_games, games, cap_per_pod));
    if (over) { c->err = "evaluate_episodes: max_steps exceeded before every pod had played num_games episodes"; return BPPO_ERR_ARG; }
    if (err & CE_ERR_ZERO_SUM) { c->err = "evaluate_episodes: the sampler's softmax sum was zero"; return BPPO_ERR_NONFINITE; }
    return BPPO_OK;
}
