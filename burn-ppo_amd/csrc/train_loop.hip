// train_loop.hip — the host-side orchestration of one update (collect_rollouts ->
// bootstrap + GAE -> ppo_update, main.rs:724-963) and of whole iterations
// (bppo_train_step, bppo_train_steps).  No kernel lives here: every function enqueues
// launchers of the other translation units and reads their results.
#include <algorithm>
#include <pthread.h>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>
#include <x86intrin.h>
#include "bppo_internal.h"
#include "shuffle_host.h"
#include "bppo_wide.h"
#include "bppo_update_metrics.h"

using namespace bppo;

// TSC ticks per millisecond, measured once against steady_clock (shuffle engine
// diagnostics)
static double tsc_per_ms() {
    static double v = 0.0;
    if (v == 0.0) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t c0 = __rdtsc();
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
        const uint64_t c1 = __rdtsc();
        v = (double)(c1 - c0) / std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return v;
}

// wait for an event of the context stream: the host thread sleeps instead of polling
// (see sync_stream, bppo_api.hip).
// The per-update wait of bppo_train_steps (~12 ms on CfgB) repeats from one update to
// the next, so it starts with ONE coarse sleep of 70 % of the recent waits and only
// then polls at 20 us: every poll is a wake-up plus an event query, and polling the
// whole wait cost the driving thread ~1 CPU per rank (14 ms of CPU per 13.9 ms update
// in r03h), CPU the shuffle walkers of an 8-rank node need.
static hipError_t wait_event(bppo_ctx *c, hipEvent_t ev) {   // sleeping poll (see sync_stream)
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = event_query(ev);
    if (e == hipErrorNotReady) {
        if (c->wait_est_us > 200.0)
            std::this_thread::sleep_for(std::chrono::microseconds((long)(0.7 * c->wait_est_us)));
        while ((e = event_query(ev)) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->wait_est_us = c->wait_est_us > 0.0 ? 0.5 * c->wait_est_us + 500.0 * ms : 1000.0 * ms;
    c->sync_wait_ms += ms;
    return e;
}

static bppo_status tm_begin(bppo_ctx *c, int slot) {
    BPPO_HIP(c, hipEventRecord(c->ev[slot][0], c->stream));
    return BPPO_OK;
}
static bppo_status tm_end(bppo_ctx *c, int slot) {
    BPPO_HIP(c, hipEventRecord(c->ev[slot][1], c->stream));
    return BPPO_OK;
}
static void tm_read(bppo_ctx *c, int slot) {
    float ms = 0;
    if (event_ms(c->ev[slot][0], c->ev[slot][1], &ms)) c->last_ms[slot] = ms;
}

// Fisher-Yates of every epoch of the engine's job in `slot` whose J is already on
// the device (the host engine has resolved it), in epoch order on fy_stream,
// each into its own permutation buffer (ppo.rs:1816 indices.shuffle; the
// permutation of epoch e depends only on that epoch's RNG words)
static bppo_status fy_enqueue_ready(bppo_ctx *c, int slot) {
    const size_t B = (size_t)c->T * c->N;
    if (slot != c->fy_slot) {
        // a new update's permutations overwrite perm/inv, which the previous update's
        // minibatches may still be reading when its successor's rollout is enqueued
        // behind it (bppo_train_steps): wait for the end of that update
        c->fy_slot = slot; c->fy_done = 0;
        BPPO_HIP(c, hipStreamWaitEvent(c->fy_stream, c->ev_upd, 0));
    }
    if (c->shuf.failed(c->err)) return BPPO_ERR_HIP;
    while (c->fy_done < c->cfg.num_epochs && c->shuf.epoch_ready(slot, c->fy_done)) {
        const int e = c->fy_done;
        // the engine thread may have recorded a HIP failure (J upload, expansion, event) and
        // then marked this epoch ready: its J is not to be permuted
        if (c->shuf.failed(c->err)) return BPPO_ERR_HIP;
        BPPO_HIP(c, hipStreamWaitEvent(c->fy_stream, c->shuf.ev[slot][e], 0));
        if (e > 0) BPPO_HIP(c, hipStreamWaitEvent(c->fy_stream, c->fy_ev[e - 1], 0));   // shared scratch
        BPPO_HIP(c, hipEventRecord(c->ev[TM_SHUFFLE][0], c->fy_stream));
        BPPO_HIP(c, fisher_yates_device(c->shuf.d_J[slot] + (size_t)e * B, (uint32_t)B, c->d_fy, c->d_scan,
                                        c->d_perm_ep + (size_t)e * B, c->fy_stream, &c->fyr,
                                        c->d_inv_ep + (size_t)e * B));
        BPPO_HIP(c, hipEventRecord(c->ev[TM_SHUFFLE][1], c->fy_stream));
        BPPO_HIP(c, hipEventRecord(c->fy_ev[e], c->fy_stream));
        c->fy_done++;
    }
    return BPPO_OK;
}

// collect_rollouts (ppo.rs:213-500), enqueue half: everything up to the episode
// summary and the device flags' copies into pinned host words (no host wait)
// the rollout's device flags and episode partials land in one of two pinned slots, so
// a rollout enqueued behind an update (bppo_train_steps) does not overwrite the
// previous rollout's before they are read
static double *roll_host(bppo_ctx *c, int slot) { return c->h_red + 4 * 1024 + 64 + (size_t)slot * ROLL_HOST_WORDS; }

static bppo_status collect_enqueue(bppo_ctx *c, bool summary) {
    const size_t TN = (size_t)c->T * c->N;
    c->coll_slot ^= 1;
    const int tro = c->coll_slot ? TM_ROLLOUT_B : TM_ROLLOUT, trn = c->coll_slot ? TM_RETNORM_B : TM_RETNORM;
    // the episode counter and error flags start at 0: zeroed here for the wide envs, by the
    // CartPole launcher (in its Gumbel kernel where that runs on the update stream)
    if (c->wide) {
        BPPO_HIP(c, hipMemsetAsync(c->d_ep_count, 0, 4, c->stream));
        BPPO_HIP(c, hipMemsetAsync(c->d_err, 0, 4, c->stream));
        if (opp_active(c)) TRY(opp_records_clear(c));   // the finished opponent games go with the episodes
    }
    const uint64_t base = c->rng_pos;
    TRY(tm_begin(c, tro));
    if (c->wide) TRY(wide_collect(c, base));
    else {
        TRY(launch_cartpole_rollout(c, base, nullptr, nullptr, c->cfg.normalize_obs));
        TRY(popart_denorm(c, c->d_val, TN));            // ppo.rs:355-359 (multi-player: in the sampler)
    }
    TRY(tm_end(c, tro));
    // self-play: the update's shuffles start right after this rollout's Gumbel words,
    // so the epochs the engine has resolved are permuted now, beside the rollout
    // (beside the rollout is where they cost least: it leaves VGPRs and LDS free on every
    // CU, while the minibatch kernels fill them -- profiles/r03j_mb_overlap.txt)
    if (!opp_active(c)) {
        c->shuf_slot = c->shuf.ensure(base + TN * (uint64_t)c->A);
        TRY(fy_enqueue_ready(c, c->shuf_slot));
    }
    if (opp_active(c)) {
        // opponent pool: seat reshuffles drew a data-dependent number of words
        TRY(opp_rollout_end(c));
    } else {
        c->rng_pos = base + TN * (uint64_t)c->A;   // one word per (env, action) per step
        // this update's shuffles start here; the engine usually began them already
        c->shuf_slot = c->shuf.ensure(c->rng_pos);
    }
    if (c->cfg.normalize_obs) TRY(launch_obs_norm_merge(c));       // ppo.rs:495-497
    TRY(tm_begin(c, trn));
    if (c->cfg.normalize_returns) TRY(launch_return_norm(c));      // ppo.rs:390-408
    else if (!c->wide) BPPO_HIP(c, hipMemcpyAsync(c->d_rew, c->d_rew_raw, TN * 4, hipMemcpyDeviceToDevice, c->stream));
    TRY(tm_end(c, trn));
    int32_t *hv = reinterpret_cast<int32_t *>(roll_host(c, c->coll_slot));     // pinned
    c->roll_has_stats[c->coll_slot] = c->ep_stats_on != 0;
    if (summary || c->ep_stats_on) {
        // the summary kernel writes the episode count, the error flags and its partial sums in
        // the host slot's layout: into d_ep_sum and ONE copy (r05: three); the episode
        // statistics, when on, fill the rest of the slot and ride the same copy
        TRY(launch_episode_summary(c, c->d_ep_sum));
        if (c->ep_stats_on) TRY(launch_episode_stats(c, c->d_ep_sum));
        const size_t words = c->ep_stats_on ? ROLL_HOST_WORDS : ROLL_BASE_WORDS;
        BPPO_HIP(c, hipMemcpyAsync(hv, c->d_ep_sum, sizeof(double) * words, hipMemcpyDeviceToHost, c->stream));
    } else {
        BPPO_HIP(c, hipMemcpyAsync(&hv[0], c->d_ep_count, 4, hipMemcpyDeviceToHost, c->stream));
        BPPO_HIP(c, hipMemcpyAsync(&hv[1], c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
    }
    c->collected = 1; c->gae_done = 0;
    c->rollout_rng_pos[c->coll_slot] = c->rng_pos;   // RNG position after the rollout (info; the update moves it on)
    return BPPO_OK;
}

// finish half, after the stream has drained past collect_enqueue: device error
// flags -> status, episode summary -> info
static bppo_status collect_finish(bppo_ctx *c, bppo_rollout_info *info, int slot) {
    float ms = 0;
    const int tro = slot ? TM_ROLLOUT_B : TM_ROLLOUT, trn = slot ? TM_RETNORM_B : TM_RETNORM;
    if (event_ms(c->ev[tro][0], c->ev[tro][1], &ms)) c->last_ms[TM_ROLLOUT] = ms;
    if (event_ms(c->ev[trn][0], c->ev[trn][1], &ms)) c->last_ms[TM_RETNORM] = ms;
    const int32_t *hv = reinterpret_cast<const int32_t *>(roll_host(c, slot));
    const double *part = roll_host(c, slot) + 2;
    // device error bits: 1 non-finite log-prob, 2 empty action mask, 4 opponent seat
    // table names a model outside [0, n_models)
    if (hv[1] & 2) { c->err = "Empty action mask: an env has no valid action"; return BPPO_ERR_EMPTY_MASK; }
    if (hv[1] & 1) { c->err = "NaN/Inf in log probs — model producing corrupt logits"; return BPPO_ERR_NONFINITE; }
    if (hv[1] & 4) { c->err = "opponent pool: pos_to_opp names a model index outside [0, n_models)"; return BPPO_ERR_ARG; }
    if (hv[1] & 8) { c->err = "Invalid action: outside the env's action mask"; return BPPO_ERR_ARG; }   // skull.rs:1116-1128
    if (hv[1]) { c->err = "collect_rollouts: unknown device error flag"; return BPPO_ERR_HIP; }
    if (c->roll_has_stats[slot]) {
        // out of the pinned slot (there are two; bppo_train_steps runs n rollouts)
        const double *sl = roll_host(c, slot);
        bppo_ctx::EpEntry en;
        std::memcpy(&en.st, sl + ROLL_STATS_OFF, sizeof en.st);
        int32_t nt = 0;
        std::memcpy(&nt, sl + ROLL_NTAIL_OFF, 4);
        nt = std::max(0, std::min(nt, (int32_t)BPPO_EPISODE_TAIL));
        en.tail.resize((size_t)nt);
        if (nt) std::memcpy(en.tail.data(), sl + ROLL_TAIL_OFF, sizeof(bppo_episode_tail) * (size_t)nt);
        c->ep_entries.push_back(std::move(en));
    }
    if (info) {
        info->episodes = hv[0];
        info->rng_word_pos = c->rollout_rng_pos[slot];
        info->mean_return = 0; info->mean_length = 0;
        const int n = std::min(hv[0], c->eps_cap);
        if (n > 0) {
            double sr = 0, sl = 0;
            for (int b = 0; b < EP_SUMMARY_BLOCKS; b++) { sr += part[2 * b]; sl += part[2 * b + 1]; }
            info->mean_return = (float)(sr / n); info->mean_length = (float)(sl / n);
        }
    }
    return BPPO_OK;
}

extern "C" bppo_status bppo_collect_rollouts(bppo_ctx *c, bppo_rollout_info *info) {
    if (!c) return BPPO_ERR_ARG;
    c->ep_entries.clear();
    // a rollout bppo_train_steps enqueued ahead (it returned an error before using it)
    // IS the next rollout: the RNG and the envs have moved past it already
    if (c->prefetched) c->prefetched = false;
    else TRY(collect_enqueue(c, info != nullptr));
    BPPO_HIP(c, sync_stream(c));
    return collect_finish(c, info, c->coll_slot);
}

// the last rollout's kept episode records in the reference's order; *cnt = the device count
bppo_status rollout_records_sorted(bppo_ctx *c, std::vector<EpisodeRec> &recs, int32_t *cnt) {
    *cnt = 0;
    BPPO_HIP(c, hipMemcpyAsync(cnt, c->d_ep_count, 4, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, sync_stream(c));
    const int m = std::min(*cnt, c->eps_cap);
    recs.resize(m);
    if (m) {
        BPPO_HIP(c, hipMemcpyAsync(recs.data(), c->d_eps, sizeof(EpisodeRec) * m, hipMemcpyDeviceToHost, c->stream));
        BPPO_HIP(c, sync_stream(c));
    }
    // reference order: by step, then env index (env.rs:470-483 collects in env order per step)
    std::sort(recs.begin(), recs.end(), [](const EpisodeRec &a, const EpisodeRec &b) {
        return a.step != b.step ? a.step < b.step : a.env_index < b.env_index; });
    return BPPO_OK;
}

// bootstrap + GAE (main.rs:877-947)
// enqueue half (the CartPole path has no host read in it)
static bppo_status gae_enqueue(bppo_ctx *c) {
    c->prefetched = false;        // a pending rollout is consumed here (e.g. after a bppo_train_steps error)
    if (c->wide) {
        TRY(tm_begin(c, TM_GAE));
        TRY(wide_bootstrap_gae(c));
        TRY(tm_end(c, TM_GAE));
        c->gae_done = 1;
        return BPPO_OK;
    }
    TRY(tm_begin(c, TM_BOOT));
    TRY(launch_bootstrap(c, nullptr, nullptr, c->cfg.normalize_obs));
    TRY(popart_denorm(c, c->d_last_v, (size_t)c->N));   // main.rs:898-907
    TRY(tm_end(c, TM_BOOT));
    TRY(tm_begin(c, TM_GAE));
    bool packed = false;
    hipError_t he = hipSuccess;
    bppo_status s = launch_gae_1p(c->d_rew, c->d_done, c->d_val, c->d_last_v, c->T, c->N,
                                  (float)c->cfg.gamma, (float)c->cfg.gae_lambda, c->d_adv, c->d_ret,
                                  c->stream, c->rows_from_rollout ? c->d_rowB : nullptr, &packed, &he);
    c->rows_packed = packed;
    if (s != BPPO_OK) return he != hipSuccess ? hip_fail(c, he, "k_gae_1p launch") : s;
    TRY(tm_end(c, TM_GAE));
    c->gae_done = 1;
    return BPPO_OK;
}

extern "C" bppo_status bppo_compute_gae(bppo_ctx *c) {
    if (!c || !c->collected) { if (c) c->err = "compute_gae before collect_rollouts"; return BPPO_ERR_ARG; }
    TRY(gae_enqueue(c));
    BPPO_HIP(c, sync_stream(c));
    if (!c->wide) tm_read(c, TM_BOOT);
    tm_read(c, TM_GAE);
    return BPPO_OK;
}

// ppo.rs:1268-1294 compute_explained_variance as the reference computes it: f32
// iterator sums in order (each chain sequential; the two independent chains of a
// round are interleaved only for instruction-level parallelism), population
// variances, no fma contraction ((r - mean).powi(2) is a multiply, then the add)
static float ev_reference_f32(const float *v, const float *r, const float *valid, size_t n_all) {
#pragma clang fp contract(off)
    size_t n_ = 0;
    float s_r = 0.0f, s_res = 0.0f;
    for (size_t i = 0; i < n_all; i++) {
        if (valid && !(valid[i] > 0.5f)) continue;     // opponent pool: learner rows (ppo.rs:2047-2056)
        s_r += r[i];
        s_res += r[i] - v[i];
        n_++;
    }
    const float n = (float)n_;
    if (n < 2.0f) return 0.0f;
    const float mr = s_r / n, mres = s_res / n;
    float q_r = 0.0f, q_res = 0.0f;
    for (size_t i = 0; i < n_all; i++) {
        if (valid && !(valid[i] > 0.5f)) continue;
        const float d = r[i] - mr;
        q_r += d * d;
        const float e = (r[i] - v[i]) - mres;
        q_res += e * e;
    }
    const float vr = q_r / n;
    if (vr < 1e-8f) return 0.0f;
    return 1.0f - (q_res / n) / vr;
}

// mode 1: copy the buffers the metric reads (stream order: after GAE, before anything
// later rewrites them) and sum them on a host thread while the update runs
static bppo_status ev_reference_begin(bppo_ctx *c, const float *d_valid) {
    const size_t TN = (size_t)c->T * c->N;
    // a thread left by an update that returned early still reads the pinned buffers
    // (or waits on ev_copied): it ends before they are refilled or the event re-recorded
    if (c->ev_thread.joinable()) c->ev_thread.join();
    BPPO_HIP(c, hipEventRecord(c->ev_gae, c->stream));
    BPPO_HIP(c, hipStreamWaitEvent(c->ev_stream, c->ev_gae, 0));
    BPPO_HIP(c, hipMemcpyAsync(c->h_ev_v, c->d_val, TN * 4, hipMemcpyDeviceToHost, c->ev_stream));
    BPPO_HIP(c, hipMemcpyAsync(c->h_ev_r, c->d_ret, TN * 4, hipMemcpyDeviceToHost, c->ev_stream));
    if (d_valid) BPPO_HIP(c, hipMemcpyAsync(c->h_ev_valid, d_valid, TN * 4, hipMemcpyDeviceToHost, c->ev_stream));
    BPPO_HIP(c, hipEventRecord(c->ev_copied, c->ev_stream));
    const bool vf = d_valid != nullptr;
    c->ev_thread = std::thread([c, TN, vf]() {
        (void)pthread_setname_np(pthread_self(), "bppo-ev");
        (void)hipEventSynchronize(c->ev_copied);
        c->ev_ref = ev_reference_f32(c->h_ev_v, c->h_ev_r, vf ? c->h_ev_valid : nullptr, TN);
    });
    return BPPO_OK;
}

// ------------------------------------------------- ppo_update (ppo.rs:1661-2112) ----
// bppo_ppo_update below is the reference's two loops; each concern around them is one
// stage here, sharing the state of the run in UpdateRun.  The stages enqueue in the
// order the loops call them: a stage boundary never reorders work on a stream.
struct UpdateRun {
    // opponent pool: train on the learner rows only (ppo.rs:1696-1720); their count
    // varies per update, so each epoch's swap targets come from the sequential
    // host walk instead of the speculating shuffle engine
    bool opp;
    // W > 1: the ranks' learner-row counts differ, so every rank runs all M minibatch slots
    // of every epoch in lockstep (one all-reduce each); a rank whose slot is empty adds a
    // zero gradient and zero metric partials (oracle/ppo.c or_trainers_update)
    bool multi;
    // without a KL early stop or a host all-reduce nothing in the loop needs the
    // metrics on the host: the minibatches are enqueued back to back and the rows
    // are read once after the last one (no per-minibatch stream drain)
    bool deferred;
    int slot;                             // the shuffle engine's job (self-play)
    size_t B;                             // rows trained on
    int M;
    size_t base_mb, rem;                  // minibatch mb has base_mb + (mb < rem) rows
    // the deferred path times the update's last minibatch that runs: sizes do not grow with
    // the slot index, so it is slot M-1 unless B < M (then rem-1; none when B == 0); lockstep
    // slots (W > 1) all run
    int last_run_mb;
    std::vector<float> rows;              // per minibatch: WM_COUNT metric sums + 4 adv stats
    int nrow = 0, epochs_run = 0;
    bool stop = false;                    // KL early stop (ppo.rs:2019-2023)
    size_t rows_done = 0;                 // rows of the KL-stopped epoch's minibatches that ran
    bool first_mb = true;                 // the update's first minibatch: the rollout's parameters
    double wait_ms = 0.0;                 // host time blocked on the permutation source
    float fw_ms = 0, sh_ms = 0;
    bool fw_recorded = false;
    std::vector<uint32_t> Jh;             // opponent pool: every epoch's swap targets (pending H2D copies)
    uint64_t opp_pos;                     // ... and the RNG position its walks have reached
};

constexpr int WM_ROW = WM_COUNT + 4;      // floats per metric row

// mode 1 copies d_val / d_ret on ev_stream beside the update: on every return while armed
// the context stream waits for those copies, so the next rollout cannot overwrite the
// buffers under them (the normal path enqueues the wait itself, update_tail)
struct EvCopyGuard {
    bppo_ctx *c; bool armed = false;
    ~EvCopyGuard() { if (armed) (void)hipStreamWaitEvent(c->stream, c->ev_copied, 0); }
};

// host time the update spends blocked in f (a host shuffle walk, a wait for the engine)
template <class F> static void timed_wait(UpdateRun &u, F &&f) {
    const auto w0 = std::chrono::steady_clock::now();
    f();
    u.wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
}

// the permutation source and the minibatch split chosen; what precedes the first epoch enqueued
static bppo_status update_begin(bppo_ctx *c, UpdateRun &u, EvCopyGuard &ev_guard) {
    u.opp = opp_active(c);
    if (u.opp) {
        // the opponent path permutes on this stream with the shared scratch, into the
        // context's own buffer, after anything still queued on fy_stream
        if (c->fy_done > 0) BPPO_HIP(c, hipStreamWaitEvent(c->stream, c->fy_ev[c->fy_done - 1], 0));
        c->fy_slot = -1; c->fy_done = 0;
        c->d_perm = c->d_perm_base;
        TRY(opp_compact_valid(c));
    }
    if (!u.opp && c->shuf_slot < 0) c->shuf_slot = c->shuf.ensure(c->rng_pos);
    u.slot = c->shuf_slot;
    u.B = u.opp ? (size_t)c->n_valid : (size_t)c->T * c->N;
    u.Jh.assign(u.opp ? std::max<size_t>(u.B, 1) * c->cfg.num_epochs : 0, 0u);
    u.opp_pos = c->rng_pos;
    u.M = c->cfg.num_minibatches;
    u.base_mb = u.B / u.M; u.rem = u.B % u.M;
    TRY(tm_begin(c, TM_UPDATE));
    if (c->ev_mode == 1) { TRY(ev_reference_begin(c, u.opp ? c->d_valid : nullptr)); ev_guard.armed = true; }
    TRY(popart_update_begin(c, u.opp ? c->d_valid : nullptr));   // ppo.rs:1787-1808
    if (c->d_rowA && !c->rows_packed) TRY(launch_pack_rows(c));
    c->rows_packed = false;
    u.multi = c->allreduce && c->world > 1;
    u.deferred = c->cfg.target_kl < 0 && !(u.multi && !c->allreduce_async);
    u.last_run_mb = (u.base_mb > 0 || u.multi) ? u.M - 1 : (int)u.rem - 1;
    return BPPO_OK;
}

// epoch ep's permutation (ppo.rs:1816) from either source: c->d_perm names it, the compute
// stream is ordered behind it, and the shuffle timer's events are recorded
static bppo_status epoch_permutation(bppo_ctx *c, UpdateRun &u, int ep) {
    const size_t B = u.B;
    if (u.opp) {
        uint32_t *J = u.Jh.data() + (size_t)ep * B;
        timed_wait(u, [&] { u.opp_pos = shuffle_walk_host(c->rng_key, c->cfg.rng_stream, u.opp_pos, (uint32_t)B, J); });
        BPPO_HIP(c, hipMemcpyAsync(c->d_Jopp, J, sizeof(uint32_t) * B, hipMemcpyHostToDevice, c->stream));
        BPPO_HIP(c, hipEventRecord(c->ev[TM_SHUFFLE][0], c->stream));
        if (B) TRY(launch_fisher_yates(c, c->d_Jopp, (uint32_t)B));
        if (B) TRY(opp_map_perm(c, (uint32_t)B));
        BPPO_HIP(c, hipEventRecord(c->ev[TM_SHUFFLE][1], c->stream));
    } else {
        if (u.slot != c->fy_slot || ep >= c->fy_done) timed_wait(u, [&] { c->shuf.wait_epoch(u.slot, ep); });
        TRY(fy_enqueue_ready(c, u.slot));          // this epoch and any other resolved since
        BPPO_HIP(c, hipStreamWaitEvent(c->stream, c->fy_ev[ep], 0));
        c->d_perm = c->d_perm_ep + (size_t)ep * B;
    }
    return BPPO_OK;
}

// one minibatch slot (ppo.rs:1831-2017): the gradient of rows [start, start + sz) of the
// epoch's permutation, the all-reduce (W > 1), clip + Adam, and its metric row
static bppo_status minibatch_slot(bppo_ctx *c, UpdateRun &u, int ep, int mb, size_t start, size_t sz, double lr,
                                  double ent_coef) {
    const int np = (int)c->net.n_params;
    // the "minibatch" phase time is the last minibatch's (read after the update in the
    // deferred path): only that one is bracketed there -- each timestamp marker on the
    // stream costs a few us of idle compute stream
    const bool fw_timed = !u.deferred || (ep == c->cfg.num_epochs - 1 && mb == u.last_run_mb);
    if (fw_timed) BPPO_HIP(c, hipEventRecord(c->ev[TM_FWDBWD][0], c->stream));
    c->d_mb_cur = c->d_mb_stats + 4 * mb;
    // Adam's bias corrections for this step (burn-optim: per tensor, f32 powers)
    float c1[64], c2[64];
    for (int t = 0; t < 2 * c->net.n_layers; t++) {
        int ti = ++c->adam_t[t];
        adam_bias_corrections(ti, &c1[t], &c2[t]);
    }
    float *metric_dst = c->d_rows + (size_t)u.nrow * WM_ROW;
    if (sz && c->dbg_params && u.nrow < c->dbg_params_max)   // parity hook: this minibatch's parameters
        BPPO_HIP(c, hipMemcpyAsync(c->dbg_params + (size_t)u.nrow * np, c->d_params, sizeof(float) * np,
                                   hipMemcpyDeviceToHost, c->stream));
    if (sz == 0) {                 // lockstep slot without rows on this rank
        BPPO_HIP(c, hipMemsetAsync(c->d_grad, 0, sizeof(float) * ((size_t)np + 64), c->stream));   // + tail
        BPPO_HIP(c, hipMemsetAsync(c->d_mb_cur, 0, sizeof(float) * 4, c->stream));
        // value_error_max of no rows: -inf, as the oracle's (the metric row reads the
        // rank-local copy; the summed slot GRAD_VEMAX is not read)
        static const float ninf = -INFINITY;
        BPPO_HIP(c, hipMemcpyAsync(c->d_grad + np + GRAD_VEMAX_LOCAL, &ninf, sizeof(float),
                                   hipMemcpyHostToDevice, c->stream));
    } else if (c->wide) {
        TRY(wide_minibatch(c, (uint32_t)start, (uint32_t)sz, ent_coef, u.first_mb));
    } else {
        TRY(launch_minibatch(c, (uint32_t)start, (uint32_t)sz, (float)ent_coef, u.first_mb));
    }
    if (fw_timed) { BPPO_HIP(c, hipEventRecord(c->ev[TM_FWDBWD][1], c->stream)); u.fw_recorded = true; }
    u.first_mb = false;
    if (u.multi) {
        if (!c->allreduce_async) BPPO_HIP(c, sync_stream(c));
        if (c->allreduce(c->d_grad, (size_t)np + WM_COUNT, c->allreduce_user) != 0) {
            c->err = "all-reduce callback failed";
            return BPPO_ERR_COMM;
        }
    }
    // clip + Adam; the metric row (grad[np .. np+WM_COUNT) and adv stats) into the
    // update's device rows
    TRY(launch_adam(c, (float)lr, c1, c2, metric_dst, WM_COUNT));
    if (c->wide) TRY(wide_pack(c));
    u.nrow++;
    return BPPO_OK;
}

// the immediate row policy (a KL early stop, or a host all-reduce that drains the stream
// anyway): the minibatch's row and timers are read at once, and the KL test on the row
// ends the update after a minibatch that covered the epoch's rows up to `end`
static bppo_status read_row_now(bppo_ctx *c, UpdateRun &u, int mb, size_t end) {
    float row[WM_ROW];
    BPPO_HIP(c, hipMemcpyAsync(row, c->d_rows + (size_t)(u.nrow - 1) * WM_ROW, sizeof row, hipMemcpyDeviceToHost,
                               c->stream));
    BPPO_HIP(c, sync_stream(c));
    float ms = 0;
    if (event_ms(c->ev[TM_FWDBWD][0], c->ev[TM_FWDBWD][1], &ms)) u.fw_ms = ms;
    if (mb == 0 && event_ms(c->ev[TM_SHUFFLE][0], c->ev[TM_SHUFFLE][1], &ms)) u.sh_ms = ms;
    u.rows.insert(u.rows.end(), row, row + WM_ROW);
    if (c->cfg.target_kl >= 0) {
        const float n = row[WM_N] > 0 ? row[WM_N] : 1.0f;
        if (row[WM_KL] / n > (float)c->cfg.target_kl) { u.stop = true; u.rows_done = end; }   // ppo.rs:2019-2023
    }
    return BPPO_OK;
}

// the deferred row policy: one copy of all rows enqueued behind the last minibatch ...
static bppo_status deferred_rows_enqueue(bppo_ctx *c, UpdateRun &u) {
    if (!u.deferred || u.nrow == 0) return BPPO_OK;
    u.rows.resize((size_t)u.nrow * WM_ROW);
    // into pinned memory: a pageable destination makes the copy synchronous and the
    // host thread spins in it for the whole update (a CPU the shuffle walkers need);
    // read after the one stream wait of update_tail, behind the explained-variance pass
    BPPO_HIP(c, hipMemcpyAsync(c->h_rows, c->d_rows, sizeof(float) * u.rows.size(), hipMemcpyDeviceToHost, c->stream));
    return BPPO_OK;
}
// ... and read, with the two timers, after the update's stream wait
static void deferred_rows_read(bppo_ctx *c, UpdateRun &u) {
    if (!u.deferred || u.nrow == 0) return;
    std::memcpy(u.rows.data(), c->h_rows, sizeof(float) * u.rows.size());
    float ms = 0;
    if (u.fw_recorded && event_ms(c->ev[TM_FWDBWD][0], c->ev[TM_FWDBWD][1], &ms)) u.fw_ms = ms;   // else 0
    if (event_ms(c->ev[TM_SHUFFLE][0], c->ev[TM_SHUFFLE][1], &ms)) u.sh_ms = ms;
}

// the permutation source wound up: the RNG position after the epochs that started, the
// engine's walk statistics, its slot released and the next update's job chained
static bppo_status shuffle_wrapup(bppo_ctx *c, UpdateRun &u) {
    c->last_wait_ms = u.wait_ms;
    c->last_walk_ms = 0.0;
    c->last_met = 0;
    if (u.opp) {
        c->rng_pos = u.opp_pos;                             // the epochs walked (early stop: started ones)
        c->last_walk_ms = u.wait_ms;
        BPPO_HIP(c, hipStreamSynchronize(c->stream));      // Jh's copies done
    } else {
        const int slot = u.slot;
        // only started epochs consumed words (reference); windowed: the update's fixed span
        c->rng_pos = c->shuf.win ? c->shuf.job_end(slot) : c->shuf.end_pos[slot][u.epochs_run - 1];
        for (int e = 0; e < u.epochs_run; e++) {
            c->last_walk_ms += c->shuf.walk_ms[slot][e];
            c->last_met += c->shuf.coalesced[slot][e] >= 0 && e > 0;
        }
        c->last_spec_mwords = (double)c->shuf.spec_words.exchange(0) * 1e-6;
        c->last_true_mwords = (double)c->shuf.true_words.exchange(0) * 1e-6;
        c->last_walk_cpu_ms = (double)c->shuf.tsc_walk.exchange(0) / tsc_per_ms();
        c->last_words_cpu_ms = (double)c->shuf.tsc_words.exchange(0) / tsc_per_ms();
        c->shuf_slot = -1;
        // this update's reads of the J slot are enqueued (fy_stream's too: epochs
        // permuted ahead but not run after a KL early stop); the next update's
        // shuffles begin after its rollout's T*N*A Gumbel words (usually chained already)
        if (c->fy_slot == slot && c->fy_done > 0)
            BPPO_HIP(c, hipStreamWaitEvent(c->stream, c->fy_ev[c->fy_done - 1], 0));
        c->fy_slot = -1;
        c->fy_done = 0;
        BPPO_HIP(c, c->shuf.release(slot, c->stream));
        c->shuf.ensure(c->rng_pos + (uint64_t)c->T * c->N * (uint64_t)c->A);
    }
    return BPPO_OK;
}

// the update's last enqueues and its one stream wait
static bppo_status update_tail(bppo_ctx *c, UpdateRun &u, EvCopyGuard &ev_guard) {
    TRY(popart_target_stats(c, u.stop ? u.epochs_run - 1 : u.epochs_run, u.rows_done, u.opp ? c->d_valid : nullptr));
    TRY(launch_explained_variance(c, u.opp ? c->d_valid : nullptr));
    // mode 1: nothing after this update (the next rollout) overwrites the copied buffers early
    if (ev_guard.armed) { ev_guard.armed = false; BPPO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_copied, 0)); }
    BPPO_HIP(c, hipEventRecord(c->ev_upd, c->stream));      // end of this update's work
    if (c->prefetch_next) {
        // bppo_train_steps: the next rollout goes in behind this update (it needs only the
        // updated parameters and the RNG position after this update's shuffles, both in
        // stream / host order now); the host then waits for this update alone
        c->prefetch_next = false;
        c->env_step = c->prefetch_env_step;
        TRY(collect_enqueue(c, true));
        c->prefetched = true;
        BPPO_HIP(c, wait_event(c, c->ev_upd));
    } else {
        BPPO_HIP(c, sync_stream(c));
    }
    return BPPO_OK;
}

// every minibatch kernel launch of this update (BPPO_MB_EVENTS): mean / min / max, per kernel
static void fold_launch_timers(bppo_ctx *c) {
    if (c->mb_ev_n > 0) {
        double sum = 0.0, ks[2] = {0.0, 0.0};
        float lo = INFINITY, hi = 0.0f;
        int n = 0, kn[2] = {0, 0};
        for (int i = 0; i < c->mb_ev_n; i++) {
            float ms = 0.0f;
            if (!event_ms(c->mb_ev[i][0], c->mb_ev[i][1], &ms)) continue;
            sum += ms; lo = std::min(lo, ms); hi = std::max(hi, ms); n++;
            ks[c->mb_ev_split[i]] += ms; kn[c->mb_ev_split[i]]++;
        }
        if (n) { c->mb_k_mean = (float)(sum / n); c->mb_k_min = lo; c->mb_k_max = hi; }
        c->mb_k_exact = kn[0] ? (float)(ks[0] / kn[0]) : 0.0f;
        c->mb_k_split = kn[1] ? (float)(ks[1] / kn[1]) : 0.0f;
        c->mb_ev_n = 0;
    }
    c->mb_launch = 0;
}

// ppo_update (ppo.rs:1661-2112)
extern "C" bppo_status bppo_ppo_update(bppo_ctx *c, double lr, double ent_coef, bppo_update_metrics *m) {
    if (!c || !c->gae_done) { if (c) c->err = "ppo_update before compute_gae"; return BPPO_ERR_ARG; }
    UpdateRun u;
    EvCopyGuard ev_guard{c};              // armed by update_begin, handed over in update_tail
    TRY(update_begin(c, u, ev_guard));
    for (int ep = 0; ep < c->cfg.num_epochs && !u.stop; ep++) {          // ppo.rs:1811
        u.epochs_run++;
        TRY(epoch_permutation(c, u, ep));
        // no learner rows (opponent pool): the reference shuffles an empty index
        // list (no RNG words) and skips every minibatch (ppo.rs:1815-1831); lockstep
        // ranks (W > 1) run their empty slots all the same
        if (u.B == 0 && !u.multi) continue;
        if (u.B) TRY(launch_epoch_adv_stats(c, (uint32_t)u.B, u.M, u.opp ? nullptr : c->d_inv_ep + (size_t)ep * u.B));
        size_t start = 0;
        for (int mb = 0; mb < u.M; mb++) {                               // ppo.rs:1831
            const size_t sz = u.base_mb + ((size_t)mb < u.rem ? 1 : 0);
            if (sz == 0 && !u.multi) continue;
            TRY(minibatch_slot(c, u, ep, mb, start, sz, lr, ent_coef));
            if (!u.deferred) TRY(read_row_now(c, u, mb, start + sz));
            if (u.stop) break;
            start += sz;
        }
    }
    TRY(deferred_rows_enqueue(c, u));
    TRY(tm_end(c, TM_UPDATE));
    TRY(shuffle_wrapup(c, u));
    TRY(update_tail(c, u, ev_guard));
    deferred_rows_read(c, u);
    FoldArgs fa{};
    explained_variance_sums(c, fa.ev4);
    if (c->ev_thread.joinable()) c->ev_thread.join();     // mode 1: the reference's f32 sums
    tm_read(c, TM_UPDATE);
    fold_launch_timers(c);
    c->last_ms[TM_FWDBWD] = u.fw_ms;
    c->last_ms[TM_SHUFFLE] = u.sh_ms;
    c->last_rows = u.rows;
    if (m) {
        fa.value_coef = (float)c->cfg.value_coef; fa.ent_coef = (float)ent_coef;
        fa.A = c->A; fa.env_kind = c->cfg.env_kind; fa.B = u.B;
        fa.ev_mode = c->ev_mode; fa.ev_ref = c->ev_ref; fa.epochs_run = u.epochs_run;
        fa.normalize_values = c->cfg.normalize_values != 0;
        fa.pa_tsum = c->pa_tsum; fa.pa_tsq = c->pa_tsq; fa.pa_tcount = c->pa_tcount;
        fa.pa_rescale_mag = c->pa_rescale_mag;
        fold_update_metrics(u.rows.data(), (int)(u.rows.size() / WM_ROW), fa, m);
    }
    c->collected = 0; c->gae_done = 0;
    return BPPO_OK;
}

// bppo_train_steps' additions to an iteration: the env step its rollout runs at, and
// whether (and at which env step) the next iteration's rollout is enqueued behind the update
struct Pipeline { uint64_t env_step; bool prefetch_next; uint64_t next_env_step; };

// One iteration of main.rs:860-947 + ppo_update: the rollout, the
// bootstrap/GAE and the update are enqueued back to back with no host wait
// between them (bppo_collect_rollouts and bppo_compute_gae each drain the stream
// for their results).  The rollout's device error flags are read after the update:
// a non-finite log-prob or an empty mask returns its status then, with the update
// already applied (the reference panics before updating; either way the run ends).
// The two entry points differ in three arguments.  summary: the rollout's episode summary
// is asked for.  pipe (bppo_train_steps only): see Pipeline.  update_first: a failed update
// returns its status at once; on any failure the stream is drained so nothing is pending on
// return, and a rollout already enqueued ahead (ppo_update enqueues it before its wait)
// stays the context's next one (prefetched), which bppo_collect_rollouts /
// bppo_train_step(s) then use instead of drawing another.  Without it (bppo_train_step)
// the rollout's flags are read even after a failed update, and its status wins.
static bppo_status train_iteration(bppo_ctx *c, double lr, double ent_coef, bppo_rollout_info *info,
                                   bppo_update_metrics *m, bool summary, const Pipeline *pipe, bool update_first) {
    const auto t0 = std::chrono::steady_clock::now();
    c->sync_wait_ms = 0.0;
    if (!pipe) c->ep_entries.clear();     // a call of its own (bppo_train_steps clears once for its n)
    // a rollout enqueued ahead by bppo_train_steps IS this iteration's (see bppo_collect_rollouts)
    if (!c->prefetched) {
        if (pipe) c->env_step = pipe->env_step;
        TRY(collect_enqueue(c, summary));
    }
    c->prefetched = false;
    const int slot = c->coll_slot;
    TRY(gae_enqueue(c));
    if (pipe) { c->prefetch_next = pipe->prefetch_next; c->prefetch_env_step = pipe->next_env_step; }
    const bppo_status us = bppo_ppo_update(c, lr, ent_coef, m);   // drains the stream at its end
    if (pipe) c->prefetch_next = false;
    if (us != BPPO_OK && update_first) { (void)sync_stream(c); c->collected = c->prefetched ? 1 : 0; return us; }
    if (us == BPPO_OK) { if (!c->wide) tm_read(c, TM_BOOT); tm_read(c, TM_GAE); }
    const bppo_status cs = collect_finish(c, info, slot);
    if (cs != BPPO_OK && update_first) { (void)sync_stream(c); c->collected = c->prefetched ? 1 : 0; return cs; }
    // host time in the call outside stream waits: enqueue work + engine waits
    c->last_host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() -
                      c->sync_wait_ms;
    c->last_sync_ms = c->sync_wait_ms;
    return cs != BPPO_OK ? cs : us;
}

extern "C" bppo_status bppo_train_step(bppo_ctx *c, double lr, double ent_coef, bppo_rollout_info *info,
                                       bppo_update_metrics *m) {
    if (!c) return BPPO_ERR_ARG;
    return train_iteration(c, lr, ent_coef, info, m, info != nullptr, nullptr, false);
}

// n iterations of bppo_train_step in one call, software-pipelined: each update's
// last stream wait covers that update only, with the next iteration's rollout
// already enqueued behind it, so the GPU never idles between iterations (the
// host tail of one update, the caller and the next enqueue ran in that gap).
// Results are those of n sequential bppo_train_step calls with lr[k], ent[k] and
// the env step global_step0 + k*T*N; nothing is left pending when it returns.
// phase_keys/phase_sums (optional): bppo_last_kernel_ms of each key summed over the n.
extern "C" bppo_status bppo_train_steps(bppo_ctx *c, int32_t n, const double *lr, const double *ent_coef,
                                        uint64_t global_step0, bppo_rollout_info *infos, bppo_update_metrics *ms,
                                        const char *const *phase_keys, int32_t nkeys, float *phase_sums) {
    if (!c || n < 0 || !lr || !ent_coef || (nkeys > 0 && (!phase_keys || !phase_sums))) return BPPO_ERR_ARG;
    for (int k = 0; k < nkeys; k++) phase_sums[k] = 0.0f;
    c->ep_entries.clear();
    const uint64_t TN = (uint64_t)c->T * c->N * (uint64_t)c->world;   // the job's env steps per iteration
    for (int32_t k = 0; k < n; k++) {
        const Pipeline pipe{global_step0 + (uint64_t)k * TN, k + 1 < n, global_step0 + (uint64_t)(k + 1) * TN};
        TRY(train_iteration(c, lr[k], ent_coef[k], infos ? &infos[k] : nullptr, ms ? &ms[k] : nullptr, true, &pipe, true));
        for (int q = 0; q < nkeys; q++) {
            float v = 0.0f;
            if (bppo_last_kernel_ms(c, phase_keys[q], &v) == BPPO_OK) phase_sums[q] += v;
        }
    }
    return BPPO_OK;
}
