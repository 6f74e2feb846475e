// bppo_api.hip — the C-ABI (include/bppo.h): context lifecycle, state getters and
// setters, buffer access, parity hooks.  The training loop (collect_rollouts ->
// bootstrap + GAE -> ppo_update, bppo_train_step(s)) is train_loop.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <sys/prctl.h>
#include "bppo_internal.h"
#include "shuffle_host.h"
#include "bppo_wide.h"
#include "bppo_update_metrics.h"

using namespace bppo;

namespace bppo {

NetLayout make_layout(const bppo_config &c, int obs_dim, int priv_dim, int act_dim) {
    NetLayout L;
    // split_networks (mlp.rs:100-130): a second trunk of num_hidden x hidden_size on obs,
    // i.e. the CTDE structure with no privileged input (ctde.rs ignores the flag)
    const bool split = c.split_networks && !c.ctde;
    L.ctde = c.ctde || split; L.relu = c.relu;
    auto add = [&](int in, int out) {
        int i = L.n_layers++;
        L.in[i] = in; L.out[i] = out;
        return i;
    };
    int in = obs_dim;
    if (c.cnn) {
        // cnn.rs:66-150: conv stack on the (H, W, C) spatial part, FC layers on
        // [flattened conv output | extra features], heads of cnn_fc_hidden_size
        L.H = 6; L.W = 7; L.C = 2;                     // connect_four.rs:217 OBSERVATION_SHAPE
        L.E = obs_dim - L.H * L.W * L.C;
        L.ksize = c.kernel_size;
        int cin = L.C;
        for (int l = 0; l < c.num_conv_layers; l++) {
            const int co = c.conv_channels[l < 4 ? l : 3];
            L.conv_cin[l] = cin;
            add(cin * L.ksize * L.ksize, co);
            cin = co;
        }
        L.n_conv = c.num_conv_layers;
        L.fdim = L.H * L.W * cin + L.E;
        in = L.fdim;
        for (int l = 0; l < c.cnn_num_fc_layers; l++) { add(in, c.cnn_fc_hidden_size); in = c.cnn_fc_hidden_size; }
        L.n_actor_hidden = L.n_conv + c.cnn_num_fc_layers;
    } else {
        for (int l = 0; l < c.num_hidden; l++) { add(in, c.hidden_size); in = c.hidden_size; }
        L.n_actor_hidden = c.num_hidden;
    }
    L.policy = add(in, act_dim);
    if (L.ctde && c.cnn) {
        // split CNN (cnn.rs:116-135): the critic's own conv stack (same shapes) and FC layers
        L.critic_first = L.n_layers;
        for (int l = 0; l < L.n_conv; l++) add(L.in[l], L.out[l]);
        L.critic_fc0 = L.n_layers;
        int cin = L.fdim;
        for (int l = 0; l < c.cnn_num_fc_layers; l++) { add(cin, c.cnn_fc_hidden_size); cin = c.cnn_fc_hidden_size; }
        L.value = add(cin, 1);
    } else if (L.ctde) {
        int cin = split ? obs_dim : priv_dim + obs_dim;
        const int nc = split ? c.num_hidden : c.critic_num_hidden, wc = split ? c.hidden_size : c.critic_hidden_size;
        L.critic_first = L.critic_fc0 = L.n_layers;
        for (int l = 0; l < nc; l++) { add(cin, wc); cin = wc; }
        L.value = add(cin, 1);
    } else {
        L.value = add(in, 1);
    }
    // offsets in Burn record order: the layer order above, except split_networks'
    // record (mlp.rs:47-62) puts the critic layers before the policy head
    int order[16], no = 0;
    for (int l = 0; l < L.n_layers; l++)
        if (!split || l < L.n_actor_hidden || (l >= L.critic_first && l < L.value)) order[no++] = l;
    if (split) { order[no++] = L.policy; order[no++] = L.value; }
    size_t off = 0;
    for (int r = 0; r < L.n_layers; r++) {
        const int l = order[r];
        L.rec[l] = r;
        L.w[l] = off; off += (size_t)L.in[l] * L.out[l];
        L.b[l] = off; off += L.out[l];
    }
    L.n_params = off;
    return L;
}

// ----------------------------------------------------------- libm check ----
__global__ void k_libm(int which, const float *x, float *y, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = x[i];
    switch (which) {
    case 0: y[i] = bppo_math::logf_glibc(v); break;
    case 1: y[i] = bppo_math::sinf_glibc(v); break;
    case 2: y[i] = bppo_math::cosf_glibc(v); break;
    case 3: y[i] = -bppo_math::logf_glibc(-bppo_math::logf_glibc(v)); break;
    case 5: y[i] = bppo_math::tanhf_glibc_bf(v); break;   // the form the MLP kernels use
    default: y[i] = bppo_math::expf_glibc(v); break;
    }
}

bppo_status launch_libm(int which, const float *d_x, float *d_y, size_t n) {
    hipLaunchKernelGGL(k_libm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, which, d_x, d_y, n);
    return hipGetLastError() == hipSuccess ? BPPO_OK : BPPO_ERR_HIP;
}

}  // namespace bppo

// ======================================================================= ABI
extern "C" size_t bppo_config_size(void) { return sizeof(bppo_config); }
extern "C" size_t bppo_update_metrics_size(void) { return sizeof(bppo_update_metrics); }
extern "C" size_t bppo_episode_size(void) { return sizeof(bppo_episode); }
extern "C" size_t bppo_rollout_info_size(void) { return sizeof(bppo_rollout_info); }

extern "C" const char *bppo_version(void) { return "bppo-mi355x 0.1 (gfx950)"; }

extern "C" const char *bppo_last_error(const bppo_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

// wait for the context stream on a blocking-sync event: the host thread sleeps
// instead of polling (polling eats the CPU quota the shuffle walkers run on)
// (hipEventSynchronize on a blocking-sync event still spun here: measured ~1 CPU per
// process for the whole update; a sleeping poll at 20 us with 1 us timer slack frees it)
hipError_t sync_stream(bppo_ctx *c) {   // (also train_loop.hip)
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e;
    if (!c->ev_block) e = hipStreamSynchronize(c->stream);
    else {
        static thread_local bool slack = false;
        if (!slack) { (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0); slack = true; }
        e = hipEventRecord(c->ev_block, c->stream);
        while (e == hipSuccess && (e = event_query(c->ev_block)) == hipErrorNotReady) {
            std::this_thread::sleep_for(std::chrono::microseconds(20));
            e = hipSuccess;
        }
    }
    c->sync_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return e;
}

static bool cartpole_fused_net(const bppo_config &c) {
    return !c.split_networks && !c.cnn && !c.ctde && (c.hidden_size == 16 || c.hidden_size == 32 || c.hidden_size == 64) &&
           (c.num_hidden == 1 || c.num_hidden == 2);
}

static bppo_status ctx_init(bppo_ctx *c, const bppo_config *cfg, int dev, void *stream) {
    c->cfg = *cfg;
    c->dev = dev;
    // the configuration is validated before the first HIP call
    if (cfg->num_envs <= 0 || cfg->num_steps <= 0 || cfg->num_epochs <= 0 || cfg->num_minibatches <= 0) {
        c->err = "num_envs, num_steps, num_epochs, num_minibatches must be positive";
        return BPPO_ERR_ARG;
    }
    c->N = cfg->num_envs; c->T = cfg->num_steps;
    switch (cfg->env_kind) {
    case BPPO_ENV_CARTPOLE: c->D = 5; c->A = 2; c->P = 1; c->G = 0; break;
    case BPPO_ENV_CONNECT_FOUR: c->D = 86; c->A = 7; c->P = 2; c->G = 0; break;
    case BPPO_ENV_LIARS_DICE: c->D = 270; c->A = 49; c->P = 4; c->G = cfg->ctde ? 120 : 0; break;
    case BPPO_ENV_SKULL: c->D = 135; c->A = 33; c->P = 6; c->G = cfg->ctde ? 200 : 0; break;   // skull.rs:1046-1060
    default: c->err = "unknown env_kind"; return BPPO_ERR_ARG;
    }
    c->Pa = c->P;
    if (cfg->env_kind == BPPO_ENV_SKULL) {
        c->Pa = cfg->player_count ? cfg->player_count : 4;          // PlayerCountMode::default (config.rs:667-671)
        if (c->Pa < 2 || c->Pa > 6) { c->err = "Skull supports 2-6 players"; return BPPO_ERR_ARG; }   // skull.rs:159-162
    }
    // the fused CartPole kernels (k_rollout.hip, k_update.hip) cover the shared-trunk
    // MLPs of {16, 32, 64} x {1, 2}; every other CartPole net (mlp.rs:76-132 accepts any
    // width and depth; split_networks) runs on the GEMM engine path like the other envs
    c->wide = cfg->env_kind != BPPO_ENV_CARTPOLE || !cartpole_fused_net(*cfg);
    if (c->wide && !cfg->ctde) c->G = 0;
    // num_hidden = 0 would feed obs into heads of hidden_size inputs (mlp.rs:121-125), a
    // shape panic in the reference unless obs_dim == hidden_size
    if (!cfg->cnn && (cfg->hidden_size < 1 || cfg->num_hidden < 1 ||
                      (cfg->ctde && (cfg->critic_hidden_size < 1 || cfg->critic_num_hidden < 1)))) {
        c->err = "hidden_size / num_hidden (critic_*) must be positive";
        return BPPO_ERR_ARG;
    }
    if (!(cfg->reward_shaping_coef >= 0.0)) { c->err = "reward_shaping_coef must be >= 0"; return BPPO_ERR_ARG; }   // config.rs:1514-1519
    if (cfg->cnn) {
        // cnn.rs:73-74 "CNN requires OBSERVATION_SHAPE" (only Connect Four has one)
        if (cfg->env_kind != BPPO_ENV_CONNECT_FOUR || cfg->ctde) { c->err = "CNN requires OBSERVATION_SHAPE (Connect Four)"; return BPPO_ERR_ARG; }
        if (cfg->num_conv_layers < 1 || cfg->num_conv_layers > 4 || cfg->kernel_size < 1 || cfg->kernel_size > 7 ||
            !(cfg->kernel_size & 1) || cfg->cnn_num_fc_layers < 1 || cfg->cnn_fc_hidden_size < 1) {
            c->err = "CNN: 1-4 conv layers, odd kernel_size <= 7 (same padding), >= 1 FC layer";
            return BPPO_ERR_UNSUPPORTED;
        }
        for (int l = 0; l < cfg->num_conv_layers; l++)
            if (cfg->conv_channels[l < 4 ? l : 3] < 1) { c->err = "conv_channels must be positive"; return BPPO_ERR_ARG; }
    }
    // NetLayout holds at most 16 layers (its per-layer tables, Adam's 32 tensors):
    // MLP (split_networks doubles the trunk), CTDE actor + critic, CNN conv + FC stacks
    {
        const int split = cfg->split_networks && !cfg->ctde ? 2 : 1;
        const int layers = cfg->cnn ? split * (cfg->num_conv_layers + cfg->cnn_num_fc_layers) + 2
                         : cfg->ctde ? cfg->num_hidden + cfg->critic_num_hidden + 2
                                     : split * cfg->num_hidden + 2;
        if (layers > NetLayout::MAX_LAYERS) {
            c->err = "network: at most 16 layers in all (hidden / conv / FC layers + heads)";
            return BPPO_ERR_UNSUPPORTED;
        }
    }
    BPPO_HIP(c, hipSetDevice(dev));
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        // the hot path's stream at the highest priority: the shuffle engine's copy-stream
        // kernels (J expansion) only take CUs the update kernels leave free
        int lo = 0, hi = 0;
        BPPO_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
        BPPO_HIP(c, hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
        c->own_stream = true;
    }
    c->net = make_layout(*cfg, c->D, c->G, c->A);
    const size_t np = c->net.n_params;
    const size_t TN = (size_t)c->T * c->N;
    c->adam_t.assign(2 * c->net.n_layers, 0);
    BPPO_HIP(c, c->zalloc(&c->d_params, np));
    BPPO_HIP(c, c->zalloc(&c->d_m1, np));
    BPPO_HIP(c, c->zalloc(&c->d_m2, np));
    BPPO_HIP(c, c->zalloc(&c->d_grad, np + 64));
    c->slab_rows = 256 * 8;   // one 8-wave (MFMA) or 4-wave block per CU, persistent over the minibatch
    c->relu_mfma = cfg->relu ? 1 : 0;
    if (!c->wide) BPPO_HIP(c, c->zalloc(&c->d_slab, c->slab_rows * (np + 64)));
    BPPO_HIP(c, c->zalloc(&c->d_cp, (size_t)4 * c->N));
    BPPO_HIP(c, c->zalloc(&c->d_steps, (size_t)c->N));
    BPPO_HIP(c, c->zalloc(&c->d_env_pos, (size_t)c->N));
    BPPO_HIP(c, c->zalloc(&c->d_ep_ret, (size_t)c->N * c->P));
    BPPO_HIP(c, c->zalloc(&c->d_ep_len, (size_t)c->N));
    if (!c->wide) BPPO_HIP(c, c->zalloc(&c->d_obs, TN * c->D));
    BPPO_HIP(c, c->zalloc(&c->d_rew, TN));
    BPPO_HIP(c, c->zalloc(&c->d_rew_raw, TN));
    BPPO_HIP(c, c->zalloc(&c->d_done, TN));
    BPPO_HIP(c, c->zalloc(&c->d_val, TN));
    BPPO_HIP(c, c->zalloc(&c->d_logp, TN));
    BPPO_HIP(c, c->zalloc(&c->d_adv, TN));
    BPPO_HIP(c, c->zalloc(&c->d_ret, TN));
    BPPO_HIP(c, c->zalloc(&c->d_act, TN));
    if (!c->wide || cfg->normalize_returns) BPPO_HIP(c, c->zalloc(&c->d_X, TN));
    if (!c->wide && cfg->hidden_size == 64 && cfg->num_hidden == 2 && cfg->relu)
    {
        BPPO_HIP(c, c->zalloc(&c->d_gumbel, TN * 2));
        BPPO_HIP(c, c->zalloc(&c->d_rpool, (size_t)RPOOL_K * c->N));
        BPPO_HIP(c, c->zalloc(&c->d_rpos, (size_t)RPOOL_K * c->N));
    }
    BPPO_HIP(c, c->zalloc(&c->d_on, (size_t)2 * c->D + 1));
    if (!c->wide) BPPO_HIP(c, c->zalloc(&c->d_obs_part, (size_t)c->N * 2 * c->D));
    if (!c->wide) {   // VecEnv::step / get_observations scratch (wide_init's otherwise)
        BPPO_HIP(c, c->zalloc(&c->d_act_in, (size_t)c->N));
        BPPO_HIP(c, c->zalloc(&c->d_scr_r, (size_t)c->N));
        BPPO_HIP(c, c->zalloc(&c->d_bxc, (size_t)c->N * c->D));
        BPPO_HIP(c, c->mem.alloc(&c->d_scr_d, (size_t)c->N));
    }
    BPPO_HIP(c, c->zalloc(&c->d_rn_returns, (size_t)c->N * c->P));
    BPPO_HIP(c, c->zalloc(&c->d_rn_stats, 4));
    BPPO_HIP(c, c->zalloc(&c->d_scan_agg, (TN + 4095) / 4096 + 1));
    BPPO_HIP(c, c->zalloc(&c->d_last_v, (size_t)c->N));
    // room for every episode a rollout can complete (one per env-step): the episode
    // summary then sums all of them (a smaller cap kept whichever episodes claimed
    // slots first); CartPole's integer returns sum exactly in f64, so its mean does not
    // depend on the order the waves claimed their record slots
    c->eps_cap = (int)std::min<size_t>((size_t)c->T * c->N + 4096, (size_t)INT32_MAX / 2);
    BPPO_HIP(c, c->zalloc(&c->d_eps, (size_t)c->eps_cap));
    BPPO_HIP(c, c->zalloc(&c->d_ep_count, 1));
    BPPO_HIP(c, c->zalloc(&c->d_ep_sum, ROLL_HOST_WORDS));   // [count, err] + the partial sums: one host slot's layout
    BPPO_HIP(c, c->zalloc(&c->d_err, 1));
    BPPO_HIP(c, c->zalloc(&c->d_perm_base, TN));
    c->d_perm = c->d_perm_base;
    BPPO_HIP(c, c->zalloc(&c->d_perm_ep, TN * (size_t)cfg->num_epochs));
    BPPO_HIP(c, c->zalloc(&c->d_inv_ep, TN * (size_t)cfg->num_epochs));
    BPPO_HIP(c, c->zalloc(&c->d_advpart, (size_t)ADV_STREAM_BLOCKS * ADV_STREAM_MAXM * 4));
    // the context's only streams are the update stream, fy_stream and the engine's copy
    // stream: a third low-priority stream, even idle, made every device-bound run
    // 15-25 % slower outside the minibatch kernels (profiles/r06y/, r06z/)
    BPPO_HIP(c, make_side_stream(dev, &c->fy_stream));
    for (int e = 0; e < cfg->num_epochs && e < SHUF_MAX_EPOCHS; e++)
        BPPO_HIP(c, hipEventCreateWithFlags(&c->fy_ev[e], hipEventDisableTiming));
    BPPO_HIP(c, c->zalloc(&c->d_fy, 4 * TN));
    BPPO_HIP(c, c->zalloc(&c->d_scan, TN / 8192 + 2));
    BPPO_HIP(c, fy_ranges_init(c->mem, c->fyr, (uint32_t)TN));
    BPPO_HIP(c, c->zalloc(&c->d_red, RED_SCRATCH_DOUBLES));
    BPPO_HIP(c, c->zalloc(&c->d_mb_stats, (size_t)4 * std::max(cfg->num_minibatches, 2)));
    c->d_mb_cur = c->d_mb_stats;
    BPPO_HIP(c, c->zalloc(&c->d_rows, (size_t)cfg->num_epochs * cfg->num_minibatches * (WM_COUNT + 4)));
    BPPO_HIP(c, c->mem.alloc_pinned(&c->h_rows, (size_t)cfg->num_epochs * cfg->num_minibatches * (WM_COUNT + 4)));
    if (!c->wide && cfg->hidden_size == 64 && cfg->num_hidden == 2 && cfg->relu && c->D == 5)
    {
        BPPO_HIP(c, c->mem.alloc(&c->d_rowA, 2 * TN));
        BPPO_HIP(c, c->mem.alloc(&c->d_rowB, TN));
    }
    // + two slots of the rollout's flags and episode partials
    BPPO_HIP(c, c->mem.alloc_pinned(&c->h_red, (size_t)4 * 1024 + 64 + 2 * ROLL_HOST_WORDS));
    BPPO_HIP(c, hipEventCreateWithFlags(&c->ev_upd, hipEventDisableTiming));
    BPPO_HIP(c, hipEventRecord(c->ev_upd, c->stream));      // recorded once, so every wait on it is defined
    BPPO_HIP(c, hipEventCreateWithFlags(&c->ev_block, hipEventDisableTiming | hipEventBlockingSync));
    for (int i = 0; i < TM_SLOTS; i++) {
        BPPO_HIP(c, hipEventCreate(&c->ev[i][0]));
        BPPO_HIP(c, hipEventCreate(&c->ev[i][1]));
    }
    for (int i = 0; i < bppo_ctx::MB_EV; i++) {
        BPPO_HIP(c, hipEventCreate(&c->mb_ev[i][0]));
        BPPO_HIP(c, hipEventCreate(&c->mb_ev[i][1]));
    }
    c->rng_key = seed_key(cfg->seed);
    c->rng_pos = 0;
    TRY(c->shuf.init(dev, c->rng_key, cfg->rng_stream, (uint32_t)TN, cfg->num_epochs, TN * (uint64_t)c->A, c->err,
                     cfg->shuffle_windows != 0));
    c->on_mean.assign(c->D, 0.0); c->on_m2.assign(c->D, 0.0); c->on_count = 0;
    c->u_ret = c->d_ret; c->u_val = c->d_val;
    c->shaping_v.assign(1, cfg->reward_shaping_coef); c->shaping_s.assign(1, 0);   // Schedule::constant
    if (cfg->normalize_values) TRY(popart_alloc(c));
    if (c->wide) {
        TRY(wide_init(c));
        TRY(wide_reset(c));
        TRY(wide_pack(c));
    } else {
        TRY(launch_cartpole_reset(c));
    }
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" bppo_status bppo_create(const bppo_config *cfg, int hip_device, void *hip_stream,
                                   bppo_ctx **out) {
    if (!cfg || !out) return BPPO_ERR_ARG;
    bppo_ctx *c = new bppo_ctx();
    bppo_status s = ctx_init(c, cfg, hip_device, hip_stream);
    *out = c;   // returned even on failure so bppo_last_error can explain; caller destroys
    return s;
}

extern "C" void bppo_destroy(bppo_ctx *c) {
    if (!c) return;
    if (c->ev_thread.joinable()) c->ev_thread.join();
    if (c->ev_stream) { (void)hipStreamSynchronize(c->ev_stream); (void)hipStreamDestroy(c->ev_stream); }
    if (c->ev_gae) (void)hipEventDestroy(c->ev_gae);
    if (c->ev_copied) (void)hipEventDestroy(c->ev_copied);
    if (c->fy_stream) (void)hipStreamSynchronize(c->fy_stream);   // reads the engine's J buffers
    c->shuf.shutdown();
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->mem.free_all();
    if (c->ev_block) (void)hipEventDestroy(c->ev_block);
    if (c->ev_upd) (void)hipEventDestroy(c->ev_upd);
    for (int i = 0; i < TM_SLOTS; i++) {
        if (c->ev[i][0]) (void)hipEventDestroy(c->ev[i][0]);
        if (c->ev[i][1]) (void)hipEventDestroy(c->ev[i][1]);
    }
    for (auto &pr : c->mb_ev)
        for (hipEvent_t e : pr) if (e) (void)hipEventDestroy(e);
    if (c->fy_stream) { (void)hipStreamSynchronize(c->fy_stream); (void)hipStreamDestroy(c->fy_stream); }
    for (hipEvent_t e : c->fy_ev) if (e) (void)hipEventDestroy(e);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" size_t bppo_num_params(const bppo_ctx *c) { return c ? c->net.n_params : 0; }

// a rollout bppo_train_steps enqueued ahead (and left pending by an error) was drawn
// with the state these setters replace: drop it (the envs and the RNG stay where it
// left them; the next bppo_collect_rollouts draws a new one)
void drop_prefetch(bppo_ctx *c) {   // (also eval.hip)
    if (!c->prefetched) return;
    c->prefetched = false;
    c->collected = 0;
    c->gae_done = 0;
    (void)opp_records_clear(c);   // its finished opponent games go with it
}

extern "C" bppo_status bppo_params_set(bppo_ctx *c, const float *h, size_t n) {
    if (!c || !h || n != c->net.n_params) { if (c) c->err = "params_set: size mismatch"; return BPPO_ERR_ARG; }
    drop_prefetch(c);
    BPPO_HIP(c, hipMemcpyAsync(c->d_params, h, n * 4, hipMemcpyHostToDevice, c->stream));
    if (c->wide) TRY(wide_pack(c));
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" bppo_status bppo_params_get(bppo_ctx *c, float *h, size_t n) {
    if (!c || !h || n != c->net.n_params) { if (c) c->err = "params_get: size mismatch"; return BPPO_ERR_ARG; }
    BPPO_HIP(c, hipMemcpyAsync(h, c->d_params, n * 4, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" bppo_status bppo_forward(bppo_ctx *c, const float *obs, const float *priv, int32_t B,
                                    float *logits, float *values) {
    if (!c || !obs || B <= 0) return BPPO_ERR_ARG;
    if (c->wide) return wide_forward_host(c, obs, priv, B, logits, values);
    // scratch freed on every return path (an inference call, not the rollout path)
    DeviceMem mem;
    float *d_o = nullptr, *d_l = nullptr, *d_v = nullptr;
    BPPO_HIP(c, mem.alloc(&d_o, (size_t)B * c->D));
    BPPO_HIP(c, mem.alloc(&d_l, (size_t)B * c->A));
    BPPO_HIP(c, mem.alloc(&d_v, (size_t)B));
    BPPO_HIP(c, hipMemcpyAsync(d_o, obs, sizeof(float) * (size_t)B * c->D, hipMemcpyHostToDevice, c->stream));
    bppo_status s = launch_forward_rows(c, d_o, B, d_l, d_v);
    if (s == BPPO_OK) {
        if (logits) BPPO_HIP(c, hipMemcpyAsync(logits, d_l, sizeof(float) * (size_t)B * c->A, hipMemcpyDeviceToHost, c->stream));
        if (values) BPPO_HIP(c, hipMemcpyAsync(values, d_v, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    }
    // drain before the scratch is freed, whatever happened above
    const bppo_status ss = sync_stream(c) == hipSuccess ? BPPO_OK : BPPO_ERR_HIP;
    return s != BPPO_OK ? s : ss;
}

extern "C" bppo_status bppo_rng_get(bppo_ctx *c, uint64_t *p) {
    if (!c || !p) return BPPO_ERR_ARG;
    *p = c->rng_pos;
    return BPPO_OK;
}
extern "C" bppo_status bppo_rng_set(bppo_ctx *c, uint64_t p) {
    if (!c) return BPPO_ERR_ARG;
    drop_prefetch(c);
    c->shuf_slot = -1;
    c->fy_slot = -1; c->fy_done = 0;     // permutations made ahead belong to the old start
    c->rng_pos = p;
    return BPPO_OK;
}

// checkpoint.rs:390-400 save_rng_state: rng.fill_bytes(&mut [u8; 32]) — rand_core
// 0.6 BlockRng::fill_bytes takes ceil(n / 4) whole words, little-endian
extern "C" bppo_status bppo_rng_fill_bytes(bppo_ctx *c, uint8_t *dst, size_t n) {
    if (!c || (!dst && n)) return BPPO_ERR_ARG;
    const size_t nw = (n + 3) / 4;
    uint32_t blk[16];
    uint64_t cached = ~0ull;
    for (size_t i = 0; i < nw; i++) {
        const uint64_t pos = c->rng_pos + i;
        if ((pos >> 4) != cached) { chacha12_block(c->rng_key, pos >> 4, c->cfg.rng_stream, blk); cached = pos >> 4; }
        const uint32_t w = blk[pos & 15];
        for (int b = 0; b < 4 && 4 * i + b < n; b++) dst[4 * i + b] = (uint8_t)(w >> (8 * b));
    }
    c->rng_pos += nw;
    c->shuf_slot = -1;
    c->fy_slot = -1; c->fy_done = 0;
    return BPPO_OK;
}

// checkpoint.rs:405-426 load_rng_state: StdRng::from_seed(seed) — the 32 seed bytes
// are the ChaCha12 key (8 little-endian words), block counter 0.  The shuffle
// engine precomputes words of the old key, so it is restarted on the new one.
extern "C" bppo_status bppo_rng_from_seed(bppo_ctx *c, const uint8_t *seed) {
    if (!c || !seed) return BPPO_ERR_ARG;
    drop_prefetch(c);
    Key8 k;
    for (int i = 0; i < 8; i++)
        k.k[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) |
                 ((uint32_t)seed[4 * i + 3] << 24);
    BPPO_HIP(c, sync_stream(c));
    BPPO_HIP(c, hipStreamSynchronize(c->fy_stream));   // its permutations read the engine's J
    c->fy_slot = -1; c->fy_done = 0;
    c->shuf.shutdown();
    c->shuf.~ShuffleEngine();
    new (&c->shuf) ShuffleEngine();
    c->rng_key = k;
    c->rng_pos = 0;
    c->shuf_slot = -1;
    const size_t TN = (size_t)c->T * c->N;
    TRY(c->shuf.init(c->dev, c->rng_key, c->cfg.rng_stream, (uint32_t)TN, c->cfg.num_epochs, TN * (uint64_t)c->A, c->err,
                     c->cfg.shuffle_windows != 0));
    return BPPO_OK;
}

extern "C" bppo_status bppo_rng_key_get(bppo_ctx *c, uint32_t *key) {
    if (!c || !key) return BPPO_ERR_ARG;
    for (int i = 0; i < 8; i++) key[i] = c->rng_key.k[i];
    return BPPO_OK;
}

// Adam state (burn-optim AdamState: moment_1, moment_2, time per parameter tensor):
// m1/m2 flat like the parameters, steps [2 * layers] in record order (W, b per Linear)
extern "C" bppo_status bppo_optimizer_get(bppo_ctx *c, float *m1, float *m2, int32_t *steps, size_t n) {
    if (!c || n != c->net.n_params) { if (c) c->err = "optimizer_get: size mismatch"; return BPPO_ERR_ARG; }
    if (m1) BPPO_HIP(c, hipMemcpyAsync(m1, c->d_m1, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (m2) BPPO_HIP(c, hipMemcpyAsync(m2, c->d_m2, n * 4, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, sync_stream(c));
    // adam_t is indexed by layer (2 l, 2 l + 1); steps[] is in record order
    if (steps)
        for (int l = 0; l < c->net.n_layers; l++)
            for (int k = 0; k < 2; k++) steps[2 * c->net.rec[l] + k] = c->adam_t[2 * l + k];
    return BPPO_OK;
}

extern "C" bppo_status bppo_optimizer_set(bppo_ctx *c, const float *m1, const float *m2, const int32_t *steps,
                                          size_t n) {
    // (a rollout enqueued ahead does not read the Adam moments: it stays valid)
    if (!c || !m1 || !m2 || !steps || n != c->net.n_params) {
        if (c) c->err = "optimizer_set: size mismatch";
        return BPPO_ERR_ARG;
    }
    BPPO_HIP(c, hipMemcpyAsync(c->d_m1, m1, n * 4, hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemcpyAsync(c->d_m2, m2, n * 4, hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, sync_stream(c));
    for (int l = 0; l < c->net.n_layers; l++)
        for (int k = 0; k < 2; k++) c->adam_t[2 * l + k] = steps[2 * c->net.rec[l] + k];
    return BPPO_OK;
}

extern "C" size_t bppo_num_param_tensors(const bppo_ctx *c) { return c ? c->adam_t.size() : 0; }

extern "C" bppo_status bppo_vecenv_reset(bppo_ctx *c) {
    if (!c) return BPPO_ERR_ARG;
    drop_prefetch(c);
    TRY(c->wide ? wide_reset(c) : launch_cartpole_reset(c));
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" bppo_status bppo_vecenv_observe(bppo_ctx *c, float *obs, int32_t *players, uint8_t *masks,
                                           float *priv) {
    (void)priv; (void)masks;
    if (!c) return BPPO_ERR_ARG;
    if (c->wide) return wide_observe_host(c, obs, players, masks, priv);
    if (obs) {
        TRY(launch_cartpole_observe(c, c->d_bxc));
        BPPO_HIP(c, hipMemcpyAsync(obs, c->d_bxc, sizeof(float) * (size_t)c->N * c->D, hipMemcpyDeviceToHost, c->stream));
        BPPO_HIP(c, sync_stream(c));
    }
    if (players) std::fill(players, players + c->N, 0);
    return BPPO_OK;
}

extern "C" bppo_status bppo_vecenv_step(bppo_ctx *c, const int32_t *actions, float *obs, float *rewards,
                                        uint8_t *dones, bppo_episode *eps, int32_t cap, int32_t *n_eps) {
    if (!c || !actions) return BPPO_ERR_ARG;
    const int N = c->N;
    if (c->wide) {
        BPPO_HIP(c, hipMemsetAsync(c->d_ep_count, 0, 4, c->stream));
        int32_t cnt = 0;
        TRY(wide_step_host(c, actions, obs, rewards, dones, &cnt));
        if (n_eps) *n_eps = cnt;
        if (eps && cap > 0 && cnt > 0) {
            std::vector<EpisodeRec> recs(std::min(cnt, c->eps_cap));
            BPPO_HIP(c, hipMemcpy(recs.data(), c->d_eps, sizeof(EpisodeRec) * recs.size(), hipMemcpyDeviceToHost));
            std::sort(recs.begin(), recs.end(), [](const EpisodeRec &a, const EpisodeRec &b) {
                return a.env_index < b.env_index; });
            for (int i = 0; i < (int)recs.size() && i < cap; i++) {
                std::memcpy(eps[i].total_reward, recs[i].total_reward, sizeof(float) * BPPO_MAX_PLAYERS);
                eps[i].length = recs[i].length; eps[i].env_index = recs[i].env_index;
                eps[i].step = recs[i].step; eps[i].pad = 0;
            }
        }
        return BPPO_OK;
    }
    // persistent scratch (ctx_init): no allocator round-trip per step
    int32_t *d_a = c->d_act_in; float *d_r = c->d_scr_r, *d_o = c->d_bxc; uint8_t *d_d = c->d_scr_d;
    BPPO_HIP(c, hipMemcpyAsync(d_a, actions, sizeof(int32_t) * N, hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, hipMemsetAsync(c->d_ep_count, 0, 4, c->stream));
    TRY(launch_cartpole_vecenv_step(c, d_a, d_r, d_d, d_o));
    if (rewards) BPPO_HIP(c, hipMemcpyAsync(rewards, d_r, sizeof(float) * N, hipMemcpyDeviceToHost, c->stream));
    if (dones) BPPO_HIP(c, hipMemcpyAsync(dones, d_d, N, hipMemcpyDeviceToHost, c->stream));
    if (obs) BPPO_HIP(c, hipMemcpyAsync(obs, d_o, sizeof(float) * (size_t)N * c->D, hipMemcpyDeviceToHost, c->stream));
    int32_t cnt = 0;
    BPPO_HIP(c, hipMemcpyAsync(&cnt, c->d_ep_count, 4, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, sync_stream(c));
    if (n_eps) *n_eps = cnt;
    if (eps && cap > 0 && cnt > 0) {
        std::vector<EpisodeRec> recs(std::min(cnt, c->eps_cap));
        BPPO_HIP(c, hipMemcpy(recs.data(), c->d_eps, sizeof(EpisodeRec) * recs.size(), hipMemcpyDeviceToHost));
        std::sort(recs.begin(), recs.end(), [](const EpisodeRec &a, const EpisodeRec &b) {
            return a.env_index < b.env_index; });
        for (int i = 0; i < (int)recs.size() && i < cap; i++) {
            std::memcpy(eps[i].total_reward, recs[i].total_reward, sizeof(float) * BPPO_MAX_PLAYERS);
            eps[i].length = recs[i].length; eps[i].env_index = recs[i].env_index;
            eps[i].step = recs[i].step; eps[i].pad = 0;
        }
    }
    return BPPO_OK;
}

// Environment::set_step (env.rs:329-333): the step every schedulable env parameter
// (Liar's Dice reward shaping, liars_dice.rs:535, 635) is evaluated at
extern "C" bppo_status bppo_vecenv_set_step(bppo_ctx *c, uint64_t s) {
    if (!c) return BPPO_ERR_ARG;
    c->env_step = s;
    return BPPO_OK;
}

// reward_shaping_coef as a Schedule (config.rs:761-762; schedule.rs:29): milestones
// (values[i], steps[i]) in the caller's order (the reference sorts at parse time,
// schedule.rs:144, 268).  n = 0 is the empty schedule (get = 0.0).  Initial value
// must be >= 0 (config.rs:1514-1519).
extern "C" bppo_status bppo_set_reward_shaping_schedule(bppo_ctx *c, const double *values, const uint64_t *steps,
                                                        int32_t n) {
    if (!c || n < 0 || (n > 0 && (!values || !steps))) return BPPO_ERR_ARG;
    std::vector<double> v(values, values + n);
    std::vector<uint64_t> s(steps, steps + n);
    if (bppo::schedule_get(v, s, 0) < 0.0) { c->err = "reward_shaping_coef must be >= 0"; return BPPO_ERR_ARG; }
    c->shaping_v = std::move(v); c->shaping_s = std::move(s);
    return BPPO_OK;
}

extern "C" bppo_status bppo_obs_norm_get(bppo_ctx *c, double *mean, double *m2, double *count) {
    if (!c) return BPPO_ERR_ARG;
    std::vector<double> h(2 * c->D + 1);
    BPPO_HIP(c, hipMemcpyAsync(h.data(), c->d_on, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, sync_stream(c));
    if (mean) std::memcpy(mean, h.data(), sizeof(double) * c->D);
    if (m2) std::memcpy(m2, h.data() + c->D, sizeof(double) * c->D);
    if (count) *count = h[2 * c->D];
    return BPPO_OK;
}

extern "C" bppo_status bppo_obs_norm_set(bppo_ctx *c, const double *mean, const double *m2, double count) {
    if (!c || !mean || !m2) return BPPO_ERR_ARG;
    drop_prefetch(c);
    std::vector<double> h(2 * c->D + 1);
    std::memcpy(h.data(), mean, sizeof(double) * c->D);
    std::memcpy(h.data() + c->D, m2, sizeof(double) * c->D);
    h[2 * c->D] = count;
    BPPO_HIP(c, hipMemcpyAsync(c->d_on, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" bppo_status bppo_ret_norm_get(bppo_ctx *c, double *mvc, double *returns) {
    if (!c) return BPPO_ERR_ARG;
    if (mvc) BPPO_HIP(c, hipMemcpyAsync(mvc, c->d_rn_stats, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    if (returns) BPPO_HIP(c, hipMemcpyAsync(returns, c->d_rn_returns, sizeof(double) * (size_t)c->N * c->P, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" bppo_status bppo_ret_norm_set(bppo_ctx *c, const double *mvc, const double *returns) {
    if (!c) return BPPO_ERR_ARG;
    drop_prefetch(c);
    if (mvc) BPPO_HIP(c, hipMemcpyAsync(c->d_rn_stats, mvc, sizeof(double) * 3, hipMemcpyHostToDevice, c->stream));
    if (returns) BPPO_HIP(c, hipMemcpyAsync(c->d_rn_returns, returns, sizeof(double) * (size_t)c->N * c->P, hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" bppo_status bppo_popart_get(bppo_ctx *c, double *st) {
    if (!c || !st) return BPPO_ERR_ARG;
    st[0] = c->pa_mean; st[1] = c->pa_m2; st[2] = c->pa_count; st[3] = c->pa_eps;
    return BPPO_OK;
}

extern "C" bppo_status bppo_popart_set(bppo_ctx *c, const double *st) {
    if (!c || !st) return BPPO_ERR_ARG;
    drop_prefetch(c);
    c->pa_mean = st[0]; c->pa_m2 = st[1]; c->pa_count = st[2]; c->pa_eps = st[3];
    return BPPO_OK;
}

extern "C" bppo_status bppo_rollout_episode_outcomes(bppo_ctx *c, int32_t *placements, int32_t *has_outcome,
                                                     int32_t cap, int32_t *n) {
    if (!c) return BPPO_ERR_ARG;
    std::vector<EpisodeRec> recs;
    int32_t cnt = 0;
    TRY(rollout_records_sorted(c, recs, &cnt));
    for (int i = 0; i < (int)recs.size() && i < cap; i++) {
        int32_t pl[BPPO_MAX_PLAYERS];
        const bool has = opp_unpack_outcome((uint32_t)recs[i].pad, pl);
        if (placements) std::memcpy(placements + (size_t)i * BPPO_MAX_PLAYERS, pl, sizeof pl);
        if (has_outcome) has_outcome[i] = has ? 1 : 0;
    }
    if (n) *n = cnt;
    return BPPO_OK;
}

extern "C" bppo_status bppo_set_episode_stats(bppo_ctx *c, int32_t enable) {
    if (!c) return BPPO_ERR_ARG;
    if (enable && ep_key_digits((uint64_t)c->T * (uint64_t)c->N) > EPS_MAX_DIGITS) {
        c->err = "episode statistics: num_steps * num_envs above 2^33";
        return BPPO_ERR_UNSUPPORTED;
    }
    if (enable) TRY(episode_stats_alloc(c));
    c->ep_stats_on = enable ? 1 : 0;
    c->ep_entries.clear();
    return BPPO_OK;
}

extern "C" bppo_status bppo_episode_stats_get(bppo_ctx *c, int32_t k, bppo_episode_stats *out, bppo_episode_tail *tail,
                                              int32_t tail_cap, int32_t *n_tail) {
    if (!c) return BPPO_ERR_ARG;
    if (!c->ep_stats_on) { c->err = "episode statistics are off (bppo_set_episode_stats)"; return BPPO_ERR_ARG; }
    if (c->ep_entries.empty()) { c->err = "episode statistics: no rollout has run since they were switched on"; return BPPO_ERR_ARG; }
    if (k < 0 || k >= (int32_t)c->ep_entries.size()) {
        c->err = "episode statistics: rollout " + std::to_string(k) + " of a call that ran " +
                 std::to_string(c->ep_entries.size());
        return BPPO_ERR_ARG;
    }
    const bppo_ctx::EpEntry &en = c->ep_entries[(size_t)k];
    if (out) *out = en.st;
    if (tail)
        for (int i = 0; i < (int)en.tail.size() && i < tail_cap; i++) tail[i] = en.tail[(size_t)i];
    if (n_tail) *n_tail = (int32_t)en.tail.size();
    return BPPO_OK;
}

extern "C" bppo_status bppo_rollout_episodes(bppo_ctx *c, bppo_episode *eps, int32_t cap, int32_t *n) {
    if (!c) return BPPO_ERR_ARG;
    std::vector<EpisodeRec> recs;
    int32_t cnt = 0;
    TRY(rollout_records_sorted(c, recs, &cnt));
    const int m = (int)recs.size();
    for (int i = 0; i < m && i < cap; i++) {
        std::memcpy(eps[i].total_reward, recs[i].total_reward, sizeof(float) * BPPO_MAX_PLAYERS);
        eps[i].length = recs[i].length; eps[i].env_index = recs[i].env_index;
        eps[i].step = recs[i].step; eps[i].pad = 0;
    }
    if (n) *n = cnt;
    return BPPO_OK;
}

extern "C" bppo_status bppo_set_explained_variance_mode(bppo_ctx *c, int32_t mode) {
    if (!c || mode < 0 || mode > 1) return BPPO_ERR_ARG;
    if (mode == 1 && !c->h_ev_v) {
        // every resource into a local first: committed together, or all released
        const size_t TN = (size_t)c->T * c->N;
        hipStream_t st = nullptr;
        hipEvent_t e_gae = nullptr, e_cp = nullptr;
        float *hv = nullptr, *hr = nullptr, *hm = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&e_gae, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&e_cp, hipEventDisableTiming | hipEventBlockingSync);
        if (e == hipSuccess) e = c->mem.alloc_pinned(&hv, TN);
        if (e == hipSuccess) e = c->mem.alloc_pinned(&hr, TN);
        if (e == hipSuccess) e = c->mem.alloc_pinned(&hm, TN);
        if (e != hipSuccess) {
            (void)c->mem.release(hv); (void)c->mem.release(hr); (void)c->mem.release(hm);
            if (e_cp) (void)hipEventDestroy(e_cp);
            if (e_gae) (void)hipEventDestroy(e_gae);
            if (st) (void)hipStreamDestroy(st);
            return hip_fail(c, e, "explained-variance reference mode: allocation");
        }
        c->ev_stream = st; c->ev_gae = e_gae; c->ev_copied = e_cp;
        c->h_ev_r = hr; c->h_ev_valid = hm;
        c->h_ev_v = hv;                    // last: marks the set complete
    }
    c->ev_mode = mode;
    return BPPO_OK;
}

extern "C" bppo_status bppo_debug_record_params(bppo_ctx *c, float *host, int32_t max_minibatches) {
    if (!c || max_minibatches < 0) return BPPO_ERR_ARG;
    c->dbg_params = max_minibatches > 0 ? host : nullptr;
    c->dbg_params_max = host ? max_minibatches : 0;
    return BPPO_OK;
}

extern "C" bppo_status bppo_set_minibatch_kernel(bppo_ctx *c, int32_t mode) {
    if (!c || mode < 0 || mode > 2) return BPPO_ERR_ARG;
    c->mb_kernel = mode;
    return BPPO_OK;
}

// W > 1.  PopArt's statistics are all-gathered (popart.hip): its
// scratch is sized for the world here
static bppo_status check_world(bppo_ctx *c, int32_t world) {
    if (world > 1 && c->cfg.normalize_values) {
        BPPO_HIP(c, c->mem.release(c->d_pa_gather));
        BPPO_HIP(c, c->mem.alloc(&c->d_pa_gather, 9 * (size_t)world));
    }
    return BPPO_OK;
}

extern "C" bppo_status bppo_set_rank(bppo_ctx *c, int32_t rank) {
    if (!c || rank < 0) return BPPO_ERR_ARG;
    c->rank = rank;
    return BPPO_OK;
}

extern "C" bppo_status bppo_set_allreduce(bppo_ctx *c, bppo_allreduce_fn fn, void *user, int32_t world) {
    if (!c || world < 1) return BPPO_ERR_ARG;
    TRY(check_world(c, world));
    c->allreduce = fn; c->allreduce_user = user; c->world = world; c->allreduce_async = 0;
    return BPPO_OK;
}

extern "C" bppo_status bppo_set_allreduce_async(bppo_ctx *c, bppo_allreduce_fn fn, void *user, int32_t world) {
    if (!c || world < 1) return BPPO_ERR_ARG;
    TRY(check_world(c, world));
    c->allreduce = fn; c->allreduce_user = user; c->world = world; c->allreduce_async = 1;
    return BPPO_OK;
}

extern "C" bppo_status bppo_get_stream(bppo_ctx *c, void **stream) {
    if (!c || !stream) return BPPO_ERR_ARG;
    *stream = (void *)c->stream;
    return BPPO_OK;
}

struct BufDesc { void *ptr; size_t bytes; };
static BufDesc find_buf(bppo_ctx *c, const char *name) {
    const size_t TN = (size_t)c->T * c->N;
    if (!strcmp(name, "obs")) return {c->d_obs, TN * c->D * 4};
    if (!strcmp(name, "actions")) return {c->d_act, TN * 4};
    if (!strcmp(name, "rewards")) return {c->d_rew, TN * 4};
    if (!strcmp(name, "raw_rewards")) return {c->d_rew_raw, TN * 4};
    if (!strcmp(name, "valid")) return {c->d_valid, c->d_valid ? TN * 4 : 0};
    if (!strcmp(name, "dones")) return {c->d_done, TN * 4};
    if (!strcmp(name, "values")) return {c->d_val, TN * 4};
    if (!strcmp(name, "log_probs")) return {c->d_logp, TN * 4};
    if (!strcmp(name, "advantages")) return {c->d_adv, TN * 4};
    if (!strcmp(name, "returns")) return {c->d_ret, TN * 4};
    if (!strcmp(name, "all_rewards")) return {c->d_rew, TN * 4};
    if (!strcmp(name, "perm")) return {c->d_perm, TN * 4};
    if (!strncmp(name, "perm_ep:", 8)) {          // epoch e's permutation of the last update
        const int e = atoi(name + 8);
        if (e < 0 || e >= c->cfg.num_epochs || !c->d_perm_ep) return {nullptr, 0};
        return {c->d_perm_ep + (size_t)e * TN, TN * 4};
    }
    if (!strcmp(name, "last_values")) return {c->d_last_v, (size_t)c->N * 4};
    if (!strcmp(name, "grad")) return {c->d_grad, c->net.n_params * 4};
    return {nullptr, 0};
}

extern "C" bppo_status bppo_buffer_get(bppo_ctx *c, const char *name, void *host, size_t bytes) {
    if (!c || !name || !host) return BPPO_ERR_ARG;
    if (c->wide) {
        bool handled = false;
        bppo_status s = wide_buffer_get(c, name, host, bytes, &handled);
        if (handled) return s;
    }
    BufDesc b = find_buf(c, name);
    if (!b.ptr || bytes < b.bytes) { c->err = std::string("buffer_get: unknown buffer or too small: ") + name; return BPPO_ERR_ARG; }
    BPPO_HIP(c, hipMemcpyAsync(host, b.ptr, b.bytes, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, sync_stream(c));
    return BPPO_OK;
}

extern "C" int32_t bppo_minibatch_rows(bppo_ctx *c, float *out, int32_t max_rows, int32_t *row_width) {
    if (!c) return -1;
    const int32_t w = WM_COUNT + 4;
    const int32_t n = (int32_t)(c->last_rows.size() / (size_t)w);
    if (row_width) *row_width = w;
    if (out && max_rows > 0)
        std::memcpy(out, c->last_rows.data(), sizeof(float) * (size_t)std::min(n, max_rows) * (size_t)w);
    return n;
}

extern "C" bppo_status bppo_buffer_set(bppo_ctx *c, const char *name, const void *host, size_t bytes) {
    if (!c || !name || !host) return BPPO_ERR_ARG;
    BufDesc b = find_buf(c, name);
    if (!b.ptr || bytes != b.bytes) { c->err = std::string("buffer_set: unknown buffer or size mismatch: ") + name; return BPPO_ERR_ARG; }
    BPPO_HIP(c, hipMemcpyAsync(b.ptr, host, b.bytes, hipMemcpyHostToDevice, c->stream));
    BPPO_HIP(c, sync_stream(c));
    if (!strcmp(name, "advantages") || !strcmp(name, "returns")) c->gae_done = c->collected = 1;
    c->rows_packed = c->rows_from_rollout = false;   // the update re-packs its rows from the buffers
    return BPPO_OK;
}

extern "C" bppo_status bppo_gae_device(const float *r, const float *d, const float *v, const float *lv,
                                       int32_t T, int32_t N, float gamma, float lambda, float *adv,
                                       float *ret, void *stream) {
    if (!r || !d || !v || !lv || !adv || !ret || T < 0 || N < 0) return BPPO_ERR_ARG;
    return launch_gae_1p(r, d, v, lv, T, N, gamma, lambda, adv, ret, (hipStream_t)stream);
}

extern "C" bppo_status bppo_gae_rows_device(const float *r, const float *d, const float *v, const float *lv,
                                            int32_t T, int32_t N, float gamma, float lambda, float *adv,
                                            float *ret, float *rows, void *stream) {
    if (!r || !d || !v || !lv || !adv || !ret || !rows || T < 0 || N < 0) return BPPO_ERR_ARG;
    // only the segmented kernel writes the pairs: refuse other shapes before launching anything
    if (N % 4 != 0 || T > 128 ||
        ((uintptr_t)r | (uintptr_t)d | (uintptr_t)v | (uintptr_t)lv | (uintptr_t)adv | (uintptr_t)ret | (uintptr_t)rows) % 16)
        return BPPO_ERR_UNSUPPORTED;
    bool packed = false;
    const bppo_status s = launch_gae_1p(r, d, v, lv, T, N, gamma, lambda, adv, ret, (hipStream_t)stream,
                                        reinterpret_cast<float2 *>(rows), &packed);
    return s != BPPO_OK ? s : packed ? BPPO_OK : BPPO_ERR_UNSUPPORTED;
}

extern "C" bppo_status bppo_gae_mp_device(const float *ar, const int32_t *pl, const float *d,
                                          const float *v, const float *lvpp, int32_t T, int32_t N,
                                          int32_t P, float gamma, float lambda, float *adv, float *ret,
                                          void *stream) {
    if (!ar || !pl || !d || !v || !lvpp || !adv || !ret || T < 0 || N < 0 || P < 1 || P > BPPO_MAX_PLAYERS)
        return BPPO_ERR_ARG;
    return launch_gae_mp(ar, pl, d, v, lvpp, T, N, P, gamma, lambda, adv, ret, (hipStream_t)stream);
}

extern "C" bppo_status bppo_last_kernel_ms(bppo_ctx *c, const char *k, float *ms) {
    if (!c || !k || !ms) return BPPO_ERR_ARG;
    static const char *names[8] = {"rollout", "gae", "update", "minibatch", "return_norm", "shuffle",
                                   "adam", "bootstrap"};
    for (int i = 0; i < 8; i++)
        if (!strcmp(k, names[i])) { *ms = c->last_ms[i]; return BPPO_OK; }
    // host side of the shuffle: draw-chain walk of the last update's epochs, and the
    // time ppo_update blocked waiting for it
    if (!strcmp(k, "shuffle_walk")) { *ms = (float)c->last_walk_ms; return BPPO_OK; }
    if (!strcmp(k, "minibatch_kernel")) { *ms = c->mb_k_mean; return BPPO_OK; }   // all launches of the last update
    if (!strcmp(k, "minibatch_kernel_min")) { *ms = c->mb_k_min; return BPPO_OK; }
    if (!strcmp(k, "minibatch_kernel_max")) { *ms = c->mb_k_max; return BPPO_OK; }
    if (!strcmp(k, "minibatch_kernel_split")) { *ms = c->mb_k_split; return BPPO_OK; }   // k_minibatch_split launches
    if (!strcmp(k, "minibatch_kernel_exact")) { *ms = c->mb_k_exact; return BPPO_OK; }   // k_minibatch_mfma launches
    if (!strcmp(k, "shuffle_wait")) { *ms = (float)c->last_wait_ms; return BPPO_OK; }
    if (!strcmp(k, "host_enqueue")) { *ms = (float)c->last_host_ms; return BPPO_OK; }   // bppo_train_step outside stream waits
    if (!strcmp(k, "host_sync_wait")) { *ms = (float)c->last_sync_ms; return BPPO_OK; }
    if (!strcmp(k, "shuffle_walk_tsc_ms")) { *ms = (float)c->last_walk_cpu_ms; return BPPO_OK; }    // all walks, in chain_walk
    if (!strcmp(k, "shuffle_words_tsc_ms")) { *ms = (float)c->last_words_cpu_ms; return BPPO_OK; }  // all walks, getting words
    if (!strcmp(k, "shuffle_spec_mwords")) { *ms = (float)c->last_spec_mwords; return BPPO_OK; }   // speculative walk words (M)
    if (!strcmp(k, "shuffle_true_mwords")) { *ms = (float)c->last_true_mwords; return BPPO_OK; }   // true walk words (M)
    if (!strcmp(k, "shuffle_met")) { *ms = (float)c->last_met; return BPPO_OK; }   // epochs resolved by speculation
    return BPPO_ERR_ARG;
}

extern "C" bppo_status bppo_debug_libm(int32_t which, int32_t device, const float *x, float *y, size_t n) {
    if (!x || !y) return BPPO_ERR_ARG;
    if (!device) {
        for (size_t i = 0; i < n; i++) {
            float v = x[i];
            switch (which) {
            case 0: y[i] = bppo_math::logf_glibc(v); break;
            case 1: y[i] = bppo_math::sinf_glibc(v); break;
            case 2: y[i] = bppo_math::cosf_glibc(v); break;
            case 3: y[i] = -bppo_math::logf_glibc(-bppo_math::logf_glibc(v)); break;
            case 5: y[i] = bppo_math::tanhf_glibc(v); break;
            default: y[i] = bppo_math::expf_glibc(v); break;
            }
        }
        return BPPO_OK;
    }
    DeviceMem mem;
    float *dx = nullptr, *dy = nullptr;
    if (mem.alloc(&dx, n) != hipSuccess || mem.alloc(&dy, n) != hipSuccess) return BPPO_ERR_HIP;
    bppo_status s = BPPO_ERR_HIP;
    if (hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice) == hipSuccess &&
        launch_libm(which, dx, dy, n) == BPPO_OK && hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(y, dy, n * 4, hipMemcpyDeviceToHost) == hipSuccess)
        s = BPPO_OK;
    return s;
}

// the update's metric fold on caller-given rows (no HIP call)
extern "C" bppo_status bppo_debug_fold_metrics(const float *rows, int32_t nup, const bppo_debug_fold_args *args,
                                               bppo_update_metrics *out) {
    if (!args || !out || nup < 0 || (!rows && nup)) return BPPO_ERR_ARG;
    FoldArgs a;
    a.value_coef = args->value_coef; a.ent_coef = args->ent_coef;
    a.A = args->A; a.env_kind = args->env_kind; a.B = (size_t)args->B;
    std::memcpy(a.ev4, args->ev4, sizeof a.ev4);
    a.ev_mode = args->ev_mode; a.ev_ref = args->ev_ref; a.epochs_run = args->epochs_run;
    a.normalize_values = args->normalize_values != 0;
    a.pa_tsum = args->pa_tsum; a.pa_tsq = args->pa_tsq; a.pa_tcount = args->pa_tcount;
    a.pa_rescale_mag = args->pa_rescale_mag;
    fold_update_metrics(rows, nup, a, out);
    return BPPO_OK;
}

// shuffle parity hooks: the host draw chain alone, and the device Fisher-Yates
// on caller-given swap targets
extern "C" bppo_status bppo_debug_shuffle_chain(uint64_t seed, uint64_t stream, uint64_t word_pos, uint32_t n,
                                                uint32_t *J, uint64_t *end_pos) {
    if (!J && n) return BPPO_ERR_ARG;
    const Key8 key = seed_key(seed);
    const uint64_t e = shuffle_walk_host(key, stream, word_pos, n, J);
    if (end_pos) *end_pos = e;
    return BPPO_OK;
}

extern "C" bppo_status bppo_debug_chain_walk2(uint64_t seed, uint64_t stream, uint64_t pos_a, uint64_t pos_b,
                                              uint32_t n, uint32_t piece, uint64_t *end_a, uint64_t *end_b) {
    if (!end_a || !end_b || piece < 1) return BPPO_ERR_ARG;
    const Key8 key = seed_key(seed);
    struct Ch { uint64_t pos; uint32_t r; std::vector<uint32_t> w; size_t off, left; } ch[2];
    ch[0].pos = pos_a; ch[1].pos = pos_b;
    auto refill = [&](Ch &c) {
        const uint64_t q = (c.pos / piece + 1) * piece;
        c.w.resize(q - c.pos);
        bppo_host::chacha12_words(key.k, stream, c.pos, c.w.data(), c.w.size());
        c.off = 0;
        c.left = c.w.size();
    };
    for (Ch &c : ch) { c.r = n; refill(c); }
    auto live = [](const Ch &c) { return c.r >= 2; };
    auto advance = [&](Ch &c, size_t u) {
        c.off += u; c.left -= u; c.pos += u;
        if (live(c) && c.left == 0) refill(c);
    };
    while (live(ch[0]) && live(ch[1])) {
        size_t u0 = 0, u1 = 0;
        bppo_host::chain_walk2_nj(ch[0].w.data() + ch[0].off, ch[0].left, &ch[0].r, &u0,
                                  ch[1].w.data() + ch[1].off, ch[1].left, &ch[1].r, &u1);
        advance(ch[0], u0);
        advance(ch[1], u1);
    }
    for (Ch &c : ch)
        while (live(c)) advance(c, bppo_host::chain_walk_nj(c.w.data() + c.off, c.left, &c.r));
    *end_a = ch[0].pos;
    *end_b = ch[1].pos;
    return BPPO_OK;
}

// the full shuffle engine (GPU-made words, speculative walks) for `jobs`
// consecutive updates of `epochs` shuffles of n, the first starting at word
// position start and each next one `gap` words after the previous update's last
// shuffle (the rollout's draws): J [jobs][epochs][n] as rebuilt in HBM, end
// positions [jobs][epochs], and per epoch the checkpoints the true walk needed
// before it met a speculative walk (-1: walked the whole epoch)
extern "C" bppo_status bppo_debug_shuffle_engine(uint64_t seed, uint64_t stream, uint64_t start, uint32_t n,
                                                 int32_t epochs, uint64_t gap, int32_t jobs, int32_t windows,
                                                 uint32_t *J, uint64_t *ends, int32_t *met) {
    if (!J || !ends || n < 2 || epochs < 1 || epochs > SHUF_MAX_EPOCHS || jobs < 1) return BPPO_ERR_ARG;
    ShuffleEngine *e = new ShuffleEngine();
    std::string err;
    bppo_status s = e->init(0, seed_key(seed), stream, n, epochs, gap, err, windows != 0);
    uint64_t pos = start;
    for (int j = 0; j < jobs && s == BPPO_OK; j++) {
        const int slot = e->ensure(pos);
        for (int k = 0; k < epochs; k++) e->wait_epoch(slot, k);
        const size_t o = (size_t)j * epochs;
        if (hipStreamSynchronize(e->copy) != hipSuccess ||
            hipMemcpy(J + o * n, e->d_J[slot], sizeof(uint32_t) * (size_t)n * epochs, hipMemcpyDeviceToHost) != hipSuccess)
            s = BPPO_ERR_HIP;
        for (int k = 0; k < epochs; k++) {
            ends[o + k] = e->end_pos[slot][k];
            if (met) met[o + k] = e->coalesced[slot][k];
        }
        pos = e->job_end(slot) + gap;
    }
    e->shutdown();
    delete e;
    return s;
}

extern "C" bppo_status bppo_debug_fisher_yates(int32_t device, const uint32_t *J, uint32_t n, uint32_t *perm) {
    if (!J || !perm) return BPPO_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return BPPO_ERR_HIP;
    DeviceMem mem;
    uint32_t *dJ = nullptr, *dP = nullptr, *dS = nullptr, *dC = nullptr;
    FyRanges rg;
    bppo_status s = BPPO_ERR_HIP;
    if (mem.alloc(&dJ, (size_t)n + 1) == hipSuccess && mem.alloc(&dP, (size_t)n + 1) == hipSuccess &&
        mem.alloc(&dS, 4 * ((size_t)n + 1)) == hipSuccess && mem.alloc(&dC, (size_t)n / 8192 + 2) == hipSuccess &&
        hipMemcpy(dJ, J, 4ull * n, hipMemcpyHostToDevice) == hipSuccess &&
        fy_ranges_init(mem, rg, n) == hipSuccess &&
        fisher_yates_device(dJ, n, dS, dC, dP, nullptr, &rg) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(perm, dP, 4ull * n, hipMemcpyDeviceToHost) == hipSuccess)
        s = BPPO_OK;
    return s;
}

// apply_action_mask + sample_categorical + log_prob_categorical (utils.rs:10-45,
// 96-135) on host rows through the device sampler the multi-player rollout uses
// (k_sample_masked): Gumbel words of StdRng(seed) stream `stream` from word_pos,
// row-major [row][action]; masks may be NULL (all valid)
extern "C" bppo_status bppo_debug_sample(int32_t A, int32_t B, const float *logits, const uint8_t *masks,
                                         uint64_t seed, uint64_t stream, uint64_t word_pos, int32_t *actions,
                                         float *log_probs) {
    if (!logits || !actions || B <= 0 || (A != 2 && A != 7 && A != 49)) return BPPO_ERR_ARG;
    const size_t nA = (size_t)B * A;
    float *d_l = nullptr, *d_v = nullptr, *d_lp = nullptr, *d_val = nullptr, *d_lv = nullptr;
    uint8_t *d_m = nullptr;
    int32_t *d_p = nullptr, *d_a = nullptr, *d_e = nullptr;
    bppo_status s = BPPO_ERR_HIP;
    std::vector<uint8_t> ones;
    if (!masks) { ones.assign(nA, 1); masks = ones.data(); }
    int32_t err = 0;
    DeviceMem mem;
    if (mem.alloc(&d_l, nA) == hipSuccess && mem.alloc(&d_m, nA) == hipSuccess &&
        mem.alloc(&d_v, (size_t)B) == hipSuccess && mem.alloc(&d_lp, (size_t)B) == hipSuccess &&
        mem.alloc(&d_val, (size_t)B) == hipSuccess && mem.alloc(&d_lv, (size_t)B) == hipSuccess &&
        mem.alloc(&d_p, (size_t)B) == hipSuccess && mem.alloc(&d_a, (size_t)B) == hipSuccess &&
        mem.alloc(&d_e, 1) == hipSuccess && hipMemset(d_v, 0, 4ull * B) == hipSuccess &&
        hipMemset(d_p, 0, 4ull * B) == hipSuccess && hipMemset(d_e, 0, 4) == hipSuccess &&
        hipMemcpy(d_l, logits, nA * 4, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_m, masks, nA, hipMemcpyHostToDevice) == hipSuccess) {
        SampleArgs g;
        g.N = B; g.P = 1; g.logits = d_l; g.values = d_v; g.mask = d_m; g.players = d_p;
        g.key = seed_key(seed); g.stream = stream; g.base = word_pos;
        g.act = d_a; g.logp = d_lp; g.val = d_val; g.lvpp = d_lv; g.err = d_e;
        if (wide_sample(A, nullptr, g) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(actions, d_a, 4ull * B, hipMemcpyDeviceToHost) == hipSuccess &&
            (!log_probs || hipMemcpy(log_probs, d_lp, 4ull * B, hipMemcpyDeviceToHost) == hipSuccess) &&
            hipMemcpy(&err, d_e, 4, hipMemcpyDeviceToHost) == hipSuccess)
            s = (err & 2) ? BPPO_ERR_EMPTY_MASK : (err & 1) ? BPPO_ERR_NONFINITE : BPPO_OK;
    }
    return s;
}

// live allocations and bytes of every DeviceMem of the process (no HIP call)
extern "C" bppo_status bppo_debug_device_memory(int64_t *live_allocations, int64_t *live_bytes) {
    if (!live_allocations || !live_bytes) return BPPO_ERR_ARG;
    *live_allocations = DeviceMem::live_allocations.load();
    *live_bytes = DeviceMem::live_bytes.load();
    return BPPO_OK;
}
