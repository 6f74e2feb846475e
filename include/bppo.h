/*
 * bppo.h — C-ABI of libbppo.so, the MI355X-native replacement for burn-ppo's
 * rollout -> GAE -> PPO-update hot path.
 *
 * Plain pointers and sizes only.  Host pointers are marked "host"; the few
 * entry points taking device pointers say so.  Every entry point returns a
 * bppo_status; the reference's panics (NaN log-probs ppo.rs:363-366, empty
 * action mask utils.rs:115-123) become status codes, never aborts.
 * A context is not thread-safe: one context per host thread per GPU.
 *
 * Reference surfaces each group replaces (bhansconnect/burn-ppo):
 *   bppo_create / bppo_vecenv_*   Environment + VecEnv       env.rs:24-173, 281-487
 *   bppo_params_* / bppo_forward  ActorCriticNetwork         network/mod.rs:53-189
 *   bppo_collect_rollouts         collect_rollouts           ppo.rs:213-500
 *   bppo_compute_gae              bootstrap + compute_gae[_multiplayer]
 *                                                            main.rs:877-947, ppo.rs:1069-1264
 *   bppo_ppo_update               ppo_update (+ Adam/clip)   ppo.rs:1661-2112, main.rs:264-268
 *   bppo_gae_device               compute_gae on caller device buffers  ppo.rs:1069-1124
 *   bppo_rng_*                    the shared &mut StdRng     main.rs:189, checkpoint.rs:390-426
 *   bppo_optimizer_*              Adam record (checkpoint)   checkpoint.rs:291-335
 *   bppo_obs_norm_* / ret_norm_*  ObsNormalizer / ReturnNormalizer  normalization.rs:12-260
 */
#ifndef BPPO_H
#define BPPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    BPPO_OK = 0,
    BPPO_ERR_ARG = 1,          /* bad argument / shape mismatch */
    BPPO_ERR_NONFINITE = 2,    /* ppo.rs:363-366 "NaN/Inf in log probs" */
    BPPO_ERR_EMPTY_MASK = 3,   /* utils.rs:115-123 "Empty action mask" */
    BPPO_ERR_HIP = 4,          /* HIP runtime failure (message in bppo_last_error) */
    BPPO_ERR_COMM = 5,         /* all-reduce callback failed */
    BPPO_ERR_UNSUPPORTED = 6   /* configuration not implemented on the device path */
} bppo_status;

typedef enum { BPPO_ENV_CARTPOLE = 0, BPPO_ENV_CONNECT_FOUR = 1, BPPO_ENV_LIARS_DICE = 2, BPPO_ENV_SKULL = 3 } bppo_env_kind;
/* the widest player axis (Skull: MAX_PLAYERS = 6, envs/skull.rs:13) */
#define BPPO_MAX_PLAYERS 6

/* Mirrors the subset of config.rs:747-924 the hot path reads. */
typedef struct {
    int32_t env_kind;            /* bppo_env_kind */
    int32_t num_envs;            /* envs on THIS rank */
    int32_t num_steps;           /* T */
    int32_t hidden_size, num_hidden, relu;   /* activation == "relu" (else tanh) */
    int32_t ctde, critic_hidden_size, critic_num_hidden;
    int32_t num_epochs, num_minibatches;
    int32_t normalize_obs, normalize_returns, clip_value;
    double gamma, gae_lambda, clip_epsilon, value_coef, max_grad_norm, adam_epsilon;
    double target_kl;            /* < 0 : None */
    double return_clip;          /* ReturnNormalizer clip (config.rs:966-968) */
    double reward_shaping_coef;  /* Liar's Dice / Skull shaping (constant schedule; see below) */
    uint64_t seed;               /* main StdRng seed (main.rs:189) */
    uint64_t env_seed_base;      /* env i is seeded env_seed_base + i (main.rs:1964) */
    uint64_t rng_stream;         /* ChaCha stream id of the main RNG: 0 = reference; rank for W>1 */
    /* network_type = "cnn" (network/cnn.rs:24-50; Connect Four, OBSERVATION_SHAPE (6, 7, 2)):
     * num_conv_layers conv layers (stride 1, same padding, odd kernel_size, relu),
     * conv_channels per layer (the last repeated past the list, cnn.rs:84-90),
     * cnn_num_fc_layers FC layers of cnn_fc_hidden_size, then the heads */
    int32_t cnn, num_conv_layers, conv_channels[4], kernel_size, cnn_fc_hidden_size, cnn_num_fc_layers;
    /* normalize_values (config.rs:827-832, default false): PopArt value normalization
     * with value-head rescaling (normalization.rs:262-366, ppo.rs:1599-1653) */
    int32_t normalize_values;
    /* Skull: player_count (config.rs:767 PlayerCountMode, get_fixed_count, main.rs:1998);
     * 2..6, 0 = the default 4.  The player axis of the buffers stays NUM_PLAYERS = 6. */
    int32_t player_count;
    /* split_networks (config.rs:860, default false): separate actor and critic trunks.
     * MLP (mlp.rs:40-130, 139-206): a critic trunk of num_hidden x hidden_size on the
     * observation; flat parameters in Burn record order: layers (actor), critic_layers,
     * policy_head, value_head.  CNN (cnn.rs:116-135, 264-302): the critic's own conv stack
     * and FC layers; record order conv, fc, critic conv, critic fc, heads.  CTDE nets ignore
     * it (ctde.rs).  Any net: at most 16 layers in all (hidden / conv / FC layers + the two
     * heads), else bppo_create returns BPPO_ERR_UNSUPPORTED. */
    int32_t split_networks;
    /* shuffle_windows (not in the reference; for data-parallel ranks):
     * 0 = the reference: each epoch's shuffle (ppo.rs:1816) continues the main RNG where
     * the previous one ended.  1 = epoch e of an update draws from word S + e * (2 B + 2^20)
     * of the main stream (S = the update's first shuffle word, B = rows shuffled) and the
     * next rollout starts at S + epochs * (2 B + 2^20): every shuffle's start is known in
     * advance, so the host walks the epochs at once instead of speculating (a fraction of
     * the host CPU: what an 8-rank node can give each rank).  Self-play only. */
    int32_t shuffle_windows;
} bppo_config;

typedef struct {
    float total_reward[BPPO_MAX_PLAYERS];   /* players >= the env's NUM_PLAYERS: 0 */
    int32_t length;
    int32_t env_index;
    int32_t step;                /* rollout step t at which it ended */
    int32_t pad;
} bppo_episode;

typedef struct {
    int32_t episodes;            /* completed this rollout */
    float mean_return;           /* of player 0 */
    float mean_length;
    int32_t pad;
    uint64_t rng_word_pos;       /* main RNG position after the rollout */
} bppo_rollout_info;

/* The finished episodes of one rollout as mergeable statistics: what the reference's
 * "episode/..." scalars (main.rs:1134-1217) and compute_avg_points (env.rs:208-261) need, so a log
 * interval's scalars are the merge of its rollouts' blocks (add the sums and counts, take the
 * min of the minima and the max of the maxima).  Computed on the device from the rollout's
 * episode records (bppo_set_episode_stats).  P below = the seated player count (Skull:
 * player_count; CartPole: 1); slots >= P keep the identities.
 * Every field but return_sum is exact and independent of the order of the records.
 * return_sum is an f64 sum in the order of the device's record slots: exact whenever the
 * returns are integers (Connect Four, CartPole, the unshaped games); with shaped rewards its
 * last bits may differ from run to run, because the slots are handed out by atomics (within
 * n 2^-53 sum|x| of the exact sum, as any f64 sum of n terms).
 * No finished episode: the merge identities (length_min INT32_MAX, length_max 0, return_min
 * +inf, return_max -inf, sums 0). */
typedef struct {
    int32_t episodes;            /* finished this rollout (the device count) */
    int32_t kept;                /* of those, records kept and counted below: min(episodes, T N + 4096) */
    int32_t length_min, length_max;
    int64_t length_sum;
    int32_t with_outcome;        /* records whose env reported a game_outcome */
    int32_t draws;               /* of those: every seated placement is 1 */
    double return_sum[BPPO_MAX_PLAYERS];
    float return_min[BPPO_MAX_PLAYERS], return_max[BPPO_MAX_PLAYERS];
    int32_t outcome_games[BPPO_MAX_PLAYERS];   /* outcomes seat p took part in */
    /* twice the Swiss points of seat p: a game of n seats adds 2 n - 2 place - (tied - 1),
     * tied = the seats sharing place (env.rs:236-242 doubled: an exact integer) */
    int64_t points2_sum[BPPO_MAX_PLAYERS];
} bppo_episode_stats;

/* one episode of the last-100 window (main.rs:842-875) */
#define BPPO_EPISODE_TAIL 100
typedef struct {
    float total_reward[BPPO_MAX_PLAYERS];
    int32_t placement[BPPO_MAX_PLAYERS];    /* 1 = first; 0 beyond the seated players and without an outcome */
    int32_t length, env_index, step, has_outcome;
} bppo_episode_tail;

/* UpdateMetrics, ppo.rs:1342-1369 */
typedef struct {
    float policy_loss, value_loss, entropy, entropy_scaled, approx_kl, clip_fraction;
    float explained_variance, total_loss, value_mean, returns_mean;
    float adv_mean_raw, adv_std_raw, adv_min_raw, adv_max_raw;
    float value_error_mean, value_error_std, value_error_max;
    float avg_valid_actions, entropy_valid_pct;
    int32_t num_updates, epochs_run;
    /* PopArt (ppo.rs:2061-2068, 1799-1804): NaN when the reference's Option is None */
    float value_norm_target_mean, value_norm_target_std, value_norm_rescale_mag;
} bppo_update_metrics;

/* stats-mode evaluation (eval.rs:1621-1877), see bppo_evaluate */
typedef struct {
    int32_t num_games;           /* games to record */
    int32_t max_steps;           /* hard cap on loop iterations (VecEnv steps): BPPO_ERR_ARG beyond it */
    uint64_t seed;               /* StdRng::seed_from_u64(seed) of the evaluation */
    float temp_initial;          /* TempSchedule (eval.rs:110-216) */
    float temp_final;
    int32_t temp_cutoff;         /* move number of the cutoff; -1 = None (constant temp_initial) */
    int32_t temp_decay;          /* 1: linear decay initial -> final over temp_cutoff moves */
} bppo_eval_config;

/* one recorded game; indexed by checkpoint, not by seat (eval.rs:1798-1821) */
typedef struct {
    float total_reward[BPPO_MAX_PLAYERS];   /* checkpoints >= n_checkpoints: 0 */
    int32_t placement[BPPO_MAX_PLAYERS];    /* 1 = first; ties share a placement */
    int32_t length;              /* moves of the game */
    int32_t env_index;
    int32_t perm_index;          /* the seat permutation it was played under */
    int32_t step;                /* loop iteration at which it ended */
} bppo_eval_game;

/* one finished opponent-pool game (OpponentEpisodeCompletion, ppo.rs:505-521): the seats as
 * they were while the game was played, captured before the reshuffle (ppo.rs:871-917) */
typedef struct {
    int32_t env_index;
    int32_t step;                /* rollout step t at which it ended */
    int32_t learner_position;
    int32_t n_players;           /* the seated player count P */
    int32_t placement[BPPO_MAX_PLAYERS];              /* per seat, 1 = first; seats >= P: 0 */
    int32_t position_to_opponent[BPPO_MAX_PLAYERS];   /* device model index per seat; -1 on the
                                                       * learner's seat and on seats >= P */
} bppo_opp_completion;

typedef struct bppo_ctx bppo_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
/* hip_stream may be NULL (the context creates its own).  Resets the VecEnv
 * (VecEnv::new semantics, env.rs:281-302) and zero-initialises parameters. */
bppo_status bppo_create(const bppo_config *cfg, int hip_device, void *hip_stream, bppo_ctx **out);
void bppo_destroy(bppo_ctx *ctx);
const char *bppo_last_error(const bppo_ctx *ctx);
const char *bppo_version(void);
/* sizeof the ABI structs as this library was built: a binding (Rust #[repr(C)], ctypes)
 * asserts its own struct sizes against these before the first bppo_create */
size_t bppo_config_size(void);
size_t bppo_update_metrics_size(void);
size_t bppo_episode_size(void);
size_t bppo_rollout_info_size(void);
size_t bppo_eval_config_size(void);
size_t bppo_eval_game_size(void);
size_t bppo_opp_completion_size(void);

/* ---- ActorCritic -------------------------------------------------------- */
/* flat parameters in Burn record order: per Linear W[in][out] then b[out];
 * MLP: hidden..., policy head, value head; CTDE: actor hidden..., policy head,
 * critic hidden..., value head (mlp.rs:47-62, ctde.rs:26-44). */
size_t bppo_num_params(const bppo_ctx *ctx);
bppo_status bppo_params_set(bppo_ctx *ctx, const float *host, size_t n);
bppo_status bppo_params_get(bppo_ctx *ctx, float *host, size_t n);
/* forward on B rows of host obs [B*obs_dim] (+ priv [B*priv_dim] for CTDE) */
bppo_status bppo_forward(bppo_ctx *ctx, const float *obs, const float *priv, int32_t B,
                         float *logits, float *values);

/* ---- main RNG (StdRng = ChaCha12; state = seed key + word position) ------- */
bppo_status bppo_rng_get(bppo_ctx *ctx, uint64_t *word_pos);
bppo_status bppo_rng_set(bppo_ctx *ctx, uint64_t word_pos);
/* checkpoint.rs:390-400 save_rng_state: fill_bytes from the main RNG (ceil(n/4)
 * words, little-endian; advances the position like the reference's draw) */
bppo_status bppo_rng_fill_bytes(bppo_ctx *ctx, uint8_t *dst, size_t n);
/* checkpoint.rs:405-426 load_rng_state: the main RNG becomes StdRng::from_seed(seed[32]) */
bppo_status bppo_rng_from_seed(bppo_ctx *ctx, const uint8_t *seed);
bppo_status bppo_rng_key_get(bppo_ctx *ctx, uint32_t key[8]);

/* ---- optimizer (Adam) state, for checkpoint.rs save/load_optimizer ------- */
/* m1, m2 flat like the parameters; steps[bppo_num_param_tensors] = Adam time per
 * parameter tensor (W then b of every Linear, record order) */
size_t bppo_num_param_tensors(const bppo_ctx *ctx);
bppo_status bppo_optimizer_get(bppo_ctx *ctx, float *m1, float *m2, int32_t *steps, size_t n);
bppo_status bppo_optimizer_set(bppo_ctx *ctx, const float *m1, const float *m2, const int32_t *steps, size_t n);

/* ---- VecEnv ------------------------------------------------------------- */
bppo_status bppo_vecenv_reset(bppo_ctx *ctx);  /* VecEnv::new: factory(i) + reset() */
/* current state: obs [N*obs_dim] raw, players [N], masks [N*A] (0/1), priv [N*priv]; any may be NULL */
bppo_status bppo_vecenv_observe(bppo_ctx *ctx, float *obs, int32_t *players, uint8_t *masks,
                                float *priv);
/* VecEnv::step (env.rs:400-487): actions [N]; rewards [N*P]; dones [N];
 * completed episodes in env order (up to cap), count in *n_eps */
bppo_status bppo_vecenv_step(bppo_ctx *ctx, const int32_t *actions, float *obs, float *rewards,
                             uint8_t *dones, bppo_episode *eps, int32_t cap, int32_t *n_eps);
/* VecEnv::set_step (env.rs:329-333, main.rs:727): the step schedulable env
 * parameters are evaluated at (Liar's Dice shaping, liars_dice.rs:535, 635) */
bppo_status bppo_vecenv_set_step(bppo_ctx *ctx, uint64_t global_step);
/* reward_shaping_coef: Schedule (config.rs:761-762, schedule.rs:29-78) as n
 * (value, step) milestones, sorted by step as Schedule::parse_cli / Deserialize
 * leave them; replaces the constant config.reward_shaping_coef.  n = 0: empty
 * schedule (0.0).  BPPO_ERR_ARG when the initial value is < 0 (config.rs:1514). */
bppo_status bppo_set_reward_shaping_schedule(bppo_ctx *ctx, const double *values, const uint64_t *steps,
                                             int32_t n);

/* ---- normalizers (f64 state, normalization.rs) ------------------------ */
bppo_status bppo_obs_norm_get(bppo_ctx *ctx, double *mean, double *m2, double *count);
bppo_status bppo_obs_norm_set(bppo_ctx *ctx, const double *mean, const double *m2, double count);
/* mvc = {mean, M2, count}; returns = per (env, player) rolling returns [N*P] */
bppo_status bppo_ret_norm_get(bppo_ctx *ctx, double *mvc, double *returns);
bppo_status bppo_ret_norm_set(bppo_ctx *ctx, const double *mvc, const double *returns);
/* PopArtNormalizer state {mean, M2, count, epsilon} (normalization.rs:275-284) */
bppo_status bppo_popart_get(bppo_ctx *ctx, double *state4);
bppo_status bppo_popart_set(bppo_ctx *ctx, const double *state4);

/* ---- the hot path ------------------------------------------------------- */
bppo_status bppo_collect_rollouts(bppo_ctx *ctx, bppo_rollout_info *info);
bppo_status bppo_rollout_episodes(bppo_ctx *ctx, bppo_episode *eps, int32_t cap, int32_t *n);
/* the same episodes' game_outcome (env.rs:442-450, read before the auto-reset), in
 * bppo_rollout_episodes' order: placements [cap][6] per seat (1 = first; 0 beyond the seated
 * players and where the env reported no outcome: always for CartPole), has_outcome [cap];
 * either may be NULL; *n = the rollout's episode count.  Works with the statistics below on
 * or off. */
bppo_status bppo_rollout_episode_outcomes(bppo_ctx *ctx, int32_t *placements, int32_t *has_outcome, int32_t cap,
                                          int32_t *n);
/* Episode statistics on the device (off by default): enable != 0 makes every rollout from
 * now on, those bppo_train_steps pipelines included, leave its bppo_episode_stats and its
 * last BPPO_EPISODE_TAIL episodes beside its bppo_rollout_info: up to five small kernels over
 * the episode records and a larger copy of the same pinned slot; no record crosses PCIe.
 * Off, nothing is launched or copied that is not without this call. */
bppo_status bppo_set_episode_stats(bppo_ctx *ctx, int32_t enable);
/* rollout k of the last hot-path call: 0 for bppo_collect_rollouts / bppo_train_step, 0..n-1
 * for bppo_train_steps.  A rollout bppo_train_steps ran ahead and an error left pending is
 * not part of the failed call: it is entry 0 of the call that consumes it.  tail receives the
 * first min(tail_cap, *n_tail) of the rollout's last min(100, kept) episodes, oldest first in
 * the reference's push order (step, then env index): pushed in that order into 100-deep
 * deques they leave what main.rs:842-875 keeps.  out, tail, n_tail may be NULL.
 * BPPO_ERR_ARG with a message: the statistics are off, k is out of range, or no rollout has
 * run since they were switched on.  Reads host memory only: no HIP call. */
bppo_status bppo_episode_stats_get(bppo_ctx *ctx, int32_t k, bppo_episode_stats *out, bppo_episode_tail *tail,
                                   int32_t tail_cap, int32_t *n_tail);
size_t bppo_episode_stats_size(void);
size_t bppo_episode_tail_size(void);
bppo_status bppo_compute_gae(bppo_ctx *ctx);
bppo_status bppo_ppo_update(bppo_ctx *ctx, double lr, double ent_coef, bppo_update_metrics *m);
/* the three calls above as one (main.rs:860-947 then ppo.rs:1661-2112): enqueued back to
 * back with one host wait at the end; the rollout's error statuses are reported after
 * the update (info may be NULL) */
bppo_status bppo_train_step(bppo_ctx *ctx, double lr, double ent_coef, bppo_rollout_info *info,
                            bppo_update_metrics *m);
/* n bppo_train_step iterations (main.rs:684-988 loop body, lr[k] / ent_coef[k], env step
 * global_step0 + k*T*N*world_size), software-pipelined: each iteration's rollout is enqueued behind the
 * previous update before the host waits for that update, so the GPU does not idle between
 * iterations.  Same results as n bppo_train_step calls; the stream is drained on return.
 * After an error status the next iteration's rollout may already have run (the RNG and
 * the envs are past it): it stays the context's next rollout, which bppo_collect_rollouts,
 * bppo_train_step and bppo_train_steps use instead of drawing another one (bppo_compute_gae
 * consumes it too).  A setter of the state it was drawn with (bppo_params_set,
 * bppo_rng_set / _from_seed, bppo_obs_norm_set, bppo_ret_norm_set, bppo_popart_set,
 * bppo_vecenv_reset) discards it; the next rollout is then drawn anew (bppo_optimizer_set
 * keeps it: a rollout does not read the Adam moments).
 * infos / ms: n entries each (may be NULL); phase_keys (bppo_last_kernel_ms names, nkeys of
 * them): per-key sums over the n iterations into phase_sums */
bppo_status bppo_train_steps(bppo_ctx *ctx, int32_t n, const double *lr, const double *ent_coef,
                             uint64_t global_step0, bppo_rollout_info *infos, bppo_update_metrics *ms,
                             const char *const *phase_keys, int32_t nkeys, float *phase_sums);

/* multi-GPU: called once per minibatch with the flat f32 gradient (+ metric
 * partials) in DEVICE memory, on the context's stream, before clip + Adam.
 * The callback must leave the SUM over ranks in place; the context divides
 * by world_size.  (RCCL all-reduce over xGMI, one per minibatch.) */
typedef int (*bppo_allreduce_fn)(float *device_buf, size_t n, void *user);
/* W = world_size > 1 semantics (the reference is single-process; DESIGN.md section 7,
 * pinned by tests/test_gpu_multirank.py against the oracle's W-rank update): each rank's
 * gradient is the mean over its own minibatch rows with its own advantage normalization;
 * the SUM over ranks is scaled by 1/W before clip + Adam, so all ranks take the same step.
 * The metric partials ride along, so the UpdateMetrics are those of all ranks' rows
 * together, except value_error_max, adv_*_raw and explained_variance, which stay per rank.
 * normalize_values (PopArt) at W > 1: every rank's running return statistics absorb ALL
 * ranks' returns, rank by rank in rank order (each rank's batch statistics travel through
 * the same callback as an exact all-gather), so the value-head rescale and the normalized
 * targets are identical on every rank; needs bppo_set_rank.  Opponent pools at W > 1: each
 * rank trains on its own learner rows, cut into num_minibatches of its own sizes; the
 * minibatch slots run in lockstep (one callback each), a rank without rows in a slot
 * contributing a zero gradient and zero metric partials (its value_error_max for the slot is
 * -inf).  The SUM is scaled by 1/W in every slot, empty contributions included, so a slot
 * that some ranks have no rows for takes a proportionally smaller step (the oracle's
 * or_trainers_update does the same). */
bppo_status bppo_set_allreduce(bppo_ctx *ctx, bppo_allreduce_fn fn, void *user, int32_t world_size);
/* this context's rank among the all-reduce's world_size ranks (0-based; unset by default):
 * the slot of its PopArt batch statistics in the W > 1 all-gather.  Required for
 * normalize_values at W > 1: an update without it returns BPPO_ERR_ARG, and so does one whose
 * gathered statistics show two contexts in one slot (a duplicated rank) */
bppo_status bppo_set_rank(bppo_ctx *ctx, int32_t rank);

/* stream-ordered variant: fn is called WITHOUT draining the stream, right after
 * the minibatch's gradient kernels are enqueued; it must enqueue the SUM
 * all-reduce of device_buf on the context's stream (bppo_get_stream) and
 * return.  Clip + Adam are enqueued after it, so the host never waits per
 * minibatch (replaces the ncclAllReduce-on-stream call a Rust host would make
 * in ppo.rs's update loop; the reference has no multi-GPU path). */
bppo_status bppo_set_allreduce_async(bppo_ctx *ctx, bppo_allreduce_fn fn, void *user, int32_t world_size);
bppo_status bppo_get_stream(bppo_ctx *ctx, void **hip_stream);

/* Opponent-pool training (multi-player envs): replaces collect_rollouts_with_opponents
 * (ppo.rs:537-1063) and the learner-row filter of ppo_update (ppo.rs:165-180,
 * 1696-1753).  The host keeps the pool (OpponentPool, opponent_pool.rs: checkpoint
 * loading, win-rate sampling, rotation) and hands over the loaded models:
 *   n_models (<= 15) parameter vectors of the learner's architecture, packed
 *   [n_models][n_params]; per model an optional observation normalizer
 *   (norm_mean/norm_m2 [n_models][obs_dim], norm_count [n_models]; count < 2 or
 *   NULL arrays = none);
 *   envs [0, num_opponent_envs) play against them (main.rs:621-637), with seat
 *   state learner_pos [num_opponent_envs] and pos_to_opp [num_opponent_envs][P]
 *   (model index per seat, -1 on the learner's seat) (EnvState, opponent_pool.rs:80-124);
 *   current_opp [P - 1]: OpponentPool::sample_all_slots, the models a finished game
 *   is given before its seats are reshuffled from the main RNG.  P here is the
 *   seated player count (main.rs:552: Skull's player_count, else NUM_PLAYERS).
 * Opponent batches sample in ascending model index (the reference iterates a
 * HashMap, whose order is unspecified).  num_opponent_envs = 0 switches it off.
 * Buffer "valid" holds the learner-turn flags of the last rollout; ppo_update
 * trains on those rows only. */
bppo_status bppo_opponents_set(bppo_ctx *ctx, int32_t n_models, const float *params, const double *norm_mean,
                               const double *norm_m2, const double *norm_count, int32_t num_opponent_envs,
                               const int32_t *learner_pos, const int32_t *pos_to_opp, const int32_t *current_opp);
/* the seat state after the last rollout's reshuffles */
bppo_status bppo_opponents_get_envs(bppo_ctx *ctx, int32_t *learner_pos, int32_t *pos_to_opp);
/* opponent_completions of the last rollout (ppo.rs:505-521, 871-917): every finished game of
 * the envs [0, num_opponent_envs) whose env reported a game_outcome, with the placements and
 * the seats it was played under, in the reference's order (step, then env index).  The
 * rollout keeps as many records as it keeps episodes (num_envs * num_steps + 4096);
 * games past that are counted but not kept.  out receives the first min(cap, recorded)
 * records, *n = how many were recorded, *dropped = how many did not fit (either may be NULL;
 * out may be NULL when cap is 0).  The records belong to the rollout bppo_rollout_episodes
 * describes: a rollout bppo_train_steps ran ahead replaces both, bppo_opponents_set empties
 * both, and a state setter that discards a pending rollout empties the records.
 * BPPO_ERR_ARG when no opponents are set. */
bppo_status bppo_opponents_completions(bppo_ctx *ctx, bppo_opp_completion *out, int32_t cap, int32_t *n,
                                       int32_t *dropped);
/* OpponentPool::queue_game_result (opponent_pool.rs:578-616) summed over those games, dropped
 * ones included, per device model slot [n_models]: games = one per (game, opponent seat),
 * wins = those where the learner placed better than that seat, swiss_points = the learner's
 * P - placement added once per opponent seat.  Integers, so exact in any order; any array
 * may be NULL.  (main.rs:755-803 feeds them to apply_pending_win_rate_updates.)
 * BPPO_ERR_ARG when no opponents are set. */
bppo_status bppo_opponents_results(bppo_ctx *ctx, int32_t *wins, int32_t *games, int64_t *swiss_points);

/* Stats-mode evaluation on the device (eval.rs:1621-1877 run_stats_mode_env, the engine of
 * `eval --num-games` and of the tournament pods): plays cfg->num_games games between
 * checkpoints on this context's VecEnv (num_envs parallel games), sampling every move with
 * the temperature schedule (sample_with_temperature, eval.rs:223-272) and rotating the
 * seats over all permutations of the players (Heap's algorithm order, eval.rs:1591-1612;
 * env e starts on permutation e % n!, the next one after each game it records).
 * Multi-player contexts only (Connect Four, Liar's Dice, Skull; MLP, CTDE or CNN nets);
 * CartPole returns BPPO_ERR_UNSUPPORTED.
 *   models as in bppo_opponents_set: n_models (<= 15) parameter vectors of the context's
 *   architecture [n_models][n_params] with optional obs normalizers (count < 2 or NULL
 *   arrays = none); is_random [n_models] (may be NULL): 1 = the reference's None model,
 *   all-zero logits (eval.rs:1749-1752), its parameters are not read;
 *   seat_model [n_checkpoints] = checkpoint_to_model; n_checkpoints must equal the seated
 *   player count (the reference's permutations cover 0..num_players only).
 * RNG: StdRng(cfg->seed); its first u64 seeds the envs (env i = E::new(base + i), then the
 * two resets of VecEnv::new and set_all_num_players), the sampling draws follow from word 2:
 * per step models in ascending index, within a model its envs in ascending index, one word
 * per draw; a move at temperature 0 draws nothing.  *rng_word_pos = the position after.
 * games [cap] receives the recorded games in completion order (step, then env index),
 * *n_games their count.  The loop ends at num_games games (excess envs are frozen as the
 * reference does, eval.rs:1839-1869) or when no env is active; more than cfg->max_steps
 * iterations is an error (one small host read per step; nothing spins without a bound).
 * The call resets and overwrites the context's VecEnv and episode state and discards a
 * pending pipelined rollout, like the state setters: give evaluation a context of its
 * own with num_envs = the evaluation envs.  Parameters, optimizer, normalizers and the
 * context's main RNG are not touched. */
bppo_status bppo_evaluate(bppo_ctx *ctx, const bppo_eval_config *cfg, int32_t n_models, const float *params,
                          const double *norm_mean, const double *norm_m2, const double *norm_count,
                          const int32_t *is_random, const int32_t *seat_model, int32_t n_checkpoints,
                          bppo_eval_game *games, int32_t cap, int32_t *n_games, uint64_t *rng_word_pos);

/* Many evaluation matchups ("pods") in one loop: a tournament round.  Pod k owns envs
 * [k E, (k + 1) E), E = envs_per_pod; the context's num_envs must equal n_pods * E.  Only the
 * forward pass is shared: the rows one model moves in every pod go through one GEMM group.
 * Multi-player contexts only; CartPole returns BPPO_ERR_UNSUPPORTED.
 *   models as in bppo_evaluate with n_models 1..64; n_pods 1..1024; cfg->seed is ignored;
 *   pod_seeds [n_pods]; pod_seat_model [n_pods][P], P = the seated player count: within pod k
 *   checkpoint c is played by global model pod_seat_model[k][c].  A model's local slot in a
 *   pod is the rank of its first appearance in pod_seat_model[k][0..P) (run_pod's
 *   de-duplication, tournament.rs:1811-1838): seats [3, 1, 3] give local models [m3, m1]
 *   and the local seat map [0, 1, 0].
 * Pod k equals, in every recorded field and in its final word position, bppo_evaluate alone
 * on a context of E envs with cfg->seed = pod_seeds[k], the pod's local models in local-slot
 * order and the local seat map:
 *   RNG StdRng(pod_seeds[k]); its first u64 seeds the pod's envs (env j of the pod =
 *   E::new(base_k + j), then the two resets); draws follow from word 2, per step over the
 *   pod's models in ascending local slot, within a model over the pod's envs in ascending
 *   index, one word per draw, none at temperature 0;
 *   the permutation rotation starts at j % n!; the num_games cap and the freeze rule
 *   (eval.rs:1839-1869) apply per pod;
 *   games [n_pods][cap_per_pod]: pod k's games in completion order (step, then env) at
 *   games[k * cap_per_pod ...], env_index the index within the pod, step the shared loop
 *   iteration (all pods start at iteration 0, so it is the single call's);
 *   n_games [n_pods], rng_word_pos [n_pods] (may be NULL).
 * This departs from the reference, which hands one StdRng from pod to pod (pod k + 1 starts
 * where pod k ended, tournament.rs:2151-2184); that order is bppo_evaluate pod after pod.
 * The loop ends when every pod has num_games games or no active env; a finished pod's envs
 * are frozen.  A pod unfinished after cfg->max_steps iterations: BPPO_ERR_ARG ("max_steps").
 * BPPO_ERR_ARG with a message, before any launch: NULL pod_seeds, pod_seat_model or n_games;
 * n_pods * envs_per_pod != num_envs; a seat naming a model outside [0, n_models); n_models
 * outside 1..64; n_pods outside 1..1024; missing params when some model is not random.
 * Side effects on the context as for bppo_evaluate. */
bppo_status bppo_evaluate_pods(bppo_ctx *ctx, const bppo_eval_config *cfg, int32_t n_models, const float *params,
                               const double *norm_mean, const double *norm_m2, const double *norm_count,
                               const int32_t *is_random, int32_t n_pods, int32_t envs_per_pod,
                               const uint64_t *pod_seeds, const int32_t *pod_seat_model, bppo_eval_game *games,
                               int32_t cap_per_pod, int32_t *n_games, uint64_t *rng_word_pos);

/* Single-player stats mode: run_stats_mode_env::<CartPole> (eval.rs:1621-1877) with one
 * checkpoint, n_pods times in one launch sequence; its summary is
 * EvalStats::print_single_player_summary (eval.rs:416-469).  Pod k plays cfg->num_games episodes
 * of params[k] on envs_per_pod envs with its own StdRng(pod_seeds[k]); cfg->seed is not read.
 * One thread block plays a whole pod (csrc/eval_cartpole.hip), so a single pod uses one CU and
 * the GPU fills through pods: every checkpoint of a run, or one checkpoint under many seeds.
 * Contexts: CartPole with a net the fused kernels cover (hidden {16, 32, 64} x {1, 2} layers,
 * relu or tanh, no split_networks).  Any other CartPole net: BPPO_ERR_UNSUPPORTED; any other
 * env: BPPO_ERR_UNSUPPORTED (those are bppo_evaluate's and bppo_evaluate_pods').
 *   n_pods 1..1024; envs_per_pod 1..16384, independent of the context's num_envs;
 *   params [n_pods][n_params] of the context's net; norm_mean / norm_m2 [n_pods][5], norm_count
 *   [n_pods]: any NULL array, or count < 2, = raw observations (eval.rs:1727-1734);
 *   steps_per_launch: loop iterations per kernel launch, 0 = the default (256 / envs per
 *   thread, at least 1: a launch of about 20 ms or less); results do not depend on it.
 * Semantics per pod:
 *   RNG StdRng(pod_seeds[k]); base = its first u64, words 0 and 1 (eval.rs:1646-1648); env j =
 *   CartPole::new(base + j), reset again by VecEnv::new and by set_all_num_players (cartpole.rs:104,
 *   env.rs:289-293, 313-326): three resets from the env's own stream; draws follow from word 2;
 *   per iteration, while games < num_games and an env is active (eval.rs:1670-1674): every
 *   active env in env order samples at TempSchedule::get_temp of its move count with no mask
 *   (eval.rs:1766, 223-272; the argmax takes the last of equal maxima; one word per draw, none at
 *   temperature 0), steps, and on done records {total, length} and resets from its own stream
 *   (env.rs:400-487); move counts advance for every env, frozen ones included (eval.rs:1775-1777);
 *   finished episodes are recorded in env order up to num_games (eval.rs:1783-1831):
 *   total_reward[0] the total, placement[0] = 1, other slots 0, length, env_index within the
 *   pod, perm_index 0, step the iteration; a recorded env's move count returns to 0, an episode
 *   past the cap is dropped; then the freeze rule (eval.rs:1839-1869).
 *   games [n_pods][cap_per_pod], n_games [n_pods], rng_word_pos [n_pods] (nullable),
 *   loop_steps [n_pods] (nullable): the iterations the pod ran.  num_games = 0 runs no
 *   iteration and leaves position 2.
 * A pod unfinished after cfg->max_steps iterations: BPPO_ERR_ARG ("max_steps"); n_games,
 * rng_word_pos, loop_steps and the games so far are still written.
 * The call reads the context for the net shape, activation, stream and error slot only: its
 * VecEnv, RNG, parameters, optimizer, normalizers, rollout buffers and a pipelined prefetched
 * rollout are not touched (unlike bppo_evaluate, which resets the VecEnv).  All device memory of
 * the call is allocated by it and freed when it ends. */
bppo_status bppo_evaluate_episodes(bppo_ctx *ctx, const bppo_eval_config *cfg, int32_t n_pods, int32_t envs_per_pod,
                                   const float *params, const double *norm_mean, const double *norm_m2,
                                   const double *norm_count, const uint64_t *pod_seeds, int32_t steps_per_launch,
                                   bppo_eval_game *games, int32_t cap_per_pod, int32_t *n_games,
                                   uint64_t *rng_word_pos, int32_t *loop_steps);

/* ---- Plackett-Luce ratings (plackett_luce.rs) ----------------------------- */
/* A rating table is an object of its own, not part of a context: a tournament's or a training
 * run's ratings outlive any one evaluation context.  Games and their expanded comparisons stay in
 * device memory between calls; a fit only iterates.  Not thread-safe. */
typedef struct {            /* PlackettLuceConfig, plackett_luce.rs:102-127 */
    int32_t max_iterations;  /* 100 */
    int32_t backend;         /* 0 = device, 1 = host: the reference's arithmetic in its order */
    double convergence_threshold, epsilon, anchor_elo, ci_inflation_factor;  /* 1e-6, 1e-10, 1000, 1.3 */
} bppo_pl_config;
typedef struct {            /* RatingStats, plackett_luce.rs:80-89 */
    int32_t converged, iterations_used;
    double final_delta;
    double fit_ms;           /* wall time of the call */
    int64_t n_games, n_comparisons;
} bppo_pl_stats;
typedef struct bppo_ratings bppo_ratings;

/* hip_device = -1: a host-only table (no GPU is touched; only backend 1 fits it).  hip_stream may
 * be NULL (the table creates its own). */
bppo_status bppo_ratings_create(int hip_device, void *hip_stream, bppo_ratings **out);
void        bppo_ratings_destroy(bppo_ratings *r);
const char *bppo_ratings_last_error(const bppo_ratings *r);
bppo_status bppo_ratings_clear(bppo_ratings *r);
/* append n games of at most P (1..6) players: players [n][P] (player ids >= 0, -1 pads a shorter
 * game at its end), placements [n][P] (1 = first, ties share; ignored where players is -1),
 * weight [n] or NULL (= 1): a game listed once with weight w counts as w identical games.
 * BPPO_ERR_ARG (nothing is appended): P outside 1..6, an id < -1, an id after a -1 in its row,
 * a placement < 1, a non-finite or non-positive weight. */
bppo_status bppo_ratings_add_games(bppo_ratings *r, int64_t n, int32_t P, const int32_t *players,
                                   const int32_t *placements, const double *weight);
/* append the kept opponent completions of ctx's last rollout straight from the device records
 * (main.rs:755-790): game = [learner_player, slot_to_player[position_to_opponent[seat]] for the
 * opponent seats in seat order], placements = rating_placements (ppo.rs:890-897); a game whose
 * opponents all equal learner_player is skipped (main.rs:779-782).  *added = games appended, in
 * record order.  ctx must be on the table's device (else BPPO_ERR_ARG).  The call is ordered after
 * the context's stream and waits on the host only for its own kernels, to read *added. */
bppo_status bppo_ratings_add_completions(bppo_ratings *r, bppo_ctx *ctx, int32_t learner_player,
                                         const int32_t *slot_to_player, int32_t n_slots, int64_t *added);
bppo_status bppo_ratings_num_games(const bppo_ratings *r, int64_t *n);
/* compute_ratings (plackett_luce.rs:437-614): rating / uncertainty [num_players] on the Elo
 * scale, gamma [num_players] (centred log-strengths before the anchor shift; may be NULL).
 * Two fits of one table give identical bits, however the games were split over the add calls.
 * BPPO_ERR_ARG before any launch: anchor outside [0, num_players), a stored player id
 * >= num_players, num_players > 1024, backend 0 on a host-only table.
 * The covariance inversion (invert_matrix, :361-425) runs on the host for both backends. */
bppo_status bppo_ratings_fit(bppo_ratings *r, const bppo_pl_config *cfg, int32_t num_players, int32_t anchor,
                             double *rating, double *uncertainty, double *gamma, bppo_pl_stats *stats);
/* wall time (ms) of the last fit's phases, for scripts/bench_ratings.py: ms4 = {incidence list
 * (backend 1: the expansion), MM iterations, Fisher information with its copy to the host, the
 * host inversion + Elo conversion}; an early return leaves them as they were */
bppo_status bppo_ratings_last_fit_phases(const bppo_ratings *r, double *ms4);
size_t bppo_pl_config_size(void);
size_t bppo_pl_stats_size(void);

/* parity hooks: export / import a RolloutBuffer field.  names: "obs", "priv",
 * "actions" (i32), "rewards", "dones", "values", "log_probs", "advantages",
 * "returns", "players" (i32), "all_rewards", "masks", "last_v_pp", "perm" (u32,
 * last epoch's shuffled indices), "grad" (the last minibatch's gradient); export only,
 * multi-player nets: "hidden:<l>" = FC hidden layer l's activations of the last forward
 * ([rows_max][width] f32, rows_max = max(num_envs, ceil(T N / num_minibatches)); the last
 * minibatch's rows in "perm" order -- the device's ReLU decisions for
 * tests/test_gpu_gemm_split.py) */
/* the last update's per-minibatch metric rows in run order (parity diagnosis: which
 * minibatch's statistics first leave the bar): row k = the minibatch's sums
 * [policy_loss, 2*value_loss, entropy, approx_kl, clip_fraction, value, return, |v-R|,
 * (v-R)^2, max |v-R|, rows, ...] then 4 advantage statistics; returns the row count,
 * copies up to max_rows rows of *row_width floats into out (may be NULL) */
int32_t bppo_minibatch_rows(bppo_ctx *ctx, float *out, int32_t max_rows, int32_t *row_width);
bppo_status bppo_buffer_get(bppo_ctx *ctx, const char *name, void *host, size_t bytes);
bppo_status bppo_buffer_set(bppo_ctx *ctx, const char *name, const void *host, size_t bytes);

/* ---- standalone device kernels on caller-owned DEVICE buffers ------------ */
/* compute_gae (ppo.rs:1069-1124) on [T,N] device arrays; stream may be NULL */
bppo_status bppo_gae_device(const float *rewards, const float *dones, const float *values,
                            const float *last_values, int32_t T, int32_t N, float gamma,
                            float lambda, float *advantages, float *returns, void *hip_stream);
/* the same, plus the [advantage, return] pair of every row, pairs [T*N][2] floats (row
 * t*N+e), as the update path writes them for its minibatch gathers;
 * BPPO_ERR_UNSUPPORTED unless N % 4 == 0, T <= 128 and the arrays are 16-byte aligned */
bppo_status bppo_gae_rows_device(const float *rewards, const float *dones, const float *values,
                                 const float *last_values, int32_t T, int32_t N, float gamma,
                                 float lambda, float *advantages, float *returns, float *pairs,
                                 void *hip_stream);
/* compute_gae_multiplayer (ppo.rs:1140-1264): all_rewards [T,N,P], players [T,N] i32,
 * last_v_pp [N,P] */
bppo_status bppo_gae_mp_device(const float *all_rewards, const int32_t *players,
                               const float *dones, const float *values, const float *last_v_pp,
                               int32_t T, int32_t N, int32_t P, float gamma, float lambda,
                               float *advantages, float *returns, void *hip_stream);

/* UpdateMetrics.explained_variance (ppo.rs:1268-1294): mode 0 (default) = f64 sums on the
 * device (within 1e-6 of the exact value; the reference's f32 sums drift ~1e-3 at 10^6
 * rows); mode 1 = the reference's own arithmetic, bit for bit: four sequential f32 sums
 * over the buffer, on a host thread from device->host copies made beside the update
 * (it waits for them at the update's end: ~10 ms of one CPU per 8.4 M rows) */
bppo_status bppo_set_explained_variance_mode(bppo_ctx *ctx, int32_t mode);

/* which minibatch kernels run (a parity / A-B hook).  CartPole's 2x64 relu MLP (CfgB):
 * mode 0 (default) runs the update's first minibatch on the exact f32 kernel (it runs with
 * the rollout's parameters, so the ratio is exactly 1 and the forward equals the rollout's
 * bit for bit) and every later one on the f32-accurate split-bf16 kernel; 1 the exact kernel
 * for every minibatch; 2 the split kernel for every minibatch, the first included (its
 * gradient from the rollout's parameters can then be compared with the oracle's,
 * tests/test_gpu_split_kernel.py).  The GEMM path (Connect Four, Liar's Dice, Skull, other
 * nets; wide_api.hip wide_minibatch):
 *   mode 0 (default), minibatches below 32,768 rows (WIDE_SPLIT_MIN_ROWS): the exact forward
 *     and input-gradient f32 chains, weight gradients summed in f64 on the f64 MFMA;
 *     from 32,768 rows, MLP / CTDE nets: the update's first minibatch keeps the exact forward
 *     (ratio exactly 1) and runs its backward (input and weight gradients) on the split-bf16
 *     contraction, every later minibatch runs all its GEMMs split; CNN nets: the exact
 *     chains with f32 split-K weight gradients;
 *   mode 1: the exact chains, weight gradients in f64 row by row in order (the oracle's
 *     arithmetic exactly; a latency-bound parity mode);
 *   mode 2: MLP / CTDE nets run every minibatch's forward and backward on the split-bf16
 *     contraction (the first included); CNN nets the exact chains with f32 split-K weight
 *     gradients. */
bppo_status bppo_set_minibatch_kernel(bppo_ctx *ctx, int32_t mode);

/* parity hook: while host != NULL, every bppo_ppo_update copies the parameters it runs each
 * minibatch with (the first max_minibatches in run order) to host[k * num_params], so each
 * minibatch's statistics can be recomputed from the device's own parameters at any size
 * (tests/test_gpu_fullsize.py); "perm_ep:<e>" (bppo_buffer_get) is epoch e's permutation */
bppo_status bppo_debug_record_params(bppo_ctx *ctx, float *host, int32_t max_minibatches);

/* device timing of the last call of each phase kernel (ms), for bench.py's roofline */
bppo_status bppo_last_kernel_ms(bppo_ctx *ctx, const char *kernel, float *ms);

/* libm parity hook: which 0 = logf, 1 = sinf, 2 = cosf, 3 = gumbel(-ln(-ln u)), 4 = expf, 5 = tanhf;
 * device = 0 runs the host build of the same source, 1 runs the HIP kernel */
bppo_status bppo_debug_libm(int32_t which, int32_t device, const float *x, float *y, size_t n);

/* Device and pinned host allocations the library holds in this process, and their bytes
 * (contexts, rating tables and calls in flight; not the shuffle engine's own buffers).
 * No HIP call: works without a GPU.  Both return to their earlier values when what was
 * created since is destroyed. */
bppo_status bppo_debug_device_memory(int64_t *live_allocations, int64_t *live_bytes);

/* The update's metric fold alone: rows[nup][row_width] as bppo_minibatch_rows returns them
 * (one row per minibatch that ran) -> *out, by the function bppo_ppo_update itself calls.
 * B: the rows the update trained on; ev4: sum R, sum R^2, sum (R - V), sum (R - V)^2 over
 * them in f64 (explained variance), or ev_mode = 1 and the value to report in ev_ref; the
 * pa_* fields are PopArt's target sums, read when normalize_values != 0.
 * No HIP call: works without a GPU. */
typedef struct {
    float value_coef, ent_coef;
    int32_t A, env_kind;         /* action count; BPPO_ENV_* */
    uint64_t B;
    double ev4[4];
    int32_t ev_mode;
    float ev_ref;
    int32_t epochs_run, normalize_values;
    double pa_tsum, pa_tsq, pa_tcount;
    float pa_rescale_mag;
} bppo_debug_fold_args;
bppo_status bppo_debug_fold_metrics(const float *rows, int32_t nup, const bppo_debug_fold_args *args,
                                    bppo_update_metrics *out);

/* shuffle parity hooks (ppo.rs:1816, rand 0.8.5 SliceRandom::shuffle on StdRng):
 * the host draw chain alone — J[i] = gen_range(0..i+1) for i = n-1..1 from word
 * position word_pos of StdRng(seed) stream `stream`, *end_pos = position after —
 * and the device Fisher-Yates permutation of 0..n-1 for given swap targets J */
bppo_status bppo_debug_shuffle_chain(uint64_t seed, uint64_t stream, uint64_t word_pos, uint32_t n,
                                     uint32_t *J, uint64_t *end_pos);
bppo_status bppo_debug_fisher_yates(int32_t device, const uint32_t *J, uint32_t n, uint32_t *perm);
/* host only: two draw chains of n (from word positions pos_a, pos_b) walked together by
 * the interleaved two-chain walker the shuffle_windows engine uses, over words handed
 * over in pieces ending at multiples of `piece` words; *end_a / *end_b = the positions
 * after each shuffle (must equal bppo_debug_shuffle_chain's) */
bppo_status bppo_debug_chain_walk2(uint64_t seed, uint64_t stream, uint64_t pos_a, uint64_t pos_b, uint32_t n,
                                   uint32_t piece, uint64_t *end_a, uint64_t *end_b);
/* the whole shuffle engine (GPU-made ChaCha words, speculative walks, J rebuilt on
 * the GPU) for `jobs` updates of `epochs` shuffles of n: the first from word
 * position start, each next update `gap` words after the previous one's last
 * shuffle.  J [jobs][epochs][n], end word positions [jobs][epochs], met = checkpoints
 * walked before meeting a speculative walk (-1 = none; may be NULL).  Must equal
 * chained shuffle_chain calls.  windows = 1: the shuffle_windows layout (epoch e of
 * an update from its start + e * (2 n + 2^20), the next update gap words after its
 * start + epochs * (2 n + 2^20)): must equal shuffle_chain calls from those starts. */
bppo_status bppo_debug_shuffle_engine(uint64_t seed, uint64_t stream, uint64_t start, uint32_t n, int32_t epochs,
                                      uint64_t gap, int32_t jobs, int32_t windows, uint32_t *J, uint64_t *ends,
                                      int32_t *met);

/* sampling parity hook: apply_action_mask + sample_categorical + log_prob_categorical
 * (utils.rs:10-45, 96-135) for B host rows of A logits (A in {2, 7, 49}) on the device
 * sampler; Gumbel words from StdRng(seed) stream `stream` at word_pos, row-major;
 * masks [B*A] 0/1 or NULL.  Returns BPPO_ERR_EMPTY_MASK for a row with no valid
 * action (the reference panics, utils.rs:115-123) and BPPO_ERR_NONFINITE for a
 * non-finite log-prob (ppo.rs:363-366). */
bppo_status bppo_debug_sample(int32_t A, int32_t B, const float *logits, const uint8_t *masks, uint64_t seed,
                              uint64_t stream, uint64_t word_pos, int32_t *actions, float *log_probs);

/* evaluation parity hooks.  sample_with_temperature (eval.rs:223-272) for B host rows of A
 * logits (A in {7, 33, 49}), masks [B*A] 0/1, one temperature per row; the rows' draws are
 * taken in row order from word_pos of StdRng(seed) stream `stream`, one word each, rows at
 * temperature 0 draw nothing; draws_used [B] (may be NULL) = 1 where a row drew.  device = 0
 * runs the host build of the same source, 1 the HIP kernel. */
bppo_status bppo_debug_eval_sample(int32_t device, int32_t A, int32_t B, const float *logits, const uint8_t *masks,
                                   const float *temps, uint64_t seed, uint64_t stream, uint64_t word_pos,
                                   int32_t *actions, int32_t *draws_used);
/* episode statistics parity hook (host buffers, no context): the statistics and the tail of n
 * episode records as a rollout of T steps of N envs with P seated players would report them.
 * outcome_words [n] (NULL = no outcomes): placement of seat p in bits [4p, 4p + 4), bit 24 =
 * the env reported an outcome.  device = 0 runs the host build of the same source (a loop and
 * a sort), 1 the kernels on an uploaded copy.  tail [100], *n_tail = min(100, n).
 * BPPO_ERR_ARG before any HIP call: n < 0, P outside 1..6, T or N < 1, a NULL eps with n > 0,
 * a NULL out / tail / n_tail, a record whose step is outside [0, T) or env_index outside
 * [0, N), or two records with one (step, env_index). */
bppo_status bppo_debug_episode_stats(int32_t device, int32_t n, const bppo_episode *eps, const int32_t *outcome_words,
                                     int32_t P, int32_t N, int32_t T, bppo_episode_stats *out,
                                     bppo_episode_tail *tail, int32_t *n_tail);
/* generate_permutations (eval.rs:1591-1612): out [n!][n], n in 1..6 */
bppo_status bppo_debug_eval_perms(int32_t n, int32_t *out);

/* GEMM engine parity hook (host buffers).  mode 0: out[M][N] = act(A[M][K] B[K][N] + bias[N])
 * with matrixmultiply's KC=256 fma-chain order (Burn Linear forward, mlp.rs:140-206);
 * (act: 0 none, 1 relu, 2 tanh); mode 1: out[M][N] = (A[M][K] B[N][K]^T) * act'(H) with H = bias_or_H
 * the layer output (may be NULL): act 2 -> (1 - H^2), otherwise [H > 0];
 * mode 2: out[M][N] = A[K][M]^T B[K][N] (weight gradient), out2[N] = column sums of B */
bppo_status bppo_debug_gemm(int32_t mode, int32_t M, int32_t N, int32_t K, const float *A, const float *B,
                            const float *bias_or_H, int32_t act, float *out, float *out2);
/* ReturnNormalizer parity hook (host buffers, no context): the kernels and launch order of a
 * rollout's return normalization (normalization.rs:156-197, ppo.rs:388-428) over T steps of N
 * envs.  For t ascending, e ascending: the acting player's rolling return R = R gamma + r; a
 * valid row pushes R into the Welford statistics; rew = r / sqrt(m2 / n + 1e-8) clamped to
 * +-clip once n >= 2, the raw r before; a done step resets that player's return (valid or not).
 * players NULL: the single-player kernel (P must be 1, valid and all_rewards NULL); otherwise the
 * per-player kernel, and with all_rewards the acting player's slot of each row becomes rew, the
 * other slots stay.  valid NULL: every row counts.  stats3 = {mean, m2, count} as
 * bppo_ret_norm_get gives them.  BPPO_ERR_ARG (before any HIP call) for T or N < 1, P outside
 * 1..BPPO_MAX_PLAYERS or a NULL rew_raw / done / returns_state / stats3 / rew. */
bppo_status bppo_debug_return_norm(int32_t T, int32_t N, int32_t P, double gamma, float clip,
                                   const float *rew_raw /*[T,N]*/, const float *done /*[T,N]*/,
                                   const int32_t *players /*[T,N] or NULL*/, const float *valid /*[T,N] or NULL*/,
                                   double *returns_state /*[N,P] in/out*/, double *stats3 /*in/out*/,
                                   float *rew /*[T,N] out*/, float *all_rewards /*[T,N,P] in/out or NULL*/);
/* Parity hooks of the update's small kernels (host buffers, no context).  Each checks its
 * arguments before any HIP call.
 *
 * bppo_debug_adv_stats: the per-minibatch advantage statistics of one epoch, exactly the launches
 * of the update (its own choice of kernels and block chunking).  adv [B], perm [B] the shuffled
 * row indices, inv [B] its inverse (row -> shuffled position) or NULL, M minibatches (minibatch m
 * holds B / M + (m < B % M) consecutive shuffled positions); stats [M][4] = mean, std, min, max.
 * *path_out = 0 when the kernels over perm ran (inv NULL, M > 16 or B < M), else 4, 8 or 16, the
 * bin count of the kernels over inv.  BPPO_ERR_ARG: B < 1, M < 1, a NULL adv / perm / stats /
 * path_out, an index >= B in perm or inv; BPPO_ERR_UNSUPPORTED: more minibatches than the
 * reduction scratch holds block partials for. */
bppo_status bppo_debug_adv_stats(uint32_t B, int32_t M, const float *adv, const uint32_t *perm, const uint32_t *inv,
                                 float *stats, int32_t *path_out);
/* bppo_debug_slab_reduce: the fixed-order reduction of the minibatch kernels' partial gradient
 * rows, slab [rows][width] -> grad_out [width]: column sums, but the maximum in column
 * width - 11 + 9 (value_error_max of the 11 metric slots behind the parameters), which also goes
 * to *vemax_local_out.  grad_out holds width + 64 floats, uploaded before and read back after the
 * launch whole, so the caller sees whatever was written behind column width - 1.
 * BPPO_ERR_ARG: rows < 1, width < 11, a NULL pointer. */
bppo_status bppo_debug_slab_reduce(int32_t rows, int32_t width, const float *slab, float *grad_out,
                                   float *vemax_local_out);
/* bppo_debug_adam: per-tensor norm clip + Adam step `step` (>= 1: the bias corrections are the
 * update's f32 powers) of nt tensors laid out back to back (tensor t at the running sum of lens),
 * the gradient scaled by 1 / world first.  fused = 1: the one-launch kernel for tables whose
 * tensors all fit one 4096-element block; fused = 0: the norm pass, the update pass and the metric
 * row kernel.  params, m1, m2 in/out.  metric_row_out [nm + 4] = gtail [0, nm) with slot 9 read
 * from gtail[14] (the rank-local value_error_max), then mb_stats [4]; gtail holds 15 floats.
 * BPPO_ERR_ARG: nt outside 1..32, a len < 1, step or world < 1, fused not 0 / 1, nm outside
 * 0..14, a NULL pointer, fused = 1 with a len > 4096; BPPO_ERR_UNSUPPORTED: more 4096-element
 * blocks than the reduction scratch holds partials for (4160). */
bppo_status bppo_debug_adam(int32_t nt, const int32_t *lens, int32_t step, int32_t world, float lr, float max_norm,
                            float eps, int32_t fused, const float *grad, float *params, float *m1, float *m2,
                            const float *gtail, const float *mb_stats, int32_t nm, float *metric_row_out);
/* bppo_debug_wide_loss: the masked per-row PPO loss of the GEMM path alone (k_wide_loss<A>, A in
 * {2, 7, 33, 49}, and its metric reduction) with the block count the update launches for n rows.
 * Minibatch row r < n is buffer row perm[start + r]; perm holds perm_len entries, each below
 * buf_rows.  Indexed by buffer row: act, logp, adv (raw), ret, val [buf_rows], mask [buf_rows][A]
 * (0 / 1 bytes).  Indexed by minibatch row: logits [n][A], values [n], as the forward left them.
 * mb_stats [2] = the minibatch's advantage mean and std (the kernel normalizes with std + 1e-8f).
 * dout holds n (A + 1) + 64 floats and metrics 14 + 1 + 64; both are uploaded before and read
 * back after the launches whole, so the caller sees what was written behind the outputs.
 * dout [n][A + 1] = dL/dlogits | dL/dvalue; metrics [0, 14) = the metric slots in the order of
 * bppo_minibatch_rows, metrics [14] = the rank-local copy of value_error_max.
 * BPPO_ERR_ARG before any HIP call: another A, n < 1, buf_rows < 1, start + n > perm_len, a perm
 * entry >= buf_rows, an action outside [0, A), a NULL pointer. */
bppo_status bppo_debug_wide_loss(int32_t A, uint32_t n, uint32_t start, uint32_t perm_len, uint32_t buf_rows,
                                 const uint32_t *perm, const int32_t *act, const float *logp, const float *adv,
                                 const float *ret, const float *val, const uint8_t *mask, const float *logits,
                                 const float *values, const float *mb_stats, double clip_epsilon, double ent_coef,
                                 double value_coef, int32_t clip_value, float *dout, float *metrics);
/* Parity hook of the evaluation loop's forward (host buffers): the actor logits of n_models
 * models' row groups.  Model k owns rows [gbase[k], gbase[k + 1]) of xc [gbase[n_models]][G + D]
 * ([priv | obs] rows, raw: a model's obs normalizer is applied as the loop applies it) and of
 * logits [gbase[n_models]][A]; gbase has n_models + 1 entries, starts at >= 0 and does not
 * decrease.  params [n_models][n_params], norm_* and is_random as bppo_evaluate_pods takes them;
 * a random model's rows get zero logits.  mode 0: one model after the other (the launches of
 * bppo_forward); mode 1: the grouped launches, one per layer over all groups, which the loop
 * uses for every net without conv layers.  The context gives the net shape, the stream and
 * its hidden activation buffers, which are overwritten: as bppo_evaluate does, the call drops
 * a rollout that has not been bootstrapped yet (bppo_compute_gae) and a prefetched one.  The
 * context's parameters, envs and RNG are not touched.  At most as many rows as its buffers
 * hold (max(num_envs, minibatch size)). */
bppo_status bppo_debug_forward_groups(bppo_ctx *ctx, int32_t mode, int32_t n_models, const float *params,
                                      const double *norm_mean, const double *norm_m2, const double *norm_count,
                                      const int32_t *is_random, const int32_t *gbase, const float *xc,
                                      float *logits);

#ifdef __cplusplus
}
#endif
#endif
