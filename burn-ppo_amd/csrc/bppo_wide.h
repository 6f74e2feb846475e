// bppo_wide.h — argument blocks and launchers of the multi-player path
// (k_wide.hip) and its orchestration (wide_api.hip).
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bppo_device.h"
#include "bppo_metric_row.h"

namespace bppo {

struct EpisodeRec;

// a finished game as the evaluation loop (eval.hip) needs it: the episode's totals and
// Environment::game_outcome, captured before the auto-reset (env.rs:442-450)
struct EvalOutcome {
    float total_reward[6];   // per seat
    int32_t placement[6];    // per seat, 1 = first; valid when has_outcome
    int32_t length, has_outcome;
};

struct WideStepArgs {
    int N, t;
    void *state;
    uint64_t *env_pos;
    uint64_t seed_base;
    const int32_t *actions;
    float shaping;
    float *all_r;        // [N][P] (may be null)
    float *rew_act;      // [N] reward of the acting player (may be null)
    float *done_f;       // [N] (may be null)
    uint8_t *done_u8;    // [N] (may be null)
    float *ep_ret;       // [N][P]
    int32_t *ep_len;
    EpisodeRec *eps;
    int32_t *ep_count;
    int eps_cap;
    int32_t *err;        // bit 3: an action outside the env's mask (Skull panics, skull.rs:1113-1128)
    // evaluation only (null on every training call): envs marked terminal are neither stepped
    // nor reset (env.rs:429-432); a finished game's totals and outcome go to sink[e]
    const uint8_t *frozen = nullptr;
    EvalOutcome *sink = nullptr;
    // evaluation pods only: env e's seed from device memory instead of seed_base + e
    const uint64_t *env_seed = nullptr;
    // opponent-pool rollouts only (null otherwise): a finished game of an env in [0, n_opp)
    // leaves its game_outcome here before the reset, packed by opp_pack_outcome; k_opp_seats
    // reads it the same step (ppo.rs:871-917)
    uint32_t *opp_out = nullptr;
    int n_opp = 0;
};

// Environment::game_outcome of one finished game in one word: placement of seat p (1 = first,
// 0 beyond the seated players) in bits [4p, 4p + 4), bit 24 = the env reported an outcome
__host__ __device__ inline uint32_t opp_pack_outcome(bool has, const int32_t placement[6]) {
    uint32_t v = has ? 1u << 24 : 0u;
    for (int p = 0; p < 6; p++) v |= ((uint32_t)placement[p] & 15u) << (4 * p);
    return v;
}
// -> whether the env reported an outcome; the placements are 0 where it did not
__host__ __device__ inline bool opp_unpack_outcome(uint32_t w, int32_t placement[6]) {
    const bool has = (w >> 24) & 1u;
    for (int p = 0; p < 6; p++) placement[p] = has ? (int32_t)((w >> (4 * p)) & 15u) : 0;
    return has;
}

struct SampleArgs {
    int N, P;
    const float *logits, *values;
    const uint8_t *mask;
    const int32_t *players;
    Key8 key;
    uint64_t stream, base;
    int32_t *act;
    float *logp, *val, *lvpp;
    int32_t *err;        // bit 0: non-finite log-prob, bit 1: empty mask
    // opponent pool: row group (0 learner, 1 + model) and its position in the
    // step's draw order; the step's first word position from device memory
    const int32_t *group = nullptr, *gpos = nullptr;
    const uint64_t *dbase = nullptr;
    // PopArt (ppo.rs:355-359): stored values denormalized, v * std + mean in f64
    int pa_on = 0;
    double pa_mean = 0.0, pa_std = 1.0;
};

// (the metric slots WM_* written after the gradient, d_grad[np + k]: bppo_metric_row.h)

struct LossArgs {
    const uint32_t *perm;
    uint32_t start, n;
    const int32_t *act;
    const float *logp, *adv, *ret, *val;
    const uint8_t *mask;
    const float *logits, *values;   // minibatch forward [n][A], [n]
    const float *mb_stats;
    float *dout;                    // [n][A+1]
    double *part;                   // [blocks][WM_COUNT]
    float lo, hi, ceps, inv_mb, ent_coef, value_coef;
    // the gradient of the loss in f64, rounded once (the oracle's hand-written autodiff:
    // inv = 1 / mb, entropy / value coefficients as the config's f64 values)
    double inv_mb_d, ent_coef_d, value_coef_d;
    int clip_value;
    // the scalars of a minibatch of mb rows from the config's f64 values: one rule for the
    // update (wide_minibatch) and the parity hook (bppo_debug_wide_loss)
    void set_scalars(uint32_t start_, uint32_t mb, double clip_epsilon, double ent_coef_, double value_coef_,
                     int clip_value_) {
        start = start_; n = mb;
        lo = (float)(1.0 - clip_epsilon); hi = (float)(1.0 + clip_epsilon);
        ceps = (float)clip_epsilon; inv_mb = (float)(1.0 / (double)mb); ent_coef = (float)ent_coef_;
        value_coef = (float)value_coef_; clip_value = clip_value_;
        inv_mb_d = 1.0 / (double)mb; ent_coef_d = ent_coef_; value_coef_d = value_coef_;
    }
};
// blocks of 256 rows, capped: beyond 1024 x 256 rows k_wide_loss strides over the grid
inline int wide_loss_blocks(uint32_t mb) { return std::max(1, std::min(1024, (int)((mb + 255) / 256))); }

// players: Skull's num_players (new_with_players, main.rs:2008-2014); env_seed (device,
// [N], may be null): env e's seed instead of seed_base + e (evaluation pods)
hipError_t wide_env_reset(int kind, hipStream_t st, int N, uint64_t seed_base, int players, void *state,
                          uint64_t *env_pos, float *ep_ret, int32_t *ep_len, const uint64_t *env_seed = nullptr);
// rows [priv | obs] when with_priv (CTDE), [obs] otherwise
hipError_t wide_env_observe(int kind, int with_priv, hipStream_t st, int N, const void *state, float *xc,
                            uint8_t *mask, int32_t *players);
hipError_t wide_env_step(int kind, hipStream_t st, const WideStepArgs &a);
// Environment::reset of every env once more (VecEnv::set_all_num_players, env.rs:313-326)
hipError_t wide_env_reset_again(int kind, hipStream_t st, int N, uint64_t seed_base, void *state, uint64_t *env_pos,
                                const uint64_t *env_seed = nullptr);
hipError_t wide_sample(int A, hipStream_t st, const SampleArgs &g);
hipError_t wide_boot_lvpp(hipStream_t st, int N, int P, const float *values, const int32_t *players, float *lvpp);
hipError_t wide_gather(hipStream_t st, const uint32_t *perm, uint32_t start, uint32_t n, const float *src, int L,
                       float *dst);
hipError_t wide_pack_heads(hipStream_t st, const float *params, int K, int A, size_t wp, size_t bp, size_t wv,
                           size_t bv, float *W, float *b);
hipError_t wide_loss(int A, hipStream_t st, const LossArgs &g, int blocks, float *metrics_out);
size_t wide_state_bytes(int kind);

}  // namespace bppo
