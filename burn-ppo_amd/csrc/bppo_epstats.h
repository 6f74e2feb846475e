// bppo_epstats.h — per-record arithmetic of the episode statistics (episode_stats.hip):
// the mergeable sums behind the reference's episode/* scalars (main.rs:1134-1217,
// compute_avg_points env.rs:208-261) and the key of its last-100 window (main.rs:842-875).
// One source for the kernels and for the host build (bppo_debug_episode_stats device 0).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/bppo.h"
#include "bppo_wide.h"     // the episode record's outcome word: opp_pack_outcome / opp_unpack_outcome

namespace bppo {

constexpr int EPS_BLOCKS = 256;          // grid of the record passes = per-block partials merged in block order
constexpr int EPS_THREADS = 256;
constexpr int EPS_DIGIT_BITS = 11, EPS_BINS = 1 << EPS_DIGIT_BITS, EPS_MAX_DIGITS = 3;
// d_ep_sel: [EPS_MAX_DIGITS][EPS_BINS] histograms, then the compaction's slot counter
constexpr int EPS_SEL_WORDS = EPS_MAX_DIGITS * EPS_BINS + 1;

// position of an episode in the reference's push order (main.rs:843: step by step, within a
// step in env order, env.rs:470-483); unique, an env finishes at most one game per step
__host__ __device__ inline uint64_t ep_key(int32_t step, int32_t env_index, int32_t N) {
    return (uint64_t)(uint32_t)step * (uint64_t)(uint32_t)N + (uint64_t)(uint32_t)env_index;
}

// 11-bit digits of a key below T * N, most significant first
__host__ __device__ inline int ep_key_digits(uint64_t TN) {
    int bits = 1;
    while (bits < 64 && ((uint64_t)1 << bits) < TN) bits++;
    return (bits + EPS_DIGIT_BITS - 1) / EPS_DIGIT_BITS;
}
__host__ __device__ inline uint32_t ep_digit(uint64_t key, int d, int nd) {
    return (uint32_t)(key >> (EPS_DIGIT_BITS * (nd - 1 - d))) & (uint32_t)(EPS_BINS - 1);
}

// the merge identity: what a rollout without a finished episode reports
__host__ __device__ inline void epstats_identity(bppo_episode_stats &s) {
    s.episodes = 0; s.kept = 0;
    s.length_min = INT32_MAX; s.length_max = 0; s.length_sum = 0;
    s.with_outcome = 0; s.draws = 0;
    for (int p = 0; p < BPPO_MAX_PLAYERS; p++) {
        s.return_sum[p] = 0.0; s.return_min[p] = INFINITY; s.return_max[p] = -INFINITY;
        s.outcome_games[p] = 0; s.points2_sum[p] = 0;
    }
}

// one finished episode: totals [6], length, outcome word; P = the seated players
__host__ __device__ inline void epstats_add(bppo_episode_stats &s, const float *total, int32_t length, uint32_t word,
                                            int P) {
    s.kept += 1;
    s.length_sum += length;
    s.length_min = length < s.length_min ? length : s.length_min;
    s.length_max = length > s.length_max ? length : s.length_max;
    for (int p = 0; p < BPPO_MAX_PLAYERS; p++)
        if (p < P) {
            s.return_sum[p] += (double)total[p];
            s.return_min[p] = fminf(s.return_min[p], total[p]);
            s.return_max[p] = fmaxf(s.return_max[p], total[p]);
        }
    if (!((word >> 24) & 1u)) return;
    // compute_avg_points (env.rs:220-244): n = the outcome's seats, a seat's points =
    // n - (place + (tied - 1) / 2); doubled here, so the sum stays an integer
    int pl[6], n = 0, ones = 0;
    for (int p = 0; p < 6; p++) {
        pl[p] = (int)((word >> (4 * p)) & 15u);
        n += pl[p] != 0;
        ones += pl[p] == 1;
    }
    s.with_outcome += 1;
    s.draws += ones == n;                     // all(): an outcome without seats counts, as in the reference
    for (int p = 0; p < 6; p++)
        if (p < P && pl[p] != 0) {
            int tied = 0;
            for (int q = 0; q < 6; q++) tied += pl[q] == pl[p];
            s.points2_sum[p] += 2 * n - 2 * pl[p] - (tied - 1);
            s.outcome_games[p] += 1;
        }
}

// a += b (b after a: the f64 return sums are added in this order)
__host__ __device__ inline void epstats_merge(bppo_episode_stats &a, const bppo_episode_stats &b) {
    a.episodes += b.episodes; a.kept += b.kept;
    a.length_sum += b.length_sum;
    a.length_min = b.length_min < a.length_min ? b.length_min : a.length_min;
    a.length_max = b.length_max > a.length_max ? b.length_max : a.length_max;
    a.with_outcome += b.with_outcome; a.draws += b.draws;
    for (int p = 0; p < BPPO_MAX_PLAYERS; p++) {
        a.return_sum[p] += b.return_sum[p];
        a.return_min[p] = fminf(a.return_min[p], b.return_min[p]);
        a.return_max[p] = fmaxf(a.return_max[p], b.return_max[p]);
        a.outcome_games[p] += b.outcome_games[p];
        a.points2_sum[p] += b.points2_sum[p];
    }
}

// the record as the last-100 window keeps it
__host__ __device__ inline void eptail_fill(bppo_episode_tail &t, const float *total, int32_t length, int32_t env_index,
                                            int32_t step, uint32_t word) {
    for (int p = 0; p < BPPO_MAX_PLAYERS; p++) t.total_reward[p] = total[p];
    t.has_outcome = opp_unpack_outcome(word, t.placement) ? 1 : 0;
    t.length = length; t.env_index = env_index; t.step = step;
}

}  // namespace bppo
