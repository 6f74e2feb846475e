// opponents.hip — opponent-pool rollouts (ppo.rs:537-1063) and the learner-only
// update filter (ppo.rs:165-180, 1696-1753) on the multi-player GEMM path.
//
// Per rollout step, on the context's stream:
//   k_opp_group   each env's mover: the learner (self-play envs [n_opp, N), and
//                 opponent envs on the learner's seat) or opponent model k; and
//                 the env's position in the step's draw order: learner rows
//                 first, then each model's rows in ascending model index, env
//                 order within a group (the reference samples the learner batch,
//                 then iterates a HashMap of opponent batches: its order is not
//                 deterministic, ours is ascending)
//   learner forward on all N rows; the models' actor forwards on their own rows of
//   the raw copy, sorted into draw order, each under its own obs normalizer, their
//   logits selected into the step's logits (models_step_forward, model_set.hip)
//   sampling (k_sample_masked) at word base + position * A
//   env step, then k_opp_seats: the step's N*A Gumbel words, then for every
//   finished opponent game in env order its OpponentEpisodeCompletion record and
//   queue_game_result sums (ppo.rs:871-917, opponent_pool.rs:578-616) from the seats
//   it was played under, then OpponentPool::sample_all_slots and
//   EnvState::shuffle_positions from the main RNG (usize gen_range + u32
//   shuffle), then the learner-turn flags against the reshuffled seats.
// The main RNG position therefore lives on the device during the rollout and
// is read back once at its end.
#include "bppo_internal.h"
#include "bppo_wide.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace bppo {

constexpr int OG_THREADS = 1024;

__global__ void k_set_u64(uint64_t *p, uint64_t v) { *p = v; }

// group[e] = 0 (learner) or 1 + model; gpos[e] = the env's row in the step's
// draw order.  One block: per-thread env chunks counted per group in LDS,
// exclusive prefix per group, group bases in group order.
__global__ void __launch_bounds__(OG_THREADS) k_opp_group(int N, int n_opp, int P, int G, const int32_t *players,
                                                          const int32_t *lpos, const int32_t *p2o, int32_t *group,
                                                          int32_t *gpos, int32_t *gbase, int32_t *err) {
    __shared__ int cnt[OPP_MAX_MODELS + 1][OG_THREADS];
    __shared__ int base[OPP_MAX_MODELS + 2];
    const int tid = threadIdx.x;
    const int per = (N + OG_THREADS - 1) / OG_THREADS;
    const int e0 = tid * per, e1 = min(N, e0 + per);
    for (int g = 0; g < G; g++) cnt[g][tid] = 0;
    for (int e = e0; e < e1; e++) {
        int g = 0;
        if (e < n_opp) {
            const int cp = players[e];
            if (cp != lpos[e]) {
                const int m = p2o[(size_t)e * P + cp];
                if (m < 0 || m >= G - 1) { atomicOr(err, 4); } else g = 1 + m;
            }
        }
        group[e] = g;
        cnt[g][tid]++;
    }
    __syncthreads();
    if (tid < G) {                         // exclusive prefix of group tid over the threads
        int run = 0;
        for (int k = 0; k < OG_THREADS; k++) { const int v = cnt[tid][k]; cnt[tid][k] = run; run += v; }
        base[tid + 1] = run;
    }
    __syncthreads();
    if (tid == 0) {
        base[0] = 0;
        for (int g = 1; g <= G; g++) base[g] += base[g - 1];
        for (int g = 0; g <= G; g++) gbase[g] = base[g];
    }
    __syncthreads();
    for (int e = e0; e < e1; e++) {
        const int g = group[e];
        gpos[e] = base[g] + cnt[g][tid]++;
    }
}

// main-stream words from an LDS window [base, end) filled in parallel by the
// block; a position past the window (an env whose rejections run past it)
// falls back to computing its ChaCha block
struct WindowCursor {
    const uint32_t *buf;
    uint64_t base, end, pos;
    Key8 key;
    uint64_t stream;
    __device__ __forceinline__ uint32_t next() {
        uint32_t w;
        if (pos < end) {
            w = buf[pos - base];
        } else {
            uint32_t blk[16];
            chacha12_block(key, pos >> 4, stream, blk);
            w = blk[pos & 15];
        }
        pos++;
        return w;
    }
};

// rand 0.8.5 UniformInt<u64> / <u32>::sample_single on the counter-based main
// stream (same restatement as oracle/rng.c)
template <class Cur>
__device__ __forceinline__ uint64_t dev_range_u64(Cur &c, uint64_t range) {
    const uint64_t zone = (range << __clzll((long long)range)) - 1ull;
    for (;;) {
        const uint64_t lo32 = c.next(), hi32 = c.next();
        const uint64_t v = (hi32 << 32) | lo32;
        const uint64_t lo = v * range, hi = __umul64hi(v, range);
        if (lo <= zone) return hi;
    }
}
template <class Cur>
__device__ __forceinline__ uint32_t dev_range_u32(Cur &c, uint32_t range) {
    const uint32_t zone = (range << __clz((int)range)) - 1u;
    for (;;) {
        const uint64_t m = (uint64_t)c.next() * range;
        if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
    }
}

// after the env step: the step's N*A sampling words, then the seat reshuffle of
// every finished opponent game (env order, main RNG), then the learner-turn
// flags against the new seats (ppo.rs:874-925, 928-937)
constexpr int SEAT_THREADS = 1024, SEAT_CHUNK = 8192, SEAT_WORDS = 4096, SEAT_MARGIN = 64;
constexpr int SEAT_PER = SEAT_CHUNK / SEAT_THREADS;   // envs per thread and chunk, at most
static_assert(SEAT_CHUNK < (1 << 16), "a chunk's two counts share one word");
// the OpponentEpisodeCompletion records of one thread's envs [e0, e0 + SEAT_PER) of a chunk, from
// registers: oc = the env's outcome word (opp_pack_outcome), snap = bit 31 a record is due,
// bits [24, 27) the learner's seat, 4 bits per seat the model slot (15 = none) -- the seats
// as they were before the reshuffle.  Slots from `orec` on; past `cap` nothing is written
__device__ __forceinline__ void seat_write_records(const uint32_t (&oc)[SEAT_PER], const uint32_t (&snap)[SEAT_PER],
                                                   int e0, int orec, int t, int P, bppo_opp_completion *comp,
                                                   int cap) {
#pragma unroll
    for (int i = 0; i < SEAT_PER; i++) {
        if (!(snap[i] >> 31)) continue;
        bppo_opp_completion rec;
        rec.env_index = e0 + i; rec.step = t; rec.learner_position = (int)((snap[i] >> 24) & 7u); rec.n_players = P;
#pragma unroll
        for (int p = 0; p < BPPO_MAX_PLAYERS; p++) {
            const int m = (int)((snap[i] >> (4 * p)) & 15u);
            rec.placement[p] = p < P ? (int)((oc[i] >> (4 * p)) & 15u) : 0;
            rec.position_to_opponent[p] = (p < P && m != 15) ? m : -1;
        }
        if (orec < cap) comp[orec] = rec;
        orec++;
    }
}

__global__ void __launch_bounds__(SEAT_THREADS) k_opp_seats(int N, int n_opp, int P, int A, const float *done,
                                                            const int32_t *players, Key8 key, uint64_t stream,
                                                            const int32_t *curopp, uint64_t *rngpos, int32_t *lpos,
                                                            int32_t *p2o, float *valid, int t, const uint32_t *outcome,
                                                            bppo_opp_completion *comp, int comp_cap, OppResults *res) {
    __shared__ int list[SEAT_CHUNK];
    __shared__ int cnt[SEAT_THREADS];           // finished games | those with an outcome << 16
    __shared__ uint32_t words[SEAT_WORDS];
    __shared__ uint64_t pos;
    __shared__ int qnext;
    __shared__ int rec_base, rec_chunk;         // the rollout's records so far; before this chunk
    __shared__ int s_wins[OPP_MAX_MODELS], s_games[OPP_MAX_MODELS], s_swiss[OPP_MAX_MODELS];
    const int tid = threadIdx.x;
    if (tid == 0) { pos = *rngpos + (uint64_t)N * A; rec_base = res->count; }
    if (tid < OPP_MAX_MODELS) { s_wins[tid] = 0; s_games[tid] = 0; s_swiss[tid] = 0; }
    // finished opponent games in env order, chunk by chunk: flags read in
    // parallel and compacted, the draws (sequential in the RNG) on one thread
    float dn[SEAT_PER];
    uint32_t oc[SEAT_PER], snap[SEAT_PER];
    int e0 = 0, orec0 = 0;
    for (int c0 = 0; c0 < n_opp; c0 += SEAT_CHUNK) {
        const int c1 = min(n_opp, c0 + SEAT_CHUNK);
        const int per = (c1 - c0 + SEAT_THREADS - 1) / SEAT_THREADS;
        e0 = c0 + tid * per;
        const int e1 = min(c1, e0 + per);
        // the thread's done flags and outcome words, loaded once (clamped, none conditional)
#pragma unroll
        for (int i = 0; i < SEAT_PER; i++) {
            const int e = min(e0 + i, n_opp - 1);
            dn[i] = done[e];
            oc[i] = outcome[e];
        }
        int k = 0;
#pragma unroll
        for (int i = 0; i < SEAT_PER; i++) {
            if (i >= per || e0 + i >= e1) dn[i] = 0.0f;
            if (dn[i] != 0.0f) k += 1 + (int)(((oc[i] >> 24) & 1u) << 16);
        }
        cnt[tid] = k;
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int q = 0; q < SEAT_THREADS; q++) { const int v = cnt[q]; cnt[q] = run; run += v; }
            list[SEAT_CHUNK - 1] = run & 0xffff;   // count (list slot reused after the writes below)
            rec_chunk = rec_base;
            rec_base += run >> 16;
        }
        __syncthreads();
        const int nd = list[SEAT_CHUNK - 1];
        __syncthreads();
        // the chunk's finished games compacted in env order.  Each with an outcome adds its
        // queue_game_result terms (opponent_pool.rs:591-614) and keeps the seats it was played
        // under in a register: the barrier below stands between these reads of lpos / p2o and
        // the reshuffle that overwrites them.  Its record (slot = its rank in (step, env)
        // order) is stored once the draws are done, so no store is waited for on their way
        int o = cnt[tid] & 0xffff;
        orec0 = rec_chunk + (cnt[tid] >> 16);
#pragma unroll
        for (int i = 0; i < SEAT_PER; i++) {
            snap[i] = 0;
            if (dn[i] == 0.0f) continue;
            const int e = e0 + i;
            list[o++] = e;
            const uint32_t w = oc[i];
            if (!((w >> 24) & 1)) continue;        // no game_outcome: no record, still reshuffled (ppo.rs:877-916)
            const int lp = lpos[e];
            const int lplace = (int)((w >> (4 * lp)) & 15u);
            uint32_t sn = (1u << 31) | ((uint32_t)lp << 24);
            for (int p = 0; p < P; p++) {
                const int m = p2o[(size_t)e * P + p];
                const bool opp = p != lp && m >= 0 && m < OPP_MAX_MODELS;
                sn |= (opp ? (uint32_t)m : 15u) << (4 * p);
                if (opp) {
                    atomicAdd(&s_games[m], 1);
                    atomicAdd(&s_swiss[m], P - lplace);
                    if (lplace < (int)((w >> (4 * p)) & 15u)) atomicAdd(&s_wins[m], 1);
                }
            }
            snap[i] = sn;
        }
        __syncthreads();
        if (tid == 0) qnext = 0;
        __syncthreads();
        while (qnext < nd) {
            // the next SEAT_WORDS words from pos's block on, one ChaCha block per thread
            const uint64_t wbase = (pos >> 4) << 4;
            if (tid < SEAT_WORDS / 16) chacha12_block(key, (wbase >> 4) + tid, stream, (uint32_t *)&words[tid * 16]);
            __syncthreads();
            if (tid == 0) {
                WindowCursor c{words, wbase, wbase + SEAT_WORDS, pos, key, stream};
                int q = qnext;
                for (; q < nd && c.pos + SEAT_MARGIN <= c.end; q++) {
                    const int e = list[q];
                    const int lp = (int)dev_range_u64(c, (uint64_t)P);        // opponent_pool.rs:109
                    int other[BPPO_MAX_PLAYERS], no = 0;
                    for (int p = 0; p < P; p++) if (p != lp) other[no++] = p;
                    for (int i = no - 1; i >= 1; i--) {                          // :114-115 SliceRandom::shuffle
                        const int j = (int)dev_range_u32(c, (uint32_t)(i + 1));
                        const int t = other[i]; other[i] = other[j]; other[j] = t;
                    }
                    lpos[e] = lp;
                    int32_t *row = p2o + (size_t)e * P;
                    for (int p = 0; p < P; p++) row[p] = -1;
                    for (int i = 0; i < no; i++) row[other[i]] = curopp[i];
                }
                pos = c.pos;
                qnext = q;
            }
            __syncthreads();
        }
        // (the last chunk's records go out at the kernel's end, beside the valid flags)
        if (c0 + SEAT_CHUNK < n_opp) seat_write_records(oc, snap, e0, orec0, t, P, comp, comp_cap);
    }
    if (tid == 0) { *rngpos = pos; res->count = rec_base; }
    __threadfence_block();
    __syncthreads();
    if (n_opp > 0) seat_write_records(oc, snap, e0, orec0, t, P, comp, comp_cap);
    if (tid < OPP_MAX_MODELS && s_games[tid] != 0) {      // the launch's sums, flushed once
        atomicAdd(&res->wins[tid], s_wins[tid]);
        atomicAdd(&res->games[tid], s_games[tid]);
        atomicAdd(&res->swiss[tid], (unsigned long long)s_swiss[tid]);
    }
    for (int e = tid; e < N; e += blockDim.x)
        valid[e] = (e >= n_opp || players[e] == lpos[e]) ? 1.0f : 0.0f;
}

// learner rows of the rollout in (t, e) order (ppo.rs:165-180)
__global__ void __launch_bounds__(OG_THREADS) k_compact_valid(size_t n, const float *valid, uint32_t *vidx,
                                                              uint32_t *count) {
    __shared__ uint32_t cnt[OG_THREADS];
    const int tid = threadIdx.x;
    const size_t per = (n + OG_THREADS - 1) / OG_THREADS;
    const size_t i0 = (size_t)tid * per, i1 = min(n, i0 + per);
    uint32_t k = 0;
    for (size_t i = i0; i < i1; i++) k += valid[i] > 0.5f;
    cnt[tid] = k;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int q = 0; q < OG_THREADS; q++) { const uint32_t v = cnt[q]; cnt[q] = run; run += v; }
        *count = run;
    }
    __syncthreads();
    uint32_t o = cnt[tid];
    for (size_t i = i0; i < i1; i++)
        if (valid[i] > 0.5f) vidx[o++] = (uint32_t)i;
}

// the permutation over the learner rows, mapped to buffer rows
__global__ void k_map_perm(uint32_t n, const uint32_t *vidx, uint32_t *perm) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) perm[j] = vidx[perm[j]];
}

bool opp_active(const bppo_ctx *c) { return c->wide && c->n_opp > 0 && c->opp_models.K > 0; }

bppo_status opp_alloc(bppo_ctx *c) {
    const size_t N = c->N, TN = (size_t)c->T * c->N;
    BPPO_HIP(c, c->zalloc(&c->d_group, N));
    BPPO_HIP(c, c->zalloc(&c->d_gpos, N));
    BPPO_HIP(c, c->zalloc(&c->d_valid, TN));
    BPPO_HIP(c, c->zalloc(&c->d_rngpos, 1));
    BPPO_HIP(c, c->zalloc(&c->d_oraw, N * c->L));
    BPPO_HIP(c, c->zalloc(&c->d_oxc, N * c->L));
    BPPO_HIP(c, c->zalloc(&c->d_ologits, N * c->A));
    BPPO_HIP(c, c->zalloc(&c->d_vidx, TN));
    BPPO_HIP(c, c->zalloc(&c->d_Jopp, TN));
    BPPO_HIP(c, c->zalloc(&c->d_nvalid, 1));
    BPPO_HIP(c, c->zalloc(&c->d_curopp, 4));
    BPPO_HIP(c, c->zalloc(&c->d_gbase, OPP_MAX_MODELS + 2));
    BPPO_HIP(c, c->mem.alloc_pinned(&c->h_gbase, OPP_MAX_MODELS + 2));
    BPPO_HIP(c, c->zalloc(&c->d_opp_out, N));
    BPPO_HIP(c, c->zalloc(&c->d_comp, (size_t)c->eps_cap));
    BPPO_HIP(c, c->zalloc(&c->d_opp_res, 1));
    return BPPO_OK;
}

// the records and sums describe one rollout: emptied where the episode counter is
bppo_status opp_records_clear(bppo_ctx *c) {
    if (c->d_opp_res) BPPO_HIP(c, hipMemsetAsync(c->d_opp_res, 0, sizeof(OppResults), c->stream));
    return BPPO_OK;
}

bppo_status opp_rollout_begin(bppo_ctx *c, uint64_t base) {
    hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, c->d_rngpos, base);
    TRY(launch_check(c, __func__));
    return BPPO_OK;
}

// raw rows kept for the opponents' forwards, then movers and draw positions
bppo_status opp_step_group(bppo_ctx *c, int t) {
    const size_t r0 = (size_t)t * c->N;
    BPPO_HIP(c, hipMemcpyAsync(c->d_oraw, c->d_xc + r0 * c->L, sizeof(float) * (size_t)c->N * c->L,
                               hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_opp_group, dim3(1), dim3(OG_THREADS), 0, c->stream, c->N, c->n_opp, c->Pa, c->opp_models.K + 1,
                       c->d_players + r0, c->d_lpos, c->d_p2o, c->d_group, c->d_gpos, c->d_gbase, c->d_err);
    TRY(launch_check(c, __func__));
    // the per-model row counts size the opponents' GEMMs: one small read per step
    BPPO_HIP(c, hipMemcpyAsync(c->h_gbase, c->d_gbase, sizeof(int32_t) * (c->opp_models.K + 2), hipMemcpyDeviceToHost,
                               c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    return BPPO_OK;
}

// each model's actor forward (its own obs normalizer, ppo.rs:809-812) on its rows of the raw
// copy; its rows' logits replace the learner's in d_logits.  Nothing runs in a step where no
// opponent moves (model_set.hip)
bppo_status opp_step_forwards(bppo_ctx *c) {
    return models_step_forward(c, c->opp_models, c->d_group, c->d_gpos, c->h_gbase, c->d_gbase, c->d_oraw, c->d_oxc,
                               c->d_ologits, c->d_logits);
}

bppo_status opp_step_seats(bppo_ctx *c, int t) {
    const size_t r0 = (size_t)t * c->N;
    hipLaunchKernelGGL(k_opp_seats, dim3(1), dim3(SEAT_THREADS), 0, c->stream, c->N, c->n_opp, c->Pa, c->A, c->d_done + r0,
                       c->d_players + r0, c->rng_key, (uint64_t)c->cfg.rng_stream, c->d_curopp, c->d_rngpos,
                       c->d_lpos, c->d_p2o, c->d_valid + r0, t, c->d_opp_out, c->d_comp, (int)c->eps_cap, c->d_opp_res);
    TRY(launch_check(c, __func__));
    return BPPO_OK;
}

bppo_status opp_rollout_end(bppo_ctx *c) {
    uint64_t pos = 0;
    BPPO_HIP(c, hipMemcpyAsync(&pos, c->d_rngpos, 8, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    c->rng_pos = pos;
    return BPPO_OK;
}

bppo_status opp_compact_valid(bppo_ctx *c) {
    const size_t TN = (size_t)c->T * c->N;
    hipLaunchKernelGGL(k_compact_valid, dim3(1), dim3(OG_THREADS), 0, c->stream, TN, c->d_valid, c->d_vidx,
                       c->d_nvalid);
    uint32_t nv = 0;
    BPPO_HIP(c, hipMemcpyAsync(&nv, c->d_nvalid, 4, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    c->n_valid = nv;
    return BPPO_OK;
}

bppo_status opp_map_perm(bppo_ctx *c, uint32_t n) {
    hipLaunchKernelGGL(k_map_perm, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->d_vidx, c->d_perm);
    TRY(launch_check(c, __func__));
    return BPPO_OK;
}

}  // namespace bppo

using namespace bppo;

// ppo.rs:537-1063 / main.rs:621-651: see include/bppo.h
extern "C" bppo_status bppo_opponents_set(bppo_ctx *c, int32_t n_models, const float *params, const double *norm_mean,
                                          const double *norm_m2, const double *norm_count, int32_t num_opponent_envs,
                                          const int32_t *learner_pos, const int32_t *pos_to_opp,
                                          const int32_t *current_opp) {
    if (!c) return BPPO_ERR_ARG;
    if (!c->wide) { c->err = "opponent pool: multi-player envs only"; return BPPO_ERR_UNSUPPORTED; }
    if (n_models < 0 || n_models > OPP_MAX_MODELS) { c->err = "opponent pool: 0..15 models"; return BPPO_ERR_ARG; }
    if (num_opponent_envs < 0 || num_opponent_envs > c->N) { c->err = "opponent pool: num_opponent_envs > num_envs"; return BPPO_ERR_ARG; }
    if (num_opponent_envs > 0 && c->cfg.shuffle_windows) { c->err = "opponent pool: not with shuffle_windows"; return BPPO_ERR_UNSUPPORTED; }
    if (num_opponent_envs > 0 && (!params || !learner_pos || !pos_to_opp || !current_opp || n_models == 0)) {
        c->err = "opponent pool: models and seat state required";
        return BPPO_ERR_ARG;
    }
    const int P = c->Pa;   // EnvState seats: the active player count (main.rs:552, 649)
    if (num_opponent_envs > 0) {
        for (int e = 0; e < num_opponent_envs; e++) {
            if (learner_pos[e] < 0 || learner_pos[e] >= P) { c->err = "opponent pool: learner_pos out of range"; return BPPO_ERR_ARG; }
            for (int p = 0; p < P; p++) {
                const int m = pos_to_opp[(size_t)e * P + p];
                if (p == learner_pos[e] ? m != -1 : (m < 0 || m >= n_models)) {
                    c->err = "opponent pool: pos_to_opp must name a model on every non-learner seat";
                    return BPPO_ERR_ARG;
                }
            }
        }
        for (int i = 0; i < P - 1; i++)
            if (current_opp[i] < 0 || current_opp[i] >= n_models) { c->err = "opponent pool: current_opp out of range"; return BPPO_ERR_ARG; }
    }
    if (!c->d_opp_res) TRY(opp_alloc(c));   // once per context (d_opp_res is its last buffer)
    // the finished games on record were played under the seats and models replaced here
    TRY(opp_records_clear(c));
    BPPO_HIP(c, hipMemsetAsync(c->d_ep_count, 0, 4, c->stream));
    // the buffers sized by this call
    c->opp_models.release(c->mem);
    (void)c->mem.release(c->d_lpos);
    (void)c->mem.release(c->d_p2o);
    c->n_opp = num_opponent_envs;
    BPPO_HIP(c, c->zalloc(&c->d_lpos, (size_t)std::max(num_opponent_envs, 1)));
    BPPO_HIP(c, c->zalloc(&c->d_p2o, (size_t)std::max(num_opponent_envs, 1) * P));
    // uploads are ordered on the context stream after the allocations' zeroing memsets (a
    // blocking hipMemcpy on the null stream would not wait for that non-blocking
    // stream); the stream is drained before the host arrays may go away
    TRY(c->opp_models.upload(c, c->mem, n_models, params, norm_mean, norm_m2, norm_count, 0));
    if (num_opponent_envs > 0) {
        BPPO_HIP(c, hipMemcpyAsync(c->d_lpos, learner_pos, sizeof(int32_t) * num_opponent_envs, hipMemcpyHostToDevice, c->stream));
        BPPO_HIP(c, hipMemcpyAsync(c->d_p2o, pos_to_opp, sizeof(int32_t) * (size_t)num_opponent_envs * P,
                                   hipMemcpyHostToDevice, c->stream));
        BPPO_HIP(c, hipMemcpyAsync(c->d_curopp, current_opp, sizeof(int32_t) * (P - 1), hipMemcpyHostToDevice, c->stream));
    }
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    return BPPO_OK;
}

extern "C" bppo_status bppo_opponents_get_envs(bppo_ctx *c, int32_t *learner_pos, int32_t *pos_to_opp) {
    if (!c) return BPPO_ERR_ARG;
    if (!c->n_opp) return BPPO_OK;
    if (learner_pos) BPPO_HIP(c, hipMemcpyAsync(learner_pos, c->d_lpos, sizeof(int32_t) * c->n_opp, hipMemcpyDeviceToHost, c->stream));
    if (pos_to_opp)
        BPPO_HIP(c, hipMemcpyAsync(pos_to_opp, c->d_p2o, sizeof(int32_t) * (size_t)c->n_opp * c->Pa, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    return BPPO_OK;
}

extern "C" size_t bppo_opp_completion_size(void) { return sizeof(bppo_opp_completion); }

// ppo.rs:505-521, 871-917: see include/bppo.h
extern "C" bppo_status bppo_opponents_completions(bppo_ctx *c, bppo_opp_completion *out, int32_t cap, int32_t *n,
                                                  int32_t *dropped) {
    if (!c) return BPPO_ERR_ARG;
    if (!opp_active(c)) { c->err = "opponents_completions: no opponents set"; return BPPO_ERR_ARG; }
    if (cap < 0 || (cap > 0 && !out)) { c->err = "opponents_completions: cap < 0 or no output array"; return BPPO_ERR_ARG; }
    OppResults r;
    BPPO_HIP(c, hipMemcpyAsync(&r, c->d_opp_res, sizeof r, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    const int kept = std::min(r.count, c->eps_cap), m = std::min(kept, cap);
    if (m > 0) {
        BPPO_HIP(c, hipMemcpyAsync(out, c->d_comp, sizeof(bppo_opp_completion) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        BPPO_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (n) *n = kept;
    if (dropped) *dropped = r.count - kept;
    return BPPO_OK;
}

// opponent_pool.rs:578-616: see include/bppo.h
extern "C" bppo_status bppo_opponents_results(bppo_ctx *c, int32_t *wins, int32_t *games, int64_t *swiss_points) {
    if (!c) return BPPO_ERR_ARG;
    if (!opp_active(c)) { c->err = "opponents_results: no opponents set"; return BPPO_ERR_ARG; }
    OppResults r;
    BPPO_HIP(c, hipMemcpyAsync(&r, c->d_opp_res, sizeof r, hipMemcpyDeviceToHost, c->stream));
    BPPO_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < c->opp_models.K; k++) {
        if (wins) wins[k] = r.wins[k];
        if (games) games[k] = r.games[k];
        if (swiss_points) swiss_points[k] = (int64_t)r.swiss[k];
    }
    return BPPO_OK;
}
