// ratings.hip — Plackett-Luce ratings (plackett_luce.rs) as a device object: bppo_ratings_*.
//
// Games and their expanded comparisons live in device memory; add_* appends and expands once,
// fit iterates.  Every floating-point sum has a fixed order: per-player sums run over the
// player's incidence list (a CSR built by a stable counting sort, so its order is the comparison
// index) in a fixed strided partition and a fixed tree; no floating-point atomic is used anywhere.
// The only atomics are integer ones (games_played, histogram counts, the largest player id).
//
// Backend 1 is the reference's arithmetic in the reference's order, in plain f64 host C++ (the
// exact-parity mode; needs no GPU).  The covariance inversion runs on the host for both backends.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bppo_internal.h"
#include "bppo_scan.h"

namespace {

constexpr int MAXP = BPPO_MAX_PLAYERS;   // comparison slots: winner + up to 5 losers
constexpr int MAXN = 1024;               // players per fit
constexpr int CH = 4096;                 // incidence entries per counting-sort chunk
constexpr double ELO_SCALE = 400.0 / 2.302585092994046;   // 400 / LN_10 (plackett_luce.rs:131)

struct Meta {                 // written by the append kernels, read by the host
    long long added;          // games appended by add_completions
    long long new_cmp;        // comparisons the appended games expanded to
    int max_id;               // largest player id among them
    int bad;                  // a record the seats / slots of which are out of range
};

struct Slots { int32_t v[16]; };

// expand_games_to_comparisons (plackett_luce.rs:195-254) for one game of <= 6 seats, without a
// sort: a seat makes a comparison when somebody placed strictly worse; comparisons come in
// ascending placement, tied seats in seat order; the losers in (placement, seat) order.  Returns
// the number of comparisons; WRITE: stores them at cids[(base + k) * 6 ...], cw[base + k].
// Every array index is a compile-time constant after unrolling (no scratch on the device).
template <bool WRITE>
__host__ __device__ inline int expand_game(const int32_t *gp, const int32_t *gc, double gw, int64_t base,
                                           int32_t *cids, double *cw) {
    int32_t pl[MAXP], pc[MAXP];
    int np = 0;
#pragma unroll
    for (int s = 0; s < MAXP; s++) {
        pl[s] = gp[s];
        pc[s] = gc[s];
        np += pl[s] >= 0;
    }
    if (np <= 1) return 0;
    int n_out = 0;
#pragma unroll
    for (int s = 0; s < MAXP; s++) {
        int below = 0, tie = 0, before = 0;
#pragma unroll
        for (int t = 0; t < MAXP; t++) {
            const bool v = pl[t] >= 0;
            below += v && pc[t] > pc[s];
            tie += v && pc[t] == pc[s];
            // a seat placed no worse than s has the same players below it and more: it emits too
            before += v && (pc[t] < pc[s] || (pc[t] == pc[s] && t < s));
        }
        if (pl[s] < 0 || below == 0) continue;
        n_out++;
        if (WRITE) {
            const int64_t c = base + before;
            cw[c] = (1.0 / (double)tie) * gw;
            int32_t *o = cids + c * MAXP;
            o[0] = pl[s];
#pragma unroll
            for (int t = 0; t < MAXP; t++) {
                if (pl[t] < 0 || pc[t] <= pc[s]) continue;
                int pos = 0;
#pragma unroll
                for (int u = 0; u < MAXP; u++)
                    pos += pl[u] >= 0 && pc[u] > pc[s] && (pc[u] < pc[t] || (pc[u] == pc[t] && u < t));
                o[1 + pos] = pl[t];
            }
#pragma unroll
            for (int k = 1; k < MAXP; k++)
                if (k > below) o[k] = -1;
        }
    }
    return n_out;
}

// ------------------------------------------------------------------ append kernels ---
__device__ __forceinline__ int64_t new_games(int64_t n_bound, const Meta *meta) {
    return meta ? std::min<int64_t>((int64_t)meta->added, n_bound) : n_bound;
}

__global__ void k_expand_count(const int32_t *players, const int32_t *places, int64_t g0, int64_t n_bound,
                               const Meta *meta, int32_t *cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= new_games(n_bound, meta)) return;
    cnt[i] = expand_game<false>(players + (g0 + i) * MAXP, places + (g0 + i) * MAXP, 1.0, 0, nullptr, nullptr);
}

// one block: exclusive scan of cnt in game order, a carry from tile to tile
__global__ void __launch_bounds__(1024) k_expand_scan(const int32_t *cnt, int64_t n_bound, const Meta *meta,
                                                      int64_t cmp0, int64_t *goff, Meta *out) {
    __shared__ uint64_t wsum[16];
    const int64_t n = new_games(n_bound, meta);
    uint64_t carry = 0;
    for (int64_t b = 0; b < n; b += blockDim.x) {
        const int64_t i = b + threadIdx.x;
        const uint64_t v = i < n ? (uint64_t)cnt[i] : 0;
        uint64_t tot;
        const uint64_t ex = bppo::block_scan_excl(v, wsum, &tot);
        if (i < n) goff[i] = cmp0 + (int64_t)(carry + ex);
        carry += tot;
    }
    if (threadIdx.x == 0) out->new_cmp = (long long)carry;
}

__global__ void k_expand_write(const int32_t *players, const int32_t *places, const double *w, int64_t g0,
                               int64_t n_bound, const Meta *meta, const int64_t *goff, int32_t *cids, double *cw,
                               int32_t *games_played) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= new_games(n_bound, meta)) return;
    const int32_t *gp = players + (g0 + i) * MAXP;
    expand_game<true>(gp, places + (g0 + i) * MAXP, w[g0 + i], goff[i], cids, cw);
#pragma unroll
    for (int s = 0; s < MAXP; s++) {
        const int32_t id = gp[s];
        if (id >= 0 && id < MAXN) atomicAdd(&games_played[id], 1);   // integer: exact in any order
    }
}

// main.rs:755-790 on the device records: one block walks them in record order, a scan numbers
// the kept games (the append order is the record order)
__global__ void __launch_bounds__(1024) k_completions(const bppo_opp_completion *comp, const bppo::OppResults *res,
                                                      int cap, int32_t learner, Slots slots, int n_slots,
                                                      int32_t *players, int32_t *places, double *w, int64_t g0,
                                                      Meta *meta) {
    __shared__ uint64_t wsum[16];
    __shared__ int32_t s_slot[16];
    if (threadIdx.x < 16) s_slot[threadIdx.x] = slots.v[threadIdx.x];
    __syncthreads();
    const int kept = std::min(res->count, cap);   // the rollout keeps at most cap records
    uint64_t carry = 0;
    int max_id = -1, bad = 0;
    for (int b = 0; b < kept; b += blockDim.x) {
        const int i = b + threadIdx.x;
        bool keep = false;
        if (i < kept) {
            const bppo_opp_completion &c = comp[i];
            const int P = c.n_players, lp = c.learner_position;
            if (P < 1 || P > MAXP || lp < 0 || lp >= P) bad = 1;
            else {
                bool ok = true;
                int n_opp = 0;
#pragma unroll
                for (int s = 0; s < MAXP; s++) {
                    const int m = c.position_to_opponent[s];
                    if (s < P && m >= 0) {
                        n_opp++;
                        if (m >= n_slots) ok = false;
                        else keep = keep || s_slot[m] != learner;
                    }
                }
                if (!ok || n_opp >= MAXP) { bad = 1; keep = false; }
            }
        }
        uint64_t tot;
        const uint64_t ex = bppo::block_scan_excl(keep ? 1u : 0u, wsum, &tot);
        if (keep) {
            const bppo_opp_completion &c = comp[i];
            const int64_t g = g0 + (int64_t)(carry + ex);
            int32_t *op = players + g * MAXP, *oc = places + g * MAXP;
            op[0] = learner;
            oc[0] = c.placement[c.learner_position];
            max_id = std::max(max_id, learner);
            int k = 1;
#pragma unroll
            for (int s = 0; s < MAXP; s++) {
                const int m = c.position_to_opponent[s];
                if (s < c.n_players && m >= 0 && k < MAXP) {
                    const int32_t id = s_slot[m];
                    op[k] = id;
                    oc[k] = c.placement[s];
                    max_id = std::max(max_id, id);
                    k++;
                }
            }
#pragma unroll
            for (int q = 1; q < MAXP; q++)
                if (q >= k) { op[q] = -1; oc[q] = 0; }
            w[g] = 1.0;
        }
        carry += tot;
    }
    if (max_id >= 0) atomicMax(&meta->max_id, max_id);
    if (bad) atomicOr(&meta->bad, 1);
    if (threadIdx.x == 0) meta->added = (long long)carry;
}

// ------------------------------------------------- incidence list (stable counting sort) ---
// entry e = comparison * 6 + slot; its key is the player id in that slot (-1: empty)
__global__ void __launch_bounds__(256) k_hist(const int32_t *cids, int64_t E, int N, int32_t *cnt) {
    __shared__ int32_t h[MAXN];
    for (int p = threadIdx.x; p < N; p += blockDim.x) h[p] = 0;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * CH, e1 = std::min<int64_t>(e0 + CH, E);
    for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int32_t id = cids[e];
        if (id >= 0) atomicAdd(&h[id], 1);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < N; p += blockDim.x) cnt[(size_t)blockIdx.x * N + p] = h[p];
}

// per player: exclusive scan of its counts over the chunks (coalesced over players)
__global__ void k_chunk_scan(int32_t *cnt, int B, int N, int32_t *total) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    int32_t run = 0;
    for (int b = 0; b < B; b++) {
        const int32_t t = cnt[(size_t)b * N + p];
        cnt[(size_t)b * N + p] = run;
        run += t;
    }
    total[p] = run;
}

__global__ void __launch_bounds__(1024) k_off_scan(const int32_t *total, int N, int32_t *off) {
    __shared__ uint64_t wsum[16];
    const int p = threadIdx.x;
    uint64_t tot;
    const uint64_t ex = bppo::block_scan_excl(p < N ? (uint64_t)total[p] : 0, wsum, &tot);
    if (p < N) off[p] = (int32_t)ex;
    if (p == 0) off[N] = (int32_t)tot;
}

// one wave per chunk walks it in order, 64 entries at a time; an entry's rank among the tile's
// entries of the same player comes from ballots over the id's bits
__global__ void __launch_bounds__(64) k_fill(const int32_t *cids, int64_t E, int N, const int32_t *cnt,
                                             const int32_t *off, int32_t *list) {
    __shared__ int32_t cur[MAXN];
    const int lane = threadIdx.x;
    for (int p = lane; p < N; p += 64) cur[p] = off[p] + cnt[(size_t)blockIdx.x * N + p];
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * CH;
    for (int t = 0; t < CH / 64; t++) {
        const int64_t e = e0 + t * 64 + lane;
        if (e0 + t * 64 >= E) break;
        const int32_t id = e < E ? cids[e] : -1;
        const bool valid = id >= 0;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 10; bit++) {
            const bool mine = (id >> bit) & 1;
            const uint64_t bb = __ballot(valid && mine);
            peers &= mine ? bb : ~bb;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull)), tot = __popcll(peers);
        int32_t base = 0;
        if (valid) base = cur[id];
        __syncthreads();
        if (valid) {
            list[base + rank] = (int32_t)e;
            if (rank == tot - 1) cur[id] = base + tot;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------- fit kernels ---
// fixed tree over the block's 256 partial sums
__device__ __forceinline__ double block_tree_sum_256(double v, double *s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + h];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// With few players a list is long and a block per player leaves the GPU idle, so every per-player
// sum is cut into S = segments(N) equal pieces of the list, one block each (grid N x S), and the
// S partial sums are added in order.  A piece has at least SEG_MIN entries, so a list up to that
// length stays whole (the later blocks then add 0.0) and its sums keep the unsplit order.  The
// cut depends on N and on the list's length alone, so the sums' order does too.
constexpr int SEG_MIN = 1024;
__host__ __device__ inline int segments(int N) { return N >= 1024 ? 1 : (1024 / N > 16 ? 16 : 1024 / N); }

__device__ __forceinline__ void segment_range(const int32_t *off, int p, int &k0, int &k1) {
    const int a = off[p], b = off[p + 1], S = gridDim.y;
    const int L = std::max((b - a + S - 1) / S, SEG_MIN);
    k0 = std::min(a + (int)blockIdx.y * L, b);
    k1 = std::min(k0 + L, b);
}

// wins[p] = sum of the weights of the comparisons p won (slot 0), over p's list in order
__global__ void __launch_bounds__(256) k_wins(const int32_t *list, const int32_t *off, const double *cw, double *wins) {
    __shared__ double s[256];
    const int p = blockIdx.x;
    int k0, k1;
    segment_range(off, p, k0, k1);
    double acc = 0.0;
    for (int k = k0 + threadIdx.x; k < k1; k += 256) {
        const int32_t e = list[k];
        if (e % MAXP == 0) acc += cw[e / MAXP];
    }
    const double r = block_tree_sum_256(acc, s);
    if (threadIdx.x == 0) wins[p * gridDim.y + blockIdx.y] = r;
}

// per comparison: c = w / sum exp(gamma_p), the sum in slot order (mm_update, :286-294)
__global__ void k_cmp(const int32_t *cids, const double *cw, const double *expg, int64_t C, double eps, double *cval) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int32_t *ids = cids + c * MAXP;
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < MAXP; s++) {
        const int32_t id = ids[s];
        if (id >= 0) sum += expg[id];
    }
    cval[c] = sum > eps ? cw[c] / sum : 0.0;
}

// denom[p] = sum of c over the comparison slots p sits in
__global__ void __launch_bounds__(256) k_denom(const int32_t *list, const int32_t *off, const double *cval, double *denom) {
    __shared__ double s[256];
    const int p = blockIdx.x;
    int k0, k1;
    segment_range(off, p, k0, k1);
    double acc = 0.0;
    for (int k = k0 + threadIdx.x; k < k1; k += 256) acc += cval[list[k] / MAXP];
    const double r = block_tree_sum_256(acc, s);
    if (threadIdx.x == 0) denom[p * gridDim.y + blockIdx.y] = r;
}

// the N-wide tail of one MM iteration (:301-313, 511-523): three-branch update, mean, centring,
// max |delta|, finite check; writes gamma, exp(gamma) for the next iteration and the status pair
__global__ void __launch_bounds__(1024) k_tail(int N, int S, const double *wins, const double *denom, double *gamma,
                                               double *expg, double eps, double *status) {
    __shared__ double s[1024];
    const int p = threadIdx.x;
    double g = 0.0, ng = 0.0;
    if (p < N) {
        g = gamma[p];
        double w = 0.0, d = 0.0;
        for (int q = 0; q < S; q++) {      // the segments' partial sums, in order
            w += wins[p * S + q];
            d += denom[p * S + q];
        }
        if (w > eps && d > eps) ng = log(w / d);
        else if (d > eps) ng = g - 1.0;
        else ng = g;
    }
    s[p] = ng;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (p < h) s[p] = s[p] + s[p + h];
        __syncthreads();
    }
    const double mean = s[0] / (double)N;
    __syncthreads();
    const double c = ng - mean;
    s[p] = p < N ? fabs(g - c) : 0.0;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (p < h) s[p] = fmax(s[p], s[p + h]);   // f64::max: a NaN operand is ignored
        __syncthreads();
    }
    const int nonfinite = __syncthreads_or(p < N && !isfinite(c));
    if (p < N) {
        gamma[p] = c;
        expg[p] = exp(c);
    }
    if (p == 0) {
        status[0] = s[0];
        status[1] = nonfinite ? 0.0 : 1.0;
    }
}

// Fisher information (:320-353), row i by block i: the block walks player i's incidence list in
// order, 256 entries at a time (each thread computes one entry's softmax and its <= 6 column
// terms), then every thread applies, in list order, the terms of the columns it owns
// (column & 255 == thread): no atomics, and each element's sum runs in the reference's order
// within a segment of the list.  Block (i, s) writes segment s's partial row to H[s][i][...].
__global__ void __launch_bounds__(256) k_hess(const int32_t *list, const int32_t *off, const int32_t *cids,
                                              const double *cw, const double *gamma, int N, double *H) {
    __shared__ double row[MAXN];
    __shared__ double s_val[256][MAXP];
    __shared__ int32_t s_col[256][MAXP];
    const int i = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < N; j += 256) row[j] = 0.0;
    int k0, k1;
    segment_range(off, i, k0, k1);
    for (int kb = k0; kb < k1; kb += 256) {
        __syncthreads();
        const int k = kb + tid;
        if (k < k1) {
            const int32_t e = list[k];
            const int li = e % MAXP;
            const int64_t c = e / MAXP;
            const int32_t *ids = cids + c * MAXP;
            int32_t id[MAXP];
            double x[MAXP];
            double mx = -INFINITY;
#pragma unroll
            for (int s = 0; s < MAXP; s++) {
                id[s] = ids[s];
                x[s] = id[s] >= 0 ? gamma[id[s]] : 0.0;
                if (id[s] >= 0) mx = fmax(mx, x[s]);
            }
            double sum = 0.0;
            int n = 0;
#pragma unroll
            for (int s = 0; s < MAXP; s++)
                if (id[s] >= 0) {
                    x[s] = exp(x[s] - mx);
                    sum += x[s];
                    n++;
                }
            double pi = 0.0;
#pragma unroll
            for (int s = 0; s < MAXP; s++) {
                x[s] = sum == 0.0 ? 1.0 / (double)n : x[s] / sum;
                if (s == li) pi = x[s];
            }
            const double w = cw[c];
#pragma unroll
            for (int s = 0; s < MAXP; s++) {
                s_col[tid][s] = id[s];
                s_val[tid][s] = s == li ? w * pi * (1.0 - pi) : -(w * pi * x[s]);
            }
        }
        __syncthreads();
        const int m = std::min(256, k1 - kb);
        for (int q = 0; q < m; q++) {
#pragma unroll
            for (int s = 0; s < MAXP; s++) {
                const int32_t col = s_col[q][s];
                if (col >= 0 && (col & 255) == tid) row[col] += s_val[q][s];
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < N; j += 256) H[((size_t)blockIdx.y * N + i) * N + j] = row[j];
}

// H[0] += H[1] + ... + H[S - 1], element by element in segment order
__global__ void k_hess_reduce(double *H, int64_t NN, int S) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= NN) return;
    double acc = H[k];
    for (int s = 1; s < S; s++) acc += H[(size_t)s * NN + k];
    H[k] = acc;
}

// ------------------------------------------------------------------------ host ---
// invert_matrix (:361-425): Gauss-Jordan with partial pivoting on [A | I], its elimination order
// (row swaps through a row-pointer table: the same values in the same places)
std::vector<double> invert_matrix(const std::vector<double> &a, int n, double epsilon) {
    std::vector<double> inv((size_t)n * n, 0.0);
    if (n == 0) return inv;
    const int w = 2 * n;
    std::vector<double> aug((size_t)n * w, 0.0);
    std::vector<double *> rows(n);
    for (int i = 0; i < n; i++) {
        std::memcpy(&aug[(size_t)i * w], &a[(size_t)i * n], sizeof(double) * n);
        aug[(size_t)i * w + n + i] = 1.0;
        rows[i] = &aug[(size_t)i * w];
    }
    for (int col = 0; col < n; col++) {
        int max_row = col;
        double max_val = std::fabs(rows[col][col]);
        for (int row = col + 1; row < n; row++)
            if (std::fabs(rows[row][col]) > max_val) {
                max_val = std::fabs(rows[row][col]);
                max_row = row;
            }
        std::swap(rows[col], rows[max_row]);
        if (std::fabs(rows[col][col]) < epsilon) {
            std::fill(inv.begin(), inv.end(), 0.0);
            for (int i = 0; i < n; i++) inv[(size_t)i * n + i] = 100.0;
            return inv;
        }
        double *pr = rows[col];
        const double pivot = pr[col];
        for (int j = 0; j < w; j++) pr[j] /= pivot;
        for (int row = 0; row < n; row++) {
            if (row == col) continue;
            double *rr = rows[row];
            const double factor = rr[col];
            for (int j = 0; j < w; j++) rr[j] -= factor * pr[j];
        }
    }
    for (int i = 0; i < n; i++) std::memcpy(&inv[(size_t)i * n], rows[i] + n, sizeof(double) * n);
    return inv;
}

// :537-603 from the fitted gammas, the Fisher information and games_played
void finish_ratings(const bppo_pl_config &cfg, int N, int anchor, const std::vector<double> &gammas,
                    const std::vector<double> &hessian, const std::vector<int32_t> &games_played, double *rating,
                    double *uncertainty) {
    std::vector<int> active;
    for (int i = 0; i < N; i++)
        if (games_played[i] > 0 && i != anchor) active.push_back(i);
    const int R = (int)active.size();
    std::vector<double> red((size_t)R * R);
    for (int ri = 0; ri < R; ri++) {
        for (int rj = 0; rj < R; rj++) red[(size_t)ri * R + rj] = hessian[(size_t)active[ri] * N + active[rj]];
        red[(size_t)ri * R + ri] += 1e-6;
    }
    const std::vector<double> cov = invert_matrix(red, R, cfg.epsilon);
    std::vector<double> unc(N, 2.0);
    unc[anchor] = 0.0;
    for (int ri = 0; ri < R; ri++)
        if (cov[(size_t)ri * R + ri] > 0.0) unc[active[ri]] = std::sqrt(cov[(size_t)ri * R + ri]);
    const double target = (cfg.anchor_elo - 1500.0) / ELO_SCALE;
    const double shift = target - gammas[anchor];
    for (int i = 0; i < N; i++) {
        if (games_played[i] > 0) {
            rating[i] = 1500.0 + ELO_SCALE * (gammas[i] + shift);
            uncertainty[i] = (ELO_SCALE * unc[i]) * cfg.ci_inflation_factor;
        } else {
            rating[i] = cfg.anchor_elo;
            uncertainty[i] = 350.0;
        }
    }
}

}  // namespace

struct bppo_ratings {
    int dev = -1;                      // -1: host-only
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    bppo::DeviceMem mem;               // the device and pinned buffers below
    // host mirror of the games [h_games][6]: complete for add_games; games appended on the
    // device by add_completions are fetched when a host fit (or a later add_games) needs them
    std::vector<int32_t> h_players, h_places;
    std::vector<double> h_w;
    int64_t h_games = 0;
    int64_t n_games = 0, n_cmp = 0;
    int32_t max_id = -1;
    // device
    int32_t *d_players = nullptr, *d_places = nullptr;
    double *d_w = nullptr;
    int64_t g_cap = 0;
    int32_t *d_cids = nullptr;
    double *d_cw = nullptr;
    int64_t c_cap = 0;
    int32_t *d_gp = nullptr;           // games_played [MAXN]
    int32_t *d_cnt = nullptr;          // expansion counts of one append
    int64_t *d_goff = nullptr;
    int64_t x_cap = 0;
    Meta *d_meta = nullptr, *h_meta = nullptr;
    double *d_vec = nullptr;           // gamma, expg, wins, denom [4][MAXN], status [2]
    double *h_status = nullptr;
    hipEvent_t ev = nullptr;
    // incidence list
    bool csr_valid = false;
    int csr_N = 0;
    int32_t *d_list = nullptr, *d_off = nullptr, *d_total = nullptr, *d_hist = nullptr;
    int64_t list_cap = 0, hist_cap = 0;
    double *d_cval = nullptr, *d_H = nullptr;
    int64_t cval_cap = 0, H_cap = 0;
    // wall time of the last fit's phases: incidence list (host backend: expansion), MM iterations,
    // Fisher information (with its copy to the host), host inversion + Elo conversion
    double phase_ms[4] = {0, 0, 0, 0};
};

namespace {

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

#define RHIP(r, expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            (r)->err = std::string(#expr) + ": " + hipGetErrorString(_e);              \
            return BPPO_ERR_HIP;                                                       \
        }                                                                              \
    } while (0)

bppo_status arg_err(bppo_ratings *r, const std::string &msg) {
    r->err = msg;
    return BPPO_ERR_ARG;
}

// grow a device array to hold `need` elements, keeping the first `keep`
template <typename T>
bppo_status grow(bppo_ratings *r, T **p, int64_t *cap, int64_t need, int64_t keep, int64_t width) {
    if (need <= *cap) return BPPO_OK;
    const int64_t ncap = std::max<int64_t>(need, std::max<int64_t>(*cap * 2, 1024));
    T *q = nullptr;
    RHIP(r, r->mem.alloc(&q, (size_t)ncap * width));
    if (*p && keep > 0) RHIP(r, hipMemcpyAsync(q, *p, sizeof(T) * (size_t)keep * width, hipMemcpyDeviceToDevice, r->stream));
    RHIP(r, hipStreamSynchronize(r->stream));
    RHIP(r, r->mem.release(*p));
    *p = q;
    *cap = ncap;
    return BPPO_OK;
}

bppo_status reserve_games(bppo_ratings *r, int64_t extra, int P) {
    const int64_t need = r->n_games + extra;
    if (need > r->g_cap) {
        const int64_t keep = r->n_games;
        int64_t c1 = r->g_cap, c2 = r->g_cap, c3 = r->g_cap;
        TRY(grow(r, &r->d_players, &c1, need, keep, MAXP));
        TRY(grow(r, &r->d_places, &c2, need, keep, MAXP));
        TRY(grow(r, &r->d_w, &c3, need, keep, 1));
        r->g_cap = c1;
    }
    const int64_t cneed = r->n_cmp + extra * std::max(P - 1, 1);
    if (cneed * MAXP >= (int64_t)std::numeric_limits<int32_t>::max()) {
        r->err = "ratings: more than 2^31 / 6 comparisons";
        return BPPO_ERR_UNSUPPORTED;
    }
    if (cneed > r->c_cap) {
        int64_t c1 = r->c_cap, c2 = r->c_cap;
        TRY(grow(r, &r->d_cids, &c1, cneed, r->n_cmp, MAXP));
        TRY(grow(r, &r->d_cw, &c2, cneed, r->n_cmp, 1));
        r->c_cap = c1;
    }
    if (extra > r->x_cap) {
        int64_t c1 = r->x_cap, c2 = r->x_cap;
        TRY(grow(r, &r->d_cnt, &c1, extra, 0, 1));
        TRY(grow(r, &r->d_goff, &c2, extra, 0, 1));
        r->x_cap = c1;
    }
    return BPPO_OK;
}

// expand the games [n_games, n_games + n) already in device memory (n from *meta when given)
bppo_status launch_expand(bppo_ratings *r, int64_t n_bound, const Meta *meta) {
    if (n_bound <= 0) return BPPO_OK;
    const int blocks = (int)((n_bound + 255) / 256);
    hipLaunchKernelGGL(k_expand_count, dim3(blocks), dim3(256), 0, r->stream, r->d_players, r->d_places, r->n_games,
                       n_bound, meta, r->d_cnt);
    hipLaunchKernelGGL(k_expand_scan, dim3(1), dim3(1024), 0, r->stream, r->d_cnt, n_bound, meta, r->n_cmp, r->d_goff,
                       r->d_meta);
    hipLaunchKernelGGL(k_expand_write, dim3(blocks), dim3(256), 0, r->stream, r->d_players, r->d_places, r->d_w,
                       r->n_games, n_bound, meta, r->d_goff, r->d_cids, r->d_cw, r->d_gp);
    RHIP(r, hipGetLastError());
    return BPPO_OK;
}

// bring the host mirror up to n_games (games add_completions appended on the device)
bppo_status sync_mirror(bppo_ratings *r) {
    if (r->h_games >= r->n_games) return BPPO_OK;
    const int64_t a = r->h_games, m = r->n_games - a;
    r->h_players.resize((size_t)r->n_games * MAXP);
    r->h_places.resize((size_t)r->n_games * MAXP);
    r->h_w.resize((size_t)r->n_games);
    RHIP(r, hipMemcpyAsync(&r->h_players[(size_t)a * MAXP], r->d_players + a * MAXP, sizeof(int32_t) * (size_t)m * MAXP,
                           hipMemcpyDeviceToHost, r->stream));
    RHIP(r, hipMemcpyAsync(&r->h_places[(size_t)a * MAXP], r->d_places + a * MAXP, sizeof(int32_t) * (size_t)m * MAXP,
                           hipMemcpyDeviceToHost, r->stream));
    RHIP(r, hipMemcpyAsync(&r->h_w[(size_t)a], r->d_w + a, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, r->stream));
    RHIP(r, hipStreamSynchronize(r->stream));
    r->h_games = r->n_games;
    return BPPO_OK;
}

bppo_status build_csr(bppo_ratings *r, int N) {
    if (r->csr_valid && r->csr_N == N) return BPPO_OK;
    const int64_t E = r->n_cmp * MAXP;
    const int B = (int)((E + CH - 1) / CH);
    {
        int64_t c = r->list_cap;
        TRY(grow(r, &r->d_list, &c, E, 0, 1));
        r->list_cap = c;
        c = r->hist_cap;
        TRY(grow(r, &r->d_hist, &c, (int64_t)B * N, 0, 1));
        r->hist_cap = c;
    }
    hipLaunchKernelGGL(k_hist, dim3(B), dim3(256), 0, r->stream, r->d_cids, E, N, r->d_hist);
    hipLaunchKernelGGL(k_chunk_scan, dim3((N + 255) / 256), dim3(256), 0, r->stream, r->d_hist, B, N, r->d_total);
    hipLaunchKernelGGL(k_off_scan, dim3(1), dim3(1024), 0, r->stream, r->d_total, N, r->d_off);
    hipLaunchKernelGGL(k_fill, dim3(B), dim3(64), 0, r->stream, r->d_cids, E, N, r->d_hist, r->d_off, r->d_list);
    RHIP(r, hipGetLastError());
    r->csr_valid = true;
    r->csr_N = N;
    return BPPO_OK;
}

struct FitOut {
    bool converged = false;
    int iterations = 0;
    double final_delta = std::numeric_limits<double>::max();
    std::vector<double> gammas, hessian;
    std::vector<int32_t> games_played;
};

bppo_status fit_device(bppo_ratings *r, const bppo_pl_config &cfg, int N, FitOut &o) {
    RHIP(r, hipSetDevice(r->dev));
    auto t0 = Clock::now();
    const int S = segments(N);           // N * S <= 1024: the partial sums fit the [MAXN] arrays
    const bool rebuilt = !(r->csr_valid && r->csr_N == N);
    TRY(build_csr(r, N));
    if (rebuilt) RHIP(r, hipStreamSynchronize(r->stream));   // only to time the phase
    r->phase_ms[0] = ms_since(t0);
    t0 = Clock::now();
    {
        int64_t c = r->cval_cap;
        TRY(grow(r, &r->d_cval, &c, r->n_cmp, 0, 1));
        r->cval_cap = c;
        c = r->H_cap;
        TRY(grow(r, &r->d_H, &c, (int64_t)S * N * N, 0, 1));
        r->H_cap = c;
    }
    double *gamma = r->d_vec, *expg = r->d_vec + MAXN, *wins = r->d_vec + 2 * MAXN, *denom = r->d_vec + 3 * MAXN,
           *status = r->d_vec + 4 * MAXN;
    std::vector<double> ones(N, 1.0);   // exp(0)
    RHIP(r, hipMemsetAsync(gamma, 0, sizeof(double) * MAXN, r->stream));
    RHIP(r, hipMemcpyAsync(expg, ones.data(), sizeof(double) * N, hipMemcpyHostToDevice, r->stream));
    hipLaunchKernelGGL(k_wins, dim3(N, S), dim3(256), 0, r->stream, r->d_list, r->d_off, r->d_cw, wins);
    const int cblocks = (int)((r->n_cmp + 255) / 256);
    for (int it = 0; it < cfg.max_iterations; it++) {
        o.iterations = it + 1;
        hipLaunchKernelGGL(k_cmp, dim3(cblocks), dim3(256), 0, r->stream, r->d_cids, r->d_cw, expg, r->n_cmp, cfg.epsilon,
                           r->d_cval);
        hipLaunchKernelGGL(k_denom, dim3(N, S), dim3(256), 0, r->stream, r->d_list, r->d_off, r->d_cval, denom);
        hipLaunchKernelGGL(k_tail, dim3(1), dim3(1024), 0, r->stream, N, S, wins, denom, gamma, expg, cfg.epsilon, status);
        RHIP(r, hipMemcpyAsync(r->h_status, status, 2 * sizeof(double), hipMemcpyDeviceToHost, r->stream));
        RHIP(r, hipStreamSynchronize(r->stream));
        o.final_delta = r->h_status[0];
        if (o.final_delta < cfg.convergence_threshold) {
            o.converged = true;
            break;
        }
        if (r->h_status[1] == 0.0) {
            RHIP(r, hipMemsetAsync(gamma, 0, sizeof(double) * MAXN, r->stream));
            break;
        }
    }
    r->phase_ms[1] = ms_since(t0);
    t0 = Clock::now();
    hipLaunchKernelGGL(k_hess, dim3(N, S), dim3(256), 0, r->stream, r->d_list, r->d_off, r->d_cids, r->d_cw, gamma, N, r->d_H);
    if (S > 1)
        hipLaunchKernelGGL(k_hess_reduce, dim3((N * N + 255) / 256), dim3(256), 0, r->stream, r->d_H, (int64_t)N * N, S);
    RHIP(r, hipGetLastError());
    o.gammas.resize(N);
    o.hessian.resize((size_t)N * N);
    o.games_played.resize(N);
    RHIP(r, hipMemcpyAsync(o.gammas.data(), gamma, sizeof(double) * N, hipMemcpyDeviceToHost, r->stream));
    RHIP(r, hipMemcpyAsync(o.hessian.data(), r->d_H, sizeof(double) * (size_t)N * N, hipMemcpyDeviceToHost, r->stream));
    RHIP(r, hipMemcpyAsync(o.games_played.data(), r->d_gp, sizeof(int32_t) * N, hipMemcpyDeviceToHost, r->stream));
    RHIP(r, hipStreamSynchronize(r->stream));
    r->phase_ms[2] = ms_since(t0);
    return BPPO_OK;
}

// the reference's arithmetic in its order (:271-353, 507-535)
void fit_host(bppo_ratings *r, const bppo_pl_config &cfg, int N, FitOut &o) {
    auto t0 = Clock::now();
    const int64_t G = r->n_games;
    std::vector<int32_t> cids((size_t)r->n_cmp * MAXP);
    std::vector<double> cw((size_t)r->n_cmp);
    o.games_played.assign(N, 0);
    int64_t c = 0;
    for (int64_t g = 0; g < G; g++) {
        const int32_t *gp = &r->h_players[(size_t)g * MAXP];
        c += expand_game<true>(gp, &r->h_places[(size_t)g * MAXP], r->h_w[(size_t)g], c, cids.data(), cw.data());
        for (int s = 0; s < MAXP; s++)
            if (gp[s] >= 0 && gp[s] < N) o.games_played[gp[s]]++;
    }
    const int64_t C = r->n_cmp;
    r->phase_ms[0] = ms_since(t0);
    t0 = Clock::now();
    std::vector<double> gammas(N, 0.0), wins(N), denom(N), ng(N);
    for (int it = 0; it < cfg.max_iterations; it++) {
        o.iterations = it + 1;
        std::fill(wins.begin(), wins.end(), 0.0);
        std::fill(denom.begin(), denom.end(), 0.0);
        for (int64_t k = 0; k < C; k++) {
            const int32_t *ids = &cids[(size_t)k * MAXP];
            wins[ids[0]] += cw[k];
            double sum_exp = 0.0;
            for (int s = 0; s < MAXP && ids[s] >= 0; s++) sum_exp += std::exp(gammas[ids[s]]);
            if (sum_exp > cfg.epsilon) {
                const double contribution = cw[k] / sum_exp;
                for (int s = 0; s < MAXP && ids[s] >= 0; s++) denom[ids[s]] += contribution;
            }
        }
        for (int i = 0; i < N; i++) {
            if (wins[i] > cfg.epsilon && denom[i] > cfg.epsilon) ng[i] = std::log(wins[i] / denom[i]);
            else if (denom[i] > cfg.epsilon) ng[i] = gammas[i] - 1.0;
            else ng[i] = gammas[i];
        }
        double sum = 0.0;
        for (int i = 0; i < N; i++) sum += ng[i];
        const double mean = sum / (double)N;
        double max_change = 0.0;
        bool finite = true;
        for (int i = 0; i < N; i++) {
            const double cen = ng[i] - mean;
            max_change = std::fmax(max_change, std::fabs(gammas[i] - cen));
            gammas[i] = cen;
            finite = finite && std::isfinite(cen);
        }
        o.final_delta = max_change;
        if (max_change < cfg.convergence_threshold) {
            o.converged = true;
            break;
        }
        if (!finite) {
            std::fill(gammas.begin(), gammas.end(), 0.0);
            break;
        }
    }
    r->phase_ms[1] = ms_since(t0);
    t0 = Clock::now();
    o.hessian.assign((size_t)N * N, 0.0);
    for (int64_t k = 0; k < C; k++) {
        const int32_t *ids = &cids[(size_t)k * MAXP];
        int n = 0;
        double x[MAXP], mx = -INFINITY;
        for (; n < MAXP && ids[n] >= 0; n++) mx = std::fmax(mx, gammas[ids[n]]);
        double sum = 0.0;
        for (int s = 0; s < n; s++) {
            x[s] = std::exp(gammas[ids[s]] - mx);
            sum += x[s];
        }
        for (int s = 0; s < n; s++) x[s] = sum == 0.0 ? 1.0 / (double)n : x[s] / sum;
        for (int a = 0; a < n; a++)
            for (int b = 0; b < n; b++) {
                double &h = o.hessian[(size_t)ids[a] * N + ids[b]];
                if (a == b) h += cw[k] * x[a] * (1.0 - x[a]);
                else h -= cw[k] * x[a] * x[b];
            }
    }
    o.gammas = gammas;
    r->phase_ms[2] = ms_since(t0);
}

}  // namespace

extern "C" size_t bppo_pl_config_size(void) { return sizeof(bppo_pl_config); }
extern "C" size_t bppo_pl_stats_size(void) { return sizeof(bppo_pl_stats); }

extern "C" void bppo_ratings_destroy(bppo_ratings *r) {
    if (!r) return;
    // a host-only table holds none of these (no HIP call); one whose device initialisation
    // failed part-way (dev -2) gives back what it got
    if (r->dev >= 0) (void)hipSetDevice(r->dev);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    r->mem.free_all();
    if (r->ev) (void)hipEventDestroy(r->ev);
    if (r->own_stream && r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

static bppo_status ratings_init_device(bppo_ratings *r, void *hip_stream) {
    RHIP(r, hipSetDevice(r->dev));
    if (hip_stream) r->stream = (hipStream_t)hip_stream;
    else {
        RHIP(r, hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
        r->own_stream = true;
    }
    RHIP(r, r->mem.alloc(&r->d_gp, MAXN));
    RHIP(r, r->mem.alloc(&r->d_meta, 1));
    RHIP(r, r->mem.alloc(&r->d_vec, 4 * MAXN + 2));
    RHIP(r, r->mem.alloc(&r->d_off, MAXN + 1));
    RHIP(r, r->mem.alloc(&r->d_total, MAXN));
    RHIP(r, r->mem.alloc_pinned(&r->h_meta, 1));
    RHIP(r, r->mem.alloc_pinned(&r->h_status, 2));
    RHIP(r, hipEventCreateWithFlags(&r->ev, hipEventDisableTiming));
    RHIP(r, hipMemsetAsync(r->d_gp, 0, sizeof(int32_t) * MAXN, r->stream));
    RHIP(r, hipStreamSynchronize(r->stream));
    return BPPO_OK;
}

extern "C" bppo_status bppo_ratings_create(int hip_device, void *hip_stream, bppo_ratings **out) {
    if (!out) return BPPO_ERR_ARG;
    bppo_ratings *r = new bppo_ratings();
    *out = r;
    if (hip_device < -1) return arg_err(r, "ratings_create: hip_device < -1");
    r->dev = hip_device;
    if (hip_device >= 0) {
        const bppo_status s = ratings_init_device(r, hip_stream);
        if (s != BPPO_OK) r->dev = -2;   // a table that failed to initialise takes no calls
        return s;
    }
    return BPPO_OK;
}

extern "C" const char *bppo_ratings_last_error(const bppo_ratings *r) { return r ? r->err.c_str() : ""; }

extern "C" bppo_status bppo_ratings_clear(bppo_ratings *r) {
    if (!r || r->dev == -2) return BPPO_ERR_ARG;
    r->h_players.clear();
    r->h_places.clear();
    r->h_w.clear();
    r->h_games = r->n_games = r->n_cmp = 0;
    r->max_id = -1;
    r->csr_valid = false;
    if (r->dev >= 0) {
        RHIP(r, hipSetDevice(r->dev));
        RHIP(r, hipMemsetAsync(r->d_gp, 0, sizeof(int32_t) * MAXN, r->stream));
        RHIP(r, hipStreamSynchronize(r->stream));
    }
    return BPPO_OK;
}

extern "C" bppo_status bppo_ratings_last_fit_phases(const bppo_ratings *r, double *ms4) {
    if (!r || !ms4) return BPPO_ERR_ARG;
    std::memcpy(ms4, r->phase_ms, sizeof r->phase_ms);
    return BPPO_OK;
}

extern "C" bppo_status bppo_ratings_num_games(const bppo_ratings *r, int64_t *n) {
    if (!r || !n) return BPPO_ERR_ARG;
    *n = r->n_games;
    return BPPO_OK;
}

extern "C" bppo_status bppo_ratings_add_games(bppo_ratings *r, int64_t n, int32_t P, const int32_t *players,
                                              const int32_t *placements, const double *weight) {
    if (!r || r->dev == -2) return BPPO_ERR_ARG;
    if (P < 1 || P > MAXP) return arg_err(r, "ratings_add_games: P outside 1..6");
    if (n < 0 || (n > 0 && (!players || !placements))) return arg_err(r, "ratings_add_games: n < 0 or no games given");
    if (n == 0) return BPPO_OK;
    // validate everything before anything is appended
    std::vector<int32_t> pl((size_t)n * MAXP, -1), pc((size_t)n * MAXP, 0);
    std::vector<double> w((size_t)n, 1.0);
    int32_t max_id = r->max_id;
    int64_t new_cmp = 0;
    for (int64_t g = 0; g < n; g++) {
        bool ended = false;
        for (int s = 0; s < P; s++) {
            const int32_t id = players[g * P + s];
            if (id < -1) return arg_err(r, "ratings_add_games: player id < -1 in game " + std::to_string(g));
            if (id == -1) { ended = true; continue; }
            if (ended) return arg_err(r, "ratings_add_games: player id after a -1 in game " + std::to_string(g));
            if (placements[g * P + s] < 1) return arg_err(r, "ratings_add_games: placement < 1 in game " + std::to_string(g));
            pl[(size_t)g * MAXP + s] = id;
            pc[(size_t)g * MAXP + s] = placements[g * P + s];
            max_id = std::max(max_id, id);
        }
        if (weight) {
            if (!std::isfinite(weight[g]) || !(weight[g] > 0.0))
                return arg_err(r, "ratings_add_games: non-finite or non-positive weight in game " + std::to_string(g));
            w[(size_t)g] = weight[g];
        }
        new_cmp += expand_game<false>(&pl[(size_t)g * MAXP], &pc[(size_t)g * MAXP], 1.0, 0, nullptr, nullptr);
    }
    if (r->dev >= 0) {
        RHIP(r, hipSetDevice(r->dev));
        TRY(sync_mirror(r));
        TRY(reserve_games(r, n, P));
        RHIP(r, hipMemcpyAsync(r->d_players + r->n_games * MAXP, pl.data(), sizeof(int32_t) * pl.size(), hipMemcpyHostToDevice, r->stream));
        RHIP(r, hipMemcpyAsync(r->d_places + r->n_games * MAXP, pc.data(), sizeof(int32_t) * pc.size(), hipMemcpyHostToDevice, r->stream));
        RHIP(r, hipMemcpyAsync(r->d_w + r->n_games, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, r->stream));
        TRY(launch_expand(r, n, nullptr));
        RHIP(r, hipStreamSynchronize(r->stream));   // pl / pc / w are pageable and leave scope
    }
    r->h_players.insert(r->h_players.end(), pl.begin(), pl.end());
    r->h_places.insert(r->h_places.end(), pc.begin(), pc.end());
    r->h_w.insert(r->h_w.end(), w.begin(), w.end());
    r->n_games += n;
    r->h_games = r->n_games;
    r->n_cmp += new_cmp;
    r->max_id = max_id;
    r->csr_valid = false;
    return BPPO_OK;
}

extern "C" bppo_status bppo_ratings_add_completions(bppo_ratings *r, bppo_ctx *c, int32_t learner_player,
                                                    const int32_t *slot_to_player, int32_t n_slots, int64_t *added) {
    if (!r || r->dev == -2) return BPPO_ERR_ARG;
    if (added) *added = 0;
    if (r->dev < 0) return arg_err(r, "ratings_add_completions: a host-only table");
    if (!c) return arg_err(r, "ratings_add_completions: no context");
    if (c->dev != r->dev) return arg_err(r, "ratings_add_completions: the context is on another device");
    if (!c->d_comp || !c->d_opp_res) return arg_err(r, "ratings_add_completions: no opponents set");
    if (learner_player < 0) return arg_err(r, "ratings_add_completions: learner_player < 0");
    if (n_slots < 1 || n_slots > 16 || !slot_to_player) return arg_err(r, "ratings_add_completions: n_slots outside 1..16");
    Slots slots;
    for (int k = 0; k < 16; k++) {
        slots.v[k] = k < n_slots ? slot_to_player[k] : 0;
        if (slots.v[k] < 0) return arg_err(r, "ratings_add_completions: slot_to_player < 0");
    }
    RHIP(r, hipSetDevice(r->dev));
    const int64_t bound = c->eps_cap;     // the rollout keeps at most this many records
    TRY(reserve_games(r, bound, MAXP));
    // after the context's stream: the records are the last rollout's
    RHIP(r, hipEventRecord(r->ev, c->stream));
    RHIP(r, hipStreamWaitEvent(r->stream, r->ev, 0));
    const Meta zero = {0, 0, -1, 0};
    *r->h_meta = zero;
    RHIP(r, hipMemcpyAsync(r->d_meta, r->h_meta, sizeof(Meta), hipMemcpyHostToDevice, r->stream));
    hipLaunchKernelGGL(k_completions, dim3(1), dim3(1024), 0, r->stream, c->d_comp, c->d_opp_res, (int)c->eps_cap,
                       learner_player, slots, (int)n_slots, r->d_players, r->d_places, r->d_w, r->n_games, r->d_meta);
    RHIP(r, hipGetLastError());
    TRY(launch_expand(r, bound, r->d_meta));
    RHIP(r, hipMemcpyAsync(r->h_meta, r->d_meta, sizeof(Meta), hipMemcpyDeviceToHost, r->stream));
    RHIP(r, hipStreamSynchronize(r->stream));
    const Meta m = *r->h_meta;
    if (m.bad) {
        // nothing is kept: the games past n_games are overwritten by the next append, the
        // games_played counts of this call are taken back by a rebuild
        r->err = "ratings_add_completions: a record names a model slot >= n_slots or a seat out of range";
        std::vector<int32_t> gp(MAXN, 0);
        TRY(sync_mirror(r));
        for (size_t k = 0; k < r->h_players.size(); k++)
            if (r->h_players[k] >= 0 && r->h_players[k] < MAXN) gp[r->h_players[k]]++;
        RHIP(r, hipMemcpyAsync(r->d_gp, gp.data(), sizeof(int32_t) * MAXN, hipMemcpyHostToDevice, r->stream));
        RHIP(r, hipStreamSynchronize(r->stream));
        return BPPO_ERR_ARG;
    }
    r->n_games += m.added;
    r->n_cmp += m.new_cmp;
    r->max_id = std::max(r->max_id, (int32_t)m.max_id);
    if (m.added > 0) r->csr_valid = false;
    if (added) *added = m.added;
    return BPPO_OK;
}

extern "C" bppo_status bppo_ratings_fit(bppo_ratings *r, const bppo_pl_config *cfg, int32_t num_players, int32_t anchor,
                                        double *rating, double *uncertainty, double *gamma, bppo_pl_stats *stats) {
    if (!r || r->dev == -2) return BPPO_ERR_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    if (!cfg) return arg_err(r, "ratings_fit: no config");
    if (cfg->backend != 0 && cfg->backend != 1) return arg_err(r, "ratings_fit: backend is 0 (device) or 1 (host)");
    if (cfg->backend == 0 && r->dev < 0) return arg_err(r, "ratings_fit: backend 0 (device) on a host-only table");
    if (num_players < 0) return arg_err(r, "ratings_fit: num_players < 0");
    if (num_players > MAXN) return arg_err(r, "ratings_fit: num_players > 1024");
    if (cfg->max_iterations < 0) return arg_err(r, "ratings_fit: max_iterations < 0");
    bppo_pl_stats st = {1, 0, 0.0, 0.0, r->n_games, r->n_cmp};
    auto done = [&]() {
        st.fit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = st;
        return BPPO_OK;
    };
    if (num_players == 0) return done();                                   // :452-460
    if (anchor < 0 || anchor >= num_players) return arg_err(r, "ratings_fit: anchor outside [0, num_players)");
    if (r->max_id >= num_players)
        return arg_err(r, "ratings_fit: a stored player id (" + std::to_string(r->max_id) + ") >= num_players");
    if (!rating || !uncertainty) return arg_err(r, "ratings_fit: no output arrays");
    if (r->n_games == 0 || r->n_cmp == 0) {                                // :463-497
        for (int i = 0; i < num_players; i++) {
            rating[i] = cfg->anchor_elo;
            uncertainty[i] = 350.0;
            if (gamma) gamma[i] = 0.0;
        }
        return done();
    }
    FitOut o;
    if (cfg->backend == 0) TRY(fit_device(r, *cfg, num_players, o));
    else {
        if (r->dev >= 0) {
            RHIP(r, hipSetDevice(r->dev));
            TRY(sync_mirror(r));
        }
        fit_host(r, *cfg, num_players, o);
    }
    const auto t1 = Clock::now();
    finish_ratings(*cfg, num_players, anchor, o.gammas, o.hessian, o.games_played, rating, uncertainty);
    r->phase_ms[3] = ms_since(t1);
    if (gamma) std::memcpy(gamma, o.gammas.data(), sizeof(double) * num_players);
    st.converged = o.converged ? 1 : 0;
    st.iterations_used = o.iterations;
    st.final_delta = o.final_delta;
    return done();
}
