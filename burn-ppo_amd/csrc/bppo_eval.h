// bppo_eval.h — the arithmetic of stats-mode evaluation (eval.rs) shared verbatim
// between host C++ and HIP device code, like bppo_math.h: the temperature schedule
// (TempSchedule::get_temp, eval.rs:200-216) and sample_with_temperature
// (eval.rs:223-272).  Every f32 operation is one explicit IEEE operation (the
// device intrinsics; plain operators on the host, built with -ffp-contract=off).
// Subnormal exp results must survive: nothing on this path flushes f32 denormals
// (hipcc's default kernel mode keeps them; the Makefile does not ask for flushing).
// At the end, the host steps the two evaluation loops share: a pod's RNG key and env
// seed base, the staging of recorded games.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/bppo.h"
#include "bppo_device.h"
#include "bppo_math.h"

namespace bppo_eval {

#if defined(__HIP_DEVICE_COMPILE__)
BPPO_HD float f_add(float a, float b) { return __fadd_rn(a, b); }
BPPO_HD float f_sub(float a, float b) { return __fsub_rn(a, b); }
BPPO_HD float f_div(float a, float b) { return __fdiv_rn(a, b); }
#else
BPPO_HD float f_add(float a, float b) { return a + b; }
BPPO_HD float f_sub(float a, float b) { return a - b; }
BPPO_HD float f_div(float a, float b) { return a / b; }
#endif

struct TempSched {
    float initial, final_temp;
    int32_t cutoff;   // -1: None
    int32_t decay;
};

// eval.rs:200-216.  The decay is t.mul_add(final - initial, initial), one fma, with
// t = move as f32 / cutoff as f32.
BPPO_HD float get_temp(const TempSched &s, int move_num) {
    if (s.cutoff < 0) return s.initial;
    if (move_num >= s.cutoff) return s.final_temp;
    if (!s.decay) return s.initial;
    const float t = f_div((float)move_num, (float)s.cutoff);
    return __builtin_fmaf(t, f_sub(s.final_temp, s.initial), s.initial);
}

// rand 0.8.5 Standard for f32 (restated, verify: no Rust toolchain pins it): the
// top 24 bits of one u32 word times 2^-24, in [0, 1)
BPPO_HD float unit24_from_word(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// whether a row at this temperature takes a word from the RNG.  The other no-draw
// exit of sample_with_temperature, sum == 0.0 (eval.rs:255-258), cannot be reached:
// with a finite max the max element contributes exp(0) = 1, and with an infinite or
// NaN max every x - max is NaN, so the sum is NaN (the all-masked row: it draws and
// returns A - 1, eval.rs:2281-2292).  The device loop therefore knows each row's word
// before the logits exist; the kernels flag the exit should it ever be taken.
BPPO_HD bool temp_draws(float temp) { return !(temp == 0.0f); }

// eval.rs:223-272 on one row.  x: the logits with masked entries already -inf
// (eval.rs:230-238), overwritten; first_valid: mask.position(|v| v) or 0; word: the
// row's RNG word (read only if it draws); *used: whether it drew.  T.expf is glibc's.
template <int A, class M>
BPPO_HD int sample_with_temperature(float (&x)[A], int first_valid, float temp, uint32_t word, int *used,
                                    const M &T) {
    *used = 0;
    if (temp == 0.0f) {
        // max_by(partial_cmp(..).unwrap_or(Equal)): the LAST of equal maxima, and an
        // incomparable (NaN) pair counts as equal, so the later element wins
        int best = 0;
        float bv = x[0];
#pragma unroll
        for (int a = 1; a < A; a++)
            if (!(bv > x[a])) { bv = x[a]; best = a; }
        return best;
    }
    // scaled = x / temp; max = fold(NEG_INFINITY, f32::max) (f32::max ignores a NaN side)
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < A; a++) {
        x[a] = f_div(x[a], temp);
        mx = (x[a] > mx || mx != mx) ? x[a] : mx;
    }
    // exp = (x - max).exp(); sum sequentially from 0.0 in index order
    float sum = 0.0f;
#pragma unroll
    for (int a = 0; a < A; a++) {
        x[a] = T.expf(f_sub(x[a], mx));
        sum = f_add(sum, x[a]);
    }
    if (sum == 0.0f) return first_valid;
    *used = 1;
    const float r = unit24_from_word(word);
    // probs = exp / sum; the first index with r < cumulative, else the last index
    float cum = 0.0f;
    int res = A - 1;
    bool found = false;
#pragma unroll
    for (int a = 0; a < A; a++) {
        cum = f_add(cum, f_div(x[a], sum));
        if (!found && r < cum) { res = a; found = true; }
    }
    return res;
}

// ---- host steps shared by the two evaluation loops (eval.hip, eval_cartpole.hip) ----

// A pod's StdRng::seed_from_u64(seed): its key, and base_seed = rng.next_u64(), words 0 and
// 1, low word first, which seeds the pod's envs (env j: base_seed + j); the pod's sampling
// draws follow from word 2 (eval.rs:1646-1648)
inline bppo::Key8 pod_key(uint64_t seed, uint64_t *base_seed) {
    const bppo::Key8 key = bppo::seed_key(seed);
    uint32_t blk0[16];
    bppo::chacha12_block(key, 0, 0, blk0);
    *base_seed = ((uint64_t)blk0[1] << 32) | (uint64_t)blk0[0];
    return key;
}

// The recorded games out: pod k's first min(n_games[k], cap) games go to games[k cap_per_pod
// ...] and nothing else is written there.  On the device the pods are cap apart, so one copy
// stages them all; a lone pod's need no staging.  The stream is drained on return.
inline hipError_t fetch_pod_games(hipStream_t st, const bppo_eval_game *d_games, int n_pods, int cap,
                                  const int32_t *n_games, bppo_eval_game *games, int cap_per_pod) {
    std::vector<bppo_eval_game> h_games(n_pods > 1 ? (size_t)n_pods * cap : 0);
    const size_t ncopy = n_pods > 1 ? h_games.size() : (size_t)std::min<int>(n_games[0], cap);
    if (ncopy == 0) return hipSuccess;
    hipError_t e = hipMemcpyAsync(n_pods > 1 ? h_games.data() : games, d_games, sizeof(bppo_eval_game) * ncopy,
                                  hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    for (size_t k = 0; k * cap < h_games.size(); k++) {
        const int ng = std::min<int>(n_games[k], cap);
        if (ng > 0) std::memcpy(games + k * cap_per_pod, &h_games[k * cap], sizeof(bppo_eval_game) * (size_t)ng);
    }
    return hipSuccess;
}

}  // namespace bppo_eval
