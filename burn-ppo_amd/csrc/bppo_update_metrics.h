// bppo_update_metrics.h — the update's metric fold (ppo.rs:2025-2110): the minibatches'
// metric rows (device sums, one row of WM_COUNT + 4 floats per minibatch that ran) into the
// numbers bppo_update_metrics reports.  Host only and pure: no HIP call, nothing of the
// context, so bppo_debug_fold_metrics runs it on a machine without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include "../../include/bppo.h"
#include "bppo_metric_row.h"

namespace bppo {

struct FoldArgs {
    float value_coef, ent_coef;
    int A, env_kind;
    size_t B;                      // rows the update trained on (opponent pool: the learner rows)
    double ev4[4];                 // explained_variance_sums: sum R, sum R^2, sum (R - V), sum (R - V)^2
    int ev_mode;                   // 1: explained_variance = ev_ref (the reference's f32 sums)
    float ev_ref;
    int epochs_run;
    bool normalize_values;         // PopArt on
    double pa_tsum, pa_tsq, pa_tcount;
    float pa_rescale_mag;
};

// f32 operations in the reference's order (compiled with -ffp-contract=off)
inline void fold_update_metrics(const float *rows, int nup, const FoldArgs &a, bppo_update_metrics *m) {
    const int W = WM_COUNT + 4;
    std::memset(m, 0, sizeof *m);
    float tp = 0, tv = 0, th = 0, tk = 0, tc = 0, tl = 0, tvm = 0, trm = 0, tam = 0, tas = 0;
    float tamin = INFINITY, tamax = -INFINITY, tvem = 0, tves = 0, tvemax = -INFINITY;
    float tav = 0, tevp = 0;
    for (int u = 0; u < nup; u++) {
        const float *r = rows + (size_t)u * W;
        const float n = r[WM_N] > 0 ? r[WM_N] : 1.0f;
        const float pl = r[WM_PL] / n, vl = 0.5f * (r[WM_VL] / n), h = r[WM_H] / n;
        tp += pl; tv += vl; th += h; tk += r[WM_KL] / n; tc += r[WM_CF] / n;
        tl += pl + vl * a.value_coef + (-h) * a.ent_coef;
        tvm += r[WM_V] / n; trm += r[WM_R] / n;
        const float vem = r[WM_VE] / n;
        tvem += vem;
        const double var = n > 1 ? ((double)r[WM_VE2] - (double)n * vem * vem) / (double)(n - 1) : 0.0;
        tves += sqrtf((float)std::max(var, 0.0));
        tvemax = std::max(tvemax, r[WM_VEMAX]);
        tav += r[WM_VALID] / n;
        tevp += r[WM_NCHOICE] > 0 ? r[WM_HV] / r[WM_NCHOICE] : 0.0f;
        tam += r[WM_ADV_MEAN]; tas += r[WM_ADV_STD];
        tamin = std::min(tamin, r[WM_ADV_MIN]); tamax = std::max(tamax, r[WM_ADV_MAX]);
    }
    // averaged over the minibatches run; none run -> 0/0 = NaN as in ppo.rs:2071-2090
    const float n = (float)nup;
    m->policy_loss = tp / n; m->value_loss = tv / n; m->entropy = th / n;
    m->entropy_scaled = m->entropy / logf((float)a.A);
    m->approx_kl = tk / n; m->clip_fraction = tc / n; m->total_loss = tl / n;
    m->value_mean = tvm / n; m->returns_mean = trm / n;
    m->adv_mean_raw = tam / n; m->adv_std_raw = tas / n; m->adv_min_raw = tamin; m->adv_max_raw = tamax;
    m->value_error_mean = tvem / n; m->value_error_std = tves / n; m->value_error_max = tvemax;
    const double Bn = (double)a.B;
    const double mr = a.ev4[0] / Bn, vr = a.ev4[1] / Bn - mr * mr;
    const double mres = a.ev4[2] / Bn, vres = a.ev4[3] / Bn - mres * mres;
    // ppo.rs:1268-1294 (fewer than 2 rows or Var(R) < 1e-8 -> 0)
    m->explained_variance = (a.B < 2 || vr < 1e-8) ? 0.0f : (float)(1.0 - vres / vr);
    if (a.ev_mode == 1) m->explained_variance = a.ev_ref;
    // ppo.rs:1549-1565: only envs with action masks report these (None -> 0)
    if (a.env_kind != BPPO_ENV_CARTPOLE) { m->avg_valid_actions = tav / n; m->entropy_valid_pct = tevp / n; }
    m->num_updates = nup; m->epochs_run = a.epochs_run;
    // PopArt metrics (ppo.rs:2061-2068): None -> NaN
    m->value_norm_target_mean = m->value_norm_target_std = NAN;
    m->value_norm_rescale_mag = a.pa_rescale_mag;
    if (a.normalize_values && a.pa_tcount > 0) {
        const double mean = a.pa_tsum / a.pa_tcount, var = a.pa_tsq / a.pa_tcount - mean * mean;
        m->value_norm_target_mean = (float)mean;
        m->value_norm_target_std = (float)std::sqrt(std::max(var, 0.0));
    }
}

}  // namespace bppo
