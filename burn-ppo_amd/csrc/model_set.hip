// model_set.hip — K frozen models on the device and their forward once per env step: the
// opponents of a training rollout (opponents.hip, ppo.rs:809-843) and the checkpoints of an
// evaluation (eval.hip, eval.rs:1685-1769) are the same machine.  The caller groups the
// step's rows (group[e] = 0: nobody's / the learner's, 1 + model; gpos[e] = the row's
// draw position; gbase: model k owns the draw rows [gbase[k + 1], gbase[k + 2])), and
// models_step_forward sorts the rows into that order, runs every model's obs normalizer and
// actor on its own rows, and selects the logits back into env order.
#include <algorithm>
#include "bppo_internal.h"
#include "bppo_norm_block.h"

namespace bppo {

static_assert(OPP_MAX_MODELS <= FwdGroupTab::MAX, "an opponent pool's models fit the grouped forward's table");

bppo_status ModelSet::upload(bppo_ctx *c, DeviceMem &buf, int K_, const float *params, const double *norm_mean,
                             const double *norm_m2, const double *norm_count, uint64_t random_mask, bool table) {
    const int D = c->D;
    const size_t np = c->net.n_params, nb = (size_t)(2 * D + 1);
    if (table && K_ > FwdGroupTab::MAX) { c->err = "model set: more models than the forward's table holds"; return BPPO_ERR_ARG; }
    if (!table) random_mask = 0;                 // the mask has a bit per table entry
    K = K_;
    tab = FwdGroupTab{};
    any_norm = false;
    on.assign(nb * std::max(K, 1), 0.0);
    BPPO_HIP(c, buf.alloc(&d_params, np * K));
    BPPO_HIP(c, buf.alloc(&d_on, on.size()));
    if (!random_mask && K > 0)                   // every model has parameters: one copy
        BPPO_HIP(c, hipMemcpyAsync(d_params, params, sizeof(float) * np * K, hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < K; k++) {
        const bool random = random_mask && ((random_mask >> k) & 1ull);   // a mask only with a table: k < 64
        if (table) tab.skip[k] = random;
        if (random) continue;
        if (random_mask)
            BPPO_HIP(c, hipMemcpyAsync(d_params + (size_t)k * np, params + (size_t)k * np, sizeof(float) * np,
                                       hipMemcpyHostToDevice, c->stream));
        const bool has = pack_norm_block(D, k, norm_mean, norm_m2, norm_count, &on[(size_t)k * nb]);
        any_norm = any_norm || has;
        if (!table) continue;
        tab.params[k] = d_params + (size_t)k * np;
        tab.on[k] = d_on + (size_t)k * nb;
        tab.has_norm[k] = has;
    }
    BPPO_HIP(c, hipMemcpyAsync(d_on, on.data(), sizeof(double) * on.size(), hipMemcpyHostToDevice, c->stream));
    if (table) {
        BPPO_HIP(c, buf.alloc(&d_tab, 1));
        BPPO_HIP(c, hipMemcpyAsync(d_tab, &tab, sizeof(FwdGroupTab), hipMemcpyHostToDevice, c->stream));
    }
    return BPPO_OK;
}

// back to the empty set: nothing of the released models is left to read
void ModelSet::release(DeviceMem &buf) {
    (void)buf.release(d_params);
    (void)buf.release(d_on);
    (void)buf.release(d_tab);
    K = 0;
    tab = FwdGroupTab{};
    on.clear();
    any_norm = false;
}

// the step's raw rows in draw order: each model's rows become one contiguous slice
__global__ void k_opp_sort_rows(int N, int L, const int32_t *group, const int32_t *gpos, const float *src, float *dst) {
    const size_t n = (size_t)N * L;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i / L, k = i - e * L;
        if (group[e] != 0) dst[(size_t)gpos[e] * L + k] = src[i];
    }
}

// the models' logits (draw order) into the step's logits for their rows
__global__ void k_opp_select(int N, int A, const int32_t *group, const int32_t *gpos, const float *src, float *dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * A) return;
    const int e = i / A;
    if (group[e] != 0) dst[i] = src[(size_t)gpos[e] * A + (i - e * A)];
}

// The obs normalizers of the grouped forward (k_obs_norm_rows's arithmetic per element):
// 8 rows per block, 32 threads per row; a row's group is found by walking gbase, its
// normalizer block and has-normalizer flag come from the table.
__global__ void __launch_bounds__(256) k_obs_norm_groups(const int32_t *gbase, const FwdGroupTab *tab, int n_groups,
                                                         int D, int ld, float *x, float clip) {
    const int row = gbase[1] + (int)blockIdx.x * 8 + ((int)threadIdx.x >> 5);
    if (row >= gbase[n_groups + 1]) return;
    int g = 0;
    while (g + 1 < n_groups && row >= gbase[g + 2]) g++;   // group g owns [gbase[g + 1], gbase[g + 2])
    if (tab->skip[g] || !tab->has_norm[g]) return;
    const double *on = tab->on[g];
    const double cnt = on[2 * D];
    if (!(cnt >= 2.0)) return;
    for (int d = threadIdx.x & 31; d < D; d += 32) {
        float *p = x + (size_t)row * ld + d;
        const float v = *p;
        double sd = sqrt(on[D + d] / cnt);
        sd = sd < 1e-8 ? 1e-8 : sd;
        float z = (float)(((double)v - on[d]) / sd);
        z = z < -clip ? -clip : z;
        z = z > clip ? clip : z;
        *p = z;
    }
}

// wide_forward_actor for all the models of a set at once (nets without conv layers): model
// k's rows are [gbase[k + 1], gbase[k + 2]) of the sorted row buffer xc (and of logits, and
// of the hidden buffers); gbase and tab are device memory.  One normalizer launch (if any
// model has one) and one GEMM launch per layer, whatever the number of models; the host gives
// only the span of rows that bounds the groups.  Per group bit-identical to
// launch_obs_norm_rows_on + wide_forward_actor on that group's rows.
static bppo_status wide_forward_actor_groups(bppo_ctx *c, const int32_t *gbase, const FwdGroupTab *tab, int n_groups,
                                             bool any_norm, int span_r0, int span_rows, float *xc, int ldxc,
                                             float *logits) {
    const NetLayout &n = c->net;
    if (n.n_conv) { c->err = "wide_forward_actor_groups: no conv layers"; return BPPO_ERR_UNSUPPORTED; }
    if (span_rows <= 0) return BPPO_OK;
    if (span_r0 < 0 || span_r0 + span_rows > c->rows_max || n_groups > FwdGroupTab::MAX) {
        c->err = "wide_forward_actor_groups: rows outside the context's buffers";
        return BPPO_ERR_ARG;
    }
    if (any_norm) {
        hipLaunchKernelGGL(k_obs_norm_groups, dim3((span_rows + 7) / 8), dim3(256), 0, c->stream, gbase, tab, n_groups,
                           c->D, ldxc, xc + c->G, 10.0f);
        TRY(launch_check(c, "k_obs_norm_groups"));
    }
    const float *x = xc + c->G;
    int ldx = ldxc;
    for (int l = 0; l < n.n_actor_hidden; l++) {
        float *h = c->d_hbuf + c->hoff[l];
        BPPO_HIP(c, gemm_fwd_groups(c->stream, gbase, tab, n_groups, span_r0, span_rows, n.out[l], n.in[l], x, ldx, n.w[l],
                                    n.b[l], c->cfg.relu ? 1 : 2, h, n.out[l]));
        x = h; ldx = n.out[l];
    }
    BPPO_HIP(c, gemm_fwd_groups(c->stream, gbase, tab, n_groups, span_r0, span_rows, c->A, n.in[n.policy], x, ldx,
                                n.w[n.policy], n.b[n.policy], 0, logits, c->A));
    return BPPO_OK;
}

// The forward one model after the other, sized by the host's copy of the group bases.
static bppo_status forward_models_loop(bppo_ctx *c, const ModelSet &m, const int32_t *gb, float *xc, float *logits) {
    const int A = c->A, L = c->L;
    for (int k = 0; k < m.K; k++) {
        const int r0 = gb[k + 1], rows = gb[k + 2] - gb[k + 1];
        if (rows <= 0 || m.tab.skip[k]) continue;
        float *x = xc + (size_t)r0 * L;
        if (m.tab.has_norm[k]) TRY(launch_obs_norm_rows_on(c, rows, x + c->G, L, nullptr, m.tab.on[k]));
        TRY(wide_forward_actor(c, rows, x, L, m.tab.params[k], logits + (size_t)r0 * A));
    }
    return BPPO_OK;
}

// grouped: all models at once from the device's group bases; the host's copy gives only the
// span of rows
bppo_status forward_models(bppo_ctx *c, const ModelSet &m, const int32_t *gb, const int32_t *d_gbase, float *xc,
                           float *logits, bool grouped) {
    // both paths read the table: the loop the host's copy, which a set uploaded without one leaves empty
    if (!m.d_tab) { c->err = "forward_models: a set uploaded without its table has no forward"; return BPPO_ERR_ARG; }
    if (!grouped) return forward_models_loop(c, m, gb, xc, logits);
    return wide_forward_actor_groups(c, d_gbase, m.d_tab, m.K, m.any_norm, gb[1], gb[m.K + 1] - gb[1], xc, c->L, logits);
}

bppo_status models_step_forward(bppo_ctx *c, const ModelSet &m, const int32_t *group, const int32_t *gpos,
                                const int32_t *gb, const int32_t *d_gbase, const float *src, float *xc, float *logits,
                                float *dst) {
    bool any_fwd = false;
    for (int k = 0; k < m.K; k++) any_fwd = any_fwd || (!m.tab.skip[k] && gb[k + 2] > gb[k + 1]);
    if (!any_fwd) return BPPO_OK;
    const size_t n = (size_t)c->N * c->L;
    hipLaunchKernelGGL(k_opp_sort_rows, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0,
                       c->stream, c->N, c->L, group, gpos, src, xc);
    TRY(launch_check(c, "k_opp_sort_rows"));
    TRY(forward_models(c, m, gb, d_gbase, xc, logits, !c->net.n_conv));
    const int na = c->N * c->A;
    hipLaunchKernelGGL(k_opp_select, dim3((na + 255) / 256), dim3(256), 0, c->stream, c->N, c->A, group, gpos, logits,
                       dst);
    TRY(launch_check(c, "k_opp_select"));
    return BPPO_OK;
}

}  // namespace bppo
