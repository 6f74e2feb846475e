/*
 * net.c — ActorCritic MLP / CTDE forward + hand-written backward, categorical
 * policy helpers, minibatch PPO loss/grad and Adam with per-tensor norm
 * clipping.  TEST INFRASTRUCTURE ONLY.
 *
 * References: network/mlp.rs:16-206, network/ctde.rs:64-183,
 * utils.rs:10-135, ppo.rs:1385-1502 (loss), main.rs:264-268 (Adam + clip).
 * Burn 0.20 internals restated (not vendored, verify): Linear = x.matmul(W)+b
 * with ndarray -> matrixmultiply 0.3 sgemm (FMA micro-kernel: a k-ordered fmaf
 * chain from 0 per k-block of KC=256, blocks summed into C), log_softmax =
 * (x - max) - ln(sum(exp(x - max))), max_pair ties -> lhs, clamp gradient on
 * [min, max] inclusive, GradientClipping::Norm applied per parameter tensor,
 * Adam with bias correction m^/(sqrt(v^)+eps), betas 0.9/0.999 as f32.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "oracle.h"

#define KC 256

/* MLP row parallelism: on for the parity tests (speed), off for the timed CPU
 * baseline, whose plan keeps the MLP single-threaded as the
 * reference's matrixmultiply sgemm is; results do not depend on it */
static int g_mlp_parallel = 1;
void or_set_mlp_parallel(int on) { g_mlp_parallel = on; }

/* test hook (tests/test_gpu_gemm_split.py): per FC layer index l, an optional u8 [mb][out]
 * mask that replaces the ReLU decision y > 0 in or_minibatch_loss_grad's backward, so the
 * gradient can be recomputed with another forward's ReLU decisions (the device's split
 * forward, whose pre-activations within rounding of 0 may fall on the other side) */
static const uint8_t *g_relu_masks[32];
void or_set_relu_masks(const uint8_t *const *masks, int n) {
    for (int l = 0; l < 32; l++) g_relu_masks[l] = masks && l < n ? masks[l] : NULL;
}
/* the post-activation argument of linear_bwd for layer l: y, or the override as 0/1 */
static const float *relu_y(int l, const float *y, size_t n, float **tmp) {
    *tmp = NULL;
    if (l < 0 || l >= 32 || !g_relu_masks[l]) return y;
    *tmp = malloc(sizeof(float) * n);
    for (size_t i = 0; i < n; i++) (*tmp)[i] = g_relu_masks[l][i] ? 1.0f : 0.0f;
    return *tmp;
}

typedef struct { int in, out; size_t w, b; } layer_t;

/* two trunks: CTDE, or split_networks (the critic on obs alone) */
static int two_trunk(const or_net_desc *d) { return d->ctde || d->split; }

/* parameter layout = Burn record order (mlp.rs:47-62, ctde.rs:26-44).  Layer
 * indices: actor hidden, policy, [critic hidden, value | value]; the offsets follow
 * the record, which for split_networks holds critic_layers before the heads. */
static int net_layers(const or_net_desc *d, layer_t *L, int *n_actor_total) {
    int n = 0; int in = d->obs_dim;
    if (d->cnn) {
        /* conv layers first (Burn record order: weight [Cout][Cin][k][k], bias),
         * as layers with in = Cin k k, out = Cout; the FC stack then reads the
         * flattened conv output + the extra features */
        int cin = d->C;
        for (int i = 0; i < d->n_conv; i++) {
            L[n].in = cin * d->ksize * d->ksize; L[n].out = d->conv_ch[i]; cin = d->conv_ch[i]; n++;
        }
        in = d->H * d->W * cin + (d->obs_dim - d->H * d->W * d->C);
    }
    for (int i = 0; i < d->n_actor; i++) { L[n].in = in; L[n].out = d->actor_width; in = d->actor_width; n++; }
    L[n].in = in; L[n].out = d->act_dim; n++;                 /* policy head */
    *n_actor_total = n;
    if (two_trunk(d) && d->cnn) {
        /* split CNN (cnn.rs:116-135): the critic's own conv stack and FC layers */
        int cin = d->C;
        for (int i = 0; i < d->n_conv; i++) {
            L[n].in = cin * d->ksize * d->ksize; L[n].out = d->conv_ch[i]; cin = d->conv_ch[i]; n++;
        }
        int fin = d->H * d->W * cin + (d->obs_dim - d->H * d->W * d->C);
        for (int i = 0; i < d->n_critic; i++) { L[n].in = fin; L[n].out = d->critic_width; fin = d->critic_width; n++; }
        L[n].in = fin; L[n].out = 1; n++;
    } else if (two_trunk(d)) {
        int cin = d->priv_dim + d->obs_dim;
        for (int i = 0; i < d->n_critic; i++) { L[n].in = cin; L[n].out = d->critic_width; cin = d->critic_width; n++; }
        L[n].in = cin; L[n].out = 1; n++;
    } else {
        L[n].in = in; L[n].out = 1; n++;
    }
    int order[32], no = 0;
    for (int i = 0; i < n; i++)
        if (!d->split || (i != *n_actor_total - 1 && i != n - 1)) order[no++] = i;
    if (d->split) { order[no++] = *n_actor_total - 1; order[no++] = n - 1; }
    size_t off = 0;
    for (int r = 0; r < n; r++) {
        layer_t *l = &L[order[r]];
        l->w = off; off += (size_t)l->in * l->out;
        l->b = off; off += l->out;
    }
    return n;
}

void or_net_value_head(const or_net_desc *d, size_t *w, size_t *b, int *in) {
    layer_t L[32]; int na;
    int n = net_layers(d, L, &na);
    *w = L[n - 1].w; *b = L[n - 1].b; *in = L[n - 1].in;
}

size_t or_net_num_params(const or_net_desc *d) {
    layer_t L[32]; int na;
    int n = net_layers(d, L, &na);
    return L[n - 1].b + 1;       /* the value head is last in every record */
}

static float act_fwd(float y, int relu) { return relu ? (y > 0.0f ? y : 0.0f) : tanhf(y); }

/* One Burn Linear: y = x.matmul(W) + b (matrixmultiply k-ordered fma chain).
 * Each (row, o) element is the chain acc = fmaf(x[k], W[k][o], acc) from 0 over
 * one KC block, blocks summed in order, then + b[o].  The loops run o innermost
 * (independent chains, vectorisable) and rows in parallel: the arithmetic of
 * every element is unchanged, so the result does not depend on the thread count. */
void or_linear(const float *x, const float *W, const float *b, size_t B, int in, int out,
               int relu, float *y) {
#pragma omp parallel if (g_mlp_parallel && B * (size_t)in * (size_t)out > (1u << 18))
    {
        float *acc = malloc(sizeof(float) * (size_t)out), *tot = malloc(sizeof(float) * (size_t)out);
#pragma omp for schedule(static)
        for (size_t r = 0; r < B; r++) {
            const float *xr = x + r * in;
            for (int kb = 0; kb < in; kb += KC) {
                int ke = kb + KC < in ? kb + KC : in;
                for (int o = 0; o < out; o++) acc[o] = 0.0f;
                for (int k = kb; k < ke; k++) {
                    const float xk = xr[k];
                    const float *wk = W + (size_t)k * out;
                    for (int o = 0; o < out; o++) acc[o] = fmaf(xk, wk[o], acc[o]);
                }
                if (kb == 0) for (int o = 0; o < out; o++) tot[o] = acc[o];
                else for (int o = 0; o < out; o++) tot[o] = tot[o] + acc[o];
            }
            for (int o = 0; o < out; o++) {
                float v = tot[o] + b[o];
                y[r * out + o] = relu >= 0 ? act_fwd(v, relu) : v;
            }
        }
        free(acc); free(tot);
    }
}

/* activations cache for backward: buf[l] = output of FC layer l (l < 32), buf[31] =
 * the CTDE critic input, buf[ACT_CONV + 8 s + l] = conv layer l of stack s (0 actor /
 * shared, 1 the split critic), buf[ACT_F + s] = the features F of stack s */
enum { ACT_CONV = 40, ACT_F = 56, ACT_N = 64 };
typedef struct {
    float *buf[ACT_N];
} acts_t;

/* ------------------------------------------------------------------ CNN --
 * cnn.rs:241-330 with Burn Conv2d as im2col + the same Linear chain order:
 * A[b*HW + hw][(ci*k + kh)*k + kw] (zero padded), Y = relu(A Wt + bias), Wt[k][co]
 * = weight[co][k]; the input of layer 0 is obs[:, :HWC] read channels-last
 * ([B, H, W, C] then permuted, cnn.rs:252-262) although the observation is
 * plane-major; activations NHWC rows; flatten NCHW (c*HW + hw) + extra features. */
static void im2col(const or_net_desc *d, int layer, const float *src, int ld, size_t B, int cin, float *A) {
    const int ks = d->ksize, pad = ks / 2, HW = d->H * d->W, K = cin * ks * ks;
    for (size_t b = 0; b < B; b++)
        for (int hw = 0; hw < HW; hw++)
            for (int k = 0; k < K; k++) {
                const int ci = k / (ks * ks), kh = (k % (ks * ks)) / ks, kw = k % ks;
                const int h = hw / d->W + kh - pad, w = hw % d->W + kw - pad;
                float v = 0.0f;
                if (h >= 0 && h < d->H && w >= 0 && w < d->W) {
                    const int hw2 = h * d->W + w;
                    v = layer == 0 ? src[b * ld + (size_t)hw2 * cin + ci] : src[(b * HW + hw2) * cin + ci];
                }
                A[(b * HW + hw) * K + k] = v;
            }
}

static float *conv_wt(const float *w, int cout, int K) {   /* [Cout][K] -> [K][Cout] */
    float *t = malloc(sizeof(float) * (size_t)cout * K);
    for (int co = 0; co < cout; co++)
        for (int k = 0; k < K; k++) t[(size_t)k * cout + co] = w[(size_t)co * K + k];
    return t;
}

/* conv stack s (its conv layers are L[0 .. n_conv)) + flatten:
 * A->buf[ACT_CONV + 8 s + l] = conv outputs, A->buf[ACT_F + s] = features F */
static void cnn_trunk(const or_net_desc *d, const layer_t *L, const float *p, const float *obs, size_t B, acts_t *A,
                      int s) {
    const int HW = d->H * d->W;
    const float *src = obs;
    int cin = d->C;
    for (int l = 0; l < d->n_conv; l++) {
        const int K = L[l].in, co = L[l].out;
        float *a = malloc(sizeof(float) * B * HW * K);
        im2col(d, l, src, d->obs_dim, B, cin, a);
        float *wt = conv_wt(p + L[l].w, co, K);
        float *y = malloc(sizeof(float) * B * HW * co);
        or_linear(a, wt, p + L[l].b, B * HW, K, co, 1, y);
        free(a); free(wt);
        A->buf[ACT_CONV + 8 * s + l] = y;
        src = y; cin = co;
    }
    const int E = d->obs_dim - HW * d->C, fd = HW * cin + E;
    float *F = malloc(sizeof(float) * B * fd);
    for (size_t b = 0; b < B; b++) {
        for (int c = 0; c < cin; c++)
            for (int hw = 0; hw < HW; hw++) F[b * fd + (size_t)c * HW + hw] = src[(b * HW + hw) * cin + c];
        for (int j = 0; j < E; j++) F[b * fd + (size_t)HW * cin + j] = obs[b * d->obs_dim + (size_t)HW * d->C + j];
    }
    A->buf[ACT_F + s] = F;
}

static void forward_cached(const or_net_desc *d, const float *p, const float *obs,
                           const float *priv, size_t B, float *logits, float *values,
                           acts_t *A) {
    layer_t L[32]; int na;
    int n = net_layers(d, L, &na);
    const float *x = obs;
    const int l0 = d->cnn ? d->n_conv : 0;
    if (d->cnn) {
        cnn_trunk(d, L, p, obs, B, A, 0);
        x = A->buf[ACT_F];
    }
    for (int i = l0; i < na - 1; i++) {
        float *y = malloc(sizeof(float) * B * L[i].out);
        or_linear(x, p + L[i].w, p + L[i].b, B, L[i].in, L[i].out, d->relu, y);
        if (A) A->buf[i] = y;
        x = y;
    }
    or_linear(x, p + L[na - 1].w, p + L[na - 1].b, B, L[na - 1].in, L[na - 1].out, -1, logits);
    if (!two_trunk(d)) {
        or_linear(x, p + L[na].w, p + L[na].b, B, L[na].in, 1, -1, values);
    } else if (d->cnn) {
        /* split CNN critic: its conv stack on the same spatial input, its FC layers */
        cnn_trunk(d, L + na, p, obs, B, A, 1);
        const float *xx = A->buf[ACT_F + 1];
        for (int i = na + d->n_conv; i < n - 1; i++) {
            float *y = malloc(sizeof(float) * B * L[i].out);
            or_linear(xx, p + L[i].w, p + L[i].b, B, L[i].in, L[i].out, d->relu, y);
            A->buf[i] = y;
            xx = y;
        }
        or_linear(xx, p + L[n - 1].w, p + L[n - 1].b, B, L[n - 1].in, 1, -1, values);
    } else {
        int cin = d->priv_dim + d->obs_dim;
        float *xc = malloc(sizeof(float) * B * cin);
        for (size_t r = 0; r < B; r++) {
            if (d->priv_dim) memcpy(xc + r * cin, priv + r * d->priv_dim, sizeof(float) * d->priv_dim);
            memcpy(xc + r * cin + d->priv_dim, obs + r * d->obs_dim, sizeof(float) * d->obs_dim);
        }
        if (A) A->buf[31] = xc;
        const float *xx = xc;
        for (int i = na; i < n - 1; i++) {
            float *y = malloc(sizeof(float) * B * L[i].out);
            or_linear(xx, p + L[i].w, p + L[i].b, B, L[i].in, L[i].out, d->relu, y);
            if (A) A->buf[i] = y;
            xx = y;
        }
        or_linear(xx, p + L[n - 1].w, p + L[n - 1].b, B, L[n - 1].in, 1, -1, values);
    }
    if (!A) {
        /* free temporaries */
        /* (re-run allocation pattern: buffers were not recorded) */
    }
}

static void free_acts(acts_t *A) {
    for (int i = 0; i < ACT_N; i++) { free(A->buf[i]); A->buf[i] = NULL; }
}

void or_net_forward(const or_net_desc *d, const float *params, const float *obs,
                    const float *priv, size_t B, float *logits, float *values) {
    acts_t A; memset(&A, 0, sizeof A);
    forward_cached(d, params, obs, priv, B, logits, values, &A);
    free_acts(&A);
}

/* dx = dz W^T as linear_bwd computes it: per row, each input k an f32 fma chain over the
 * outputs o in order from 0 (W [in][out]) */
static void dx_chain(const float *dz, const float *W, size_t B, int in, int out, float *dx, int big) {
    float *WT = malloc(sizeof(float) * (size_t)in * out);
    for (int k = 0; k < in; k++)
        for (int o = 0; o < out; o++) WT[(size_t)o * in + k] = W[(size_t)k * out + o];
#pragma omp parallel if (big)
    {
        float *acc = malloc(sizeof(float) * (size_t)in);
#pragma omp for schedule(static)
        for (size_t r = 0; r < B; r++) {
            for (int k = 0; k < in; k++) acc[k] = 0.0f;
            for (int o = 0; o < out; o++) {
                const float g = dz[r * out + o];
                const float *wo = WT + (size_t)o * in;
                for (int k = 0; k < in; k++) acc[k] = fmaf(g, wo[k], acc[k]);
            }
            for (int k = 0; k < in; k++) dx[r * in + k] = acc[k];
        }
        free(acc);
    }
    free(WT);
}

/* test hook: the input gradient of one Linear (dz [B][out], W [in][out] -> dx [B][in]) */
void or_linear_dx(const float *dz, const float *W, size_t B, int in, int out, float *dx) {
    dx_chain(dz, W, B, in, out, dx, B * (size_t)in * (size_t)out > (1u << 18));
}

/* backward of one Linear + activation given the post-activation output y:
 * dW += x^T dz (f64, each element summed over rows in row order), db += sum dz,
 * dx = dz W^T (f32 fma chain over o).  Parallel over k (dW) and rows (dx):
 * per-element arithmetic and order are fixed, independent of the thread count. */
static void linear_bwd(const float *x, const float *y, const float *dy, const float *W,
                       size_t B, int in, int out, int act, double *gW, double *gb, float *dx) {
    float *dz = malloc(sizeof(float) * B * out);
    const int big = g_mlp_parallel && B * (size_t)in * (size_t)out > (1u << 18);
#pragma omp parallel for schedule(static) if (big)
    for (size_t r = 0; r < B; r++)
        for (int o = 0; o < out; o++) {
            float g = dy[r * out + o];
            if (act == 1) g = y[r * out + o] > 0.0f ? g : 0.0f;
            else if (act == 0) { float t = y[r * out + o]; g = g * (1.0f - t * t); }
            dz[r * out + o] = g;
        }
    for (size_t r = 0; r < B; r++)
        for (int o = 0; o < out; o++) gb[o] += (double)dz[r * out + o];
#pragma omp parallel for schedule(dynamic, 1) if (big)
    for (int k = 0; k < in; k++) {
        double *gk = gW + (size_t)k * out;
        for (size_t r = 0; r < B; r++) {
            const double xk = (double)x[r * in + k];
            const float *dzr = dz + r * out;
            for (int o = 0; o < out; o++) gk[o] += xk * (double)dzr[o];
        }
    }
    if (dx) dx_chain(dz, W, B, in, out, dx, big);
    free(dz);
}

/* conv stack backward from dF = dL/d[features]: relu' of the last conv output,
 * un-flatten, then per layer dWt = A^T dY (f64), db = sum dY, dA = dY Wt^T and the
 * col2im gather (taps in (kh, kw) order, f32 adds) times relu' of the input */
static void cnn_bwd(const or_net_desc *d, const layer_t *L, const float *p, const float *obs, size_t B,
                    const acts_t *A, int s, const float *dF, double *g) {
    float *const *Y = A->buf + ACT_CONV + 8 * s;   /* this stack's conv outputs */
    const int HW = d->H * d->W, last = d->n_conv - 1, ks = d->ksize, pad = ks / 2;
    const int cl = L[last].out, E = d->obs_dim - HW * d->C, fd = HW * cl + E;
    float *dy = malloc(sizeof(float) * B * HW * cl);
    const float *yl = Y[last];
    for (size_t b = 0; b < B; b++)
        for (int hw = 0; hw < HW; hw++)
            for (int c = 0; c < cl; c++) {
                const size_t r = (b * HW + hw) * cl + c;
                dy[r] = yl[r] > 0.0f ? dF[b * fd + (size_t)c * HW + hw] : 0.0f;
            }
    for (int l = last; l >= 0; l--) {
        const int K = L[l].in, co = L[l].out, cin = l ? L[l - 1].out : d->C;
        float *a = malloc(sizeof(float) * B * HW * K);
        im2col(d, l, l ? Y[l - 1] : obs, d->obs_dim, B, cin, a);
        float *wt = conv_wt(p + L[l].w, co, K);
        double *gwt = calloc((size_t)K * co, sizeof(double));
        float *da = l ? malloc(sizeof(float) * B * HW * K) : NULL;
        linear_bwd(a, NULL, dy, wt, B * HW, K, co, -1, gwt, g + L[l].b, da);
        for (int c = 0; c < co; c++)
            for (int k = 0; k < K; k++) g[L[l].w + (size_t)c * K + k] += gwt[(size_t)k * co + c];
        free(a); free(wt); free(gwt); free(dy);
        dy = NULL;
        if (!l) break;
        const float *yp = Y[l - 1];
        dy = malloc(sizeof(float) * B * HW * cin);
        for (size_t b = 0; b < B; b++)
            for (int hw = 0; hw < HW; hw++)
                for (int ci = 0; ci < cin; ci++) {
                    const int h = hw / d->W, w = hw % d->W;
                    float s = 0.0f;
                    for (int kh = 0; kh < ks; kh++)
                        for (int kw = 0; kw < ks; kw++) {
                            const int ho = h - kh + pad, wo = w - kw + pad;
                            if (ho < 0 || ho >= d->H || wo < 0 || wo >= d->W) continue;
                            s += da[(b * HW + ho * d->W + wo) * K + (ci * ks + kh) * ks + kw];
                        }
                    const size_t r = (b * HW + hw) * cin + ci;
                    dy[r] = yp[r] > 0.0f ? s : 0.0f;
                }
        free(da);
    }
    free(dy);
}

/* ---------------------------------------------------------------- policy -- */
/* log_softmax over one row (Burn activation::log_softmax, verify) */
void or_log_softmax_row(const float *x, int A, float *out) {
    float m = -INFINITY;
    for (int a = 0; a < A; a++) if (x[a] > m) m = x[a];
    float s = 0.0f;
    for (int a = 0; a < A; a++) s += expf(x[a] - m);
    float l = logf(s);
    for (int a = 0; a < A; a++) out[a] = (x[a] - m) - l;
}

float or_log_prob(const float *logits, int A, int32_t a) {
    float ls[64];
    or_log_softmax_row(logits, A, ls);
    return ls[a];
}

/* utils.rs:52-58: -sum(exp(ls) * ls) */
float or_entropy(const float *logits, int A) {
    float ls[64];
    or_log_softmax_row(logits, A, ls);
    float s = 0.0f;
    for (int a = 0; a < A; a++) s += expf(ls[a]) * ls[a];
    return -s;
}

/* utils.rs:10-31: u = gen_range(1e-10f32..1.0) row-major, g = -ln(-ln u),
 * argmax(logits + g) (first maximum). */
void or_sample_categorical(or_rng *rng, const float *logits, size_t B, int A, int32_t *actions) {
    for (size_t r = 0; r < B; r++) {
        int best = 0; float bv = 0.0f;
        for (int a = 0; a < A; a++) {
            float u = or_gen_range_f32(rng, 1e-10f, 1.0f);
            float g = -logf(-logf(u));
            float v = logits[r * A + a] + g;
            if (a == 0 || v > bv) { bv = v; best = a; }
        }
        actions[r] = best;
    }
}

/* utils.rs:96-135 apply_action_mask: 0 for a valid action, -inf otherwise;
 * returns the first row with no valid action (the reference panics,
 * utils.rs:115-123), or -1 */
long or_apply_action_mask(float *logits, const uint8_t *mask, size_t B, int A) {
    for (size_t r = 0; r < B; r++) {
        int any = 0;
        for (int a = 0; a < A; a++) any |= mask[r * A + a];
        if (!any) return (long)r;
    }
    for (size_t q = 0; q < B * (size_t)A; q++) logits[q] += mask[q] ? 0.0f : -INFINITY;
    return -1;
}

/* utils.rs:80-89: (a - mean) / (sqrt(var_unbiased) + 1e-8); raw stats ppo.rs:1905-1913.
 * Reductions accumulate in f64 (the reference's ndarray f32 order is unknowable). */
void or_normalize_advantages(const float *adv, size_t n, float *out, float *mean_o, float *std_o,
                             float *mn, float *mx) {
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (size_t i = 0; i < n; i++) {
        s += adv[i];
        if (adv[i] < lo) lo = adv[i];
        if (adv[i] > hi) hi = adv[i];
    }
    float mean = (float)(s / (double)n);
    double v = 0.0;
    for (size_t i = 0; i < n; i++) { double dd = (double)adv[i] - (double)mean; v += dd * dd; }
    float var = n > 1 ? (float)(v / (double)(n - 1)) : NAN;
    float sd = sqrtf(var);
    float denom = sd + 1e-8f;
    if (out) for (size_t i = 0; i < n; i++) out[i] = (adv[i] - mean) / denom;
    if (mean_o) *mean_o = mean;
    if (std_o) *std_o = sd;
    if (mn) *mn = lo;
    if (mx) *mx = hi;
}

/* The per-row body of or_minibatch_loss_grad on forwarded logits [mb][A] and values [mb]:
 * ppo.rs:1385-1502 (loss) with its hand-written backward and ppo.rs:1507-1592 (metrics).
 * dlogits [mb][A], dv [mb]: dL/dlogits and dL/dvalue of the minibatch loss (1 / mb included).
 * terms [mb][OR_LT_COUNT] (may be NULL): the f32 per-row terms the metrics sum.
 * decisions [mb][3] (may be NULL): take_rhs (pl1 < pl2: the clipped branch of the policy max;
 * a tie takes the unclipped one), lo <= ratio <= hi (the clamp passes the gradient, boundaries
 * included), and the value branch: 0 unclipped (or clip_value off; a tie l1 == l2 goes here),
 * 1 clipped with -eps <= v - v_old <= eps (gradient passes), 2 clipped and the gradient cut. */
void or_loss_rows(int A, size_t mb, const float *logits, const float *values, const int32_t *actions,
                  const float *old_logp, const float *adv_n, const float *returns, const float *old_values,
                  const float *masks, const or_ppo_cfg *c, double ent_coef, float *dlogits, float *dv,
                  float *terms, int32_t *decisions) {
    const float lo = (float)(1.0 - c->clip_epsilon_d), hi = (float)(1.0 + c->clip_epsilon_d);
    const float ceps = (float)c->clip_epsilon_d;
    const double inv = 1.0 / (double)mb;
    for (size_t i = 0; i < mb; i++) {
        float x[64], ls[64], pr[64];
        int nvalid = 0;
        for (int a = 0; a < A; a++) {
            float add = masks ? (masks[i * A + a] - 1.0f) * 1e9f : 0.0f;
            x[a] = logits[i * A + a] + add;
            if (masks) nvalid += masks[i * A + a] > 0.5f;
        }
        or_log_softmax_row(x, A, ls);
        float H = 0.0f;
        for (int a = 0; a < A; a++) { pr[a] = expf(ls[a]); H += pr[a] * ls[a]; }
        H = -H;
        float newlp = ls[actions[i]];
        float log_ratio = newlp - old_logp[i];
        float ratio = expf(log_ratio);
        float na = -adv_n[i];
        float pl1 = na * ratio;
        float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
        float pl2 = na * rc;
        int take_rhs = pl1 < pl2;
        float pl = take_rhs ? pl2 : pl1;
        const int in_range = ratio >= lo && ratio <= hi;
        /* value loss */
        float v = values[i], R = returns[i];
        float vl;
        float dvl;  /* d(vl_i)/dv */
        float dlt = 0.0f;
        int vbranch = 0;
        if (c->clip_value) {
            float vo = old_values[i];
            dlt = v - vo;
            float dc = dlt < -ceps ? -ceps : (dlt > ceps ? ceps : dlt);
            float vc = vo + dc;
            float l1 = (v - R) * (v - R), l2 = (vc - R) * (vc - R);
            if (l1 < l2) {
                vl = l2;
                vbranch = (dlt >= -ceps && dlt <= ceps) ? 1 : 2;
                dvl = vbranch == 1 ? 2.0f * (vc - R) : 0.0f;
            } else { vl = l1; dvl = 2.0f * (v - R); }
        } else {
            vl = (v - R) * (v - R);
            dvl = 2.0f * (v - R);
        }
        if (terms) {
            float *t = terms + i * OR_LT_COUNT;
            t[OR_LT_PL] = pl; t[OR_LT_VL] = vl; t[OR_LT_H] = H;
            t[OR_LT_KL] = (ratio - 1.0f) - log_ratio;
            t[OR_LT_CF] = fabsf(ratio - 1.0f) > ceps ? 1.0f : 0.0f;
            t[OR_LT_VE] = fabsf(v - R);
            t[OR_LT_NVALID] = (float)nvalid;
            t[OR_LT_HV] = nvalid > 1 ? H / logf((float)nvalid) : 0.0f;
            t[OR_LT_RATIO] = ratio;
            t[OR_LT_VDELTA] = dlt;
        }
        if (decisions) {
            decisions[3 * i] = take_rhs; decisions[3 * i + 1] = in_range; decisions[3 * i + 2] = vbranch;
        }
        /* backward: policy term */
        double g_ratio;
        if (!take_rhs) g_ratio = -(double)adv_n[i] * inv;
        else g_ratio = in_range ? -(double)adv_n[i] * inv : 0.0;
        double g_lr = g_ratio * (double)ratio;
        for (int a = 0; a < A; a++) {
            double g = g_lr * ((a == actions[i] ? 1.0 : 0.0) - (double)pr[a]);
            g += ent_coef * inv * (double)pr[a] * ((double)ls[a] + (double)H);
            dlogits[i * A + a] = (float)g;
        }
        dv[i] = (float)(c->value_coef * 0.5 * inv * (double)dvl);
    }
}

/* ppo.rs:1385-1502 compute_minibatch_loss + autodiff backward (hand-written)
 * and ppo.rs:1507-1592 compute_minibatch_metrics: forward, or_loss_rows, the metric sums over
 * its per-row terms in row order, then the backward through the net. */
void or_minibatch_loss_grad(const or_net_desc *d, const float *p, size_t mb, const float *obs,
                            const float *priv, const int32_t *actions, const float *old_logp,
                            const float *adv_n, const float *returns, const float *old_values,
                            const float *masks, const or_ppo_cfg *c, double ent_coef,
                            float *grads, or_mb_stats *st) {
    const int A = d->act_dim;
    float *logits = malloc(sizeof(float) * mb * A);
    float *values = malloc(sizeof(float) * mb);
    acts_t acts; memset(&acts, 0, sizeof acts);
    forward_cached(d, p, obs, priv, mb, logits, values, &acts);

    const double inv = 1.0 / (double)mb;
    float *dlogits = calloc(mb * A, sizeof(float));
    float *dv = calloc(mb, sizeof(float));
    float *terms = malloc(sizeof(float) * mb * OR_LT_COUNT);
    or_loss_rows(A, mb, logits, values, actions, old_logp, adv_n, returns, old_values, masks, c, ent_coef,
                 dlogits, dv, terms, NULL);
    double s_pl = 0, s_vl = 0, s_h = 0, s_kl = 0, s_cf = 0, s_v = 0, s_r = 0, s_ve = 0;
    double s_valid = 0, s_hv = 0, n_choice = 0;
    float ve_max = -INFINITY;
    float *verr = malloc(sizeof(float) * mb);
    for (size_t i = 0; i < mb; i++) {
        const float *t = terms + i * OR_LT_COUNT;
        s_pl += t[OR_LT_PL];
        s_vl += t[OR_LT_VL];
        s_h += t[OR_LT_H];
        s_kl += (double)t[OR_LT_KL];
        s_cf += t[OR_LT_CF] != 0.0f ? 1.0 : 0.0;
        s_v += values[i]; s_r += returns[i];
        verr[i] = t[OR_LT_VE];
        s_ve += verr[i];
        if (verr[i] > ve_max) ve_max = verr[i];
        if (masks) {
            s_valid += t[OR_LT_NVALID];
            if (t[OR_LT_NVALID] > 1.0f) { n_choice += 1; s_hv += t[OR_LT_HV]; }
        }
    }
    free(terms);
    float pl_mean = (float)(s_pl * inv);
    float vl_half = (float)(s_vl * inv) * 0.5f;
    float h_mean = (float)(s_h * inv);
    float loss = pl_mean + vl_half * (float)c->value_coef + (-h_mean) * (float)ent_coef;
    if (st) {
        st->loss = loss; st->policy_loss = pl_mean; st->value_loss = vl_half; st->entropy = h_mean;
        st->approx_kl = (float)(s_kl * inv); st->clip_fraction = (float)(s_cf * inv);
        st->value_mean = (float)(s_v * inv); st->returns_mean = (float)(s_r * inv);
        float vem = (float)(s_ve * inv);
        double vv = 0;
        for (size_t i = 0; i < mb; i++) { double dd = (double)verr[i] - (double)vem; vv += dd * dd; }
        st->value_error_mean = vem;
        st->value_error_std = mb > 1 ? sqrtf((float)(vv / (double)(mb - 1))) : NAN;
        st->value_error_max = ve_max;
        st->avg_valid_actions = masks ? (float)(s_valid * inv) : 0.0f;
        st->entropy_valid_pct = (masks && n_choice > 0) ? (float)(s_hv / n_choice) : 0.0f;
    }
    /* ---- backprop ---- */
    if (grads) {
        layer_t L[32]; int na;
        int n = net_layers(d, L, &na);
        size_t np = L[n - 1].b + 1;
        double *g = calloc(np, sizeof(double));
        /* actor path */
        {
            float *dcur = dlogits;
            int li = na - 1;
            const float *xin = li > 0 ? acts.buf[li - 1] : obs;
            float *dx = li > 0 ? malloc(sizeof(float) * mb * L[li].in) : NULL;
            linear_bwd(xin, NULL, dcur, p + L[li].w, mb, L[li].in, L[li].out, -1, g + L[li].w,
                       g + L[li].b, dx);
            float *dh = dx;
            if (!two_trunk(d)) {
                /* shared backbone: add value head gradient */
                int vi = na;
                float *dx2 = malloc(sizeof(float) * mb * L[vi].in);
                linear_bwd(xin, NULL, dv, p + L[vi].w, mb, L[vi].in, 1, -1, g + L[vi].w, g + L[vi].b,
                           dh ? dx2 : NULL);
                if (dh) for (size_t q = 0; q < mb * (size_t)L[vi].in; q++) dh[q] += dx2[q];
                free(dx2);
            }
            const int l0 = d->cnn ? d->n_conv : 0;     /* first FC layer */
            for (int l = li - 1; l >= l0; l--) {
                const float *xl = l > l0 ? acts.buf[l - 1] : (d->cnn ? acts.buf[ACT_F] : obs);
                float *dxl = (l > l0 || d->cnn) ? malloc(sizeof(float) * mb * L[l].in) : NULL;
                float *ym = NULL;
                const float *yl = d->relu ? relu_y(l, acts.buf[l], mb * (size_t)L[l].out, &ym) : acts.buf[l];
                linear_bwd(xl, yl, dh, p + L[l].w, mb, L[l].in, L[l].out, d->relu,
                           g + L[l].w, g + L[l].b, dxl);
                free(ym);
                free(dh);
                dh = dxl;
            }
            if (d->cnn) cnn_bwd(d, L, p, obs, mb, &acts, 0, dh, g);   /* dh = dL/dF */
            free(dh);
        }
        if (two_trunk(d)) {
            /* critic trunk: FC layers [c0, vi) on its input x0 (CTDE / split MLP: the
             * critic rows; split CNN: the critic stack's features, then that stack) */
            int vi = n - 1;
            const int c0 = d->cnn ? na + d->n_conv : na;
            const float *x0 = d->cnn ? acts.buf[ACT_F + 1] : acts.buf[31];
            const float *xin = vi > c0 ? acts.buf[vi - 1] : x0;
            float *dh = (vi > c0 || d->cnn) ? malloc(sizeof(float) * mb * L[vi].in) : NULL;
            linear_bwd(xin, NULL, dv, p + L[vi].w, mb, L[vi].in, 1, -1, g + L[vi].w, g + L[vi].b, dh);
            for (int l = vi - 1; l >= c0; l--) {
                const float *xl = l > c0 ? acts.buf[l - 1] : x0;
                float *dxl = (l > c0 || d->cnn) ? malloc(sizeof(float) * mb * L[l].in) : NULL;
                float *ym = NULL;
                const float *yl = d->relu ? relu_y(l, acts.buf[l], mb * (size_t)L[l].out, &ym) : acts.buf[l];
                linear_bwd(xl, yl, dh, p + L[l].w, mb, L[l].in, L[l].out, d->relu,
                           g + L[l].w, g + L[l].b, dxl);
                free(ym);
                free(dh);
                dh = dxl;
            }
            if (d->cnn) cnn_bwd(d, L + na, p, obs, mb, &acts, 1, dh, g);
            free(dh);
        }
        for (size_t q = 0; q < np; q++) grads[q] = (float)g[q];
        free(g);
    }
    free_acts(&acts);
    free(logits); free(values); free(dlogits); free(dv); free(verr);
}

/* ------------------------------------------------------------------ Adam -- */
static float powi_f32(float a, int b) {   /* compiler-rt __powisf2 */
    int recip = b < 0;
    float r = 1.0f;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0f / r : r;
}

void or_adam_init(or_adam *a, const or_net_desc *d) {
    size_t np = or_net_num_params(d);
    a->m1 = calloc(np, sizeof(float));
    a->m2 = calloc(np, sizeof(float));
    a->time = calloc(64, sizeof(int32_t));
    a->has_state = 0;
}
void or_adam_free(or_adam *a) { free(a->m1); free(a->m2); free(a->time); }

/* main.rs:264-268: AdamConfig{epsilon, grad_clipping: Norm(max_grad_norm)};
 * ppo.rs:1983-1984 optimizer.step(lr, model, grads). Per tensor: clip, then Adam. */
void or_adam_step(const or_net_desc *d, or_adam *a, float *params, float *grads, double lr,
                  float max_norm, float eps) {
    layer_t L[32]; int na;
    int n = net_layers(d, L, &na);
    const float b1 = 0.9f, b2 = 0.999f;
    const float f1 = 1.0f - b1, f2 = 1.0f - b2;
    const float lrf = (float)lr;
    for (int t = 0; t < 2 * n; t++) {
        size_t off = (t & 1) ? L[t >> 1].b : L[t >> 1].w;
        size_t len = (t & 1) ? (size_t)L[t >> 1].out : (size_t)L[t >> 1].in * L[t >> 1].out;
        float *g = grads + off;
        double ss = 0.0;
        for (size_t i = 0; i < len; i++) ss += (double)g[i] * (double)g[i];
        float norm = (float)sqrt(ss);
        if (norm > max_norm) {
            float scale = max_norm / norm;
            for (size_t i = 0; i < len; i++) g[i] = g[i] * scale;
        }
        int ti = ++a->time[t];
        float c1 = 1.0f - powi_f32(b1, ti), c2 = 1.0f - powi_f32(b2, ti);
        for (size_t i = 0; i < len; i++) {
            float m1 = a->m1[off + i] * b1 + g[i] * f1;
            float m2 = a->m2[off + i] * b2 + (g[i] * g[i]) * f2;
            a->m1[off + i] = m1; a->m2[off + i] = m2;
            float m1c = m1 / c1, m2c = m2 / c2;
            float upd = m1c / (sqrtf(m2c) + eps);
            params[off + i] = params[off + i] - upd * lrf;
        }
    }
    a->has_state = 1;
}
