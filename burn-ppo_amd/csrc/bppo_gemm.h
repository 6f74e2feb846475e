// bppo_gemm.h — launchers of the f32 MFMA GEMM engine (k_gemm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/bppo.h"

namespace bppo {

struct DeviceMem;

constexpr int GEMM_MAX_SPLITS = 1024;   // narrow conv weight gradients (Kin x Co = 72 x 8) need ~4 blocks per CU

// Y = act(X W + b): X [M][K] (ldx), W [K][N] (ldw), bias [N]; columns [0, n0)
// go to out0 (ld0), [n0, N) to out1 (ld1) when out1 != nullptr.  Bit-exact
// with matrixmultiply's KC=256 k-ordered fma chains (see k_gemm.hip).
// act: 0 none, 1 relu, 2 tanh (glibc tanhf, bit-exact).
// split != 0: the split-bf16 contraction (k_gemm_split: f32 accuracy, not the chains)
hipError_t gemm_fwd(hipStream_t st, int M, int N, int K, const float *X, int ldx, const float *W,
                    int ldw, const float *bias, int act, float *out0, int ld0, int n0, float *out1,
                    int ld1, int split = 0);
// The actor forward of many models in one launch per layer (k_gemm_fwd_groups): model k owns
// the rows [gbase[k + 1], gbase[k + 2]) of X and of out.
struct FwdGroupTab {
    static constexpr int MAX = 64;
    const float *params[MAX];    // model k's parameters
    const double *on[MAX];       // its obs normalizer block [mean D | m2 D | count]
    uint8_t has_norm[MAX];       // whether the normalizer applies (count >= 2)
    uint8_t skip[MAX];           // the random player: no forward, no tile
};
// K frozen models on the device (model_set.hip), the one owner of "the models of an opponent
// pool or an evaluation": parameters [K][n_params], normalizer blocks [K][mean D | m2 D |
// count] (pack_norm_block, bppo_norm_block.h) and the table the forward reads them through
// (table = false: none, and no limit on K; CartPole's pods, one model each, run no forward
// here).  upload's copies are ordered on the context's stream, after the zeroing memsets of
// the context's allocations (a blocking hipMemcpy on the null stream would not wait for that
// non-blocking stream), and read the caller's arrays and this struct's: both outlive the
// stream's next drain.  release returns the buffers to the DeviceMem that upload took them
// from, for a set that is uploaded again at another size.
struct ModelSet {
    int K = 0;
    float *d_params = nullptr;
    double *d_on = nullptr;
    FwdGroupTab *d_tab = nullptr;
    FwdGroupTab tab{};
    std::vector<double> on;
    bool any_norm = false;
    // random_mask bit k: model k is the random player (no parameters read, no forward)
    bppo_status upload(bppo_ctx *c, DeviceMem &buf, int K, const float *params, const double *norm_mean,
                       const double *norm_m2, const double *norm_count, uint64_t random_mask, bool table = true);
    void release(DeviceMem &buf);
};
// One layer: out rows of group k = act(X rows W_k + b_k), W_k = params[k] + woff ([K][N]), b_k =
// params[k] + boff.  gbase and tab are device memory; [span_r0, span_r0 + span_rows) bounds
// the groups' rows (it sizes the grid, and the tanh pass of act 2 runs over it).  Per group
// bit-identical to gemm_fwd on that group's rows.
hipError_t gemm_fwd_groups(hipStream_t st, const int32_t *gbase, const FwdGroupTab *tab, int n_groups, int span_r0,
                           int span_rows, int N, int K, const float *X, int ldx, size_t woff, size_t boff, int act,
                           float *out, int ldo);
// out = (dZ W^T) * act'(H) given the layer OUTPUT H (may be null: no factor):
// act 2 tanh -> (1 - H^2), otherwise relu -> [H > 0].  dZ [M][K] (ldz), W [N][K] (ldw).
// Each element is the k-ordered fmaf chain from 0 (the oracle's linear_bwd dx).  xa / xw
// (may be null): + round(xa[row * ldxa] * xw[col]) after the chain, before act' -- a
// one-column head's input gradient added as its own rounded product (a shared trunk's
// value head beside the policy head's chain)
hipError_t gemm_dx(hipStream_t st, int M, int N, int K, const float *dZ, int ldz, const float *W,
                   int ldw, const float *H, int ldh, int act, float *out, int ldo, const float *xa = nullptr,
                   int ldxa = 0, const float *xw = nullptr, int split = 0);
// dW = X^T dZ over `rows` rows: X [rows][Kin] (ldx), dZ [rows][N] (ldz).
// Columns [0, n0) -> dW0 [Kin][ldw0], [n0, N) -> dW1 [Kin][ldw1] (when dW1);
// bias gradient (column sums of dZ) -> db0 / db1 likewise (either may be null).
// part: [splits][Kin][N] scratch, colsum: [splits][N] scratch (sized for doubles when exact).
// exact 0: f32 MFMA chains per split, f64 reduce; 1: f64 products and sums (k_gemm_wg64),
// the f32 result equal to the oracle's f64 sum's rounding but for rare ordering ties;
// 2: row-ordered f64 sums (k_wg_seq), the oracle's arithmetic exactly (latency-bound);
// -1: the split-bf16 contraction (k_gemm_split) per split, f64 reduce.
hipError_t gemm_wgrad(hipStream_t st, int Kin, int N, int rows, const float *X, int ldx, const float *dZ,
                      int ldz, float *part, float *colsum, float *dW0, int ldw0, int n0, float *dW1, int ldw1,
                      float *db0, float *db1, int splits, int exact = 0);
int gemm_wg_splits(int Kin, int N, int rows);

// Implicit-GEMM convolutions on Connect Four's 6 x 7 board (k_gemm.hip ConvA): NHWC
// activation rows [rows*42][C]; layer 0 reads the observation rows (obs_ld > 0: row
// stride, channels-last (h*7 + w)*Cin + ci, cnn.rs:252-262).
//   fwd   Y = relu(im2col(src) Wt + bias), Wt [Cin*ks*ks][Co] -- bit-identical to the
//         materialised im2col GEMM (same k order and KC blocks)
//   wgrad dWt = im2col(src)^T dY, db = column sums of dY (split-K, fixed-order reduce)
//   dx    dX = (taps(dY) Wd^T) * [H > 0], Wd [Cin][ks*ks*cpad]: one chain per tap (Co
//         channels, zero-padded to cpad), the taps summed in (kh, kw) order -- the
//         oracle's col2im gather
hipError_t gemm_conv_fwd(hipStream_t st, int rows, int Co, int Cin, int ks, const float *src, int obs_ld,
                         const float *Wt, const float *bias, float *out);
hipError_t gemm_conv_wgrad(hipStream_t st, int rows, int Co, int Cin, int ks, const float *src, int obs_ld,
                           const float *dY, float *part, float *colsum, float *dWt, float *db, int splits,
                           int exact = 0);
hipError_t gemm_conv_dx(hipStream_t st, int rows, int Cin, int Co, int ks, const float *dY, const float *Wd,
                        const float *H, float *out);
int gemm_conv_tap_pad(int Co);   // k's per tap of gemm_conv_dx's Wd (Co rounded up to 32)

}  // namespace bppo
