// bppo_metric_row.h — the slots of one minibatch's metric row.  Host and device code
// share the names; nothing here needs a HIP header.
#pragma once

namespace bppo {

// metric slots written after the gradient (d_grad[np + k]); the first 11 are
// shared with the CartPole kernel (k_update.hip M_*)
enum { WM_PL = 0, WM_VL, WM_H, WM_KL, WM_CF, WM_V, WM_R, WM_VE, WM_VE2, WM_VEMAX, WM_N, WM_VALID, WM_HV,
       WM_NCHOICE, WM_COUNT };
// a metric row of the update (d_rows, bppo_minibatch_rows) is WM_COUNT + 4 floats: the sums
// above, then the minibatch's raw-advantage statistics
enum { WM_ADV_MEAN = WM_COUNT, WM_ADV_STD, WM_ADV_MIN, WM_ADV_MAX };

}  // namespace bppo
