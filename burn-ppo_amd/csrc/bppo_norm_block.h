// bppo_norm_block.h — a frozen model's obs normalizer block as the device reads it,
// [mean D | m2 D | count].  Plain host C++, no HIP: the model sets of the multi-player
// envs (model_set.hip) and the CartPole evaluation (D = 5) pack through it.
#pragma once
#include <cstddef>
#include <cstring>

namespace bppo {

// Model k's block into blk (zero on entry).  Returns whether the normalizer applies: with
// count < 2, or without statistics, the block stays zero and the model sees raw observations
// (ObsNormalizer::normalize_batch).
inline bool pack_norm_block(int D, int k, const double *mean, const double *m2, const double *count, double *blk) {
    if (!count || !mean || !m2 || count[k] < 2.0) return false;
    std::memcpy(blk, mean + (size_t)k * D, sizeof(double) * D);
    std::memcpy(blk + D, m2 + (size_t)k * D, sizeof(double) * D);
    blk[2 * D] = count[k];
    return true;
}

}  // namespace bppo
