// bppo_scan.h — the block-level ordered scan of the evaluation kernels (eval.hip,
// eval_cartpole.hip): counts taken in thread order, so whatever a block numbers with it
// (draw words, recorded games, envs to freeze) is numbered in env order for any block size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bppo {

// exclusive scan of a (rows, draws) pair packed in 64 bits over the block's threads in
// thread order; *total = the block's sum.  wsum: one slot per wave.
__device__ __forceinline__ uint64_t block_scan_excl(uint64_t v, uint64_t *wsum, uint64_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint64_t inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();               // the previous scan's readers are done with wsum
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
    for (int i = 0; i < nw; i++) {
        const uint64_t s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

}  // namespace bppo
