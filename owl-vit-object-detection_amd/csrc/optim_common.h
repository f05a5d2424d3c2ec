// What the segmented AdamW steps share (optim_groups.hip, optim_ema.hip): the segment table passed by value and the fixed-order f64 reduction of the
// clip prologue.
#pragma once
#include "common.h"

#define OWL_OPT_MAX_SEGS 32
#define SUMSQ_MAX_BLOCKS 1024      // <= 256 * SUMSQ_PER_THREAD: the step's prologue reads SUMSQ_PER_THREAD partials per thread
#define SUMSQ_PER_THREAD 4

struct SegTable {
    int64_t end[OWL_OPT_MAX_SEGS];     // exclusive end offset of segment s (elements; multiples of 4, strictly increasing, end[nseg-1] == n)
    float lr[OWL_OPT_MAX_SEGS];
    float wd[OWL_OPT_MAX_SEGS];
};

// xor butterfly: a + b is commutative, so lanes l and l ^ o hold the same bits after every stage -- the order is fixed by the lane ids alone
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lanes (butterfly), then the four waves through LDS in wave order; the result is valid in every thread
__device__ __forceinline__ double block_sum_f64(double v, double* wsum) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

static inline int64_t sumsq_blocks(int64_t n) {
    int64_t blocks = (n / 4 + 255) / 256;
    return blocks > SUMSQ_MAX_BLOCKS ? SUMSQ_MAX_BLOCKS : blocks;
}
