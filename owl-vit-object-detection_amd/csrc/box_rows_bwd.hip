// Box head backward on the rows that carry a gradient.
//
// The box losses read pred_boxes at the matched predictions only, so d(pred_boxes) [rows, 4] is zero in all but a handful of rows (at most
// sum(targets per image); the host knows that bound without a sync), and so are du1 and du0, the box head's two upstream gradients.  The two dX GEMMs of
// the section (du0 through the erf-GELU', and the product into d(feats)) therefore run on a compact list of the non-zero rows: compaction -> gather of
// du1 / ub0 rows -> the same GEMMs at M = cap_pad -> scatter-add into d(feats).  A GEMM output row depends on its own A row alone: same bits.
// Everything that is a SUM OVER ROWS -- the six box-head gradients -- stays with the dense launches (box_final_bwd_kernel, the two weight-gradient
// products): where a row sits in their workgroups, K-tiles and splits decides how its term is rounded in, and a training run follows every bit of
// its gradients (the matcher amplifies a last-bit difference within a few steps).  du0 reaches its product as the listed rows put into a dense
// buffer that is zero elsewhere (owl_box_rows_put), cleared again afterwards.
// The kernels here take the row count from device memory and are launched with grids sized from the host's bound `cap`: no host sync anywhere.
//
// count_flag: int32 [2 + owl_box_rows_compact_blocks(rows)] in device memory, written by the compaction: [0] = listed rows (<= cap), [1] = 1 if MORE than
// cap rows were non-zero, [2 ..] the compaction's own scratch (non-zero rows per workgroup).  The gather turns a set flag into NaN in every row it
// writes, from where it reaches du0, dense0's gradients and -- through the GEMMs and the scatter-add -- d(feats): loud, no host sync (the convention
// of out-of-range labels, loss.hip).
#include "common.h"


__device__ __forceinline__ bool box_row_nonzero(const float4& g) {
    // NaN and inf are not == 0: they stay listed and propagate; -0.0 == 0
    return !(g.x == 0.f) || !(g.y == 0.f) || !(g.z == 0.f) || !(g.w == 0.f);
}

// Two launches, 1024 rows per workgroup, one row per thread (coalesced 16-byte loads): the first counts each workgroup's non-zero rows, the second
// adds up the counts of the workgroups in front of it (its base), ranks its own rows by wave ballots and writes the indices in ascending order.  No
// atomics: the list is a function of the input alone.  (One workgroup walking all rows took 105 us at 73 728 rows: a chain of dependent load rounds.)
#define BOX_ROWS_CB 1024         // rows per workgroup of the compaction

__device__ __forceinline__ int box_rows_block_sum(int v, int* lds16) {          // sum over the 1024 threads, returned to every thread
    const int t = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();          // (lds16 may still be read from a previous use)
    if ((t & 63) == 0) lds16[t >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < BOX_ROWS_CB / 64; w++) s += lds16[w];
    return s;
}

__global__ __launch_bounds__(BOX_ROWS_CB) void box_rows_count_kernel(const float* __restrict__ dboxes, int64_t rows, int* __restrict__ block_count) {
    __shared__ int lds16[BOX_ROWS_CB / 64];
    const int64_t r = (int64_t)blockIdx.x * BOX_ROWS_CB + threadIdx.x;
    const int nz = (r < rows && box_row_nonzero(*(const float4*)(dboxes + r * 4))) ? 1 : 0;
    const int n = box_rows_block_sum(nz, lds16);
    if (threadIdx.x == 0) block_count[blockIdx.x] = n;
}

__global__ __launch_bounds__(BOX_ROWS_CB) void box_rows_compact_kernel(const float* __restrict__ dboxes, int64_t rows, int cap, const int* __restrict__ block_count,
                                                                       int* __restrict__ row_list, int* __restrict__ count_flag) {
    __shared__ int lds16[BOX_ROWS_CB / 64];
    __shared__ int wave_tot[BOX_ROWS_CB / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int before = 0;
    for (int j = t; j < (int)blockIdx.x; j += BOX_ROWS_CB) before += block_count[j];
    const int base = box_rows_block_sum(before, lds16);
    const int64_t r = (int64_t)blockIdx.x * BOX_ROWS_CB + t;
    const bool nz = r < rows && box_row_nonzero(*(const float4*)(dboxes + r * 4));
    const unsigned long long m = __ballot(nz);
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int at = base + __popcll(m & ((1ull << lane) - 1ull)), own = 0;
#pragma unroll
    for (int w = 0; w < BOX_ROWS_CB / 64; w++) {
        const int v = wave_tot[w];
        if (w < wave) at += v;
        own += v;
    }
    if (nz && at < cap) row_list[at] = (int)r;
    if (blockIdx.x == gridDim.x - 1) {          // the last workgroup knows the total
        const int total = base + own, count = min(total, cap);
        for (int i = count + t; i < cap; i += BOX_ROWS_CB) row_list[i] = 0;          // (never read as a row: every reader stops at count)
        if (t == 0) { count_flag[0] = count; count_flag[1] = total > cap ? 1 : 0; }
    }
}

// dst_k[row_list[i], :] = src_k[i, :] for i < count -- or zeros where src_k is null (clears what an earlier call put); k = blockIdx.y over two pairs
struct BoxRowsPutP {
    const uint4* src[2];
    uint4* dst[2];
};
__global__ __launch_bounds__(128) void box_rows_put_kernel(BoxRowsPutP p, const int* __restrict__ row_list, const int* __restrict__ count_flag, int64_t rows, int D8) {
    const uint4* src = p.src[blockIdx.y];
    uint4* dst = p.dst[blockIdx.y];
    const int i = blockIdx.x;
    if (!dst || i >= count_flag[0]) return;
    const int r = row_list[i];
    if (r < 0 || r >= rows) return;
    for (int c = threadIdx.x; c < D8; c += 128) dst[(int64_t)r * D8 + c] = src ? src[(int64_t)i * D8 + c] : make_uint4(0, 0, 0, 0);
}

// dst_k[i, :] = src_k[row_list[i], :] for i < count, zero rows up to cap_pad; k = blockIdx.y over up to three [rows, D] bf16 sources (a null pair is skipped)
struct BoxRowsGatherP {
    const uint4* src[3];
    uint4* dst[3];
};
__global__ __launch_bounds__(128) void box_rows_gather_kernel(BoxRowsGatherP p, const int* __restrict__ row_list, const int* __restrict__ count_flag,
                                                              int64_t rows, int D8) {
    const uint4* src = p.src[blockIdx.y];
    uint4* dst = p.dst[blockIdx.y];
    if (!src || !dst) return;
    const int i = blockIdx.x;
    int r = -1;
    if (i < count_flag[0]) {
        r = row_list[i];
        if (r < 0 || r >= rows) r = -1;
    }
    const bool overflow = count_flag[1] != 0;          // more non-zero rows than promised: every listed row becomes NaN, and so does what is computed from it
    const uint4 qnan = make_uint4(0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u);
    for (int c = threadIdx.x; c < D8; c += 128)
        dst[(int64_t)i * D8 + c] = r >= 0 ? (overflow ? qnan : src[(int64_t)r * D8 + c]) : make_uint4(0, 0, 0, 0);
}

// dfeats[row_list[i], :] += dfc[i, :] (f32) for i < count.  The listed rows are distinct: plain read-add-write, no atomics.
__global__ __launch_bounds__(256) void box_rows_scatter_add_kernel(const float* __restrict__ dfc, float* __restrict__ dfeats, const int* __restrict__ row_list,
                                                                   const int* __restrict__ count_flag, int64_t rows, int D4) {
    const int i = blockIdx.x;
    if (i >= count_flag[0]) return;
    const int r = row_list[i];
    if (r < 0 || r >= rows) return;
    const float4* s = (const float4*)dfc + (int64_t)i * D4;
    float4* d = (float4*)dfeats + (int64_t)r * D4;
    for (int c = threadIdx.x; c < D4; c += 256) {
        const float4 a = d[c], b = s[c];
        d[c] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}

OWL_API int owl_box_rows_compact_blocks(int64_t rows) { return (int)((rows + BOX_ROWS_CB - 1) / BOX_ROWS_CB); }

OWL_API int owl_box_rows_compact(void* stream, const float* dboxes, int64_t rows, int64_t cap, int* row_list, int* count_flag) {
    OWL_CHECK_ARG(dboxes && row_list && count_flag, "owl_box_rows_compact: null pointer");
    OWL_CHECK_ARG(rows >= 1 && rows < (1LL << 31) && cap >= 1 && cap < (1LL << 31), "owl_box_rows_compact: 1 <= rows, cap < 2^31");
    const int nblk = owl_box_rows_compact_blocks(rows);
    hipLaunchKernelGGL(box_rows_count_kernel, dim3((unsigned)nblk), dim3(BOX_ROWS_CB), 0, (hipStream_t)stream, dboxes, rows, count_flag + 2);
    OWL_LAUNCH_CHECK();
    hipLaunchKernelGGL(box_rows_compact_kernel, dim3((unsigned)nblk), dim3(BOX_ROWS_CB), 0, (hipStream_t)stream, dboxes, rows, (int)cap, (const int*)(count_flag + 2),
                       row_list, count_flag);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_box_rows_put(void* stream, const void* src0, const void* src1, void* dst0, void* dst1, const int* row_list, const int* count_flag,
                             int64_t rows, int64_t cap, int64_t D) {
    OWL_CHECK_ARG(row_list && count_flag && (dst0 || dst1), "owl_box_rows_put: null pointer");
    OWL_CHECK_ARG((!src0 || dst0) && (!src1 || dst1), "owl_box_rows_put: a source needs its destination");
    OWL_CHECK_ARG(D >= 8 && D % 8 == 0 && rows >= 1 && rows < (1LL << 31) && cap >= 1 && cap < (1LL << 31), "owl_box_rows_put: D %% 8, 1 <= rows, cap < 2^31");
    BoxRowsPutP p;
    p.src[0] = (const uint4*)src0; p.src[1] = (const uint4*)src1; p.dst[0] = (uint4*)dst0; p.dst[1] = (uint4*)dst1;
    hipLaunchKernelGGL(box_rows_put_kernel, dim3((unsigned)cap, 2), dim3(128), 0, (hipStream_t)stream, p, row_list, count_flag, rows, (int)(D / 8));
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_box_rows_gather(void* stream, const void* src0, const void* src1, const void* src2, void* dst0, void* dst1, void* dst2,
                                const int* row_list, const int* count_flag, int64_t rows, int64_t cap_pad, int64_t D) {
    OWL_CHECK_ARG(row_list && count_flag, "owl_box_rows_gather: null pointer");
    OWL_CHECK_ARG((!src0 == !dst0) && (!src1 == !dst1) && (!src2 == !dst2), "owl_box_rows_gather: a source and its destination go together");
    OWL_CHECK_ARG(D >= 8 && D % 8 == 0 && rows >= 1 && rows < (1LL << 31) && cap_pad >= 1 && cap_pad < (1LL << 31), "owl_box_rows_gather: D %% 8, 1 <= rows, cap_pad < 2^31");
    BoxRowsGatherP p;
    p.src[0] = (const uint4*)src0; p.src[1] = (const uint4*)src1; p.src[2] = (const uint4*)src2;
    p.dst[0] = (uint4*)dst0; p.dst[1] = (uint4*)dst1; p.dst[2] = (uint4*)dst2;
    hipLaunchKernelGGL(box_rows_gather_kernel, dim3((unsigned)cap_pad, 3), dim3(128), 0, (hipStream_t)stream, p, row_list, count_flag, rows, (int)(D / 8));
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_box_rows_scatter_add(void* stream, const float* dfc, float* dfeats, const int* row_list, const int* count_flag, int64_t rows,
                                     int64_t cap, int64_t D) {
    OWL_CHECK_ARG(dfc && dfeats && row_list && count_flag, "owl_box_rows_scatter_add: null pointer");
    OWL_CHECK_ARG(D >= 4 && D % 4 == 0 && rows >= 1 && rows < (1LL << 31) && cap >= 1 && cap < (1LL << 31), "owl_box_rows_scatter_add: D %% 4, 1 <= rows, cap < 2^31");
    hipLaunchKernelGGL(box_rows_scatter_add_kernel, dim3((unsigned)cap), dim3(256), 0, (hipStream_t)stream, dfc, dfeats, row_list, count_flag, rows, (int)(D / 4));
    OWL_LAUNCH_CHECK();
    return 0;
}
