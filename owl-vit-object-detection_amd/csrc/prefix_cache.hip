// Frozen-prefix activation cache (prefix_cache.py): the f32 residual stream at the entry of the first non-frozen consumer, kept per image.
//   prefix_emit_kernel    freshly computed images: s = (xs + delta1) + delta2 (the operands and order of ln_fwd_kernel, norm.hip; plain f32 adds) ->
//                         the image's row block of the full batch and, where the image was admitted, its cache slot
//   prefix_gather_kernel  cached images: slot -> the image's row block of the full batch
// Pure streams, HBM-bound: 16 bytes per lane, no atomics, no scratch.  The per-image addresses travel BY VALUE in the launch arguments (as
// owl_adamw_step_grouped passes its segment table), so a step issues no host-to-device copy for them; one launch takes at most
// OWL_PREFIX_MAX_IMAGES images and the entry points loop over longer lists.
#include "common.h"

#define OWL_PREFIX_MAX_IMAGES 64
#define PREFIX_UNROLL 4            // float4 per thread per trip: four independent 16-byte loads in flight per operand
#define PREFIX_MAX_BLOCKS 2048     // grid cap (8 workgroups per CU); the rest is a grid-stride loop

struct PrefixTable {
    float* dst[OWL_PREFIX_MAX_IMAGES];         // the image's row block in the full batch
    float* slot[OWL_PREFIX_MAX_IMAGES];        // emit: its cache slot (null: not admitted) / gather: the block to copy from
};

__device__ __forceinline__ void add_bf4(float4& v, const uint2 u) {
    v.x += bf2f(u.x & 0xffff); v.y += bf2f(u.x >> 16); v.z += bf2f(u.y & 0xffff); v.w += bf2f(u.y >> 16);
}

// grid (workgroups per image, images).  Image j of the launch reads block j of the compacted operands.  nvec = float4 per image.
__global__ __launch_bounds__(256) void prefix_emit_kernel(const float* __restrict__ xs, const bf16_t* __restrict__ d1, const bf16_t* __restrict__ d2,
                                                          int64_t nvec, const PrefixTable tab) {
    const int img = blockIdx.y;
    const float* x = xs + (int64_t)img * nvec * 4;
    const uint2* a = d1 ? (const uint2*)(d1 + (int64_t)img * nvec * 4) : nullptr;
    const uint2* b = d2 ? (const uint2*)(d2 + (int64_t)img * nvec * 4) : nullptr;
    float* dst = tab.dst[img];
    float* slot = tab.slot[img];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < nvec; i0 += stride * PREFIX_UNROLL) {
        float4 v[PREFIX_UNROLL];
        // the compacted operands are dead once read: streaming loads (common.h)
#pragma unroll
        for (int k = 0; k < PREFIX_UNROLL; k++) {
            const int64_t i = i0 + k * stride;
            if (i < nvec) v[k] = ld_stream_f4(x + 4 * i);
        }
        if (a) {
#pragma unroll
            for (int k = 0; k < PREFIX_UNROLL; k++) {
                const int64_t i = i0 + k * stride;
                if (i < nvec) add_bf4(v[k], ld_stream_u2(a + i));
            }
        }
        if (b) {
#pragma unroll
            for (int k = 0; k < PREFIX_UNROLL; k++) {
                const int64_t i = i0 + k * stride;
                if (i < nvec) add_bf4(v[k], ld_stream_u2(b + i));
            }
        }
#pragma unroll
        for (int k = 0; k < PREFIX_UNROLL; k++) {
            const int64_t i = i0 + k * stride;
            if (i < nvec) {
                *(float4*)(dst + 4 * i) = v[k];                    // the next kernel (a LayerNorm) reads it: plain store
                if (slot) st_stream_f4(slot + 4 * i, v[k]);        // read again an epoch later: streaming store
            }
        }
    }
}

__global__ __launch_bounds__(256) void prefix_gather_kernel(int64_t nvec, const PrefixTable tab) {
    const int img = blockIdx.y;
    const float* src = tab.slot[img];
    float* dst = tab.dst[img];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < nvec; i0 += stride * PREFIX_UNROLL) {
        float4 v[PREFIX_UNROLL];
#pragma unroll
        for (int k = 0; k < PREFIX_UNROLL; k++) {
            const int64_t i = i0 + k * stride;
            if (i < nvec) v[k] = ld_stream_f4(src + 4 * i);         // a slot is read once per epoch: it should not age the GEMMs' operands out of the caches
        }
#pragma unroll
        for (int k = 0; k < PREFIX_UNROLL; k++) {
            const int64_t i = i0 + k * stride;
            if (i < nvec) *(float4*)(dst + 4 * i) = v[k];
        }
    }
}

static inline unsigned prefix_blocks(int64_t nvec, int images) {
    int64_t want = (nvec + 256 * PREFIX_UNROLL - 1) / (256 * PREFIX_UNROLL);
    const int64_t cap = PREFIX_MAX_BLOCKS / images > 0 ? PREFIX_MAX_BLOCKS / images : 1;
    if (want > cap) want = cap;
    return (unsigned)(want < 1 ? 1 : want);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

OWL_API int owl_prefix_emit(void* stream, const float* xs, const void* delta1_bf16, const void* delta2_bf16, int64_t n, int64_t block_elems,
                            const int64_t* dst_addr, const int64_t* slot_addr) {
    OWL_CHECK_ARG(xs && dst_addr && slot_addr, "owl_prefix_emit: null pointer (xs; dst_addr, slot_addr: host arrays of n entries)");
    OWL_CHECK_ARG(n >= 1, "owl_prefix_emit: n >= 1, got %lld", (long long)n);
    OWL_CHECK_ARG(block_elems > 0 && block_elems % 8 == 0, "owl_prefix_emit: block_elems = %lld must be a positive multiple of 8 (D %% 8 == 0)", (long long)block_elems);
    OWL_CHECK_ARG(delta1_bf16 || !delta2_bf16, "owl_prefix_emit: delta2 without delta1");
    OWL_CHECK_ARG(aligned16(xs) && aligned16(delta1_bf16) && aligned16(delta2_bf16), "owl_prefix_emit: xs and the deltas must be 16-byte aligned");
    const int64_t bytes = block_elems * 4;
    for (int64_t j = 0; j < n; j++) {
        OWL_CHECK_ARG(dst_addr[j] != 0 && dst_addr[j] % 16 == 0, "owl_prefix_emit: dst_addr[%lld] must be a non-null, 16-byte aligned device address", (long long)j);
        OWL_CHECK_ARG(slot_addr[j] % 16 == 0, "owl_prefix_emit: slot_addr[%lld] must be 16-byte aligned (0: no slot)", (long long)j);
        // the destination must not overlap the compacted source (another workgroup may not have read it yet)
        const int64_t lo = (int64_t)(uintptr_t)xs, hi = lo + n * bytes;
        OWL_CHECK_ARG(dst_addr[j] + bytes <= lo || dst_addr[j] >= hi, "owl_prefix_emit: dst_addr[%lld] overlaps the compacted source xs", (long long)j);
        OWL_CHECK_ARG(slot_addr[j] == 0 || slot_addr[j] + bytes <= lo || slot_addr[j] >= hi, "owl_prefix_emit: slot_addr[%lld] overlaps the compacted source xs", (long long)j);
    }
    const int64_t nvec = block_elems / 4;
    for (int64_t j0 = 0; j0 < n; j0 += OWL_PREFIX_MAX_IMAGES) {
        const int cnt = (int)(n - j0 < OWL_PREFIX_MAX_IMAGES ? n - j0 : OWL_PREFIX_MAX_IMAGES);
        PrefixTable tab = {};
        for (int j = 0; j < cnt; j++) {
            tab.dst[j] = (float*)(uintptr_t)dst_addr[j0 + j];
            tab.slot[j] = (float*)(uintptr_t)slot_addr[j0 + j];
        }
        hipLaunchKernelGGL(prefix_emit_kernel, dim3(prefix_blocks(nvec, cnt), (unsigned)cnt), dim3(256), 0, (hipStream_t)stream, xs + j0 * block_elems,
                           delta1_bf16 ? (const bf16_t*)delta1_bf16 + j0 * block_elems : nullptr,
                           delta2_bf16 ? (const bf16_t*)delta2_bf16 + j0 * block_elems : nullptr, nvec, tab);
        OWL_LAUNCH_CHECK();
    }
    return 0;
}

OWL_API int owl_prefix_gather(void* stream, int64_t n, int64_t block_elems, const int64_t* src_addr, const int64_t* dst_addr) {
    OWL_CHECK_ARG(src_addr && dst_addr, "owl_prefix_gather: null pointer (src_addr, dst_addr: host arrays of n entries)");
    OWL_CHECK_ARG(n >= 1, "owl_prefix_gather: n >= 1, got %lld", (long long)n);
    OWL_CHECK_ARG(block_elems > 0 && block_elems % 8 == 0, "owl_prefix_gather: block_elems = %lld must be a positive multiple of 8 (D %% 8 == 0)", (long long)block_elems);
    for (int64_t j = 0; j < n; j++) {
        OWL_CHECK_ARG(src_addr[j] != 0 && src_addr[j] % 16 == 0, "owl_prefix_gather: src_addr[%lld] must be a non-null, 16-byte aligned device address", (long long)j);
        OWL_CHECK_ARG(dst_addr[j] != 0 && dst_addr[j] % 16 == 0, "owl_prefix_gather: dst_addr[%lld] must be a non-null, 16-byte aligned device address", (long long)j);
    }
    const int64_t nvec = block_elems / 4;
    for (int64_t j0 = 0; j0 < n; j0 += OWL_PREFIX_MAX_IMAGES) {
        const int cnt = (int)(n - j0 < OWL_PREFIX_MAX_IMAGES ? n - j0 : OWL_PREFIX_MAX_IMAGES);
        PrefixTable tab = {};
        for (int j = 0; j < cnt; j++) {
            tab.slot[j] = (float*)(uintptr_t)src_addr[j0 + j];
            tab.dst[j] = (float*)(uintptr_t)dst_addr[j0 + j];
        }
        hipLaunchKernelGGL(prefix_gather_kernel, dim3(prefix_blocks(nvec, cnt), (unsigned)cnt), dim3(256), 0, (hipStream_t)stream, nvec, tab);
        OWL_LAUNCH_CHECK();
    }
    return 0;
}
