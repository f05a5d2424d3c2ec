// Open-vocabulary criterion on device: the DETR-family bipartite loss with sigmoid focal classification over the [B, P, Q] logits of
// owl_class_logits_fwd (open_vocab.hip) -- what transformers' DeformableDetrHungarianMatcher + DeformableDetrImageLoss(losses = labels, boxes)
// compute on (logits, corners_to_center(pred_boxes)), restated for per-image query lists with a query mask:
//   cost      costT[b][j][p] = w_bbox L1(centre forms) + w_class (pos - neg) + w_giou (-GIoU(corners)),   p = sigmoid(logits[b, p, label_j])
//               pos = alpha (1 - p)^2 (-log(p + 1e-8)),  neg = (1 - alpha) p^2 (-log(1 - p + 1e-8))           (HF's order and its 1e-8)
//   assign    owl_hungarian (loss.hip), unchanged, with bg = Q
//   class     element(x, t) = alpha_t softplus(z) sigmoid(z)^2,  z = t ? -x : x,  t = (target_classes[b, p] == q)
//               = HF's alpha_t bce_with_logits(x, t) (1 - p_t)^2: 1 - p_t is sigmoid(z), evaluated as such (1 - sigmoid(x) cancels for large x),
//               and bce_with_logits(x, t) is softplus(z) = max(z, 0) + log1p(exp(-|z|)); both share one expf
//   boxes     matched pairs: sum L1 on centre forms, sum 1 - GIoU on corners, unscaled gradients on the CORNERS (dl1, dgiou)
//   reduce    loss_ce = sum over (b, p, live q) / num_boxes,  loss_bbox = sum / num_boxes,  loss_giou = sum / num_boxes
//   backward  dlogits = (g_ce / num_boxes) d element / dx, recomputed from x and t, +0.0 under the mask;  dboxes = (g_bbox dl1 + g_giou dgiou) / num_boxes
// Masked columns are selected out, never multiplied: whatever bits stand there, NaN included, change nothing.
// Compiled with contraction off (csrc/build.sh): every written f32 operation rounds once, the count tests/open_vocab_loss_reference.py bounds.
// Sums are f64: per thread, wave butterfly, one partial per workgroup into the caller's scratch, the partials added in one fixed order.  No atomics,
// nothing allocated, no host sync; every summation order is a function of (B, P, Q) alone: two runs give equal bits.
#include "common.h"
#include <math.h>

#define OVL_MAX_QUERIES 4096
#define OVL_MAX_PATCHES 8192
#define OVL_UNITS 8            // units (one float, or one float4) per thread and chunk
#define OVL_MAX_PARTS 1024     // workgroups of the class kernels: at most this many, each walks chunks g, g + G, ...

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool ovl_label_ok(int64_t lab, const unsigned char* mrow, int Q) {
    if (lab < 0 || lab >= Q) return false;
    return !mrow || mrow[lab] != 0;
}

// (the operation order of giou_pair, loss.hip)
__device__ __forceinline__ float ovl_giou(const float4 a, const float4 b) {
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f), h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = w * h;
    const float uni = area_a + area_b - inter;
    const float iou = inter / uni;
    const float cw = fmaxf(fmaxf(a.z, b.z) - fminf(a.x, b.x), 0.f), ch = fmaxf(fmaxf(a.w, b.w) - fminf(a.y, b.y), 0.f);
    const float area_c = cw * ch;
    return iou - (area_c - uni) / area_c;
}

// ---------------------------------------------------------------------------------------------------
// 1. matching cost, transposed (the layout owl_hungarian reads)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ovl_cost_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ mask, const float* __restrict__ boxes,
                                                       const int64_t* __restrict__ labels, const float* __restrict__ tgt, const int* __restrict__ counts,
                                                       float* costT, int P, int Q, int nmasks, int Nmax, float alpha, float oma, float w_class, float w_bbox,
                                                       float w_giou) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int n = max(0, min(counts[b], Nmax));
    const unsigned char* mrow = mask ? mask + (int64_t)(nmasks == 1 ? 0 : b) * Q : nullptr;
    const float* row = logits + ((int64_t)b * P + p) * Q;
    const float4 bx = *(const float4*)(boxes + ((int64_t)b * P + p) * 4);
    const float acx = (bx.x + bx.z) * 0.5f, acy = (bx.y + bx.w) * 0.5f, aw = bx.z - bx.x, ah = bx.w - bx.y;
    for (int j = 0; j < n; j++) {
        // a label outside [0, Q), or one that names a masked query, never indexes the logits: zero class term here, NaN in loss_ce (ovl_pairs_kernel)
        const int64_t lab = labels[(int64_t)b * Nmax + j];
        float cls = 0.f;
        if (ovl_label_ok(lab, mrow, Q)) {
            const float x = row[lab];
            const float pr = 1.0f / (1.0f + expf(-x));
            const float om = 1.0f - pr;
            const float pos = (alpha * (om * om)) * (-logf(pr + 1e-8f));
            const float neg = (oma * (pr * pr)) * (-logf(om + 1e-8f));
            cls = pos - neg;
        }
        const float4 t = *(const float4*)(tgt + ((int64_t)b * Nmax + j) * 4);
        const float tcx = (t.x + t.z) * 0.5f, tcy = (t.y + t.w) * 0.5f, tw = t.z - t.x, th = t.w - t.y;
        const float l1 = fabsf(acx - tcx) + fabsf(acy - tcy) + fabsf(aw - tw) + fabsf(ah - th);
        const float g = ovl_giou(bx, t);
        costT[((int64_t)b * Nmax + j) * P + p] = (w_bbox * l1 + w_class * cls) + w_giou * (-g);
    }
}

// ---------------------------------------------------------------------------------------------------
// 2. sigmoid focal term of one logit and its derivative wrt the logit
// ---------------------------------------------------------------------------------------------------
template <bool GRAD>
__device__ __forceinline__ float ovl_focal(float x, bool t, float alpha, float oma, bool use_alpha) {
    const float z = t ? -x : x;
    const float a = fabsf(z);
    const float e = expf(-a);
    const float d = 1.0f + e;
    const float l = log1pf(e);
    const float sp = fmaxf(z, 0.f) + l;                 // softplus(z) = bce_with_logits(x, t)
    const bool nn = z >= 0.f;
    const float s = (nn ? 1.0f : e) / d;                // sigmoid(z) = 1 - p_t
    const float m = s * s;
    const float at = t ? alpha : oma;
    if (!GRAD) {
        float v = sp * m;
        if (use_alpha) v = at * v;
        return v;
    }
    const float c = (nn ? e : 1.0f) / d;                // sigmoid(-z)
    const float k = (2.0f * c) * sp + s;                // d[s^2 sp]/dz = s^2 (2 (1 - s) sp + s)
    float gz = m * k;
    if (use_alpha) gz = at * gz;
    return t ? -gz : gz;
}

// A unit is VEC consecutive logits of one row (VEC = 4 where Q % 4 == 0: 16 bytes per lane).  Workgroup g takes chunks g, g + G, ... of 256 * OVL_UNITS
// units; thread t of a chunk takes units t, t + 256, ...
template <int VEC, bool BWD>
__global__ __launch_bounds__(256) void ovl_focal_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ mask,
                                                        const int64_t* __restrict__ target_classes, const float* __restrict__ g3, float* dlogits,
                                                        double* partials, int64_t units, int P, int Q, int nmasks, float alpha, float oma, int use_alpha,
                                                        float inv_nb) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int QV = Q / VEC;
    const int64_t chunk = 256 * OVL_UNITS;
    const int64_t nchunks = (units + chunk - 1) / chunk;
    float gs = 0.f;
    if (BWD) gs = g3[0] * inv_nb;
    double acc = 0.0;
    // (row, column) of a thread's next unit: one 64-bit division per chunk, then 256 units further = step_r rows and step_c columns with a carry
    const int step_r = 256 / QV, step_c = 256 - step_r * QV;
    const bool per_image = mask && nmasks != 1;
    for (int64_t ck = blockIdx.x; ck < nchunks; ck += gridDim.x) {
        const int64_t u0 = ck * chunk + tid;
        int64_t r = u0 / QV;
        int cu = (int)(u0 - r * QV);
#pragma unroll
        for (int k = 0; k < OVL_UNITS; k++, r += step_r, cu += step_c) {
            if (cu >= QV) { cu -= QV; r += 1; }
            if (u0 + k * 256 >= units) continue;
            const int q0 = cu * VEC;
            const unsigned char* mrow = mask ? mask + (per_image ? (int64_t)((unsigned)r / (unsigned)P) * Q : 0) : nullptr;
            const int64_t tcv = target_classes[r];
            float x[VEC], o[VEC];
            if (VEC == 4) {
                const float4 v = *(const float4*)(logits + r * Q + q0);
                x[0] = v.x; x[1 % VEC] = v.y; x[2 % VEC] = v.z; x[3 % VEC] = v.w;
            } else {
                x[0] = logits[r * Q + q0];
            }
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                const bool live = !mrow || mrow[q0 + i] != 0;
                const bool t = tcv == (int64_t)(q0 + i);
                if (BWD) {
                    float g = 0.f;                       // (selected, not multiplied: exactly +0.0 under the mask)
                    if (live) g = gs * ovl_focal<true>(x[i], t, alpha, oma, use_alpha != 0);
                    o[i] = g;
                } else {
                    if (live) acc += (double)ovl_focal<false>(x[i], t, alpha, oma, use_alpha != 0);
                }
            }
            if (BWD) {
                if (VEC == 4) *(float4*)(dlogits + r * Q + q0) = make_float4(o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC]);
                else dlogits[r * Q + q0] = o[0];
            }
        }
    }
    if (!BWD) {
        acc = wave_sum_f64(acc);
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// ---------------------------------------------------------------------------------------------------
// 3. matched pairs of one image: sum L1 on centre forms, sum 1 - GIoU, unscaled gradients wrt the corner boxes; torch's conventions as box_loss_kernel
//    (loss.hip): the 0.5 / 0.5 split of a max / min tie, pass-through of clamp(min=0) at exactly 0, sign(0) = 0.
//    per_image[b] = {sum L1, sum 1 - GIoU, 0 or NaN (a label outside [0, Q) or on a masked query, or an index outside the image)}
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ovl_wmax(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }   // d max(a,b)/da
__device__ __forceinline__ float ovl_wmin(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }   // d min(a,b)/da
__device__ __forceinline__ float ovl_sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void ovl_pairs_kernel(const float* __restrict__ boxes, const unsigned char* __restrict__ mask,
                                                        const int64_t* __restrict__ labels, const float* __restrict__ tgt,
                                                        const int64_t* __restrict__ pred_idx, const int64_t* __restrict__ tgt_idx,
                                                        const int* __restrict__ counts, double* per_image, float* dl1, float* dgiou, int P, int Q, int nmasks,
                                                        int Nmax) {
    __shared__ double red[3][4];
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int n = max(0, min(counts[b], Nmax));
    const unsigned char* mrow = mask ? mask + (int64_t)(nmasks == 1 ? 0 : b) * Q : nullptr;
    if (dl1) for (int i = tid; i < P * 4; i += NT) { dl1[(int64_t)b * P * 4 + i] = 0.f; dgiou[(int64_t)b * P * 4 + i] = 0.f; }
    __syncthreads();
    double s_l1 = 0.0, s_g = 0.0, s_bad = 0.0;
    for (int k = tid; k < n; k += NT) {
        if (!ovl_label_ok(labels[(int64_t)b * Nmax + k], mrow, Q)) s_bad = __builtin_nan("");
        const int64_t pi = pred_idx[(int64_t)b * Nmax + k], ti = tgt_idx[(int64_t)b * Nmax + k];
        if (pi < 0 || pi >= P || ti < 0 || ti >= Nmax) { s_bad = __builtin_nan(""); continue; }      // (never from owl_hungarian; nothing is indexed with it)
        const float4 a = *(const float4*)(boxes + ((int64_t)b * P + pi) * 4);
        const float4 t = *(const float4*)(tgt + ((int64_t)b * Nmax + ti) * 4);
        const float dcx = (a.x + a.z) * 0.5f - (t.x + t.z) * 0.5f, dcy = (a.y + a.w) * 0.5f - (t.y + t.w) * 0.5f;
        const float dw = (a.z - a.x) - (t.z - t.x), dh = (a.w - a.y) - (t.w - t.y);
        s_l1 += (double)(fabsf(dcx) + fabsf(dcy) + fabsf(dw) + fabsf(dh));
        const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (t.z - t.x) * (t.w - t.y);
        const float ltx = fmaxf(a.x, t.x), lty = fmaxf(a.y, t.y), rbx = fminf(a.z, t.z), rby = fminf(a.w, t.w);
        const float w = fmaxf(rbx - ltx, 0.f), h = fmaxf(rby - lty, 0.f);
        const float inter = w * h, uni = area_a + area_b - inter, iou = inter / uni;
        const float cx0 = fminf(a.x, t.x), cy0 = fminf(a.y, t.y), cx1 = fmaxf(a.z, t.z), cy1 = fmaxf(a.w, t.w);
        const float cw = fmaxf(cx1 - cx0, 0.f), ch = fmaxf(cy1 - cy0, 0.f), area_c = cw * ch;
        const float giou = iou - (area_c - uni) / area_c;
        s_g += (double)(1.f - giou);
        if (dl1) {
            // cx = (x0 + x1) / 2, w = x1 - x0:  d|cx - .|/dx0 = d|cx - .|/dx1 = sgn / 2,  d|w - .|/dx0 = -sgn, d|w - .|/dx1 = +sgn  (exact values)
            const float sx = 0.5f * ovl_sgn(dcx), sy = 0.5f * ovl_sgn(dcy), sw = ovl_sgn(dw), sh = ovl_sgn(dh);
            float* o1 = dl1 + ((int64_t)b * P + pi) * 4;
            o1[0] = sx - sw; o1[1] = sy - sh; o1[2] = sx + sw; o1[3] = sy + sh;
            // forward-mode partials wrt (a.x, a.y, a.z, a.w)
            const float dw_on = (rbx - ltx >= 0.f) ? 1.f : 0.f, dh_on = (rby - lty >= 0.f) ? 1.f : 0.f;
            const float dcw_on = (cx1 - cx0 >= 0.f) ? 1.f : 0.f, dch_on = (cy1 - cy0 >= 0.f) ? 1.f : 0.f;
            float d_inter[4], d_area_a[4], d_area_c[4];
            d_inter[0] = dw_on * (-ovl_wmax(a.x, t.x)) * h;   d_inter[2] = dw_on * (ovl_wmin(a.z, t.z)) * h;
            d_inter[1] = w * dh_on * (-ovl_wmax(a.y, t.y));   d_inter[3] = w * dh_on * (ovl_wmin(a.w, t.w));
            d_area_a[0] = -(a.w - a.y); d_area_a[2] = (a.w - a.y); d_area_a[1] = -(a.z - a.x); d_area_a[3] = (a.z - a.x);
            d_area_c[0] = dcw_on * (-ovl_wmin(a.x, t.x)) * ch; d_area_c[2] = dcw_on * (ovl_wmax(a.z, t.z)) * ch;
            d_area_c[1] = cw * dch_on * (-ovl_wmin(a.y, t.y)); d_area_c[3] = cw * dch_on * (ovl_wmax(a.w, t.w));
            float* o2 = dgiou + ((int64_t)b * P + pi) * 4;
            for (int e = 0; e < 4; e++) {
                const float d_uni = d_area_a[e] - d_inter[e];
                const float d_iou = (d_inter[e] * uni - inter * d_uni) / (uni * uni);
                const float d_ratio = (d_uni * area_c - uni * d_area_c[e]) / (area_c * area_c);   // d(union/area_c)
                o2[e] = -(d_iou + d_ratio);
            }
        }
    }
    s_l1 = wave_sum_f64(s_l1); s_g = wave_sum_f64(s_g); s_bad = wave_sum_f64(s_bad);
    if ((tid & 63) == 0) { red[0][tid >> 6] = s_l1; red[1][tid >> 6] = s_g; red[2][tid >> 6] = s_bad; }
    __syncthreads();
    if (tid < 3) per_image[b * 3 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// 4. the three outputs: one wave; lane l adds partials l, l + 64, ... in ascending order, then the butterfly; the per-image terms in index order
__global__ __launch_bounds__(64) void ovl_reduce_kernel(const double* __restrict__ partials, const double* __restrict__ per_image, float* losses, int nparts, int B,
                                                        double num_boxes) {
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int i = lane; i < nparts; i += 64) s += partials[i];
    s = wave_sum_f64(s);
    if (lane == 0) {
        double l1 = 0.0, gi = 0.0;
        for (int b = 0; b < B; b++) { l1 += per_image[b * 3 + 0]; gi += per_image[b * 3 + 1]; s += per_image[b * 3 + 2]; }
        losses[0] = (float)(s / num_boxes);
        losses[1] = (float)(l1 / num_boxes);
        losses[2] = (float)(gi / num_boxes);
    }
}

// 5. dboxes = (g_bbox dl1 + g_giou dgiou) / num_boxes
__global__ __launch_bounds__(256) void ovl_boxes_bwd_kernel(const float* __restrict__ g3, const float* __restrict__ dl1, const float* __restrict__ dgiou, float* dboxes,
                                                            int64_t n, float inv_nb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gb = g3[1] * inv_nb, gg = g3[2] * inv_nb;
    dboxes[i] = gb * dl1[i] + gg * dgiou[i];
}

// ---------------------------------------------------------------------------------------------------
static int ovl_check_shape(const char* who, int64_t B, int64_t P, int64_t Q, int64_t nmasks, const void* mask) {
    OWL_CHECK_ARG(B >= 1 && P >= 1 && P <= OVL_MAX_PATCHES && B * P < ((int64_t)1 << 31), "%s: B >= 1, 1 <= P <= %d and B P < 2^31 required (B=%lld P=%lld)", who,
                  OVL_MAX_PATCHES, (long long)B, (long long)P);
    OWL_CHECK_ARG(Q >= 1 && Q <= OVL_MAX_QUERIES, "%s: 1 <= Q <= %d required (Q=%lld)", who, OVL_MAX_QUERIES, (long long)Q);
    OWL_CHECK_ARG(!mask || nmasks == 1 || nmasks == B, "%s: mask is [nmasks, Q] with nmasks = B or 1 (got %lld for B=%lld)", who, (long long)nmasks, (long long)B);
    return 0;
}

static int64_t ovl_units(int64_t B, int64_t P, int64_t Q) { return B * P * (Q % 4 == 0 ? Q / 4 : Q); }
static int ovl_parts(int64_t B, int64_t P, int64_t Q) {
    const int64_t chunk = 256 * OVL_UNITS, nchunks = (ovl_units(B, P, Q) + chunk - 1) / chunk;
    return (int)(nchunks < OVL_MAX_PARTS ? nchunks : OVL_MAX_PARTS);
}

// workspace (f64): per_image [B, 3], then one partial per workgroup of the class kernel
OWL_API int owl_focal_loss_workspace_bytes(int64_t B, int64_t P, int64_t Q, int64_t* bytes) {
    OWL_CHECK_ARG(bytes, "owl_focal_loss_workspace_bytes: null pointer");
    if (ovl_check_shape("owl_focal_loss_workspace_bytes", B, P, Q, 1, nullptr)) return -1;
    *bytes = 8 * (3 * B + (int64_t)ovl_parts(B, P, Q));
    return 0;
}

static int ovl_check_workspace(const char* who, const void* workspace, int64_t workspace_bytes, int64_t B, int64_t P, int64_t Q) {
    OWL_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0, "%s: workspace must be non-null and 8-byte aligned", who);
    const int64_t need = 8 * (3 * B + (int64_t)ovl_parts(B, P, Q));
    OWL_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed (owl_focal_loss_workspace_bytes)", who, (long long)workspace_bytes,
                  (long long)need);
    return 0;
}

OWL_API int owl_focal_match_cost(void* stream, const float* logits, const unsigned char* mask, const float* boxes, const int64_t* labels, const float* tgt_boxes,
                                 const int* counts, float* costT, int64_t B, int64_t P, int64_t Q, int64_t nmasks, int64_t Nmax, float alpha, float w_class,
                                 float w_bbox, float w_giou) {
    OWL_CHECK_ARG(logits && boxes && labels && tgt_boxes && counts && costT, "owl_focal_match_cost: null pointer");
    if (ovl_check_shape("owl_focal_match_cost", B, P, Q, nmasks, mask)) return -1;
    OWL_CHECK_ARG(Nmax >= 1 && Nmax <= P, "owl_focal_match_cost: need 1 <= Nmax <= P");
    // (tgt_boxes: PackedTargets lays it behind the labels in one staging buffer, 8-byte aligned -- as for owl_match_cost, whose float4 loads gfx950 takes unaligned)
    OWL_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)tgt_boxes & 3) == 0, "owl_focal_match_cost: boxes must be 16-byte aligned");
    hipLaunchKernelGGL(ovl_cost_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, mask, boxes, labels, tgt_boxes,
                       counts, costT, (int)P, (int)Q, (int)nmasks, (int)Nmax, alpha, 1.0f - alpha, w_class, w_bbox, w_giou);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_focal_loss_fwd(void* stream, const float* logits, const unsigned char* mask, const int64_t* target_classes, void* workspace,
                               int64_t workspace_bytes, int64_t B, int64_t P, int64_t Q, int64_t nmasks, float alpha) {
    OWL_CHECK_ARG(logits && target_classes, "owl_focal_loss_fwd: null pointer");
    if (ovl_check_shape("owl_focal_loss_fwd", B, P, Q, nmasks, mask)) return -1;
    if (ovl_check_workspace("owl_focal_loss_fwd", workspace, workspace_bytes, B, P, Q)) return -1;
    OWL_CHECK_ARG(Q % 4 != 0 || ((uintptr_t)logits & 15) == 0, "owl_focal_loss_fwd: logits must be 16-byte aligned where Q %% 4 == 0");
    double* partials = (double*)workspace + 3 * B;
    const int G = ovl_parts(B, P, Q);
    const int64_t units = ovl_units(B, P, Q);
    const float a = alpha >= 0.f ? alpha : 0.f;
    if (Q % 4 == 0)
        hipLaunchKernelGGL((ovl_focal_kernel<4, false>), dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, logits, mask, target_classes, (const float*)nullptr,
                           (float*)nullptr, partials, units, (int)P, (int)Q, (int)nmasks, a, 1.0f - a, alpha >= 0.f ? 1 : 0, 0.f);
    else
        hipLaunchKernelGGL((ovl_focal_kernel<1, false>), dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, logits, mask, target_classes, (const float*)nullptr,
                           (float*)nullptr, partials, units, (int)P, (int)Q, (int)nmasks, a, 1.0f - a, alpha >= 0.f ? 1 : 0, 0.f);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_box_pair_loss(void* stream, const float* boxes, const unsigned char* mask, const int64_t* labels, const float* tgt_boxes, const int64_t* pred_idx,
                              const int64_t* tgt_idx, const int* counts, void* workspace, int64_t workspace_bytes, float* dl1, float* dgiou, int64_t B, int64_t P,
                              int64_t Q, int64_t nmasks, int64_t Nmax) {
    OWL_CHECK_ARG(boxes && labels && tgt_boxes && pred_idx && tgt_idx && counts, "owl_box_pair_loss: null pointer");
    OWL_CHECK_ARG((dl1 == nullptr) == (dgiou == nullptr), "owl_box_pair_loss: gradient buffers are all-or-none");
    if (ovl_check_shape("owl_box_pair_loss", B, P, Q, nmasks, mask)) return -1;
    if (ovl_check_workspace("owl_box_pair_loss", workspace, workspace_bytes, B, P, Q)) return -1;
    OWL_CHECK_ARG(Nmax >= 1 && Nmax <= P, "owl_box_pair_loss: need 1 <= Nmax <= P");
    // (tgt_boxes: PackedTargets lays it behind the labels in one staging buffer, 8-byte aligned -- as for owl_match_cost, whose float4 loads gfx950 takes unaligned)
    OWL_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)tgt_boxes & 3) == 0, "owl_box_pair_loss: boxes must be 16-byte aligned");
    hipLaunchKernelGGL(ovl_pairs_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, boxes, mask, labels, tgt_boxes, pred_idx, tgt_idx, counts,
                       (double*)workspace, dl1, dgiou, (int)P, (int)Q, (int)nmasks, (int)Nmax);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_open_vocab_loss_reduce(void* stream, const void* workspace, int64_t workspace_bytes, float* losses, int64_t B, int64_t P, int64_t Q,
                                       double num_boxes) {
    OWL_CHECK_ARG(losses, "owl_open_vocab_loss_reduce: null pointer");
    if (ovl_check_shape("owl_open_vocab_loss_reduce", B, P, Q, 1, nullptr)) return -1;
    if (ovl_check_workspace("owl_open_vocab_loss_reduce", workspace, workspace_bytes, B, P, Q)) return -1;
    OWL_CHECK_ARG(num_boxes > 0.0, "owl_open_vocab_loss_reduce: num_boxes must be positive");
    const double* ws = (const double*)workspace;
    hipLaunchKernelGGL(ovl_reduce_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ws + 3 * B, ws, losses, ovl_parts(B, P, Q), (int)B, num_boxes);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_focal_loss_bwd(void* stream, const float* g3, const float* logits, const unsigned char* mask, const int64_t* target_classes, float* dlogits,
                               int64_t B, int64_t P, int64_t Q, int64_t nmasks, float alpha, double num_boxes) {
    OWL_CHECK_ARG(g3 && logits && target_classes && dlogits, "owl_focal_loss_bwd: null pointer");
    if (ovl_check_shape("owl_focal_loss_bwd", B, P, Q, nmasks, mask)) return -1;
    OWL_CHECK_ARG(num_boxes > 0.0, "owl_focal_loss_bwd: num_boxes must be positive");
    OWL_CHECK_ARG(Q % 4 != 0 || (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0, "owl_focal_loss_bwd: logits and dlogits must be 16-byte aligned where Q %% 4 == 0");
    const int G = ovl_parts(B, P, Q);
    const int64_t units = ovl_units(B, P, Q);
    const float a = alpha >= 0.f ? alpha : 0.f;
    const float inv_nb = (float)(1.0 / num_boxes);
    if (Q % 4 == 0)
        hipLaunchKernelGGL((ovl_focal_kernel<4, true>), dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, logits, mask, target_classes, g3, dlogits,
                           (double*)nullptr, units, (int)P, (int)Q, (int)nmasks, a, 1.0f - a, alpha >= 0.f ? 1 : 0, inv_nb);
    else
        hipLaunchKernelGGL((ovl_focal_kernel<1, true>), dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, logits, mask, target_classes, g3, dlogits,
                           (double*)nullptr, units, (int)P, (int)Q, (int)nmasks, a, 1.0f - a, alpha >= 0.f ? 1 : 0, inv_nb);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_box_pair_loss_bwd(void* stream, const float* g3, const float* dl1, const float* dgiou, float* dboxes, int64_t B, int64_t P, double num_boxes) {
    OWL_CHECK_ARG(g3 && dl1 && dgiou && dboxes, "owl_box_pair_loss_bwd: null pointer");
    OWL_CHECK_ARG(B >= 1 && P >= 1 && B * P < ((int64_t)1 << 31), "owl_box_pair_loss_bwd: B >= 1, P >= 1 and B P < 2^31 required");
    OWL_CHECK_ARG(num_boxes > 0.0, "owl_box_pair_loss_bwd: num_boxes must be positive");
    const int64_t n = B * P * 4;
    hipLaunchKernelGGL(ovl_boxes_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g3, dl1, dgiou, dboxes, n,
                       (float)(1.0 / num_boxes));
    OWL_LAUNCH_CHECK();
    return 0;
}
