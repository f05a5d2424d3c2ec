// Thread-local error string + version for libowlhip's C ABI (include/owl_hip.h).
#include <stdarg.h>
#include <stdio.h>
#include "../../include/owl_hip.h"
#define OWL_API extern "C" __attribute__((visibility("default")))   // (as in common.h: the library is linked with -fvisibility=hidden)

static thread_local char g_err[512] = "";

void owl_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

OWL_API const char* owl_last_error(void) { return g_err; }
OWL_API int owl_abi_version(void) { return OWL_ABI_VERSION; }

// ---------------------------------------------------------------------------------------------------------------------
// Host side of the device input pipeline (ref src/dataset.py:69-71 -> HF OwlViTImageProcessor
// -> PIL Image.resize(BICUBIC)).  Pillow's Resample.c computes the separable filter taps in f64 on the host and converts
// them to 22-bit fixed point; the device kernels (preprocess.hip) consume exactly these tables, so the resize is
// bit-identical to Pillow's.  Built with -ffp-contract=off: the f64 expressions must round like Pillow's.
// ---------------------------------------------------------------------------------------------------------------------
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static inline double pil_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's precompute_coeffs for one axis and a source box [in0, in1) (Image.resize(size, BICUBIC, box=...)): the taps are clipped to the IMAGE
// [0, in_size), not to the box.  in0 = 0, in1 = in_size is the whole-axis resize: x - 0.0 and 0.0 + x are exact, so both entries share this body bit for bit.
static int bicubic_coeffs_impl(const char* who, int64_t in_size, double in0, double in1, int64_t out_size, int* bounds, int* kk, int64_t kk_capacity, int* ksize_out) {
    const int PRECISION_BITS = 32 - 8 - 2;
    double scale, filterscale;
    filterscale = scale = (in1 - in0) / (double)out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    if ((int64_t)ksize * out_size > kk_capacity) {
        owl_set_error("%s: kk capacity %lld < %lld", who, (long long)kk_capacity, (long long)ksize * out_size);
        return -1;
    }
    *ksize_out = ksize;
    const double ss = 1.0 / filterscale;
    double w[4096];
    if (ksize > 4096) { owl_set_error("%s: ksize %d too large", who, ksize); return -1; }
    for (int64_t xx = 0; xx < out_size; xx++) {
        const double center = in0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = (int)in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) {
            w[x] = pil_bicubic((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int* k = kk + xx * ksize;
        for (int x = 0; x < xmax; x++) {
            double v = w[x];
            if (ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
        for (int x = xmax; x < ksize; x++) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return 0;
}

// bounds[2*out] = {first tap, tap count}; kk[out*ksize] fixed-point weights (zero padded).  HOST pointers.
OWL_API int owl_bicubic_coeffs(int64_t in_size, int64_t out_size, int* bounds, int* kk, int64_t kk_capacity, int* ksize_out) {
    if (in_size <= 0 || out_size <= 0 || !bounds || !kk || !ksize_out) {
        owl_set_error("owl_bicubic_coeffs: bad arguments (in=%lld out=%lld)", (long long)in_size, (long long)out_size);
        return -1;
    }
    return bicubic_coeffs_impl("owl_bicubic_coeffs", in_size, 0.0, (double)in_size, out_size, bounds, kk, kk_capacity, ksize_out);
}

// The same tables for the source box [in0, in1) of an axis of in_size pixels (float edges; 0 <= in0 < in1 <= in_size): a crop folded into the resize.
OWL_API int owl_bicubic_coeffs_box(int64_t in_size, double in0, double in1, int64_t out_size, int* bounds, int* kk, int64_t kk_capacity, int* ksize_out) {
    if (in_size <= 0 || in_size > INT32_MAX || out_size <= 0 || !bounds || !kk || !ksize_out || !(in0 >= 0.0) || !(in1 > in0) || !(in1 <= (double)in_size)) {
        owl_set_error("owl_bicubic_coeffs_box: bad arguments (in=%lld box=[%g, %g) out=%lld)", (long long)in_size, in0, in1, (long long)out_size);
        return -1;
    }
    return bicubic_coeffs_impl("owl_bicubic_coeffs_box", in_size, in0, in1, out_size, bounds, kk, kk_capacity, ksize_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// OWLv2's input stage (HF Owlv2ImageProcessorPil: pad bottom / right to a square of side S = max(H, W), scipy.ndimage.gaussian_filter with
// sigma = max(0, (S/N - 1)/2), scipy.ndimage.zoom(order=1, mode="mirror", grid_mode=True) to N x N).  Blur and zoom are separable and linear and the pad
// is a constant, so per axis the stage is one matrix A = Z G (N x S): the bilinear rows times the mirrored Gaussian.  Row i of A, restricted to the columns
// below `in_extent` (the real pixels; the others multiply the pad), is what the device kernels (pad_resize.hip) consume.  All in f64, scipy's conventions:
// lw = int(4 sigma + 0.5), weights exp(-x^2 / (2 sigma^2)) normalised over [-lw, lw] (no blur at all for sigma <= 1e-15), `mirror` (no edge repeat) at
// the PADDED length for both operators, centre (i + 0.5) S/N - 0.5.
// ---------------------------------------------------------------------------------------------------------------------
#define OWL_PAD_RESIZE_MAX_TAPS 64          // per output index and axis: 2 lw + 2 <= 62 at S = 16 N

static inline int64_t mirror_index(int64_t i, int64_t n) {
    if (n <= 1) return 0;
    const int64_t period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// bounds[2*i] = {first source index, tap count} of output i (count 0: every tap of the row lies in the pad; leading / trailing zero weights trimmed),
// w[i*ksize + t] the f64 weights rounded once to f32 (zero padded to ksize = the largest count, at least 1), wsum[i] = the f64 sum of the kept weights
// rounded once (1 - wsum_x wsum_y is the weight of the pad under an output pixel).  HOST pointers; w_capacity in floats.
OWL_API int owl_pad_resize_coeffs(int64_t in_extent, int64_t padded, int64_t out_size, int* bounds, float* w, int64_t w_capacity, int* ksize_out, float* wsum) {
    if (in_extent <= 0 || padded < in_extent || padded > INT32_MAX || out_size <= 0 || !bounds || !w || !ksize_out || !wsum) {
        owl_set_error("owl_pad_resize_coeffs: bad arguments (extent=%lld padded=%lld out=%lld)", (long long)in_extent, (long long)padded, (long long)out_size);
        return -1;
    }
    if (padded > 16 * out_size) {
        owl_set_error("owl_pad_resize_coeffs: padded side %lld > 16 x the output side %lld: the blur would need more than %d taps per output pixel",
                      (long long)padded, (long long)out_size, OWL_PAD_RESIZE_MAX_TAPS);
        return -1;
    }
    const double f = (double)padded / (double)out_size;
    double sigma = (f - 1.0) / 2.0;
    if (sigma < 0.0) sigma = 0.0;
    int lw = 0;
    double g[2 * 32 + 1];
    g[0] = 1.0;
    if (sigma > 1e-15) {
        lw = (int)(4.0 * sigma + 0.5);
        if (lw > 32) { owl_set_error("owl_pad_resize_coeffs: blur radius %d too large", lw); return -1; }
        double sum = 0.0;
        for (int k = -lw; k <= lw; k++) { g[k + lw] = exp(-0.5 / (sigma * sigma) * (double)(k * k)); sum += g[k + lw]; }
        for (int k = 0; k <= 2 * lw; k++) g[k] /= sum;
    }
    // pass 1: the rows into a scratch of OWL_PAD_RESIZE_MAX_TAPS per output (ksize is known only afterwards)
    double* rows = (double*)malloc(sizeof(double) * (size_t)out_size * OWL_PAD_RESIZE_MAX_TAPS);
    if (!rows) { owl_set_error("owl_pad_resize_coeffs: out of memory"); return -1; }
    int ksize = 1, rc = 0;
    for (int64_t i = 0; i < out_size && rc == 0; i++) {
        const double cc = ((double)i + 0.5) * f - 0.5;
        const double fl = floor(cc), t = cc - fl;
        const int64_t z0 = (int64_t)fl;
        const double zw[2] = {1.0 - t, t};
        int64_t idx[2 * 65];
        double val[2 * 65];
        int n = 0;
        int64_t lo = INT64_MAX, hi = -1;
        for (int a = 0; a < 2; a++) {
            if (zw[a] == 0.0) continue;
            const int64_t zi = mirror_index(z0 + a, padded);
            for (int k = -lw; k <= lw; k++) {
                idx[n] = mirror_index(zi + k, padded);
                val[n] = zw[a] * g[k + lw];
                if (idx[n] < lo) lo = idx[n];
                if (idx[n] > hi) hi = idx[n];
                n++;
            }
        }
        if (hi >= in_extent) hi = in_extent - 1;                  // indices in the pad drop out
        double* row = rows + i * OWL_PAD_RESIZE_MAX_TAPS;
        int count = 0;
        if (lo <= hi) {
            if (hi - lo + 1 > OWL_PAD_RESIZE_MAX_TAPS) { owl_set_error("owl_pad_resize_coeffs: output %lld spans %lld source pixels", (long long)i, (long long)(hi - lo + 1)); rc = -1; break; }
            count = (int)(hi - lo + 1);
            for (int q = 0; q < count; q++) row[q] = 0.0;
            for (int q = 0; q < n; q++)                            // reflected taps add onto their index, in tap order
                if (idx[q] <= hi) row[idx[q] - lo] += val[q];
            int head = 0;
            while (head < count && row[head] == 0.0) head++;
            while (count > head && row[count - 1] == 0.0) count--;
            count -= head;
            for (int q = 0; q < count; q++) row[q] = row[q + head];
            lo += head;
        }
        double s = 0.0;
        for (int q = 0; q < count; q++) s += row[q];
        wsum[i] = (float)s;
        bounds[2 * i] = count ? (int)lo : 0;
        bounds[2 * i + 1] = count;
        if (count > ksize) ksize = count;
    }
    if (rc == 0 && (int64_t)ksize * out_size > w_capacity) {
        owl_set_error("owl_pad_resize_coeffs: w capacity %lld < %lld", (long long)w_capacity, (long long)ksize * out_size);
        rc = -1;
    }
    if (rc == 0) {
        for (int64_t i = 0; i < out_size; i++)
            for (int q = 0; q < ksize; q++)
                w[i * ksize + q] = q < bounds[2 * i + 1] ? (float)rows[i * OWL_PAD_RESIZE_MAX_TAPS + q] : 0.0f;
        *ksize_out = ksize;
    }
    free(rows);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// The path's ONE collective: SUM of the flat f32 gradient bucket over the data-parallel ranks, in place, on the caller's
// stream, through the caller's RCCL communicator.  For hosts WITHOUT PyTorch: the Python host of this repo issues the same collective through
// torch.distributed (backend "nccl" = RCCL; ddp.py) because torch owns its communicator and does not hand it out.  librccl is bound lazily
// (dlopen at the first call), so libowlhip.so has no load-time dependency on it: single-GPU users never touch it.
// ---------------------------------------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <stddef.h>

typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, void*);    // ncclAllReduce(send, recv, count, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t)
typedef const char* (*nccl_errstr_fn)(int);

OWL_API int owl_allreduce_sum_f32(void* stream, void* rccl_comm, float* buf, int64_t n) {
    if (!rccl_comm || !buf || n <= 0) {
        owl_set_error("owl_allreduce_sum_f32: null communicator / buffer or n = %lld", (long long)n);
        return -1;
    }
    static nccl_allreduce_fn allreduce = nullptr;          // (resolved once; a benign race resolves the same symbol twice)
    static nccl_errstr_fn errstr = nullptr;
    if (!allreduce) {
        // the RCCL instance the process ALREADY has (the one the caller built `rccl_comm` with: e.g. PyTorch's bundled copy) before loading another one
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { owl_set_error("owl_allreduce_sum_f32: cannot load librccl.so (%s)", dlerror()); return -2; }
        allreduce = (nccl_allreduce_fn)dlsym(h, "ncclAllReduce");
        errstr = (nccl_errstr_fn)dlsym(h, "ncclGetErrorString");
        if (!allreduce) { owl_set_error("owl_allreduce_sum_f32: librccl.so has no ncclAllReduce"); return -2; }
    }
    const int rc = allreduce(buf, buf, (size_t)n, /* ncclFloat32 */ 7, /* ncclSum */ 0, rccl_comm, stream);
    if (rc != 0) {
        owl_set_error("owl_allreduce_sum_f32: ncclAllReduce failed: %s", errstr ? errstr(rc) : "unknown RCCL error");
        return -3;
    }
    return 0;
}
