"""Float64 references, derived error bounds, input profiles and an f32 simulation for the bf16 MFMA GEMM family (csrc/gemm.hip, gemm_pp2.hip,
gemm_pph.hip, the shared epilogues of csrc/gemm_common.h and the dispatcher owl_gemm_nt_bf16).  Checker side; device-agnostic: every function
works on whatever device its inputs live on.

Reference
---------
`exact(epi, A, W, bias, alpha, resid, aux_in, splits)`  the epilogues of gemm_common.h:10-24 in float64 on bf16-exact A [M, K], W [N, K] and
f32-exact bias / resid:  acc = A W^T,  pre = alpha acc (+ bias),
    BIAS  out = pre                     QGELU  out = pre s, s = sigmoid(1.702 pre); aux = quick_gelu'(pre) = s (1 + 1.702 pre (1 - s))
    GELU  out = pre Phi(pre); aux = pre RESID / ACC  out = resid + pre              F32    out = pre
    SLAB  out[s] = alpha A[:, Ks] W[:, Ks]^T per split, `reduced` = their sum (+ resid with accumulate)
    DQGELU out = pre aux_in             DGELU  out = pre (Phi(a) + a phi(a)), a = aux_in
The derivative epilogues are judged on the bf16 `aux_in` they are given, as the kernel receives it.  The result also carries the float64
intermediates the bounds need (acc, acc_abs = |A| |W|^T, pre).

Bounds (elementwise, derived, no fitted constant)
-------------------------------------------------
u = 2^-8 is bf16's unit round-off (half an ulp, relative), f = 2^-24 is f32's, gamma(n) = n f / (1 - n f) (the conventions of
attention_reference.py:24-25); "1 ulp" of v_exp_f32 / v_rcp_f32 is a relative 2 f (attention_reference.py:31).  T = 2^-126 is the smallest
normal of f32 and bf16: the MFMAs, v_exp / v_rcp and the bf16 conversion do not keep denormals.

 accumulation.  The products of two bf16 are exact in f32; the kernels add them with v_mfma_f32_32x32x16_bf16, 16 products per instruction
   into one accumulator, K / 16 instructions in a row, K-tile after K-tile (gemm.hip, gemm_nt_kernel's main loop; gemm_pp2.hip / gemm_pph.hip: same order).
   ASSUMPTION 1: the rounding of the MFMA's internal adds is not documented as round-to-nearest, so every add is budgeted at 2 f (truncation)
   and the order of the 16 products inside one instruction is taken as unknown.  A product then passes at most 16 adds inside its own
   instruction (15 among the products, 1 onto the accumulator) and one add per later instruction:
       n_acc(K) = K / 16 + 16,    |acc~ - acc| <= gamma2(n_acc) acc_abs,   gamma2(n) = 2 n f / (1 - 2 n f)
   For every K >= 64 this lies below gamma2(K + 1) acc_abs, the bound that holds for ANY summation order (`acc_bound(..., any_order=True)`):
   the any-order bound is 1 % of acc_abs at K = 4096 -- wider than two bf16 roundings of a typical output -- so the chain the kernels
   actually run is used; the CPU test holds the simulation (K-tiles of 64 in f32, the order inside a tile the BLAS's own) to it all the same.
 pre-activation.  v = fl(fl(alpha acc~) + bias) in epi_quad / epi_tile_f32 (gemm_common.h:72-76,486-490), one fma in epi_tile_bf16 /
   epi_lines_bf16 (gemm_common.h:258-259,422-423); the two-rounding form bounds both:
       E_al = |alpha| E_acc + f |alpha| (|acc| + E_acc);   E_pre = E_al + f (|pre| + E_al) with a bias, E_al without;  + T
 store.  bf16 (pack_bf2, common.h:30-33, RNE):  tol = E + u (|ref| + E) + T.   f32: the value itself, tol = E + T.
   RESID / ACC add the residual in f32 (gemm_common.h:104-106,493-495): tol = E_pre + f (|ref| + E_pre) + T.
 quick-GELU (sigmoid1702_f, gemm_common.h:46-48,263-275): t = fl(c x), c = f32(-1.702 log2 e): |dt| <= 2 f |c x| (the constant's and the
   product's rounding: GROWS with |x|); e~ = v_exp(t): rel  re = 2^dt (1 + 2 f) - 1;  d = fl(1 + e~) (f), r = v_rcp(d) (2 f):
       s~ = s (1 + dr) / ((1 + (1 - s) de) (1 + dd))  =>  rs = (1 + 2 f) / ((1 - (1 - s) re) (1 - f)) - 1
   out = fl(x s~): ro = (1 + rs)(1 + f) - 1.  For x < -51.3 the sigmoid is below T (2^-126 <-> t = 126) and v_rcp returns 0, for x < -52.1
   v_exp overflows to inf: the product x s~ is then -0 where the exact value is up to |x| T: + |x| T ("a factor flushed inside a product").
   propagation of E_pre through the activation, first order with the explicit remainder: |g'(pre)| E_pre + sup|g''| E_pre^2 / 2,
   sup |quick_gelu''| = 0.851 (at 0) <= QG_SUP2.
   saved derivative (dqgelu_from_s, gemm_common.h:53-56): t1 = fl(1.702f x) (2 f), om = fl(1 - s~): |d om| <= s rs + f (1 - s),
       h = fma(t1, om, 1): |dh| <= 1.702 |x| (2 f (1 - s) + (1 + 2 f) d om) + f |h|;  aux = fl(s~ h~): |s h| ro + s (1 + ro) dh + (|h| + 1) T
   propagated with |quick_gelu''(pre)| E_pre + sup|quick_gelu'''| E_pre^2 / 2, sup <= QG_SUP3 (test_gemm_reference.py checks both sups on a grid).
   The evaluation errors are formed at pre, the f32 point lies within E_pre of it: + 1.2 E_pre (ro + 16 f) (|g'| <= 1.2; erf-GELU: 16 f).
 erf-GELU (gelu_f, gemm_common.h:58): z = fl(x / sqrt 2) (2 f), the argument error moves erf by (2 / sqrt pi) exp(-z^2) |z| 2 f;
   ASSUMPTION 2: erff (the device libm's) is within 4 ulp = 8 f of its result (a cap well below u); w = fl(1 + erf~) (f); 0.5 x is exact;
   out = fl(0.5 x w):  E = 0.5 |x| (d_arg + 8 f |erf| + f |w|) (1 + f) + f |g|.  In the negative tail 1 + erff cancels: the absolute error
   stays 0.5 |x| 8 f while g -> -0, so the bound there is absolute -- the kernel returns -0 from x = -5.6 on (erff = -1), the reference a
   subnormal from x = -13.  sup |gelu''| = 0.798 <= GELU_SUP2.  aux = bf16(v): the plain store bound on E_pre.
 DQGELU (gemm_common.h:101,294,445): out = fl(v a), a exact:  E = |a| E_pre + f (|pre a| + |a| E_pre) + (|a| + |pre| + 1) T.
 DGELU (dgelu_erf_f, common.h:70-77) at the exact bf16 a:  x = fl(|a| / sqrt 2) (2 f); den = fma(p, x, 1): rel 4 f; t = v_rcp: rt = 6 f + ...;
   e~ = v_exp(fl(a a c2)), a a exact, |dt| <= 2 f c2 a^2 (GROWS with a^2), rel re as above, flushed to 0 below T (|a| > 13.2): + T;
   Horner's five fmas on rounded coefficients: |d poly| <= 7 f S0 + rt S1, S0 = sum |a_i| t^i, S1 = sum i |a_i| t^i (elementwise, float64);
   erf_abs = fma(-poly, e, 1):  d_erf = AS_ERR + e (|d poly| (1 + re) + poly re) + f,  AS_ERR = 1.5e-7 (Abramowitz & Stegun 7.1.26, published);
   Phi = fma(0.5, +-erf_abs, 0.5): 0.5 d_erf + f Phi;  a phi = fl(fl(a k) e~): |a phi| (3 f + re) (1 + f);  the sum: f |d|:
       d_eval = 0.5 d_erf + f Phi + |a phi| ((1 + 3 f)(1 + re) - 1) + f |d| + (|a| + 1) T
   out = fl(v d~):  E = |d| E_pre + (|pre| + E_pre) d_eval + f (|pre d| + ...) + T.
 slab path (EPI_SLAB_F32 + owl_slab_reduce, gemm.hip: slab_reduce_kernel): slab s is bounded with n_acc of its own K range; the reduce adds nsplit
   (+ 1 with accumulate) values in f32: gamma(nsplit + 1) (sum_s (|slab_s| + tol_s) + |out_old|) on top of sum_s tol_s.

`check(name, got, ref, tol)` tests every element (no exclusions), `untouched` every element outside [0, M) x [0, N) bit for bit.
`emulate` is an f32 simulation of the kernels' arithmetic (K-tiles of 64, the epilogue formulas in the order the source writes them, RNE bf16
store) for the CPU test of the bounds; it is NOT a reference for the GPU test.
"""
import math

import torch

U = 2.0 ** -8            # bf16 unit round-off
F = 2.0 ** -24           # f32 unit round-off
TINY = 2.0 ** -126       # smallest normal f32 / bf16
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
BK = 64                  # K-tile
MFMA_K = 16              # products per MFMA instruction
A_Q = 1.702
C_Q = 2.4554669595930156          # 1.702 log2 e                     gemm_common.h:47
C_D = 0.72134752044448170         # log2 e / 2                       common.h:73
RSQRT2 = 0.70710678118654752
RSQRT2PI = 0.39894228040143268
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
AS_ERR = 1.5e-7          # |erf - (1 - poly exp(-x^2))| of Abramowitz & Stegun 7.1.26
ERFF_ULPS = 4.0          # ASSUMPTION 2
QG_SUP2 = 0.86           # >= sup |quick_gelu''|  (0.851 at 0)
QG_SUP3 = 1.1            # >= sup |quick_gelu'''| (0.893)
GELU_SUP2 = 0.80         # >= sup |gelu''|        (0.798 at 0)

EPI_BIAS, EPI_QGELU, EPI_GELU, EPI_RESID, EPI_F32 = 0, 1, 2, 3, 4
EPI_DQGELU, EPI_DGELU, EPI_ACC, EPI_SLAB = 8, 9, 10, 11
EPI_NAMES = {0: "BIAS", 1: "QGELU", 2: "GELU", 3: "RESID", 4: "F32", 8: "DQGELU", 9: "DGELU", 10: "ACC", 11: "SLAB"}
BF16_OUT = (EPI_BIAS, EPI_QGELU, EPI_GELU, EPI_DQGELU, EPI_DGELU)


def gamma(n):
    return n * F / (1.0 - n * F)


def gamma2(n):
    """n chained f32 adds whose rounding mode is unknown (2 f each)."""
    return 2.0 * n * F / (1.0 - 2.0 * n * F)


def n_acc(K):
    return K // MFMA_K + MFMA_K


def acc_bound(K, acc_abs, any_order=False):
    return (gamma2(K + 1) if any_order else gamma2(n_acc(K))) * acc_abs


def bf16_round(x):
    """Round to bf16 (nearest even) and return in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def split_ranges(K, splits):
    """K ranges of the slabs owl_gemm_nt_bf16 writes for (K, splits) (gemm.hip, owl_gemm_effective_splits)."""
    nk = K // BK
    splits = max(1, min(splits, nk))
    per = (nk + splits - 1) // splits
    ns = (nk + per - 1) // per
    return [(s * per * BK, min(nk, (s + 1) * per) * BK) for s in range(ns)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 functions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _sig(x):
    return torch.sigmoid(A_Q * x)


def qgelu(x):
    return x * _sig(x)


def qgelu_d1(x):
    s = _sig(x)
    return s * (1.0 + A_Q * x * (1.0 - s))


def qgelu_d2(x):
    s = _sig(x)
    return A_Q * s * (1.0 - s) * (2.0 + A_Q * x * (1.0 - 2.0 * s))


def qgelu_d3(x):
    s = _sig(x)
    p = s * (1.0 - s)
    return A_Q * A_Q * p * (3.0 * (1.0 - 2.0 * s) + A_Q * x * (1.0 - 6.0 * p))


def _Phi(x):
    return 0.5 * torch.erfc(-x * RSQRT2)           # no cancellation in the negative tail


def _phi(x):
    return RSQRT2PI * torch.exp(-0.5 * x * x)


def gelu(x):
    return x * _Phi(x)


def gelu_d1(x):
    return _Phi(x) + x * _phi(x)


def gelu_d2(x):
    return _phi(x) * (2.0 - x * x)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def exact(epi, A, W, bias=None, alpha=1.0, resid=None, aux_in=None, splits=1, accumulate=0):
    """float64 reference of one epilogue (module docstring).  Returns a dict: out, aux (QGELU / GELU), acc, acc_abs, pre and, for SLAB, `ranges`,
    out [ns, M, N], slab_abs [ns, M, N] and reduced."""
    A, W = A.double(), W.double()
    r = {"epi": epi, "alpha": float(alpha), "K": A.shape[1], "has_bias": bias is not None}
    if epi == EPI_SLAB:
        r["ranges"] = rg = split_ranges(A.shape[1], splits)
        r["out"] = torch.stack([alpha * (A[:, a:b] @ W[:, a:b].t()) for a, b in rg])
        r["slab_abs"] = torch.stack([A[:, a:b].abs() @ W[:, a:b].abs().t() for a, b in rg])
        r["reduced"] = r["out"].sum(0) + (resid.double() if accumulate else 0.0)
        r["resid"] = resid.double() if accumulate else None
        return r
    acc = A @ W.t()
    r["acc"], r["acc_abs"] = acc, A.abs() @ W.abs().t()
    pre = alpha * acc
    if bias is not None:
        pre = pre + bias.double()
    r["pre"] = pre
    if epi in (EPI_BIAS, EPI_F32):
        r["out"] = pre
    elif epi == EPI_QGELU:
        r["out"], r["aux"] = qgelu(pre), qgelu_d1(pre)
    elif epi == EPI_GELU:
        r["out"], r["aux"] = gelu(pre), pre
    elif epi in (EPI_RESID, EPI_ACC):
        r["resid"] = resid.double()
        r["out"] = r["resid"] + pre
    elif epi == EPI_DQGELU:
        r["a"] = aux_in.double()
        r["out"] = pre * r["a"]
    elif epi == EPI_DGELU:
        r["a"] = aux_in.double()
        r["out"] = pre * gelu_d1(r["a"])
    else:
        raise ValueError(epi)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _pre_bound(r, any_order=False):
    al = abs(r["alpha"])
    E_acc = acc_bound(r["K"], r["acc_abs"], any_order)
    E = al * E_acc + F * al * (r["acc"].abs() + E_acc)
    if r["has_bias"]:
        E = E + F * (r["pre"].abs() + E)
    return E + TINY


def _store_bf16(ref, E):
    return E + U * (ref.abs() + E) + TINY


def _rel_exp(dt):
    """relative error of v_exp_f32 on an argument that is off by dt (log2 units)."""
    return torch.expm1(LN2 * dt + math.log1p(2.0 * F))


def _qgelu_eval(x):
    """evaluation errors (out, saved derivative) of the f32 quick-GELU formulas at the f32 point x."""
    s = _sig(x)
    re = _rel_exp(2.0 * F * C_Q * x.abs())
    rs = (1.0 + 2.0 * F) / ((1.0 - (1.0 - s) * re) * (1.0 - F)) - 1.0
    ro = (1.0 + rs) * (1.0 + F) - 1.0
    e_out = (x * s).abs() * ro + (x.abs() + 1.0) * TINY
    h = 1.0 + A_Q * x * (1.0 - s)
    d_om = s * rs + F * (1.0 - s)
    dh = A_Q * x.abs() * (2.0 * F * (1.0 - s) + (1.0 + 2.0 * F) * d_om) + F * h.abs()
    e_aux = (s * h).abs() * ro + s * (1.0 + ro) * dh + (h.abs() + 1.0) * TINY
    return e_out, e_aux, ro


def _gelu_eval(x):
    z = x * RSQRT2
    erf = torch.erf(z)
    d_arg = (2.0 / math.sqrt(math.pi)) * torch.exp(-z * z) * z.abs() * 2.0 * F
    w = 2.0 * _Phi(x)
    return 0.5 * x.abs() * (d_arg + ERFF_ULPS * 2.0 * F * erf.abs() + F * w) * (1.0 + F) + F * gelu(x).abs() + TINY


def dgelu_eval(a):
    """evaluation error of dgelu_erf_f (common.h:70-77) at the exact point a, the published error of the polynomial included."""
    x = a.abs() * RSQRT2
    t = 1.0 / (1.0 + AS_P * x)
    rt = (1.0 + 2.0 * F) / (1.0 - 4.0 * F) - 1.0
    e = torch.exp(-0.5 * a * a)
    re = _rel_exp(2.0 * F * C_D * a * a)
    S0 = sum(abs(c) * t ** (i + 1) for i, c in enumerate(AS_A))
    S1 = sum((i + 1) * abs(c) * t ** (i + 1) for i, c in enumerate(AS_A))
    poly = sum(c * t ** (i + 1) for i, c in enumerate(AS_A))
    d_poly = 7.0 * F * S0 + rt * S1
    d_erf = AS_ERR + e * (d_poly * (1.0 + re) + poly.abs() * re) + F
    Phi, aphi = _Phi(a), (a * _phi(a)).abs()
    return 0.5 * d_erf + F * Phi + aphi * ((1.0 + 3.0 * F) * (1.0 + re) - 1.0) * (1.0 + F) + F * gelu_d1(a).abs() + (a.abs() + 1.0) * TINY


def bounds(r, any_order=False):
    """Elementwise tolerances for a result of exact(): {"out": tol, "aux": tol (QGELU / GELU)}; SLAB: {"out": [ns, M, N], "reduced": [M, N]}."""
    epi = r["epi"]
    if epi == EPI_SLAB:
        al = abs(r["alpha"])
        tols = []
        for (a, b), sa, so in zip(r["ranges"], r["slab_abs"], r["out"]):
            E = acc_bound(b - a, sa, any_order)
            tols.append(al * E + F * al * (so.abs() / max(al, TINY) + E) + TINY)
        tol = torch.stack(tols)
        ns = len(tols)
        mag = (r["out"].abs() + tol).sum(0) + (r["resid"].abs() if r["resid"] is not None else 0.0)
        return {"out": tol, "reduced": tol.sum(0) + gamma(ns + 1) * mag + TINY}
    E = _pre_bound(r, any_order)
    pre, out = r["pre"], r["out"]
    if epi == EPI_BIAS:
        return {"out": _store_bf16(out, E)}
    if epi == EPI_F32:
        return {"out": E}
    if epi in (EPI_RESID, EPI_ACC):
        return {"out": E + F * (out.abs() + E) + TINY}
    if epi == EPI_QGELU:
        e_out, e_aux, ro = _qgelu_eval(pre)           # at pre; the f32 point x lies within E of it: third-order terms E (ro + 16 f)
        Eo = qgelu_d1(pre).abs() * E + 0.5 * QG_SUP2 * E * E + e_out + 1.2 * E * (ro + 16.0 * F)
        Ea = qgelu_d2(pre).abs() * E + 0.5 * QG_SUP3 * E * E + e_aux + 1.2 * E * (ro + 16.0 * F)
        return {"out": _store_bf16(out, Eo), "aux": _store_bf16(r["aux"], Ea)}
    if epi == EPI_GELU:
        Eo = gelu_d1(pre).abs() * E + 0.5 * GELU_SUP2 * E * E + _gelu_eval(pre) + 1.2 * E * 16.0 * F
        return {"out": _store_bf16(out, Eo), "aux": _store_bf16(pre, E)}
    if epi == EPI_DQGELU:
        a = r["a"].abs()
        Eo = a * E + F * (out.abs() + a * E) + (a + pre.abs() + 1.0) * TINY
        return {"out": _store_bf16(out, Eo)}
    if epi == EPI_DGELU:
        d = gelu_d1(r["a"]).abs()
        de = dgelu_eval(r["a"])
        Eo = d * E + (pre.abs() + E) * de
        Eo = Eo + F * (out.abs() + Eo) + (d + pre.abs() + 1.0) * TINY
        return {"out": _store_bf16(out, Eo)}
    raise ValueError(epi)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref, tol):
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)


def check(name, got, ref, tol, fails=None):
    """Every element of `got` within `tol` of `ref` (NaN counts as outside).  Returns the worst err / tol; on failure raises -- or, given a list
    `fails`, appends the message -- with the count, the worst ratio and the first indices."""
    r = ratios(got, ref, tol)
    worst = float(r.max())
    bad = r > 1.0
    nb = int(bad.sum())
    if nb:
        first = []
        for idx in bad.nonzero()[:6].tolist():
            i = tuple(idx)
            first.append(f"{list(i)}: got {float(got[i]):.9g} ref {float(ref[i]):.9g} tol {float(tol[i]):.3g}")
        msg = f"{name}: {nb}/{bad.numel()} outside the bound, worst err / tol {worst:.3f}; " + "; ".join(first)
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return worst


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def untouched(name, buf, before, M, col0, N, fails=None):
    """`buf` [rows, ld] after a call that may write rows [0, M) x columns [col0, col0 + N) only, `before` its copy from before the call: every
    other element must hold its exact bits (NaN sentinels included)."""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:M, col0:col0 + N] = False
    bad = (bits(buf) != bits(before)) & keep
    nb = int(bad.sum())
    if nb:
        msg = f"{name}: {nb} elements outside [0, {M}) x [{col0}, {col0 + N}) changed; first at {bad.nonzero()[:6].tolist()}"
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return nb


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input profiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILES = ("randn", "tails", "tails_wide", "cancel", "resid_large")
TAIL = 14.0
TAIL_WIDE = 60.0         # reaches the overflow of v_exp in the quick-GELU sigmoid (pre-activation < -52.1), which +-14 cannot


def make_inputs(profile, M, N, K, seed, epi):
    """Seeded, bf16- / f32-exact inputs on the CPU: dict A [M, K], W [N, K] (float32 holding bf16 values), bias [N] f32, resid [M, N] f32 (RESID /
    ACC / slab accumulate), aux_in [M, N] (float32 holding bf16 values; derivative epilogues)."""
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + M * 10007 + N * 101 + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g) * 0.5
    resid = torch.randn(M, N, generator=g)
    aux_in = torch.randn(M, N, generator=g)
    if epi == EPI_DQGELU:
        aux_in = qgelu_d1(aux_in.double() * 2.0).float()          # a saved quick-GELU derivative
    if profile in ("tails", "tails_wide"):
        lim = TAIL if profile == "tails" else TAIL_WIDE
        sweep = torch.linspace(-lim, lim, N)
        bias = sweep.clone()
        if epi == EPI_DGELU:
            aux_in = aux_in * 0.05 + sweep
        elif epi == EPI_DQGELU:
            aux_in = qgelu_d1((aux_in.double() * 0.05 + sweep.double())).float()
    elif profile == "cancel":
        # rows of A from +- pairs against pairwise (nearly) equal columns of W: |acc| << acc_abs
        half = A[:, :K // 2]
        A = torch.cat([half, -half], 1)
        W[:, K // 2:] = W[:, :K // 2] * (1.0 + 2.0 ** -6 * torch.randn(N, K // 2, generator=g))
        bias = bias * 2.0 ** -6
    elif profile == "resid_large":
        resid = resid * 1e3
    elif profile != "randn":
        raise ValueError(profile)
    return {"A": bf16_round(A), "W": bf16_round(W), "bias": bias, "resid": resid, "aux_in": bf16_round(aux_in)}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation of the kernels' arithmetic (CPU test: are the bounds wide enough for a correct kernel and tight enough for a wrong one?)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.double() * b.double() + (c.double() if torch.is_tensor(c) else c)).float()


def emulate_acc(A, W, k0=0, k1=None, hooks=None):
    """A W^T over [k0, k1) accumulated K-tile by K-tile in float32.  hooks["partial"](acc, kt) -> acc after every K-tile; hooks["acc"](acc)."""
    A, W = A.float(), W.float()
    k1 = A.shape[1] if k1 is None else k1
    hooks = hooks or {}
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float32)
    for k in range(k0, k1, BK):
        acc = acc + A[:, k:k + BK] @ W[:, k:k + BK].t()
        if "partial" in hooks:
            acc = hooks["partial"](acc, k // BK)
    if "acc" in hooks:
        acc = hooks["acc"](acc)
    return acc


def sigmoid1702_f32(x):
    return 1.0 / (1.0 + torch.exp2(torch.tensor(-C_Q, dtype=torch.float32) * x))


def dqgelu_from_s_f32(x, s):
    return s * _fma32(torch.tensor(A_Q, dtype=torch.float32) * x, 1.0 - s, 1.0)


def dgelu_erf_f32(a, with_phi_term=True):
    """dgelu_erf_f (common.h:70-77) operation by operation in float32."""
    c = lambda v: torch.tensor(v, dtype=torch.float32)
    x = a.abs() * c(RSQRT2)
    t = 1.0 / _fma32(c(AS_P), x, 1.0)
    e = torch.exp2(a * a * c(-C_D))
    p = _fma32(t, c(AS_A[4]), c(AS_A[3]))
    p = _fma32(t, p, c(AS_A[2]))
    p = _fma32(t, p, c(AS_A[1]))
    p = _fma32(t, p, c(AS_A[0]))
    poly = t * p
    erf_abs = _fma32(-poly, e, 1.0)
    Phi = _fma32(c(0.5), torch.copysign(erf_abs, a), 0.5)
    return Phi + a * c(RSQRT2PI) * e if with_phi_term else Phi


def emulate(epi, A, W, bias=None, alpha=1.0, resid=None, aux_in=None, splits=1, accumulate=0, hooks=None):
    """f32 simulation of one GEMM call (module docstring).  Returns a dict: out (bf16 values in float32, or float32), aux, pre (the f32
    pre-activation) and, for SLAB, out [ns, M, N] and reduced.  `hooks` lets a test plant an error at a stage: "partial" / "acc"
    (emulate_acc), "pre"(v) -> v, "reduce"(slabs) -> slabs."""
    hooks = hooks or {}
    al = torch.tensor(alpha, dtype=torch.float32)
    if epi == EPI_SLAB:
        slabs = torch.stack([emulate_acc(A, W, a, b, hooks) * al for a, b in split_ranges(A.shape[1], splits)])
        use = hooks["reduce"](slabs) if "reduce" in hooks else slabs
        red = resid.float().clone() if accumulate else torch.zeros_like(slabs[0])
        for s in use:
            red = red + s
        return {"out": slabs, "reduced": red}
    v = emulate_acc(A, W, hooks=hooks) * al
    if bias is not None:
        v = v + bias.float()
    if "pre" in hooks:
        v = hooks["pre"](v)
    r = {"pre": v}
    if epi == EPI_BIAS:
        r["out"] = bf16_round(v)
    elif epi == EPI_F32:
        r["out"] = v
    elif epi in (EPI_RESID, EPI_ACC):
        r["out"] = resid.float() + v
    elif epi == EPI_QGELU:
        s = sigmoid1702_f32(v)
        r["out"], r["aux"] = bf16_round(v * s), bf16_round(dqgelu_from_s_f32(v, s))
    elif epi == EPI_GELU:
        g = torch.tensor(0.5, dtype=torch.float32) * v * (1.0 + torch.erf(v * torch.tensor(RSQRT2, dtype=torch.float32)))
        r["out"], r["aux"] = bf16_round(g), bf16_round(v)
    elif epi == EPI_DQGELU:
        r["out"] = bf16_round(v * aux_in.float())
    elif epi == EPI_DGELU:
        r["out"] = bf16_round(v * dgelu_erf_f32(aux_in.float()))
    else:
        raise ValueError(epi)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the planner's conditions (gemm_plan.h, gemm_plan: what owl_gemm_nt_bf16 launches), restated, and the case set shared by the CPU and the GPU test
# ---------------------------------------------------------------------------------------------------------------------------------------------
NUM_CUS = 256
PP2_EPIS = (EPI_BIAS, EPI_QGELU, EPI_DQGELU, EPI_GELU, EPI_DGELU, EPI_F32, EPI_ACC)      # gemm_plan.h, pp2_takes (less the patch gathers)
PPH_EPIS = (EPI_BIAS, EPI_QGELU, EPI_DQGELU, EPI_GELU, EPI_DGELU)                        # gemm_plan.h, pph_takes


def gemm_split(M, N, tile):
    """M_main of the automatic kernel choice (whole rounds of 256 x 256 tiles + one round of half-height remainder tiles), or None: the
    arithmetic of gemm_plan.h, gemm_whole_round_rows, restated."""
    if tile != 0 or N > 1024:
        return None
    tm, tn = (M + 255) // 256, (N + 255) // 256
    items = tm * tn
    full_rounds = items // NUM_CUS
    tm_main = (full_rounds * NUM_CUS) // tn
    rem_tiles = (tm - tm_main) * tn
    if full_rounds >= 1 and tm_main >= 1 and rem_tiles > 0 and 2 * rem_tiles <= NUM_CUS and items - full_rounds * NUM_CUS > 0:
        return tm_main * 256
    return None


def dispatch_path(epi, M, N, K, tile, a_rows=None):
    """[(kernel, rows)] the shipped library launches: 'pp2' two-phase 256 x 256 (gemm_pp2.hip), 'pph' half-height 128 x 256 (gemm_pph.hip), 'sp256' /
    'sp128' the single-phase kernels of gemm.hip.  The independent restatement of gemm_plan.h's gemm_plan: tests/test_gemm_plan.py holds the
    library's own answer (library_path) to it."""
    a_rows = M if a_rows is None else a_rows
    want_half = tile == 6
    ft = 0 if want_half else tile
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    auto_big = M >= 512 and N >= 256 and t256 >= 48
    if ft == 7 and K >= 128 and epi in PP2_EPIS:
        return [("pp2", M)]
    if ft == 0 and auto_big and K >= 128:
        if want_half and a_rows >= M and 2 * t256 <= NUM_CUS and epi in PPH_EPIS:
            return [("pph", M)]
        M_main = gemm_split(M, N, 0) if (epi not in (EPI_F32, EPI_ACC) and a_rows >= M) else None
        if M_main is not None and epi in PP2_EPIS:
            return [("pp2", M_main), ("pph" if epi in PPH_EPIS else "pp2", M - M_main)]
        if epi in PP2_EPIS:
            return [("pp2", M)]
    big = (ft == 256) if ft else auto_big
    return [("sp256" if big else "sp128", M)]


_PLAN = {}


def library_path(epi, M, N, K, tile, a_rows=None, has_aux=1, Tp=0, splits=1):
    """[(kernel, rows)] in dispatch_path's names, ASKED of the library: owl_gemm_nt_plan runs the argument checks and the planner of the launch itself
    (host only, no device).  Raises OwlLibError with the library's message for arguments the launch refuses."""
    from owl_vit_object_detection_amd import _lib
    if not _PLAN:
        import ctypes
        _PLAN.update(fn=_lib.load().owl_gemm_nt_plan, kernels=(ctypes.c_int * 2)(), rows=(ctypes.c_int64 * 2)(),
                     names={v: k.lower() for h in (_lib.HEADER, _lib.TUNING_HEADER) for k, v in _lib.header_constants("OWL_GEMM_KERNEL_", h).items()})
    n = _PLAN["fn"](epi, M, N, K, M if a_rows is None else a_rows, has_aux, Tp, splits, tile, _PLAN["kernels"], _PLAN["rows"])
    if n < 0:
        raise _lib.OwlLibError(f"owl_gemm_nt_plan failed (rc={n}): {_lib.last_error()}")
    return [(_PLAN["names"][_PLAN["kernels"][i]], _PLAN["rows"][i]) for i in range(n)]


def sample_rows(M, M_main):
    """Rows to check of a tall problem: the first tile, one row of every 128-row band (offset varying), both sides of M_main, the last rows."""
    rows = {0, 1, 127, 128, 255, M - 1, M - 2, M - 129}
    rows.update(b * 128 + (b * 37) % 128 for b in range((M + 127) // 128))
    if M_main is not None:
        rows.update({M_main - 256, M_main - 1, M_main, M_main + 1, M_main + 127, M_main + 128})
    return sorted(r for r in rows if 0 <= r < M)


SHAPES = [(1, 8, 64), (127, 136, 128), (129, 264, 192), (300, 256, 192), (513, 520, 256), (130, 264, 4096), (2900, 1000, 128)]
TOWER_SHAPES = [(35, 192, 64), (35, 128, 128)]      # the text tower's row count at N = 5, S = 7 (tests/test_text_reference_gpu.py) with K = width of tiny / small
TALL = (76700, 256, 128)       # N = 248 of the first draft fails the dispatcher's N >= 256: the nearest shape with 300 x 1 tiles of 256
LAYOUT_SHAPES = [(129, 264, 192), (513, 520, 256)]
TILES = (128, 256, 7, 0, 6)
SAME_BITS_TILES = (256, 7, 0, 6)

# a FORM is one way of calling an epilogue: (name, epi, alpha, with bias, in place, splits)
FORMS = [
    ("bias", EPI_BIAS, 1.0, True, False, 1),
    ("qgelu", EPI_QGELU, 1.0, True, False, 1),
    ("gelu", EPI_GELU, 1.0, True, False, 1),
    ("resid_inplace", EPI_RESID, 1.0, True, True, 1),
    ("resid", EPI_RESID, 1.0, True, False, 1),
    ("f32_a1_b", EPI_F32, 1.0, True, False, 1), ("f32_a1", EPI_F32, 1.0, False, False, 1),
    ("f32_a0.5_b", EPI_F32, 0.5, True, False, 1), ("f32_a0.5", EPI_F32, 0.5, False, False, 1),
    ("f32_a-2_b", EPI_F32, -2.0, True, False, 1), ("f32_a-2", EPI_F32, -2.0, False, False, 1),
    ("acc", EPI_ACC, 1.0, False, True, 1),
    ("slab1", EPI_SLAB, 1.0, False, False, 1), ("slab2", EPI_SLAB, 1.0, False, False, 2),
    ("slab3", EPI_SLAB, 1.0, False, False, 3), ("slab5", EPI_SLAB, 1.0, False, False, 5),
    ("dqgelu", EPI_DQGELU, 1.0, False, False, 1),
    ("dgelu", EPI_DGELU, 1.0, False, False, 1),
]
FORM = {f[0]: f for f in FORMS}


def profiles_of(epi):
    return PROFILES if epi in (EPI_RESID, EPI_ACC, EPI_SLAB) else PROFILES[:4]


def cases():
    """[(M, N, K, form name, profile)]: every form meets every shape; the profiles rotate over the shapes, and the shapes below 200 000 outputs
    take a second profile, so that every epilogue meets each of its profiles at least twice."""
    out = []
    for fi, (name, epi, *_rest) in enumerate(FORMS):
        pl = profiles_of(epi)
        for si, (M, N, K) in enumerate(SHAPES + TOWER_SHAPES):
            out.append((M, N, K, name, pl[(si + fi) % len(pl)]))
            if M * N < 200000:
                out.append((M, N, K, name, pl[(si + fi + 2) % len(pl)]))
    return out
