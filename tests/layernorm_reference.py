"""Float64 references, derived error bounds, input profiles and an f32 simulation for the LayerNorm family: csrc/norm.hip (ln_fwd_kernel and its
fused x + delta (+ delta2) forms, cls_ln_kernel, merge_ln_kernel, cls_rows_kernel) and csrc/backward.hip (ln_bwd_body in every instantiation,
ln_bwd_kernel_768, merge_ln_bwd_kernel, cls_ln_bwd_kernel, partials_reduce_kernel).  Checker side; device-agnostic: every function works on whatever device its inputs live on, and
nothing here imports the package's Python ops.

Reference (float64 on the kernel's exact inputs: f32 values, bf16 values upcast, eps as the f32 the launcher receives)
---------
`exact_fwd(x, gamma, beta, eps, delta, delta2)`   s = fl(fl(x + delta) + delta2) formed with torch f32 adds (NOT taken from the code under test: x_out
    is asserted bit for bit against it); mean = sum(s) / D, rstd = (sum((s - mean)^2) / D + eps)^-1/2, y = (s - mean) rstd gamma + beta.
`exact_merge(x [B, T, D], g1, b1, g2, b2, eps, delta)`   y1 = LN1(s) on every token, cls_ln = y1[:, 0], z = y1[:, 1:] * y1[:, :1],
    feats = LN2(z); stats1 over every token, stats2 over the patch tokens.
`exact_merge_bwd(dfeats, x, g1, b1, g2, eps, given)`   dx (all tokens), dcls, dg1, db1, dg2, db2, colsum(dx): see "merge backward" below.
`exact_bwd(dy, x, mean, rstd, gamma, dres)`   the closed form of backward.hip:61-62 at the statistics the kernel is GIVEN (f32, upcast):
    xhat = (x - mean) rstd, gd = gamma dy, s1 = mean(gd), s2 = mean(gd xhat), dx = rstd (gd - s1 - xhat s2) (+ dres), dgamma = sum_rows dy xhat,
    dbeta = sum_rows dy, colsum = sum_rows dx.  test_layernorm_reference.py shows that it equals float64 autograd of F.layer_norm at exact statistics.

Bounds (elementwise, derived, no fitted constant)
-------------------------------------------------
u, f, T and gamma(n) = n f / (1 - n f) are those of gemm_reference.py:18-20 and are imported from it.  Every product below is bounded by
    mul(a, Ea, b, Eb) = |a| Eb + |b| Ea + Ea Eb       (both factors in error),      and one rounding of a result r with error E costs f (|r| + E).

 sum chain.  Lane l holds vectors l, l + 64, ... (norm.hip:12-13): per vector ((x + y) + z) + w and one add onto the lane's sum, 4 adds per
   vector, nv = ceil(D / 256) vectors; wave_sum is six xor-shuffle levels (common.h:142-146):
       n_s = 4 ceil(D / 256) + 6          add statements of the chain (`n_sum(D)`; the simulation counts the same number).  An UPPER bound of the
                                          longest path of one element, which is 3 + ceil(D / 256) + 6: gamma(n_s) holds a fortiori
   -- not D - 1: at D = 1024 that is 22, not 1023.
 row_stats (norm.hip:9-23) on elements v known to E_in (0 for the first LayerNorm):
   mean~ = fl(S~ / D), D exact, one rounding:       E_mean = (sum E_in + gamma(n_s + 1) sum(|v| + E_in)) / D
   d~ = fl(v~ - mean~):                               E_d = E_in + E_mean + f (1 + f) (|d| + E_in + E_mean)
   second moment: d~_i = (d_i + e_i - dm) (1 + eps_i) with e_i the input's error (|e_i| <= E_in), dm the error of the mean, COMMON to the row,
   and |eps_i| <= f.  sum_i d_i = 0 for the exact mean, so the term 2 dm sum d_i that a bound by |d| E_d would charge vanishes identically:
       sum (d_i + e_i - dm)^2 - sum d_i^2 = 2 sum d_i e_i + sum (e_i - dm)^2       <= sum (2 |d| E_in + E_c^2),   E_c = E_in + E_mean
   (this is why the two-pass variance is good at a large mean, and what E[x^2] - mean^2 does not have); the rounding of d~ adds
   ((1 + f)^2 - 1) (|d| + E_c)^2 per square; the squares carry one more rounding (or none, fused), the chain is the same, the division one more:
       E_var = (sum (2 |d| E_in + E_c^2 + r2 q) + gamma(n_s + 2) sum (1 + r2) q) / D,     q = (|d| + E_c)^2,  r2 = (1 + f)^2 - 1
       ve~ = fl(var~ + eps):    E_ve = E_var + f (var + eps + E_var),     rho = E_ve / (var + eps)  (< 1: var + eps >= eps)
   rstd through x^-1/2: |ve~^-1/2 / ve^-1/2 - 1| <= (1 - rho)^-1/2 - 1, which is the first-order term rho / 2 WITH its remainder.
   ASSUMPTION 1: rsqrtf of this toolchain is within 2 ulp = 4 f of the exact reciprocal square root.  The ROCm tree this was written against
   carries no HIP math accuracy document (searched for one that names rsqrtf; none), so the 2 ulp budget the issue sets for that event is used:
       r_rstd = (1 + 4 f) (1 - rho)^-1/2 - 1,     E_rstd = rstd r_rstd.
 output.  (v - mean~) rstd~ g + b is written without contract(off) (norm.hip:64-65): the compiler may fuse the last multiply-add.  One rounding per
   written operation bounds both:   t = d~ rstd~: E_t = mul(d, E_d, rstd, E_rstd) + f(.);  w = t g: E_w = |g| E_t + f(.);  y = w + b: E_y = E_w + f(.).
   store (pack_bf2, RNE): bf16 tol = E + u (|ref| + E) + T;  f32 tol = E + T.
 merge (norm.hip:123-175).  cls_ln is the f32 store of LN1 on token 0, so the patch rows read c~ within E_c of c;  z~ = fl(y1~ c~):
   E_z = mul(y1, E_y1, c, E_c) + f(.), then row_stats and the affine map once more with E_in = E_z.
 backward (ln_bwd_body, backward.hip:108-127: contraction off, explicit fmaf, so the rounding count is exact; mean and rstd are exact inputs):
   xh~ = fl(fl(x - m) r):      E_xh = ((1 + f)^2 - 1) |xh|                    gd~ = fl(dy g):  E_gd = f |gd|
   s1~ = fl(S1~ / D), 4 adds per vector + 6 levels + the division:   E_s1 = (sum E_gd + gamma(n_s + 1) sum (|gd| + E_gd)) / D
   s2: gd.x xh.x rounded, three fmaf, one add per vector, 6 levels, the division; p = gd xh, E_p = mul(gd, E_gd, xh, E_xh):
                                                                     E_s2 = (sum E_p + gamma(n_s + 2) sum (|p| + E_p)) / D
   dx = r fmaf(-xh~, s2~, fl(gd~ - s1~)):   t = gd - s1: E_t = E_gd + E_s1 + f(.);   v = t - xh s2: E_v = E_t + mul(xh, E_xh, s2, E_s2) + f(.);
       o = r v: E_o = r E_v + f(.);   with dres one more add: E = E_o + f(.).    bf16 copy: E + u (|ref| + E) + T (and == bf16(own f32 dx), bit test).
 row reductions (dgamma, dbeta, colsum(dx)): a wave adds rows w, w + 4, ... of its 64-row block in order (16 adds, dgamma by fmaf: the product is
   not rounded), the four waves' sums are added in order (3), partials_reduce_kernel adds slabs j, j + 16, ... in order (ceil(nblk / 16)), then the 16
   lane sums in order (15), then the old value of the accumulator (1):
       n_r = 16 + 3 + ceil(nblk / 16) + 15 + 1     (`n_rows(rows)`; counted by the simulation)
       tol = gamma(n_r) (sum_rows (|term| + E_term) + |old|) + sum_rows E_term + T,      E_term = |dy| E_xh (dgamma), 0 (dbeta), E_dx (colsum).
 merge backward (merge_ln_bwd_kernel, cls_ln_bwd_kernel; backward.hip:229-366).  `exact_merge_bwd` is the closed form of the chain LN2 backward ->
   d(cls_ln) = sum_p dz y1, dy1 = dz cls_ln -> LN1 backward, in float64 at the statistics and the class row the kernels are GIVEN; the CPU test shows
   it equal to float64 autograd of the merge expression at the exact ones.  Both kernels leave contraction to the compiler, so every WRITTEN operation
   is charged one rounding (`_V`): a fused multiply-add only removes one.  Row moments of merge_ln_bwd_kernel: a thread adds its 4 columns (3), six
   levels, the 4 waves in order (3), and the multiply by invD = fl(1 / D) (2 roundings): N_MOMENT = 14, the products of the second moment rounded
   before.  cls_ln_bwd_kernel's moments run the lane chain: n_s + 1.  Row reductions: a thread adds the rows of its 64-row block in order (64: MLR = 2
   rows per step, 32 steps, one add per row -- twice the 32 steps, which is what counts), partials_reduce_kernel adds B nbx slabs (nbx per image and no
   accumulate for dcls): `n_rows_merge`; the class rows add B terms through a second reduce with accumulate: `n_rows_cls`.  The class rows read the
   kernel's own dcls, known to E_dcls, which is carried through cls_ln_bwd_kernel's arithmetic.
       tol = gamma(n) (sum_rows (|term| + E_term) + |old|) + sum_rows E_term + T,     n = n_rows_merge (+ n_rows_cls for dg1, db1, colsum)

Profiles (`make_inputs`) -- what each is meant to reach; test_layernorm_reference.py asserts that it reaches it
--------
 randn    2 randn + 0.3, gamma = 1 + 0.1 randn: the case every earlier test runs; the baseline.
 outlier  unit rows with 2-4 channels at +-(64 ... 256), one in vector 0 of lane 0 (column 0), one in the row's last vector (column D - 1): a trained
          ViT stream.  The normalised values are small (median |y| < 0.2 for D >= 252) so a tolerance relative to max |y| would hide them.
 offset   row mean +-2^10 ... 2^12, unit spread: E[x^2] - mean^2 in f32 loses every digit of the variance here.
 flat     spread 1e-4 about a constant of order 1 (var << eps, rstd within 1 % of eps^-1/2 = 316), every third row exactly zero (out = store(beta)).
 scaled   rows times 2^-40 (even) / 2^40 (odd).  The range stops there because D (2^40 2^8)^2 = 2^106 (an outlier-sized element squared, summed) is
          still below f32's 2^128 while 2^60 is not, and the squares of elements down to 2^-23 of a 2^-40 row stay above T = 2^-126.
 affine "hard": gamma with exact zeros, negative entries and magnitudes up to 8; beta = -xhat[0] gamma on every fourth column, so y[0] cancels to ~0.
 dy       white 0.1 randn;  aligned: gamma dy = a + b xhat + 1e-3 noise (dx is a cancellation);  sparse: one nonzero per row.  bf16 or f32.

`check` / `untouched` / `bits` are gemm_reference's.  `emulate_*` simulate the kernels' arithmetic in f32 in the order the source writes it
(lane-strided partial sums, six butterfly levels, two-pass statistics, RNE bf16 store, block / wave / strided reduce order) and take `hooks` that
plant errors; they serve the CPU test only and are NEVER a reference on the GPU.
"""
import math

import torch

from tests.gemm_reference import F, TINY, U, bf16_round, bits, check, gamma as gam, ratios, untouched  # noqa: F401

EPS = 1e-5
RSQRT_ULPS = 2.0         # ASSUMPTION 1
ROWS_PER_BLOCK = 64      # backward.hip:199
WAVES = 4
REDUCE_LANES = 16        # partials_reduce_kernel: slab lanes j = 0..15


def eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32))


def nv_of(D):
    return (D // 4 + 63) // 64


def n_sum(D):
    return 4 * nv_of(D) + 6


def n_rows(rows, accumulate=1):
    nblk = (rows + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    return ROWS_PER_BLOCK // WAVES + (WAVES - 1) + (nblk + REDUCE_LANES - 1) // REDUCE_LANES + (REDUCE_LANES - 1) + accumulate


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def f32_sum(x, delta=None, delta2=None):
    s = x.float()
    if delta is not None:
        s = s + delta.float()
        if delta2 is not None:
            s = s + delta2.float()
    return s


def _ln64(v, g, b, eps):
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return mean, var, rstd, d, d * rstd * g + b


def exact_fwd(x, gamma, beta, eps=EPS, delta=None, delta2=None):
    s = f32_sum(x, delta, delta2)
    e = eps32(eps)
    mean, var, rstd, d, y = _ln64(s.double(), gamma.double(), beta.double(), e)
    return {"s": s, "mean": mean[..., 0], "rstd": rstd[..., 0], "y": y, "var": var[..., 0], "d": d, "eps": e,
            "gamma": gamma.double(), "beta": beta.double()}


def exact_merge(x, g1, b1, g2, b2, eps=EPS, delta=None):
    """x [B, T, D] (token 0 the class token).  -> cls_ln [B, D], feats [B, T - 1, D], stats1 [B, T, 2], stats2 [B, T - 1, 2], y1, z, s and the two
    exact_fwd-style records r1 / r2 the bounds need."""
    r1 = exact_fwd(x, g1, b1, eps, delta)
    y1 = r1["y"]
    z = y1[:, 1:] * y1[:, :1]
    e = r1["eps"]
    mean2, var2, rstd2, d2, feats = _ln64(z, g2.double(), b2.double(), e)
    r2 = {"mean": mean2[..., 0], "rstd": rstd2[..., 0], "y": feats, "var": var2[..., 0], "d": d2, "eps": e, "gamma": g2.double(), "beta": b2.double()}
    return {"s": r1["s"], "cls_ln": y1[:, 0], "feats": feats, "stats1": torch.stack([r1["mean"], r1["rstd"]], -1),
            "stats2": torch.stack([r2["mean"], r2["rstd"]], -1), "y1": y1, "z": z, "r1": r1, "r2": r2}


def exact_bwd(dy, x, mean, rstd, gamma, dres=None):
    dy, x, g = dy.double(), x.double(), gamma.double()
    m, r = mean.double()[:, None], rstd.double()[:, None]
    xh = (x - m) * r
    gd = dy * g
    s1 = gd.mean(-1, keepdim=True)
    s2 = (gd * xh).mean(-1, keepdim=True)
    dx0 = r * (gd - s1 - xh * s2)
    dx = dx0 + dres.double() if dres is not None else dx0
    return {"dx": dx, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0), "colsum": dx.sum(0), "xh": xh, "gd": gd, "s1": s1, "s2": s2,
            "dx0": dx0, "r": r, "dy": dy, "has_dres": dres is not None}


def exact_merge_bwd(dfeats, x, g1, b1, g2, eps=EPS, given=None):
    """Backward of feats = LN2(LN1(x)[:, 1:] * LN1(x)[:, :1]) for upstream dfeats [B, P, D]; x [B, T, D] f32 (the saved sum), token 0 the class token.
    Closed form: the LayerNorm backward of `exact_bwd` applied to LN2 and then to LN1, with d(cls_ln) = sum_p dz y1 in between -- evaluated in float64 at
    the statistics and class row the kernels are GIVEN (`given` = {"stats1" [B, T, 2], "stats2" [B, P, 2], "cls_ln" [B, D]}, f32 upcast), or at the exact
    ones when `given` is None; test_layernorm_reference.py shows that at the exact ones it equals float64 autograd of the merge expression.
    -> dx [B, T, D], dcls [B, D], dg1, db1, dg2, db2, colsum [D] and the intermediates the bounds need."""
    x, df = x.double(), dfeats.double()
    g1, b1, g2 = g1.double(), b1.double(), g2.double()
    if given is None:
        m = exact_merge(x.float(), g1, b1, g2, torch.zeros_like(g2), eps)
        given = {"stats1": m["stats1"], "stats2": m["stats2"], "cls_ln": m["cls_ln"]}
    st1, st2, c = given["stats1"].double(), given["stats2"].double(), given["cls_ln"].double()[:, None]
    m1, r1 = st1[:, 1:, :1], st1[:, 1:, 1:]
    m2, r2 = st2[..., :1], st2[..., 1:]
    xh = (x[:, 1:] - m1) * r1
    y = xh * g1 + b1
    zh = (y * c - m2) * r2
    gz = df * g2
    M1, M2 = gz.mean(-1, keepdim=True), (gz * zh).mean(-1, keepdim=True)
    dz = r2 * (gz - M1 - zh * M2)
    dcls = (dz * y).sum(1)
    dy = dz * c
    gd = dy * g1
    N1, N2 = gd.mean(-1, keepdim=True), (gd * xh).mean(-1, keepdim=True)
    dxp = r1 * (gd - N1 - xh * N2)
    m0, r0 = st1[:, 0, :1], st1[:, 0, 1:]
    xh0 = (x[:, 0] - m0) * r0
    gd0 = dcls * g1
    S1, S2 = gd0.mean(-1, keepdim=True), (gd0 * xh0).mean(-1, keepdim=True)
    dx0 = r0 * (gd0 - S1 - xh0 * S2)
    dx = torch.cat([dx0[:, None], dxp], 1)
    return {"dx": dx, "dcls": dcls, "dg1": (dy * xh).sum((0, 1)) + (dcls * xh0).sum(0), "db1": dy.sum((0, 1)) + dcls.sum(0),
            "dg2": (df * zh).sum((0, 1)), "db2": df.sum((0, 1)), "colsum": dx.sum((0, 1)),
            "in": {"x": x, "df": df, "g1": g1, "b1": b1, "g2": g2, "c": c, "m1": m1, "r1": r1, "m2": m2, "r2": r2, "m0": m0, "r0": r0}}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _mul(a, Ea, b, Eb):
    return a.abs() * Eb + b.abs() * Ea + Ea * Eb


def _rnd(ref, E):
    """E after one more f32 rounding of the result."""
    return E + F * (ref.abs() + E)


def _ln_bound(v, r, E_in=None):
    """Bounds of row_stats + the affine map on elements v (float64) known to E_in; r: the exact record (mean, var, rstd, d, y, gamma, beta, eps).
    -> dict mean, rstd (per row), y (pre-store)."""
    D = v.shape[-1]
    ns = n_sum(D)
    E_in = torch.zeros_like(v) if E_in is None else E_in
    mag = v.abs() + E_in
    E_mean = (E_in.sum(-1, keepdim=True) + gam(ns + 1) * mag.sum(-1, keepdim=True)) / D + TINY
    d = r["d"]
    E_d = E_in + E_mean + F * (1.0 + F) * (d.abs() + E_in + E_mean)
    E_c = E_in + E_mean                                     # what d~ is off by before its own rounding
    r2 = (1.0 + F) ** 2 - 1.0
    sq = (d.abs() + E_c) ** 2
    E_var = ((2.0 * d.abs() * E_in + E_c * E_c + r2 * sq).sum(-1, keepdim=True) + gam(ns + 2) * ((1.0 + r2) * sq).sum(-1, keepdim=True)) / D + TINY
    ve = r["var"][..., None] + r["eps"]
    E_ve = _rnd(ve, E_var)
    rho = E_ve / ve
    rstd = r["rstd"][..., None]
    r_rstd = (1.0 + RSQRT_ULPS * 2.0 * F) / torch.sqrt(1.0 - rho) - 1.0
    E_rstd = rstd * r_rstd
    t = d * rstd
    E_t = _rnd(t, _mul(d, E_d, rstd, E_rstd))
    g = r["gamma"]
    w = t * g
    E_w = _rnd(w, g.abs() * E_t)
    E_y = _rnd(r["y"], E_w) + TINY
    return {"mean": E_mean[..., 0] + TINY, "rstd": E_rstd[..., 0] + TINY, "y": E_y}


def store_f32(E):
    return E + TINY


def store_bf16(ref, E):
    return E + U * (ref.abs() + E) + TINY


def bounds_fwd(r):
    """-> {"mean", "rstd", "f32", "bf16"}: tolerances of the statistics and of the output in either store."""
    b = _ln_bound(r["s"].double(), r)
    return {"mean": b["mean"], "rstd": b["rstd"], "f32": store_f32(b["y"]), "bf16": store_bf16(r["y"], b["y"])}


def bounds_merge(m):
    r1, r2 = m["r1"], m["r2"]
    b1 = _ln_bound(m["s"].double(), r1)
    E_y1 = b1["y"]
    E_c = store_f32(E_y1[:, :1])
    y1p, c = m["y1"][:, 1:], m["y1"][:, :1]
    E_z = _rnd(m["z"], _mul(y1p, E_y1[:, 1:], c, E_c)) + TINY
    b2 = _ln_bound(m["z"], r2, E_z)
    return {"cls_ln": E_c[:, 0], "stats1": torch.stack([b1["mean"], b1["rstd"]], -1), "stats2": torch.stack([b2["mean"], b2["rstd"]], -1),
            "feats": store_bf16(m["feats"], b2["y"])}


def bounds_bwd(e, rows_chain=None, old=None):
    """e = exact_bwd(...).  -> tolerances dx, dx_bf16, dgamma, dbeta, colsum.  `old` = {"dgamma", "dbeta", "colsum"}: the accumulators' values before
    the call (the reference the caller compares against is old + sum); rows_chain = n_rows(rows) by default."""
    xh, gd, s1, s2, r, dy = e["xh"], e["gd"], e["s1"], e["s2"], e["r"], e["dy"]
    rows, D = xh.shape
    ns = n_sum(D)
    E_xh = ((1.0 + F) ** 2 - 1.0) * xh.abs() + TINY
    E_gd = F * gd.abs() + TINY
    E_s1 = (E_gd.sum(-1, keepdim=True) + gam(ns + 1) * (gd.abs() + E_gd).sum(-1, keepdim=True)) / D + TINY
    p = gd * xh
    E_p = _mul(gd, E_gd, xh, E_xh)
    E_s2 = (E_p.sum(-1, keepdim=True) + gam(ns + 2) * (p.abs() + E_p).sum(-1, keepdim=True)) / D + TINY
    t = gd - s1
    E_t = _rnd(t, E_gd + E_s1)
    v = t - xh * s2
    E_v = _rnd(v, E_t + _mul(xh, E_xh, s2, E_s2))
    E_dx = _rnd(e["dx0"], r * E_v) + TINY
    if e["has_dres"]:
        E_dx = _rnd(e["dx"], E_dx) + TINY
    n = n_rows(rows) if rows_chain is None else rows_chain
    old = old or {}

    def red(term, E_term, key):
        o = old.get(key)
        o = o.double().abs() if o is not None else 0.0
        return gam(n) * ((term.abs() + E_term).sum(0) + o) + E_term.sum(0) + TINY

    return {"dx": E_dx, "dx_bf16": store_bf16(e["dx"], E_dx), "dgamma": red(dy * xh, dy.abs() * E_xh, "dgamma"),
            "dbeta": red(dy, torch.zeros_like(dy), "dbeta"), "colsum": red(e["dx"], E_dx, "colsum")}


class _V:
    """a float64 value v of the reference that the kernel holds to within E (elementwise); every operation below charges the propagated error of its
    operands plus ONE rounding of its result (and T for a result that may underflow)."""
    def __init__(self, v, E=None):
        self.v, self.E = v, (torch.zeros_like(v) if E is None else E)

    def _out(self, r, E):
        return _V(r, E + F * (r.abs() + E) + TINY)

    def __mul__(self, o):
        return self._out(self.v * o.v, _mul(self.v, self.E, o.v, o.E))

    def __add__(self, o):
        return self._out(self.v + o.v, self.E + o.E)

    def __sub__(self, o):
        return self._out(self.v - o.v, self.E + o.E)

    def fma(self, o, c):                       # fmaf(self, o, c): one rounding
        return self._out(self.v * o.v + c.v, _mul(self.v, self.E, o.v, o.E) + c.E)

    def mean(self, n, D):
        """sum over the last axis by a chain of n roundings, then the division (or the multiply by a rounded 1 / D) counted in n."""
        return _V(self.v.sum(-1, keepdim=True) / D, (self.E.sum(-1, keepdim=True) + gam(n) * (self.v.abs() + self.E).sum(-1, keepdim=True)) / D + TINY)


N_MOMENT = 3 + 6 + 3 + 2          # merge_ln_bwd_kernel: 4 elements of a thread, 6 levels, 4 waves in order, invD = fl(1 / D) and the multiply by it


def n_rows_merge(B, P, groups_together=True):
    """merge_ln_bwd_kernel's row chain: a thread adds the rows of its 64-row block in order (64), partials_reduce_kernel the B nbx slabs (nbx for dcls,
    one group per image, no accumulate)."""
    nbx = (P + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    nblk = B * nbx if groups_together else nbx
    return ROWS_PER_BLOCK + (nblk + REDUCE_LANES - 1) // REDUCE_LANES + (REDUCE_LANES - 1) + (1 if groups_together else 0)


def n_rows_cls(B):
    """the class-row pass: B terms through a second partials_reduce_kernel with accumulate."""
    return (B + REDUCE_LANES - 1) // REDUCE_LANES + (REDUCE_LANES - 1) + 1


def bounds_merge_bwd(e, old=None):
    """e = exact_merge_bwd(..., given=...).  -> tolerances dx, dx_bf16, dcls, dg1, db1, dg2, db2, colsum (`old`: the accumulators before the call)."""
    i = e["in"]
    B, T, D = i["x"].shape
    P = T - 1
    X, df, g1, b1, g2, c = _V(i["x"][:, 1:]), _V(i["df"]), _V(i["g1"]), _V(i["b1"]), _V(i["g2"]), _V(i["c"])
    m1, r1, m2, r2 = _V(i["m1"]), _V(i["r1"]), _V(i["m2"]), _V(i["r2"])
    xh = (X - m1) * r1
    y = xh.fma(g1, b1)
    zh = (y * c - m2) * r2
    gz = df * g2
    M1, M2 = gz.mean(N_MOMENT, D), (gz * zh).mean(N_MOMENT, D)
    dz = r2 * (gz - M1 - zh * M2)
    t_c = dz * y
    dy = dz * c
    t_g1 = dy * xh
    gd = dy * g1
    N1, N2 = gd.mean(N_MOMENT, D), (gd * xh).mean(N_MOMENT, D)
    dxp = r1 * (gd - N1 - xh * N2)
    t_g2 = df * zh
    old = old or {}

    def o_(key):
        o = old.get(key)
        return o.double().abs() if o is not None else 0.0

    def red(terms, n, key=None):
        """terms: list of _V [.., D] whose leading axes are summed; n roundings on the longest path."""
        mag = sum((t.v.abs() + t.E).reshape(-1, D).sum(0) for t in terms)
        Es = sum(t.E.reshape(-1, D).sum(0) for t in terms)
        return gam(n) * (mag + (o_(key) if key else 0.0)) + Es + TINY

    np_, nc = n_rows_merge(B, P), n_rows_cls(B)
    # dcls[b]: per-image groups, written (not accumulated)
    nd = n_rows_merge(B, P, False)
    E_dcls = gam(nd) * (t_c.v.abs() + t_c.E).sum(1) + t_c.E.sum(1) + TINY
    # class rows (cls_ln_bwd_kernel): dy0 = the kernel's own dcls, known to E_dcls
    d0 = _V(e["dcls"], E_dcls)
    X0, m0, r0 = _V(i["x"][:, 0]), _V(i["m0"]), _V(i["r0"])
    ns = n_sum(D)
    xh0 = (X0 - m0) * r0
    gd0 = d0 * g1
    S1, S2 = gd0.mean(ns + 1, D), (gd0 * xh0).mean(ns + 1, D)
    dx0 = r0 * (gd0 - S1 - xh0 * S2)
    t0_g1 = d0 * xh0
    E_dx = torch.cat([dx0.E[:, None], dxp.E], 1)
    return {"dx": E_dx + TINY, "dx_bf16": store_bf16(e["dx"], E_dx), "dcls": E_dcls,
            "dg1": red([t_g1, t0_g1], np_ + nc, "dg1"), "db1": red([dy, d0], np_ + nc, "db1"),
            "dg2": red([t_g2], np_, "dg2"), "db2": red([df], np_, "db2"), "colsum": red([dxp, dx0], np_ + nc, "colsum")}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input profiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILES = ("randn", "outlier", "offset", "flat", "scaled")
AFFINE_OF = {"randn": "plain", "outlier": "plain", "offset": "hard", "flat": "hard", "scaled": "hard"}
DY_KINDS = ("white", "aligned", "sparse")


def _gen(seed, rows, D, salt=0):
    return torch.Generator(device="cpu").manual_seed(seed * 1000003 + rows * 10007 + D * 101 + salt)


def row_scale(profile, rows):
    """per-row power of two of the `scaled` profile (1 elsewhere)."""
    sc = torch.ones(rows, 1)
    if profile == "scaled":
        sc[0::2] = 2.0 ** -40
        sc[1::2] = 2.0 ** 40
    return sc


def make_inputs(profile, rows, D, seed, affine=None):
    """Seeded inputs on the CPU: x [rows, D] f32, delta / delta2 (float32 holding bf16 values), gamma, beta [D] f32 (module docstring)."""
    g = _gen(seed, rows, D)
    n = torch.randn(rows, D, generator=g)
    dscale = torch.ones(rows, 1)
    if profile == "randn":
        x = n * 2.0 + 0.3
    elif profile == "outlier":
        x = n.clone()
        cols = [0, D - 1]
        if D > 8:
            extra = torch.randperm(D - 2, generator=g)[:int(torch.randint(0, 3, (1,), generator=g))] + 1
            cols += extra.tolist()
        for c in cols:
            mag = 64.0 + 192.0 * torch.rand(rows, generator=g)
            sign = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0)
            x[:, c] = mag * sign
    elif profile == "offset":
        m = 2.0 ** (10.0 + 2.0 * torch.rand(rows, 1, generator=g))
        x = n + m * torch.where(torch.rand(rows, 1, generator=g) < 0.5, -1.0, 1.0)
    elif profile == "flat":
        c = (0.5 + torch.rand(rows, 1, generator=g)) * torch.where(torch.rand(rows, 1, generator=g) < 0.5, -1.0, 1.0)
        x = c + 1e-4 * n
        dscale = torch.full((rows, 1), 1e-4)
        x[1::3] = 0.0
        dscale[1::3] = 0.0
    elif profile == "scaled":
        dscale = row_scale(profile, rows)
        x = n * dscale
    else:
        raise ValueError(profile)
    delta = bf16_round(0.5 * torch.randn(rows, D, generator=g) * dscale)
    delta2 = bf16_round(0.5 * torch.randn(rows, D, generator=g) * dscale)
    kind = affine or AFFINE_OF[profile]
    ga = 1.0 + 0.1 * torch.randn(D, generator=g)
    be = 0.1 * torch.randn(D, generator=g)
    if kind == "hard":
        ga = torch.randn(D, generator=g) * 2.0
        ga[0::5] = 0.0
        ga[1::5] = -8.0 * torch.rand(ga[1::5].shape, generator=g)
        ga[2::7] = 8.0
        xd = x.double()[0]
        xh0 = (xd - xd.mean()) / torch.sqrt(xd.var(unbiased=False) + eps32(EPS))
        be[3::4] = (-xh0 * ga.double()).float()[3::4]
        be = be + 0.0                # (no -0: a zero row gives +0 gamma + beta)
    elif kind != "plain":
        raise ValueError(kind)
    return {"x": x.float(), "delta": delta, "delta2": delta2, "gamma": ga.float(), "beta": be.float()}


def make_dy(kind, x, mean, rstd, gamma, seed, bf16):
    """Upstream gradient [rows, D] on the CPU for saved activations x with statistics (mean, rstd): f32, or bf16 values held in float32."""
    rows, D = x.shape
    g = _gen(seed, rows, D, salt=17)
    n = torch.randn(rows, D, generator=g)
    if kind == "white":
        dy = 0.1 * n
    elif kind == "aligned":
        xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
        a = torch.randn(rows, 1, generator=g).double()
        b = torch.randn(rows, 1, generator=g).double()
        gd = a + b * xh + 1e-3 * n.double()
        gg = gamma.double()
        dy = torch.where(gg != 0, gd / torch.where(gg != 0, gg, torch.ones_like(gg)), 0.1 * n.double()).float()
    elif kind == "sparse":
        dy = torch.zeros(rows, D)
        r = torch.arange(rows)
        dy[r, (r * 7 + 3) % D] = n[r, 0] + 2.0
    else:
        raise ValueError(kind)
    return bf16_round(dy) if bf16 else dy.float()


DFEATS_KINDS = ("white", "aligned")


def make_dfeats(kind, x, given, g1, b1, g2, seed):
    """Upstream gradient [B, P, D] f32 of the merge backward: `make_dy` on the second LayerNorm's own input z = y1[:, 1:] cls_ln at the given statistics
    (aligned: g2 dfeats = a + b zhat + 1e-3 noise, so dz is a cancellation)."""
    B, T, D = x.shape
    st1, st2 = given["stats1"].double(), given["stats2"].double()
    y = (x.double()[:, 1:] - st1[:, 1:, :1]) * st1[:, 1:, 1:] * g1.double() + b1.double()
    z = (y * given["cls_ln"].double()[:, None]).reshape(B * (T - 1), D)
    return make_dy(kind, z, st2[..., 0].reshape(-1), st2[..., 1].reshape(-1), g2, seed, False).reshape(B, T - 1, D)


def padded(t, pad, fill):
    """t with `pad` more rows of `fill` (NaN for inputs, a sentinel for outputs)."""
    out = torch.full((t.shape[0] + pad,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _lanes(v):
    """[R, D] -> ([R, nv, 64, 4], mask [nv, 64]): vector idx = lane + 64 i of the row, as the kernels index it; absent vectors are zero."""
    R, D = v.shape
    nvec, nv = D // 4, nv_of(D)
    buf = torch.zeros(R, nv * 256, dtype=v.dtype)
    buf[:, :D] = v
    mask = (torch.arange(nv * 64) < nvec).reshape(nv, 64)
    return buf.reshape(R, nv, 64, 4), mask


def _wave_sum(s, cnt):
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
        cnt[0] += 1
    return s


def _lane_sum(V, mask, cnt, skip_last=False):
    """every lane's in-order sum of its vectors ((x + y) + z) + w, then the six butterfly levels; cnt[0] counts the adds on the path."""
    R, nv = V.shape[0], V.shape[1]
    s = torch.zeros(R, 64, dtype=torch.float32)
    for i in range(nv):
        if skip_last and i == nv - 1 and not bool(mask[i].all()):
            continue
        t = ((V[:, i, :, 0] + V[:, i, :, 1]) + V[:, i, :, 2]) + V[:, i, :, 3]
        s = s + torch.where(mask[i], t, torch.zeros_like(t))
        cnt[0] += 4
    return _wave_sum(s, cnt)[:, :1]


def emulate_row_stats(v, eps=EPS, hooks=(), counts=None):
    """row_stats (norm.hip:9-23) on v [R, D] f32 -> mean, rstd [R, 1].  hooks: "one_pass", "skip_tail", "dm1", "eps_outside"."""
    R, D = v.shape
    V, mask = _lanes(v)
    Df = torch.tensor(float(D), dtype=torch.float32)
    e = torch.tensor(eps, dtype=torch.float32)
    cnt = [0]
    skip = "skip_tail" in hooks
    mean = _lane_sum(V, mask, cnt, skip) / Df
    if counts is not None:
        counts["n_sum"] = cnt[0]
    if "one_pass" in hooks:
        var = _lane_sum(V * V, mask, [0]) / Df - mean * mean
    else:
        d = torch.where(mask[None, :, :, None], V - mean[:, :, None, None], torch.zeros_like(V))
        var = _lane_sum(d * d, mask, [0], skip) / (Df - 1.0 if "dm1" in hooks else Df)
    rstd = 1.0 / (torch.sqrt(var) + e) if "eps_outside" in hooks else torch.rsqrt(var + e)
    return mean, rstd


def emulate_fwd(x, gamma, beta, eps=EPS, delta=None, delta2=None, out_bf16=True, hooks=(), counts=None):
    """ln_fwd_kernel -> s, mean, rstd, y (bf16 values in float32, or float32).  hooks: those of emulate_row_stats and "assoc" (x + (d + d2))."""
    s = x.float() + (delta.float() + delta2.float()) if "assoc" in hooks else f32_sum(x, delta, delta2)
    mean, rstd = emulate_row_stats(s, eps, hooks, counts)
    y = (s - mean) * rstd * gamma.float() + beta.float()
    return {"s": s, "mean": mean[:, 0], "rstd": rstd[:, 0], "y": bf16_round(y) if out_bf16 else y, "y32": y}


def emulate_merge(x, g1, b1, g2, b2, eps=EPS, delta=None, hooks=()):
    """cls_ln_kernel + merge_ln_kernel on x [B, T, D]."""
    B, T, D = x.shape
    fl = lambda t: t.reshape(B * T, D) if t is not None else None
    r1 = emulate_fwd(fl(x), g1, b1, eps, fl(delta), None, False, hooks)
    y1 = r1["y"].reshape(B, T, D)
    z = (y1[:, 1:] * y1[:, :1]).reshape(B * (T - 1), D)
    mean2, rstd2 = emulate_row_stats(z, eps, hooks)
    feats = bf16_round((z - mean2) * rstd2 * g2.float() + b2.float())
    return {"s": r1["s"].reshape(B, T, D), "cls_ln": y1[:, 0], "feats": feats.reshape(B, T - 1, D),
            "stats1": torch.stack([r1["mean"], r1["rstd"]], -1).reshape(B, T, 2),
            "stats2": torch.stack([mean2[:, 0], rstd2[:, 0]], -1).reshape(B, T - 1, 2)}


def emulate_reduce(part, old=None, hooks=(), counts=None):
    """partials_reduce_kernel on part [nblk, D]: lane j adds slabs j, j + 16, ... in order, the 16 lane sums are added in order, then the old value.
    hook "drop_slab16"."""
    nblk, D = part.shape
    a = torch.zeros(REDUCE_LANES, D, dtype=torch.float32)
    strided = 0
    for j in range(REDUCE_LANES):
        k = 0
        for s in range(j, nblk, REDUCE_LANES):
            if "drop_slab16" in hooks and s == 16:
                continue
            a[j] = a[j] + part[s]
            k += 1
        strided = max(strided, k)
    t = a[0]
    for j in range(1, REDUCE_LANES):
        t = t + a[j]
    n = strided + REDUCE_LANES - 1
    if old is not None:
        t = t + old.float()
        n += 1
    if counts is not None:
        counts["n_reduce"] = n
    return t


def emulate_bwd(dy, x, mean, rstd, gamma, dres=None, old=None, hooks=(), counts=None):
    """ln_bwd_body + partials_reduce_kernel -> dx, dx_bf16, dgamma, dbeta, colsum (the latter three added onto old[...] when given).
    hooks: "no_s2", "mean_dy", "no_dres", "drop_last_row", "drop_slab16"."""
    dy, x, g = dy.float(), x.float(), gamma.float()
    rows, D = x.shape
    m, r = mean.float()[:, None], rstd.float()[:, None]
    Df = torch.tensor(float(D), dtype=torch.float32)
    xh = (x - m) * r
    gd = dy * g
    Vg, mask = _lanes(dy if "mean_dy" in hooks else gd)
    cnt = [0]
    s1 = _lane_sum(Vg, mask, cnt) / Df
    G, X = _lanes(gd)[0], _lanes(xh)[0]
    s = torch.zeros(rows, 64, dtype=torch.float32)
    for i in range(G.shape[1]):
        t = G[:, i, :, 0] * X[:, i, :, 0]
        for k in (1, 2, 3):
            t = _fma32(G[:, i, :, k], X[:, i, :, k], t)
        s = s + t
    s2 = _wave_sum(s, [0])[:, :1] / Df
    if "no_s2" in hooks:
        s2 = torch.zeros_like(s2)
    dx = r * _fma32(-xh, s2.expand_as(xh), gd - s1)
    if dres is not None and "no_dres" not in hooks:
        dx = dx + dres.float()
    # row reductions: wave w of block k adds rows 64 k + w, + 4, ... in order
    nblk = (rows + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    parts = torch.zeros(3, nblk, D, dtype=torch.float32)
    per_wave = 0
    last = rows - 1 if ("drop_last_row" in hooks and rows % ROWS_PER_BLOCK) else -1
    for k in range(nblk):
        acc = torch.zeros(3, WAVES, D, dtype=torch.float32)
        steps = 0
        for i in range(ROWS_PER_BLOCK // WAVES):
            base = k * ROWS_PER_BLOCK + i * WAVES
            if base >= rows:
                break
            steps += 1
            for w in range(min(WAVES, rows - base)):
                rr = base + w
                if rr != last:
                    acc[0, w] = _fma32(dy[rr], xh[rr], acc[0, w])
                acc[1, w] = acc[1, w] + dy[rr]
                acc[2, w] = acc[2, w] + dx[rr]
        per_wave = max(per_wave, steps)
        parts[:, k] = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    old = old or {}
    c2 = {}
    out = {"dx": dx, "dx_bf16": bf16_round(dx)}
    for i, key in enumerate(("dgamma", "dbeta", "colsum")):
        out[key] = emulate_reduce(parts[i], old.get(key), hooks, c2)
    if counts is not None:
        counts["n_sum"] = cnt[0]
        counts["n_rows"] = per_wave + (WAVES - 1) + c2["n_reduce"]
    return out


def _moment(v, D):
    """merge_ln_bwd_kernel's row moment of v [R, D]: thread t adds its columns 4 t .. 4 t + 3 in order, wave_sum, the four waves in order, * fl(1 / D)."""
    R_ = v.shape[0]
    buf = torch.zeros(R_, 1024, dtype=torch.float32)
    buf[:, :D] = v
    q = buf.reshape(R_, WAVES, 64, 4)
    t = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    w = torch.stack([_wave_sum(t[:, k], [0])[:, 0] for k in range(WAVES)], 1)
    invD = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(D), dtype=torch.float32)
    return ((((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]) * invD)[:, None]


def emulate_merge_bwd(dfeats, x, cls_ln, st1, st2, g1, b1, g2, old=None, hooks=(), counts=None):
    """merge_ln_bwd_kernel + partials_reduce_kernel (dcls per image; the parameter gradients over every slab) + cls_ln_bwd_kernel + its reduce, in f32.
    hook "no_cls_param": the class rows' contribution to dg1 / db1 left out."""
    B, T, D = x.shape
    P = T - 1
    df, x, c = dfeats.float(), x.float(), cls_ln.float()[:, None]
    g1, b1, g2 = g1.float(), b1.float(), g2.float()
    m1, r1, m2, r2 = st1[:, 1:, :1].float(), st1[:, 1:, 1:].float(), st2[..., :1].float(), st2[..., 1:].float()
    xh = (x[:, 1:] - m1) * r1
    y = _fma32(xh, g1.expand_as(xh), b1.expand_as(xh))
    zh = (y * c - m2) * r2
    gz = df * g2
    fl = lambda t: t.reshape(B * P, D)
    M1, M2 = _moment(fl(gz), D).reshape(B, P, 1), _moment(fl(gz * zh), D).reshape(B, P, 1)
    dz = r2 * (gz - M1 - zh * M2)
    dy = dz * c
    gd = dy * g1
    N1, N2 = _moment(fl(gd), D).reshape(B, P, 1), _moment(fl(gd * xh), D).reshape(B, P, 1)
    dxp = r1 * (gd - N1 - xh * N2)
    terms = torch.stack([dz * y, dy * xh, dy, df * zh, df, dxp])              # {dcls, dg1, db1, dg2, db2, sum dx} [6, B, P, D]
    nbx = (P + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    part = torch.zeros(6, B, nbx, D, dtype=torch.float32)
    longest = 0
    for k in range(nbx):
        for p in range(k * ROWS_PER_BLOCK, min(P, (k + 1) * ROWS_PER_BLOCK)):
            part[:, :, k] = part[:, :, k] + terms[:, :, p]
        longest = max(longest, min(P, (k + 1) * ROWS_PER_BLOCK) - k * ROWS_PER_BLOCK)
    old = old or {}
    c1, c2, c3 = {}, {}, {}
    dcls = torch.stack([emulate_reduce(part[0, b], None, (), c1) for b in range(B)])
    out = {"dcls": dcls}
    for i_, key in ((1, "dg1"), (2, "db1"), (3, "dg2"), (4, "db2"), (5, "colsum")):
        out[key] = emulate_reduce(part[i_].reshape(B * nbx, D), old.get(key), (), c2)
    # class rows
    m0, r0 = st1[:, 0, :1].float(), st1[:, 0, 1:].float()
    xh0 = (x[:, 0] - m0) * r0
    gd0 = dcls * g1
    Df = torch.tensor(float(D), dtype=torch.float32)
    V0, mask = _lanes(gd0)
    S1 = _lane_sum(V0, mask, [0]) / Df
    S2 = _lane_sum(_lanes(gd0 * xh0)[0], mask, [0]) / Df
    dx0 = r0 * (gd0 - S1 - xh0 * S2)
    for key, t in (("dg1", dcls * xh0), ("db1", dcls), ("colsum", dx0)):
        if "no_cls_param" in hooks and key != "colsum":
            continue
        out[key] = emulate_reduce(t, out[key], (), c3)
    dx = torch.cat([dx0[:, None], dxp], 1)
    out["dx"], out["dx_bf16"] = dx, bf16_round(dx)
    if counts is not None:
        counts["n_dcls"] = longest + c1["n_reduce"]
        counts["n_param"] = longest + c2["n_reduce"]
        counts["n_cls"] = c3.get("n_reduce")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case set shared by the CPU and the GPU test
# ---------------------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (4, 128, 252, 260, 768, 1020, 1024, 64, 512)     # (64, 512: the text tower's widths, last so that the rotation of merge_cases stays)
FULL_WIDTHS = (260, 768, 1024)            # every profile; the other widths take randn + outlier
FWD_ROWS = (1, 5, 67)
BWD_ROWS = (1, 67, 131)
BWD_LONG = ((128, 1100), (128, 2100))     # nblk = 18 and 33: partials_reduce_kernel's strided loop with remainders 2 and 1
MERGE_BP = ((1, 1), (2, 37), (3, 67))
FWD_FORMS = ("bf16", "f32", "f32_inplace", "delta", "delta_alias", "delta2", "nostore", "nostats")


def profiles_of(D):
    return PROFILES if D in FULL_WIDTHS else PROFILES[:2]


def fwd_cases():
    return [(D, p, rows) for D in WIDTHS for p in profiles_of(D) for rows in FWD_ROWS]


def bwd_cases():
    return [(D, p, rows) for D in WIDTHS for p in profiles_of(D) for rows in BWD_ROWS] + [(D, p, rows) for D, rows in BWD_LONG for p in PROFILES[:2]]


def merge_cases():
    """every (width, profile) meets one (B, P), rotating; flat (z ~ 0, rstd2 ~ 316) and offset meet all three at the full widths, randn at D = 260."""
    out = []
    i = 0
    for D in WIDTHS:
        for p in profiles_of(D):
            out.append((D, p) + MERGE_BP[i % 3])
            i += 1
    every = [(D, p) for D in FULL_WIDTHS for p in ("flat", "offset")] + [(260, "randn")]
    out += [dp + bp for dp in every for bp in MERGE_BP if dp + bp not in out]
    return out


def roundup(n, m):
    return (n + m - 1) // m * m
