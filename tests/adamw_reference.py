"""Float64 reference and derived element-wise error bounds for one fused AdamW step: adamw_kernel (csrc/optim.hip:16-21), adamw_grouped_kernel
(csrc/optim_groups.hip:60-65) and adamw_ema_kernel (csrc/optim_ema.hip:50-55).  Checker side, numpy, device-agnostic.

What the kernels compute, per element (the three write the same expression sequence; `coef` exists in the grouped and EMA kernels only):

    gg    = g * grad_scale [* coef]                   optim.hip:16   optim_groups.hip:60   optim_ema.hip:50
    p    *= (1.f - lr * wd)                           optim.hip:17   optim_groups.hip:61   optim_ema.hip:51
    m'    = b1 * m + (1.f - b1) * gg                  optim.hip:18   optim_groups.hip:62   optim_ema.hip:52
    v'    = b2 * v + (1.f - b2) * gg * gg             optim.hip:19   optim_groups.hip:63   optim_ema.hip:53
    denom = sqrtf(v') / bc2_sqrt + eps                optim.hip:20   optim_groups.hip:64   optim_ema.hip:54
    p'    = p - (lr / bc1) * (m' / denom)             optim.hip:21   optim_groups.hip:65   optim_ema.hip:55

with lr, wd taken per segment of the bucket (optim_groups.hip:54-55, optim_ema.hip:42-43) and, on the host, in f32 (optim.hip:36-37,
optim_groups.hip:113-114, optim_ema.hip:107-108)

    bc1 = 1.f - powf(beta1, (float)step)              bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step))

Reference
---------
`step_reference` runs one step in float64 on the values the kernel is GIVEN: the f32 arrays p, g, m, v (v >= 0), the f32 scalars lr, wd (scalars or one
value per element: the segment's row, found from the element index alone by `rows`), beta1, beta2, eps, grad_scale, and the clip coefficient.  It does not
ask whether they are good hyper-parameters.  The bias corrections are formed in float64 from the f32 betas, B1 = 1 - beta1^t and
B2 = sqrt(1 - beta2^t) (`bias_corrections`).  A trajectory is judged step by step from the kernel's own previous outputs, so nothing compounds and no
propagation across steps is needed.  Out of scope: overflow of gg^2, non-finite gradients, eps = 0 and betas outside (0, 1).

Conventions
-----------
u = 2^-24 is f32's unit round-off, so fl(x) = x (1 + d), |d| <= u, for a correctly rounded operation.  T = 2^-126, the smallest normal f32, is added
once per rounding (the flush allowance of gemm_reference.py: a result below T may be kept as a subnormal, error <= 2^-150, or flushed to zero, error
<= T), and once per input array (an input below T may be read as zero).  x~ is the kernel's value of the reference's x and E_x >= |x~ - x|.

The files are compiled with the default contraction, so a product feeding an add may or may not be fused.  Every multiply and every add is budgeted
with a rounding of its own: a fused multiply-add is the unfused pair with the product's d = 0, so both forms lie inside (and so does any mix of them).

ASSUMPTION 1  sqrtf on the device is correctly rounded under the default flags (u); the bound budgets the limit OpenCL's full profile documents for
              sqrt, 3 ulp = 6 u relative (1 ulp <= 2 u relative, as in gemm_reference.py), so that a flag change cannot fail the test for the wrong
              reason:  SQRT_REL = 6 u.
ASSUMPTION 2  the two f32 divisions are correctly rounded under the default flags (u); budgeted at OpenCL's documented 2.5 ulp:  DIV_REL = 5 u.
ASSUMPTION 3  the host's powf is within 1 ulp = 2 u relative of x^y (glibc documents 1 ulp), and powf(x, 1) = x exactly (the result is representable
              and an implementation within 1 ulp that rounds a more precise intermediate returns it);  the host's sqrtf is correctly rounded.
ASSUMPTION 4  no kernel value overflows (g^2 scaled stays below f32's largest finite number) and eps > 0.

Bias corrections  (`bias_corrections`; bc~ = B (1 + r), |r| <= R)
----------------
P = beta^t.  (float)step is exact up to 2^24; beyond it tf = fl(t) and |beta^tf - beta^t| <= beta^min(t, tf) |tf - t| |ln beta| =: E_t.
powf: E_P = E_t + 2 u (P + E_t) + T for t > 1, E_P = 0 for t = 1 (ASSUMPTION 3).
1.f - P~: exact by Sterbenz's lemma when t = 1 and beta >= 0.5 (1 lies in [beta, 2 beta]); otherwise one rounding, u (X + E_P), X = 1 - P.
    R_X = (E_P + u (X + E_P)) / X            -- large where 1 - beta^t cancels: t = 2, beta2 = 0.999 gives X = 0.002 and R_X ~ 1e3 u
    R1  = R_X(beta1)
    R2  = (1 + R_X / (1 + sqrt(1 - R_X))) (1 + u) - 1,  R_X = R_X(beta2)
the last from sqrt(X (1 + r)) = sqrt(X) sqrt(1 + r), |sqrt(1 + r) - 1| <= 1 - sqrt(1 - R) = R / (1 + sqrt(1 - R)), and the root's own rounding.
At step 1 with beta >= 0.5, R1 = 0 and R2 = u.

Clip coefficient  (`clip_coef`; optim_groups.hip:8-13,22-29,42-48)
----------------
The reference coefficient is c = min(1, max_norm / (norm64 |grad_scale| + 1e-6)) in float64, norm64 the float64 L2 norm of g.  The kernels add the n
squares in float64 with fmas (every element passes fewer than n additions whatever the grouping into threads, waves and workgroups), take the root,
two more float64 operations and a division: relative (n / 2 + 4) 2^-53 at most; numpy's own float64 sum is budgeted the same.  The one f32 rounding is
`(float)c` (optim_groups.hip:48):
    R_c = (1 + u) (1 + (n + 8) 2^-53) - 1                 (0 without a clip: coef = 1.f exactly)
Where c is within R_c of 1 the kernel may take either branch of `c < 1.0`; both values are within R_c of the reference's.

Bounds  (`step_reference`; R = relative part, A = absolute part, E = R |x| + A)
------
 gg.   fl(fl(g gs) coef~): two roundings and the coefficient's R_c (one rounding without a coefficient):
         R_g = (1 + u)^k (1 + R_c) - 1, k = 2 or 1;    A_g = T (|c| (1 + R_c) + 1) + T |gs c|;    E_g = R_g |gg| + A_g
 m'.   a = fl(b1 m): u |b1 m| + T (1 + b1).   omb = fl(1 - b1): u.   c = fl(omb~ gg~): ((1 + u)^2 - 1) |c| + (1 - b1) (1 + u)^2 E_g + T.
         E_m = (E_a + E_c) + u (|m'| + E_a + E_c) + T               -- when m' cancels, what is left is u times the two terms: an absolute bound
 v'.   a sum of non-negative terms, so its error is relative apart from the flush terms.  a = fl(b2 v): u a + T (1 + b2).
       c = fl(fl(omb2~ gg~) gg~): relative (1 + u)^3 (1 + R_g)^2 - 1 =: r_c, absolute
         A_c = (1 - b2) (1 + u)^3 (2 |gg| (1 + R_g) A_g + A_g^2) + T (1 + u) (|gg| (1 + R_g) + A_g) + T
       the add:  R_v = (1 + u) (u a + r_c c) / v' + u  (0 where v' = 0),   A_v = (1 + u) (T (1 + b2) + A_c) + T,   E_v = R_v v' + A_v
 root. v~ = v' (1 + r) + a with |r| <= R_v, |a| <= A_v and both arguments non-negative: |sqrt(x + a) - sqrt(x)| <= sqrt(|a|), so
         E_s0 = S R_v / (1 + sqrt(1 - R_v)) + sqrt(A_v),  S = sqrt(v');    E_s = E_s0 + SQRT_REL (S + E_s0) + T
       (sqrt(A_v) is about 1e-19 against eps >= 1e-8.)
 d1 = S / B2.   The kernel divides by bc2_sqrt~ = B2 (1 + r2):  E_d0 = (E_s + S R2) / (B2 (1 - R2));   E_d1 = E_d0 + DIV_REL (d1 + E_d0) + T
 den = d1 + eps.   E_den = E_d1 + u (den + E_d1) + T;  den >= eps > E_den is asserted.
 q = m' / den.   |m~ / den~ - m' / den| = |(m~ - m') den - m' (den~ - den)| / (den den~) <= (E_m + |q| E_den) / (den - E_den) =: E_q0;
         E_q = E_q0 + DIV_REL (|q| + E_q0) + T
 sl = lr / B1.   E_sl0 = |sl| R1 / (1 - R1);   E_sl = E_sl0 + DIV_REL (|sl| + E_sl0) + T
 upd = sl q.   E_u0 = |sl| E_q + |q| E_sl + E_sl E_q;   E_u = E_u0 + u (|upd| + E_u0) + T
 decay.   lw = fl(lr wd): E_lw = u |lr wd| + T.   c = fl(1 - lw~): E_c = E_lw + u (|c| + E_lw) + T.
          pd = fl(p c~): E_pd0 = |p| E_c + T (|c| + E_c);   E_pd = E_pd0 + u (|pd| + E_pd0) + T
 p' = pd - upd, one rounding:   E_p = (E_pd + E_u) + u (|p'| + E_pd + E_u) + T
At lr = 3e-6 and |p| of order 1 the three roundings on p (about 3 u |p|) are several percent of the update: that is f32's resolution of p', not slack
in the derivation; m', v' and the small elements of p carry the discrimination there.

The reference's own float64 arithmetic (unit round-off 2^-53 = u 2^-29) errs, term by term, by 2^-29 of what the bound already holds for the same
operation in f32; every bound is returned times 1 + 2^-28, which also covers the double rounding of an emulation that forms a fused multiply-add in
float64 first.  Nothing is fitted: a result outside a bound has made a rounding that is not counted above, or has used other inputs.

`emulate` is the kernels' expression sequence in f32 numpy, unfused or with the contractions a compiler may pick; it serves the CPU test of the bounds
and is NEVER a reference for the GPU test.  `MUTANTS` names subtly wrong variants of it.  `profile` returns named input regimes.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
U64 = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -28
SQRT_REL = 6.0 * U          # ASSUMPTION 1
DIV_REL = 5.0 * U           # ASSUMPTION 2
POWF_REL = 2.0 * U          # ASSUMPTION 3

PROFILES = ("unit", "fresh", "eps_band", "tiny", "zero_grad", "large", "cancel")
MUTANTS = ("eps_inside_root", "eps_before_bc2", "no_bc2", "bc2_not_rooted", "no_bc1", "decay_after_update", "l2_decay", "beta2_for_m",
           "v_unscaled_grad")


def f32(x) -> float:
    """x rounded to f32, as a Python float: what a `float` argument of the C entries receives."""
    return float(np.float32(x))


# ---- bias corrections ---------------------------------------------------------------------------------------------------------------------------------
def _one_minus_pow(beta, step):
    """-> (X = 1 - beta^t in float64, R_X: the relative allowance of the host's f32 `1.f - powf(beta, (float)t)`)."""
    b, t = f32(beta), int(step)
    assert 0.0 < b < 1.0 and t >= 1
    tf = f32(t)
    P = b ** t
    X = 1.0 - P
    if t == 1:
        EP = 0.0
    else:
        Et = b ** min(t, tf) * abs(tf - t) * abs(math.log(b))
        EP = Et + POWF_REL * (P + Et) + TINY
    Esub = 0.0 if (t == 1 and b >= 0.5) else U * (X + EP)
    return X, (EP + Esub) / X


def bias_corrections(beta1, beta2, step):
    """-> (B1, R1, B2, R2): B1 = 1 - beta1^t, B2 = sqrt(1 - beta2^t) in float64 from the f32 betas; the kernels' f32 bc1 / bc2_sqrt are within the
    relative R1 / R2 of them."""
    X1, R1 = _one_minus_pow(beta1, step)
    X2, RX = _one_minus_pow(beta2, step)
    assert R1 < 1.0 and RX < 1.0
    R2 = (1.0 + RX / (1.0 + math.sqrt(1.0 - RX))) * (1.0 + U) - 1.0
    return X1, R1, math.sqrt(X2), R2


def host_bias_corrections(beta1, beta2, step):
    """f32 (bc1, bc2_sqrt) the way the entries form them, with numpy's f32 power: for `emulate` and the CPU test of the allowance."""
    one, t = np.float32(1.0), np.float32(int(step))
    bc1 = one - np.power(np.float32(beta1), t)
    bc2 = np.sqrt(one - np.power(np.float32(beta2), t))
    assert bc1.dtype == np.float32 and bc2.dtype == np.float32
    return bc1, bc2


# ---- clip coefficient ----------------------------------------------------------------------------------------------------------------------------------
def clip_coef(g, grad_scale, max_norm):
    """-> (c, R_c): the float64 coefficient from the float64 norm of g, and the relative allowance of the kernel's f32 one.  max_norm <= 0: (None, 0)."""
    mn = f32(max_norm)
    if not mn > 0.0:
        return None, 0.0
    g = np.asarray(g)
    assert g.dtype == np.float32
    norm = math.sqrt(float(np.sum(g.astype(np.float64) ** 2))) * abs(f32(grad_scale))
    c = min(1.0, mn / (norm + 1e-6))
    return c, (1.0 + U) * (1.0 + (g.size + 8) * U64) - 1.0


def rows(ends, values, n):
    """The per-element value of a segment table: element i takes the row of the first end above i.  -> f32 array [n]."""
    ends = np.asarray(ends, dtype=np.int64)
    values = np.asarray(values, dtype=np.float32)
    assert ends.shape == values.shape and ends[-1] == n and np.all(np.diff(ends) > 0)
    return values[np.searchsorted(ends, np.arange(n, dtype=np.int64), side="right")]


# ---- the reference step and its bounds ----------------------------------------------------------------------------------------------------------------
def _per_element(x):
    x = np.asarray(x)
    if x.ndim:
        assert x.dtype == np.float32
    return np.float32(x).astype(np.float64) if x.ndim == 0 else x.astype(np.float64)


def step_reference(p, g, m, v, *, lr, wd, beta1, beta2, eps, grad_scale, step, coef=None, coef_rel=0.0):
    """One AdamW step in float64 on the given f32 inputs -> dict: the references `p`, `m`, `v`, their bounds `bound_p`, `bound_m`, `bound_v`, and the
    intermediates `gg`, `sqrt_v`, `denom`, `update`.  lr / wd: f32 scalars or per-element f32 arrays (`rows`); coef / coef_rel: from `clip_coef`."""
    for x in (p, g, m, v):
        assert isinstance(x, np.ndarray) and x.dtype == np.float32
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    assert np.all(v >= 0.0)
    lr, wd = _per_element(lr), _per_element(wd)
    b1, b2, eps, gs = f32(beta1), f32(beta2), f32(eps), f32(grad_scale)
    assert eps > 0.0
    B1, R1, B2, R2 = bias_corrections(b1, b2, step)
    c, k = (1.0, 1) if coef is None else (float(coef), 2)
    T = TINY

    gg = g * gs * c
    Rg = (1.0 + U) ** k * (1.0 + coef_rel) - 1.0
    Ag = T * (abs(c) * (1.0 + coef_rel) + 1.0) + T * abs(gs * c)
    Eg = Rg * np.abs(gg) + Ag

    a, omb = b1 * m, 1.0 - b1
    cm = omb * gg
    m1 = a + cm
    Ea = U * np.abs(a) + T * (1.0 + b1)
    Ec = ((1.0 + U) ** 2 - 1.0) * np.abs(cm) + omb * (1.0 + U) ** 2 * Eg + T
    Em = (Ea + Ec) + U * (np.abs(m1) + Ea + Ec) + T

    av, omb2 = b2 * v, 1.0 - b2
    cv = omb2 * gg * gg
    v1 = av + cv
    rc = (1.0 + U) ** 3 * (1.0 + Rg) ** 2 - 1.0
    agg = np.abs(gg) * (1.0 + Rg)
    Ac = omb2 * (1.0 + U) ** 3 * (2.0 * agg * Ag + Ag * Ag) + T * (1.0 + U) * (agg + Ag) + T
    num = U * av + rc * cv
    Rv = (1.0 + U) * np.divide(num, v1, out=np.zeros_like(v1), where=v1 > 0.0) + U
    Rv = np.where(v1 > 0.0, Rv, 0.0)
    Av = (1.0 + U) * (T * (1.0 + b2) + Ac) + T
    Ev = Rv * v1 + Av

    S = np.sqrt(v1)
    Es0 = S * Rv / (1.0 + np.sqrt(1.0 - Rv)) + np.sqrt(Av)
    Es = Es0 + SQRT_REL * (S + Es0) + T
    d1 = S / B2
    Ed0 = (Es + S * R2) / (B2 * (1.0 - R2))
    Ed1 = Ed0 + DIV_REL * (d1 + Ed0) + T
    den = d1 + eps
    Eden = Ed1 + U * (den + Ed1) + T
    assert np.all(Eden < den)
    q = m1 / den
    Eq0 = (Em + np.abs(q) * Eden) / (den - Eden)
    Eq = Eq0 + DIV_REL * (np.abs(q) + Eq0) + T
    sl = lr / B1
    Esl0 = np.abs(sl) * R1 / (1.0 - R1)
    Esl = Esl0 + DIV_REL * (np.abs(sl) + Esl0) + T
    upd = sl * q
    Eu0 = np.abs(sl) * Eq + np.abs(q) * Esl + Esl * Eq
    Eu = Eu0 + U * (np.abs(upd) + Eu0) + T

    lw = lr * wd
    Elw = U * np.abs(lw) + T
    cd = 1.0 - lw
    Ecd = Elw + U * (np.abs(cd) + Elw) + T
    pd = p * cd
    Epd0 = np.abs(p) * Ecd + T * (np.abs(cd) + Ecd)
    Epd = Epd0 + U * (np.abs(pd) + Epd0) + T
    p1 = pd - upd
    Ep = (Epd + Eu) + U * (np.abs(p1) + Epd + Eu) + T

    return dict(p=p1, m=m1, v=v1, bound_p=Ep * SLACK, bound_m=Em * SLACK, bound_v=Ev * SLACK, gg=gg, sqrt_v=S, denom=den, update=upd)


def miss_factor(got, ref, bound):
    """max |got - ref| / bound over EVERY element (no exclusions): at most 1 inside the bound.  bound >= T > 0; a NaN in `got` gives NaN, which fails
    `<= 1`."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == bound.shape and np.all(bound > 0.0)
    return float(np.max(np.abs(got - ref) / bound))


def miss_factors(got_p, got_m, got_v, ref):
    """-> {"p": .., "m": .., "v": ..} of one step against `step_reference`'s dict."""
    return {k: miss_factor(x, ref[k], ref["bound_" + k]) for k, x in (("p", got_p), ("m", got_m), ("v", got_v))}


# ---- f32 emulations (CPU test only) -------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl(a b + c) for f32 operands: the product is exact in float64 (24 x 24 bits); the sum is rounded to float64, then to f32."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    return (a * b + c).astype(np.float32)


def emulate(p, g, m, v, *, lr, wd, beta1, beta2, eps, grad_scale, bc1, bc2_sqrt, coef=None, contracted=False, mutant=None):
    """The kernels' expression sequence in f32 numpy, in the order the source writes it -> (p', m', v') f32.  contracted=False: every operation
    rounded; True: b1 m, b2 v, lr wd and the final product fused into the add that consumes them.  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    F = np.float32
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    lr, wd = np.asarray(lr, dtype=F), np.asarray(wd, dtype=F)
    b1, b2, eps, gs, bc1, bc2 = F(beta1), F(beta2), F(eps), F(grad_scale), F(bc1), F(bc2_sqrt)
    one = F(1.0)
    gg = g * gs
    if coef is not None:
        gg = gg * F(coef)
    if mutant == "l2_decay":
        gg = gg + wd * p
        dec = one
    else:
        dec = _fma(-lr, wd, one) if contracted else one - lr * wd
    pd = p if mutant == "decay_after_update" else p * dec
    bm = b2 if mutant == "beta2_for_m" else b1
    gv = g if mutant == "v_unscaled_grad" else gg
    if contracted:
        m1 = _fma(bm, m, (one - bm) * gg)
        v1 = _fma(b2, v, (one - b2) * gv * gv)
    else:
        m1 = bm * m + (one - bm) * gg
        v1 = b2 * v + (one - b2) * gv * gv
    if mutant == "eps_inside_root":
        den = np.sqrt(v1 + eps) / bc2
    elif mutant == "eps_before_bc2":
        den = (np.sqrt(v1) + eps) / bc2
    elif mutant == "no_bc2":
        den = np.sqrt(v1) + eps
    elif mutant == "bc2_not_rooted":
        den = np.sqrt(v1) / (bc2 * bc2) + eps
    else:
        den = np.sqrt(v1) / bc2 + eps
    sl = lr if mutant == "no_bc1" else lr / bc1
    q = m1 / den
    p1 = _fma(-sl, q, pd) if contracted else pd - sl * q
    if mutant == "decay_after_update":
        p1 = p1 * dec
    for x in (p1, m1, v1):
        assert x.dtype == F
    return p1, m1, v1


# ---- input profiles ----------------------------------------------------------------------------------------------------------------------------------
def profile(name, n, seed=0, beta1=0.9, scale=1.0):
    """-> (p, g, m, v) f32 [n].  p is of order 1 everywhere.  beta1 / scale (= grad_scale coef) shape `cancel` only."""
    rng = np.random.default_rng([seed, PROFILES.index(name)])
    F = np.float32
    p = rng.standard_normal(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)

    def band(lo, hi):          # |g| log-uniform over 10^lo .. 10^hi, v within a decade of g^2, m within |g|
        g = sign * 10.0 ** rng.uniform(lo, hi, n)
        return g, g * rng.uniform(-1.0, 1.0, n), g * g * 10.0 ** rng.uniform(-1.0, 1.0, n)

    if name == "unit":
        g, m, v = rng.standard_normal(n), 0.1 * rng.standard_normal(n), (0.1 * rng.standard_normal(n)) ** 2
    elif name == "fresh":
        g, m, v = rng.standard_normal(n), np.zeros(n), np.zeros(n)
    elif name == "eps_band":          # sqrt(v^) below, around and above eps
        g, m, v = band(-12.0, -4.0)
    elif name == "tiny":              # g^2 underflows, some v are subnormal or zero
        g, m, v = band(-30.0, -15.0)
    elif name == "zero_grad":         # a warm state with g = 0; a quarter cold: 0 / eps
        g, m, v = np.zeros(n), 0.1 * rng.standard_normal(n), (0.1 * rng.standard_normal(n)) ** 2
        cold = np.arange(n) % 4 == 1
        m[cold], v[cold] = 0.0, 0.0
    elif name == "large":
        g, m, v = band(0.0, 17.0)
    elif name == "cancel":            # m' = b1 m + (1 - b1) gg cancels to rounding
        g = rng.standard_normal(n)
        b1 = float(F(beta1))
        m, v = -(g.astype(F).astype(np.float64) * scale) * (1.0 - b1) / b1, (0.1 * rng.standard_normal(n)) ** 2
    else:
        raise ValueError(f"profile: unknown name {name!r} (one of {PROFILES})")
    return p.astype(F), g.astype(F), m.astype(F), v.astype(F)
