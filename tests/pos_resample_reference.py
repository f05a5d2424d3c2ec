"""Float64 reference, derived error bounds and an f32 simulation for csrc/pos_resample.hip (owl_pos_resample, owl_pos_resample_bwd): the position table
[g0 g0 + 1, D] resampled to another grid g, and the adjoint.  Checker side; nothing here imports the package's Python ops.

Reference (float64, tap-matrix form)
---------
Per axis, output index o has source coordinate s = (o + 0.5) g0 / g - 0.5 = num / den with num = (2 o + 1) g0 - g, den = 2 g (integers, so f = floor(s)
and t = s - f = r / den are exact rationals), taps f - 1 .. f + 2 clamped to [0, g0 - 1] and cubic-convolution weights with A = -0.75:
    w0 = c2(t + 1), w1 = c1(t), w2 = c1(1 - t), w3 = c2(2 - t),   c1(x) = ((A + 2) x - (A + 3)) x x + 1,   c2(x) = ((A x - 5 A) x + 8 A) x - 4 A.
`tap_matrix(g0, g)` is M [g, g0] with M[o, c] = the sum of the weights of o whose clamped tap is c; the patch rows of the used table are
(M (x) M) pos_patch, row 0 (the class token) is copied: `forward64`.  `adjoint64` applies the transpose.  test_pos_resample_reference.py holds both to
torch.nn.functional.interpolate(mode="bicubic", align_corners=False) and its autograd in float64.  `variant=` builds the WRONG tables the bound must
reject: "a05" (A = -0.5), "align" (align_corners=True), "reflect" (taps mirrored at the border instead of clamped).

Bounds (elementwise, derived from the kernels' evaluation order; u, F, TINY, gamma(n) are gemm_reference's, `_V` is layernorm_reference's
value-with-error: every operation charges the propagated error of its operands plus ONE rounding of its result)
------
The kernels are compiled with contraction off and write their multiply-adds as fmaf, so the count below is the code's (pos_resample.hip: axis_taps).
 t = fl(r / den), r and den exact integers below 2^24.  ASSUMPTION: the f32 division is within 1 ulp (2 F relative); HIP's default is the correctly
   rounded one (0.5 ulp), so this is the conservative reading.                                                                         1 rounding
 x0 = t + 1, u = 1 - t, x3 = 2 - t                                                                                                    1 rounding each
 w0, w3: ((A x + 3.75) x - 6) x + 3: mul, add, mul, sub, mul, add                                                                      6 roundings
 w1, w2: ((1.25 x - 2.25) x) x + 1: mul, sub, mul, mul, add                                                                            5 roundings
   -> at most 8 roundings on the path of a weight; every constant is exact in f32.  `axis_weights` carries them through `_V`: w known to E_w.
 forward, per output element: 16 terms in (i outer, j inner) order, each w_ij = fl(wy_i wx_j) (1 rounding) and acc = fmaf(w_ij, p, acc) (1 rounding):
   |w~_ij| <= (1 + F) a_i b_j with a = |wy| + E_wy, b = |wx| + E_wx, and E_ij = (1 + F) a_i b_j - |wy_i wx_j|, so
       tol = sum_ij |p_ij| (E_ij + gamma(16) (|w_ij| + E_ij)) = (1 + gamma(16)) (1 + F) (Ma (x) Mb) |pos| - (M|w| (x) M|w|) |pos|      (+ T)
   with Ma the tap matrix built from a (clamped taps add up).  The class row is a copy: tol = 0.
 backward, per source cell: per axis m(o) = the weights of o on the cell added in tap order (k taps: k - 1 adds),
       E_m = sum E_w + gamma(k - 1) sum (|w| + E_w),      a' = |m| + E_m;
   then n = ny nx terms (the rectangle of output cells that touch the cell: `touch_counts`), each fl(my mx) and one fmaf, and ONE add onto the
   value already there: n + 1 roundings on the chain,
       tol = (1 + gamma(n + 1)) (1 + F) (A'^T (x) A'^T) |dU| - (|M|^T (x) |M|^T) |dU| + gamma(n + 1) |old|                               (+ T)
   The class row is old + dU[0]: one rounding, tol = gamma(1) (|dU[0]| + |old[0]|).

`emulate_fwd` / `emulate_bwd` run the kernels' arithmetic in f32 in the order the source writes it (and `touch_range` restates the backward's integer
range formula); they serve the CPU test only and are NEVER a reference on the GPU.
"""
import torch

from tests.gemm_reference import F, TINY, check, gamma as gam, ratios  # noqa: F401
from tests.layernorm_reference import _V

A = -0.75
DIV_ULPS = 1.0            # ASSUMPTION (module docstring)
N_FWD = 16                # fmaf statements of one output element
# the pairs (g0, g) of the CPU test and the shapes (g0, g, D) of the GPU test (the issue's lists)
PAIRS = ((6, 8), (6, 10), (6, 4), (6, 5), (3, 7), (2, 5), (1, 4), (24, 30))
GPU_SHAPES = ((6, 8, 128), (6, 5, 128), (6, 4, 128), (3, 7, 64), (2, 5, 64), (1, 4, 64), (24, 30, 768), (7, 10, 1024))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _c1(x, a):
    return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0


def _c2(x, a):
    return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a


def taps64(g0, g, variant=None):
    """-> idx [g, 4] int64 (border rule applied), w [g, 4] float64, t [g] float64."""
    o = torch.arange(g, dtype=torch.int64)
    if variant == "align":
        s = o.double() * ((g0 - 1) / (g - 1)) if g > 1 else torch.zeros(g, dtype=torch.float64)
        f = torch.floor(s).long()
        t = s - f.double()
    else:
        num, den = (2 * o + 1) * g0 - g, 2 * g
        f = torch.div(num, den, rounding_mode="floor")
        t = (num - f * den).double() / den
    a = -0.5 if variant == "a05" else A
    w = torch.stack([_c2(t + 1.0, a), _c1(t, a), _c1(1.0 - t, a), _c2(2.0 - t, a)], 1)
    raw = f[:, None] - 1 + torch.arange(4)
    if variant == "reflect":
        if g0 < 2:
            raise ValueError("a one-cell table has nothing to reflect")
        period = 2 * (g0 - 1)
        m = raw % period
        idx = torch.where(m < g0, m, period - m)
    else:
        idx = raw.clamp(0, g0 - 1)
    return idx, w, t


def _scatter(idx, val, g0):
    """[g, g0] with out[o, idx[o, i]] += val[o, i]."""
    out = torch.zeros(idx.shape[0], g0, dtype=torch.float64)
    out.scatter_add_(1, idx, val)
    return out


def tap_matrix(g0, g, variant=None):
    idx, w, _ = taps64(g0, g, variant)
    return _scatter(idx, w, g0)


def _kron_apply(My, Mx, pos, g0):
    """patch rows [g0 g0, D] -> (My (x) Mx) rows [gy gx, D]."""
    D = pos.shape[-1]
    return torch.einsum("yi,xj,ijd->yxd", My, Mx, pos.reshape(g0, g0, D)).reshape(-1, D)


def forward64(pos, g0, g, variant=None):
    """pos [g0 g0 + 1, D] -> U [g g + 1, D] float64."""
    pos = pos.double()
    M = tap_matrix(g0, g, variant)
    return torch.cat([pos[:1], _kron_apply(M, M, pos[1:], g0)], 0)


def adjoint64(dU, g0, g):
    """dU [g g + 1, D] -> K^T dU [g0 g0 + 1, D] float64."""
    dU = dU.double()
    Mt = tap_matrix(g0, g).t().contiguous()
    return torch.cat([dU[:1], _kron_apply(Mt, Mt, dU[1:], g)], 0)


def abs_sum(pos, g0, g):
    """sum over the 16 taps of |w| |pos| per output element (the class row: |pos[0]|)."""
    idx, w, _ = taps64(g0, g)
    Mw = _scatter(idx, w.abs(), g0)
    pa = pos.double().abs()
    return torch.cat([pa[:1], _kron_apply(Mw, Mw, pa[1:], g0)], 0)


def touch_counts(g0, g):
    """per source index on one axis: how many output indices have a clamped tap on it."""
    idx, w, _ = taps64(g0, g)
    return (_scatter(idx, torch.ones_like(w), g0) > 0).sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def axis_weights(g0, g):
    """-> idx [g, 4], w [g, 4] float64, E_w [g, 4]: the bound of the f32 weights of axis_taps (module docstring)."""
    idx, w, t = taps64(g0, g)
    c = lambda v: _V(torch.full_like(t, v))
    tv = _V(t, DIV_ULPS * 2.0 * F * t.abs() + TINY)
    x0, u, x3 = tv + c(1.0), c(1.0) - tv, c(2.0) - tv
    outer = lambda x: ((c(-0.75) * x + c(3.75)) * x - c(6.0)) * x + c(3.0)
    inner = lambda x: ((c(1.25) * x - c(2.25)) * x) * x + c(1.0)
    ws = [outer(x0), inner(tv), inner(u), outer(x3)]
    assert float((torch.stack([v.v for v in ws], 1) - w).abs().max()) < 1e-14          # the same polynomials as taps64
    return idx, w, torch.stack([v.E for v in ws], 1)


def bound_fwd(pos, g0, g):
    """tolerance [g g + 1, D] of owl_pos_resample against forward64 on the same f32 table."""
    idx, w, E = axis_weights(g0, g)
    Ma, Mw = _scatter(idx, w.abs() + E, g0), _scatter(idx, w.abs(), g0)
    pa = pos.double().abs()
    tol = (1.0 + gam(N_FWD)) * (1.0 + F) * _kron_apply(Ma, Ma, pa[1:], g0) - _kron_apply(Mw, Mw, pa[1:], g0) + TINY * (1.0 + 17.0 * float(pa.max()))
    return torch.cat([torch.zeros_like(pa[:1]), tol], 0)


def bound_bwd(dU, old, g0, g):
    """tolerance [g0 g0 + 1, D] of owl_pos_resample_bwd against old + adjoint64(dU) (`old`: dpos before the call)."""
    idx, w, E = axis_weights(g0, g)
    k = _scatter(idx, torch.ones_like(w), g0)                                   # taps of o on the cell
    M = _scatter(idx, w, g0)
    Em = _scatter(idx, E, g0) + gam((k - 1.0).clamp_min(0.0)) * _scatter(idx, w.abs() + E, g0)
    At, Mt = (M.abs() + Em).t().contiguous(), M.abs().t().contiguous()
    cnt = touch_counts(g0, g).double()
    n = (cnt[:, None] * cnt[None, :]).reshape(-1, 1) + 1.0                        # roundings on the chain of a source cell
    da, oa = dU.double().abs(), old.double().abs()
    tol = (1.0 + gam(n)) * (1.0 + F) * _kron_apply(At, At, da[1:], g) - _kron_apply(Mt, Mt, da[1:], g) + gam(n) * oa[1:] \
        + TINY * (1.0 + 2.0 * float(n.max()) * float(da.max()))
    return torch.cat([gam(1) * (da[:1] + oa[:1]) + TINY, tol], 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate_taps(g0, g):
    """axis_taps in f32 for every o: idx [g, 4], w [g, 4] float32."""
    o = torch.arange(g, dtype=torch.int64)
    num, den = (2 * o + 1) * g0 - g, 2 * g
    f = torch.div(num, den, rounding_mode="floor")
    t = (num - f * den).float() / torch.tensor(float(den), dtype=torch.float32)
    one, two = torch.tensor(1.0), torch.tensor(2.0)
    x0, u, x3 = t + one, one - t, two - t
    outer = lambda x: ((-0.75 * x + 3.75) * x - 6.0) * x + 3.0
    inner = lambda x: ((1.25 * x - 2.25) * x) * x + 1.0
    w = torch.stack([outer(x0), inner(t), inner(u), outer(x3)], 1)
    assert w.dtype == torch.float32
    return (f[:, None] - 1 + torch.arange(4)).clamp(0, g0 - 1), w


def emulate_fwd(pos, g0, g, hooks=()):
    """pos_resample_kernel.  hooks: "skip_last_tap" (the 16th term dropped)."""
    pos = pos.float()
    D = pos.shape[1]
    idx, w = emulate_taps(g0, g)
    patch = pos[1:].reshape(g0, g0, D)
    acc = torch.zeros(g, g, D, dtype=torch.float32)
    for i in range(4):
        for j in range(4):
            if "skip_last_tap" in hooks and i == 3 and j == 3:
                continue
            wij = (w[:, None, i] * w[None, :, j])[..., None]
            acc = _fma32(wij.expand_as(acc), patch[idx[:, i]][:, idx[:, j]], acc)
    return torch.cat([pos[:1], acc.reshape(g * g, D)], 0)


def _floor_div(a, b):
    return a // b          # Python's // floors


def first_with_floor(Fl, g0, g):
    q = -_floor_div(-(2 * g * Fl + g), g0)
    return max(_floor_div(q, 2), 0)


def touch_range(s, g0, g):
    """pos_resample.hip touch_range: the output indices [lo, hi] whose clamped taps reach source index s."""
    lo = 0 if s == 0 else min(first_with_floor(s - 2, g0, g), g)
    hi = g - 1 if s == g0 - 1 else min(first_with_floor(s + 2, g0, g), g) - 1
    return lo, hi


def emulate_bwd(dU, old, g0, g, hooks=()):
    """pos_resample_bwd_kernel on old (accumulated into).  hooks: "overwrite" (= instead of +=)."""
    dU, out = dU.float(), old.float().clone()
    D = dU.shape[1]
    idx, w = emulate_taps(g0, g)
    rows = dU[1:].reshape(g, g, D)

    def m_on(o, s):
        m = torch.tensor(0.0)
        for i in range(4):
            if int(idx[o, i]) == s:
                m = m + w[o, i]
        return m

    out[0] = dU[0] if "overwrite" in hooks else out[0] + dU[0]
    ranges = [touch_range(s, g0, g) for s in range(g0)]
    ms = [{o: m_on(o, s) for o in range(ranges[s][0], ranges[s][1] + 1)} for s in range(g0)]
    for sy in range(g0):
        for sx in range(g0):
            acc = torch.zeros(D, dtype=torch.float32)
            for y, my in ms[sy].items():
                for x, mx in ms[sx].items():
                    acc = _fma32((my * mx).expand(D), rows[y, x], acc)
            c = 1 + sy * g0 + sx
            out[c] = acc if "overwrite" in hooks else out[c] + acc
    return out


def make_case(g0, g, D, seed=0):
    """Seeded inputs on the CPU: pos [g0 g0 + 1, D], dU [g g + 1, D], old [g0 g0 + 1, D] (non-zero: the backward accumulates), all f32.  The table has the
    scale of a trained one (std 0.02) with a few sink-like outliers of 60 (weights.TRAINED_LIKE) -- a tolerance relative to max |pos| would hide the rest."""
    gen = torch.Generator(device="cpu").manual_seed(1000003 * seed + 10007 * g0 + 101 * g + D)
    pos = 0.02 * torch.randn(g0 * g0 + 1, D, generator=gen)
    pos[1 + (g0 * g0) // 2, D // 3] = 60.0
    pos[g0 * g0, D - 1] = -60.0
    dU = torch.randn(g * g + 1, D, generator=gen)
    old = torch.randn(g0 * g0 + 1, D, generator=gen) * float(g) / float(g0)
    return pos.float(), dU.float(), old.float()
