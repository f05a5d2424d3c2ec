"""Kernel forms that only model-sized calls reach, each against a float64 reference of the same operation.

Several kernels choose their code at launch time from D, from the row count or from which pointers are null, and the per-kernel suite
(test_kernels_gpu.py) mostly runs them at shapes that pick the small forms.  Every test below names the form it targets and the reason its
shape reaches that form; the references are float64 (on the device, or on sampled rows where the full product is large)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops, rng  # noqa: E402
from tests import gemm_reference  # noqa: E402

DEV = "cuda"


def report(name, got, ref, atol, rtol):
    """Fail with the first offending indices if |got - ref| > atol + rtol |ref| anywhere (atol may be a tensor broadcast against ref)."""
    got = got.double(); ref = ref.double()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = ~(err <= tol)
    if bad.any():
        idx = bad.nonzero()[:8].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} off; max err {float(err[~err.isnan()].max()) if (~err.isnan()).any() else float('nan'):.4g} "
                             f"(ref max {float(ref.abs().max()):.4g}); first bad idx {idx}; got {got[bad][:4].tolist()} ref {ref[bad][:4].tolist()}")


def randn(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. box_final forward
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _box_final_rpw(rows):
    """Rows per wave, as owl_box_final_fwd chooses it (heads.hip)."""
    return min(max((rows + 4095) // 4096, 1), 16)


def _box_final_exits(rows):
    """How the waves of a launch leave box_final_rows_kernel's 3-row loop: 'break1' (r + 1 >= row1), 'break2' (r + 2 >= row1) or 'cond'."""
    rpw = _box_final_rpw(rows)
    counts = {rpw} if rows >= rpw else set()
    if rows % rpw:
        counts.add(rows % rpw)
    return {("cond", "break1", "break2")[n % 3] for n in counts}


BOX_ROWS = [1, 2304, 4097, 8195, 12290, 57600, 73728]


def test_box_final_row_counts_reach_every_form():
    """The row counts of test_box_final_forward_model_forms give rows per wave 1, 2, 3, 4, 15 and 16 and leave the 3-row loop by each of its exits."""
    assert {_box_final_rpw(r) for r in BOX_ROWS} == {1, 2, 3, 4, 15, 16}
    assert set().union(*(_box_final_exits(r) for r in BOX_ROWS)) == {"cond", "break1", "break2"}


def _box_final_ref(h, w2, b2, bb, rows, P):
    s = torch.sigmoid(h[:rows].double() @ w2.double().t() + b2.double() + bb.double()[torch.arange(rows, device=DEV) % P])
    return s, torch.stack([s[:, 0] - 0.5 * s[:, 2], s[:, 1] - 0.5 * s[:, 3], s[:, 0] + 0.5 * s[:, 2], s[:, 1] + 0.5 * s[:, 3]], -1)


@pytest.mark.parametrize("P", [2304, 3600])
@pytest.mark.parametrize("rows", BOX_ROWS)
@pytest.mark.parametrize("D", [128, 512, 520, 768, 1024])
def test_box_final_forward_model_forms(D, rows, P):
    """box_final_rows_kernel<1> (D <= 512; 512 is its last width) and <2> (D = 520: only lane 0 live in the second 512-wide chunk; D = 768 / 1024:
    the model's widths), at rows per wave 1 .. 16 (rpw = ceil(rows / 4096) capped at 16; 73 728 = B/16 batch 32, 57 600 = L/14 batch 16) with
    waves that leave the 3-row pipeline by each exit (test_box_final_row_counts_reach_every_form).  sig and boxes against float64
    sigmoid(h W2^T + b2 + box_bias[r % P]) -> xyxy; rows past `rows` untouched."""
    seed = D * 7 + rows + P
    h = randn(rows, D, seed=seed, dtype=torch.bfloat16)
    w2 = randn(4, D, seed=seed + 1, scale=1.0 / math.sqrt(D)); b2 = randn(4, seed=seed + 2, scale=0.5); bb = randn(P, 4, seed=seed + 3)
    extra = 64
    boxes = torch.full((rows + extra, 4), 7.0, device=DEV); sig = torch.full((rows + extra, 4), -3.0, device=DEV)
    ops.box_final(h, w2, b2, bb, boxes, sig, rows, P, D)
    s, ref = _box_final_ref(h, w2, b2, bb, rows, P)
    report(f"box_final sig D={D} rows={rows}", sig[:rows], s, 1e-6, 1e-6)
    report(f"box_final boxes D={D} rows={rows}", boxes[:rows], ref, 2e-6, 1e-6)
    assert bool((boxes[rows:] == 7.0).all()) and bool((sig[rows:] == -3.0).all()), "box_final wrote past its rows"


@pytest.mark.parametrize("D", [768, 1024])
def test_box_final_batch_rows_carry_their_batch1_bits(D):
    """Batch independence (README): at rows = 32 x 2304 (rpw = 16, many rows per wave) the rows of image b hold exactly the bits of a separate
    rows = 2304 call (rpw = 1) on image b alone."""
    P, B = 2304, 32
    rows = B * P
    h = randn(rows, D, seed=D, dtype=torch.bfloat16)
    w2 = randn(4, D, seed=D + 1, scale=1.0 / math.sqrt(D)); b2 = randn(4, seed=D + 2, scale=0.5); bb = randn(P, 4, seed=D + 3)
    boxes = torch.zeros(rows, 4, device=DEV); sig = torch.zeros(rows, 4, device=DEV)
    ops.box_final(h, w2, b2, bb, boxes, sig, rows, P, D)
    for b in (0, 1, 17, 31):
        hb = h[b * P:(b + 1) * P].contiguous()
        bx1 = torch.zeros(P, 4, device=DEV); sg1 = torch.zeros(P, 4, device=DEV)
        ops.box_final(hb, w2, b2, bb, bx1, sg1, P, P, D)
        assert torch.equal(boxes[b * P:(b + 1) * P], bx1) and torch.equal(sig[b * P:(b + 1) * P], sg1), f"image {b}: batch bits differ from batch-1 bits"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [73984, 57728, 1001])
@pytest.mark.parametrize("bf16_dy", [True, False], ids=["dy_bf16", "dy_f32"])
@pytest.mark.parametrize("D", [768, 1024, 128])
def test_layernorm_bwd_model_forms(D, bf16_dy, rows):
    """owl_layernorm_bwd in every form it has at the model's widths and row counts (73 984 = B/16 batch 32 x 2312, 57 728 = L/14 batch 16 x 3608,
    1001: a ragged last 64-row block):
    - parameter-only (dx = None: ln_bwd_kernel_768<*, false, false> at D = 768, ln_bwd_kernel<*, false, 4, false> at 1024, <*, false, 0, false> at 128),
      the trainable layer's LN1 on every step;
    - full (dx + bf16 copy + residual gradient: ln_bwd_kernel_768<*, false, true>, ln_bwd_kernel<*, false, 4 | 0, true>);
    - column-sum (bf16 dy only: ln_bwd_kernel<true, true, 3 | 4 | 0, true>).
    dgamma / dbeta accumulate onto nonzero buffers; everything against float64 autograd of F.layer_norm.  The parameter-only form must give the
    full form's dgamma / dbeta bits: ln_bwd_body forms them identically in both, contraction off."""
    g = torch.Generator(device=DEV).manual_seed(rows + D + bf16_dy)
    x = torch.randn(ops.pad_rows(rows), D, device=DEV, generator=g) * 2 + 0.3
    gamma = torch.randn(D, device=DEV, generator=g); beta = torch.randn(D, device=DEV, generator=g)
    dy = torch.randn(ops.pad_rows(rows), D, device=DEV, generator=g) * 0.1
    if bf16_dy:
        dy = dy.bfloat16()
    dres = torch.randn(ops.pad_rows(rows), D, device=DEV, generator=g) * 0.05
    h = torch.zeros(ops.pad_rows(rows), D, device=DEV, dtype=torch.bfloat16); stats = torch.zeros(ops.pad_rows(rows), 2, device=DEV)
    ops.layernorm(x, gamma, beta, h, rows, D, stats)
    # float64 reference
    xr = x[:rows].double().requires_grad_(True); gr = gamma.double().requires_grad_(True); br = beta.double().requires_grad_(True)
    dyd = dy[:rows].double()
    F.layer_norm(xr, (D,), gr, br, 1e-5).backward(dyd)
    with torch.no_grad():
        xhat = (xr - xr.mean(-1, keepdim=True)) * torch.rsqrt(xr.var(-1, unbiased=False, keepdim=True) + 1e-5)
        # f32 partial sums over many rows: the tolerance scales with the column sums of |term|
        tol_g = 2e-6 * (dyd * xhat).abs().sum(0) + 1e-6
        tol_b = 2e-6 * dyd.abs().sum(0) + 1e-6
        want_dx = xr.grad + dres[:rows].double()
        tol_cs = 2e-6 * want_dx.abs().sum(0) + 1e-6
    del xhat
    g0 = torch.linspace(-0.5, 0.75, D, device=DEV); b0 = torch.linspace(1.0, -0.25, D, device=DEV)

    # parameter-only form
    dg_p = g0.clone(); db_p = b0.clone()
    ops.layernorm_bwd(dy, x, stats, gamma, None, None, dg_p, db_p, rows, D)
    report(f"ln_bwd param-only dgamma D={D}", dg_p.double() - g0.double(), gr.grad, tol_g, 0.0)
    report(f"ln_bwd param-only dbeta D={D}", db_p.double() - b0.double(), br.grad, tol_b, 0.0)

    # full form: dx (+ residual gradient), its bf16 copy, dgamma / dbeta
    dx = torch.zeros_like(x); dxb = torch.zeros_like(h)
    dg_f = g0.clone(); db_f = b0.clone()
    ops.layernorm_bwd(dy, x, stats, gamma, dres, dx, dg_f, db_f, rows, D, dx_bf16=dxb)
    report(f"ln_bwd full dx D={D}", dx[:rows], want_dx, 1e-5 * float(want_dx.abs().max()), 1e-5)
    assert torch.equal(dxb[:rows], dx[:rows].bfloat16())
    assert float(dx[rows:].abs().max()) == 0.0 if dx.shape[0] > rows else True
    report(f"ln_bwd full dgamma D={D}", dg_f.double() - g0.double(), gr.grad, tol_g, 0.0)
    report(f"ln_bwd full dbeta D={D}", db_f.double() - b0.double(), br.grad, tol_b, 0.0)
    assert torch.equal(dg_p, dg_f) and torch.equal(db_p, db_f), \
        f"parameter-only and full forms disagree in the bits of dgamma / dbeta (max |d| {float((dg_p - dg_f).abs().max()):.3g} / {float((db_p - db_f).abs().max()):.3g})"

    # column-sum form (the trainable layer's LN2: needs a bf16 dy)
    if bf16_dy:
        dx2 = torch.zeros_like(x); dxb2 = torch.zeros_like(h)
        dg_c = g0.clone(); db_c = b0.clone(); cs = torch.full((D,), 2.0, device=DEV)
        ops.layernorm_bwd(dy, x, stats, gamma, dres, dx2, dg_c, db_c, rows, D, dx_bf16=dxb2, dx_colsum=cs)
        report(f"ln_bwd colsum-form dx D={D}", dx2[:rows], want_dx, 1e-5 * float(want_dx.abs().max()), 1e-5)
        assert torch.equal(dxb2[:rows], dx2[:rows].bfloat16())
        report(f"ln_bwd colsum-form dgamma D={D}", dg_c.double() - g0.double(), gr.grad, tol_g, 0.0)
        report(f"ln_bwd colsum-form dbeta D={D}", db_c.double() - b0.double(), br.grad, tol_b, 0.0)
        report(f"ln_bwd colsum-form colsum(dx) D={D}", cs.double() - 2.0, want_dx.sum(0), tol_cs, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. merge_ln forward
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "with_delta"])
@pytest.mark.parametrize("B,P,D", [(32, 2304, 768), (16, 3600, 1024), (3, 100, 768), (1, 67, 1024)])
def test_merge_ln_forward_model_shapes(B, P, D, fused):
    """cls_ln_kernel + merge_ln_kernel (owl_merge_ln_fwd: every forward, the input of both heads) at the model's widths and token counts
    (32 x 2304 at 768 = B/16 batch 32, 16 x 3600 at 1024 = L/14 batch 16; 1 x 67: B P % 4 != 0, a partly empty last workgroup), with and
    without the fused final residual add.  feats (bf16), cls_ln, stats1 over every token, stats2 and x_out against float64; the pad rows
    t in [T, Tp) hold NaN and are neither read into any result nor written."""
    T = P + 1; Tp = (T + 7) // 8 * 8
    assert Tp > T
    seed = B * 131 + P + D + fused
    x = torch.full((B * Tp, D), float("nan"), device=DEV); xv = x.view(B, Tp, D)
    xv[:, :T] = randn(B, T, D, seed=seed, scale=1.5) + 0.2
    g1 = 1 + 0.1 * randn(D, seed=seed + 1); b1 = 0.1 * randn(D, seed=seed + 2); g2 = 1 + 0.1 * randn(D, seed=seed + 3); b2 = 0.1 * randn(D, seed=seed + 4)
    cls_ln = torch.zeros(B, D, device=DEV)
    feats = torch.full((ops.pad_rows(B * P) + 8, D), 5.0, device=DEV, dtype=torch.bfloat16)
    s1 = torch.full((B * Tp, 2), -9.0, device=DEV); s2 = torch.full((B * P + 8, 2), -9.0, device=DEV)
    xs = xv[:, :T].double()
    if fused:
        delta = torch.full((B * Tp, D), float("nan"), device=DEV, dtype=torch.bfloat16)
        delta.view(B, Tp, D)[:, :T] = randn(B, T, D, seed=seed + 5, scale=0.3, dtype=torch.bfloat16)
        xo = torch.full_like(x, -7.0)
        ops.merge_ln(x, g1, b1, g2, b2, cls_ln, feats, s1, s2, B, P, Tp, D, delta=delta, x_out=xo)
        xs = xs + delta.view(B, Tp, D)[:, :T].double()
        xov = xo.view(B, Tp, D)
        assert torch.equal(xov[:, :T], xs.float()), "x_out != x + delta"
        assert bool((xov[:, T:] == -7.0).all()), "x_out pad rows written"
    else:
        ops.merge_ln(x, g1, b1, g2, b2, cls_ln, feats, s1, s2, B, P, Tp, D)
    mean1 = xs.mean(-1); rstd1 = torch.rsqrt(xs.var(-1, unbiased=False) + 1e-5)
    y = (xs - mean1[..., None]) * rstd1[..., None] * g1.double() + b1.double()
    z = y[:, 1:] * y[:, :1]
    mean2 = z.mean(-1); rstd2 = torch.rsqrt(z.var(-1, unbiased=False) + 1e-5)
    ref = (z - mean2[..., None]) * rstd2[..., None] * g2.double() + b2.double()
    report("merge_ln feats", feats[:B * P].view(B, P, D), ref, 1e-4, 2.0 ** -7)
    report("merge_ln cls_ln", cls_ln, y[:, 0], 1e-5, 1e-5)
    s1v = s1.view(B, Tp, 2)
    report("merge_ln stats1 mean", s1v[:, :T, 0], mean1, 1e-5, 1e-5)
    report("merge_ln stats1 rstd", s1v[:, :T, 1], rstd1, 0.0, 1e-5)
    report("merge_ln stats2 mean", s2[:B * P, 0].view(B, P), mean2, 1e-5, 1e-5)
    report("merge_ln stats2 rstd", s2[:B * P, 1].view(B, P), rstd2, 0.0, 1e-5)
    assert bool((s1v[:, T:] == -9.0).all()), "stats1 pad rows written"
    assert bool((s2[B * P:] == -9.0).all()), "stats2 written past B P rows"
    assert bool((feats[B * P:] == 5.0).all()), "feats written past B P rows"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. owl_query_normalize_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dt", [64, 512, 768])
@pytest.mark.parametrize("nq", [3, 12, 30])
def test_query_normalize_bwd(nq, Dt):
    """qhat_bwd_kernel (owl_query_normalize_bwd, the prompt gradient of every step): dqueries += d(Q / |Q| + 1e-6)^T dqhat, with query norms
    from 1e-3 to 1e3, against float64 autograd.  The kernel accumulates, so dqueries starts nonzero; its rows >= nq stay untouched."""
    seed = nq * 1000 + Dt
    norms = torch.logspace(-3, 3, nq, device=DEV, dtype=torch.float64)[torch.randperm(nq, generator=torch.Generator().manual_seed(seed)).to(DEV)]
    q = randn(32, Dt, seed=seed)
    q[:nq] = (q[:nq].double() / q[:nq].double().norm(dim=1, keepdim=True) * norms[:, None]).float()
    dqhat = randn(32, Dt, seed=seed + 1)
    qr = q[:nq].double().requires_grad_(True)
    (qr / qr.norm(dim=1, keepdim=True) + 1e-6).backward(dqhat[:nq].double())
    ref = qr.grad
    rowmax = ref.abs().amax(1, keepdim=True)
    init = randn(32, Dt, seed=seed + 2) * 0.5
    init[:nq] = (init[:nq].double() * rowmax).float()
    dq = init.clone()
    _lib.call("owl_query_normalize_bwd", ops.stream(), dqhat, q, dq, nq, Dt)
    want = init[:nq].double() + ref
    report(f"dqueries nq={nq} Dt={Dt}", dq[:nq], want, 1e-5 * rowmax, 1e-6)
    assert torch.equal(dq[nq:], init[nq:]), "rows >= nq written"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. owl_cast_f32_bf16
# ---------------------------------------------------------------------------------------------------------------------------------------------
_SPECIAL_BITS = [
    0x00000000, 0x80000000,                                     # +-0
    0x00000001, 0x80000001, 0x00007fff, 0x00008000, 0x00018000, 0x0000ffff, 0x007f8000, 0x007fffff, 0x807fffff, 0x80018000,   # denormals (ties incl.)
    0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,             # exact ties: even upper half stays, odd rounds up (both signs)
    0x3f807fff, 0x3f808001, 0x40490fdb, 0x3e4ccccd,             # just below / above a tie, pi, 0.2
    0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7f8000, 0xff7fffff,  # largest finite bf16; ties / FLT_MAX round up to +-inf
    0x7f800000, 0xff800000, 0x00800000, 0x0080ffff,              # +-inf, smallest normal and its successor range
]
_NAN_BITS = [0x7fc00000, 0xffc00000, 0x7f800001, 0x7fbfffff, 0xff800001, 0x7fffffff]


def _bits_to_f32(bits):
    return torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32), dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("n", [1 << 24, 3 * (1 << 24) + 8 * 1000 + 5, 32 * 3 * 768 * 768], ids=["one_trip", "trips_vector_scalar_tail", "b16_batch32_images"])
def test_cast_f32_bf16_trip_loop(n):
    """cast_kernel's four-piece trip loop runs only when n >= 2048 x 256 x 32 = 2^24 (the image batch: 56.6 M elements at B/16 batch 32).
    n = 2^24: exactly one trip, no tail; 3 x 2^24 + 8005: three trips, a vector tail and a 5-element scalar tail; 32 x 3 x 768^2: the image
    batch.  Random bit patterns of every exponent plus +-0, denormals, exact ties (to even, both directions), values that round to +-inf, spread
    over the trips and both tails.  Bitwise equal to torch.Tensor.bfloat16(); NaN inputs only have to stay NaN."""
    g = torch.Generator(device=DEV).manual_seed(n & 0xffff)
    bits = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), device=DEV, dtype=torch.int32, generator=g)
    x = bits.view(torch.float32)
    half = n // 2
    x[half:] = torch.randn(n - half, device=DEV, generator=g) * 3.0                     # ordinary values too
    special = _bits_to_f32(_SPECIAL_BITS + _NAN_BITS).to(DEV)
    trip = 2048 * 256 * 32
    starts = sorted({0, 8 * 37, trip // 2 + 3, trip - len(special), trip, 2 * trip + 1000, n - 8 * 1000 - 5, n - 12, n - len(special), n // 3 * 2})
    for s in starts:
        if 0 <= s and s + len(special) <= n:
            x[s:s + len(special)] = special
    y = ops.cast_bf16(x)
    want = x.bfloat16()
    nan_in = x.isnan()
    assert int(nan_in.sum()) > 0
    assert bool(y[nan_in].isnan().all()), "NaN input cast to a non-NaN"
    yb = y.view(torch.int16); wb = want.view(torch.int16)
    bad = (yb != wb) & ~nan_in
    if bad.any():
        i = bad.nonzero()[:8].flatten()
        raise AssertionError(f"cast n={n}: {int(bad.sum())} elements differ from torch's round-to-nearest-even; first at {i.tolist()}: "
                             f"in {[hex(int(v) & 0xffffffff) for v in x.view(torch.int32)[i]]} got {[hex(int(v) & 0xffff) for v in yb[i]]} "
                             f"want {[hex(int(v) & 0xffff) for v in wb[i]]}")
    # the reference itself: round to nearest even on the bit pattern (independent of how torch casts)
    xb = x.view(torch.int32).to(torch.int64) & 0xffffffff
    rne = ((xb + 0x7fff + ((xb >> 16) & 1)) >> 16) & 0xffff
    assert torch.equal(rne[~nan_in], wb.to(torch.int64)[~nan_in] & 0xffff)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. GEMM at model row counts
# ---------------------------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [
    # B/16 batch 32 (M = 32 x 2312)
    ("b16_qkv", 73984, 2304, 768, ops.EPI_BIAS_BF16),
    ("b16_outproj", 73984, 768, 768, ops.EPI_BIAS_BF16),
    ("b16_fc1", 73984, 3072, 768, ops.EPI_QGELU_BF16),
    ("b16_fc2", 73984, 768, 3072, ops.EPI_BIAS_BF16),
    ("b16_fc2_dX", 73984, 3072, 768, ops.EPI_DQGELU_BF16),
    # L/14 batch 16 (M = 16 x 3608)
    ("l14_qkv", 57728, 3072, 1024, ops.EPI_BIAS_BF16),
    ("l14_fc1", 57728, 4096, 1024, ops.EPI_QGELU_BF16),
    ("l14_fc2", 57728, 1024, 4096, ops.EPI_BIAS_BF16),
    ("l14_outproj", 57728, 1024, 1024, ops.EPI_BIAS_BF16),
]


@pytest.mark.parametrize("tile", [0, 7], ids=["auto", "pingpong2"])
@pytest.mark.parametrize("name,M,N,K,epi", GEMM_SHAPES, ids=[s[0] for s in GEMM_SHAPES])
def test_gemm_model_row_counts(name, M, N, K, epi, tile):
    """The encoder's GEMMs at the model's row counts: tile 0 is the model's choice -- at B/16 N = 768 whole rounds of the 256 x 256 ping-pong kernel
    plus one round of half-height remainder tiles (gemm_pph.hip) from M_main on (asserted to happen); tile 7 the ping-pong kernel on the whole
    problem.  Sampled rows (first tile, every 128-row band, both sides of M_main, the last rows) against float64 A W^T + bias, then the epilogue
    (quick-GELU + its saved derivative quick_gelu'(u); the dX GEMM's product with a saved derivative); rows past M stay zero."""
    M_main = gemm_reference.gemm_split(M, N, tile)
    if name in ("b16_outproj", "b16_fc2") and tile == 0:
        assert M_main is not None and 0 < M_main < M, "the model's B/16 N = 768 GEMMs are expected to split into whole rounds + half-height tiles"
    seed = M + N + K + epi
    Mp = (M + 255) // 256 * 256 + 128                   # whole 256-row tiles and more: pad rows exist and no tile can reach past the buffers
    A = torch.zeros(Mp, K, dtype=torch.bfloat16, device=DEV)
    A[:M] = randn(M, K, seed=seed, dtype=torch.bfloat16)
    W = randn(N, K, seed=seed + 1, scale=1.0 / math.sqrt(K), dtype=torch.bfloat16)
    bias = randn(N, seed=seed + 2, scale=0.5)
    out = torch.zeros(Mp, N, dtype=torch.bfloat16, device=DEV)
    aux = None
    if epi == ops.EPI_QGELU_BF16:
        aux = torch.zeros(Mp, N, dtype=torch.bfloat16, device=DEV)
    elif epi == ops.EPI_DQGELU_BF16:
        aux = torch.zeros(Mp, N, dtype=torch.bfloat16, device=DEV)
        uu = randn(M, N, seed=seed + 3, scale=2.0)
        s = torch.sigmoid(1.702 * uu)
        aux[:M] = (s * (1.0 + 1.702 * uu * (1.0 - s))).bfloat16()          # a saved quick-GELU derivative
        del uu, s
    ops.gemm(epi, A, W, out, bias=None if epi == ops.EPI_DQGELU_BF16 else bias, aux=aux, M=M, tile=tile)
    r = torch.tensor(gemm_reference.sample_rows(M, M_main), device=DEV)
    acc = A[r].double() @ W.double().t()
    atol = K * 2.0 ** -20                                # f32 accumulation over K
    rtol = 2.0 ** -7                                     # two bf16 rounding steps (half an ulp each) at the worst place in a binade
    if epi == ops.EPI_BIAS_BF16:
        report(f"{name} bias", out[r], acc + bias.double(), atol, rtol)
    elif epi == ops.EPI_QGELU_BF16:
        u = acc + bias.double()
        sg = torch.sigmoid(1.702 * u)
        report(f"{name} quick-GELU", out[r], u * sg, atol, rtol)
        report(f"{name} quick_gelu'(u)", aux[r], sg * (1.0 + 1.702 * u * (1.0 - sg)), atol + 1e-4, rtol)
    else:
        report(f"{name} dX * saved derivative", out[r], acc * aux[r].double(), atol, rtol)
    assert float(out[M:].abs().max()) == 0.0, "GEMM wrote rows past M"
    if aux is not None and epi == ops.EPI_QGELU_BF16:
        assert float(aux[M:].abs().max()) == 0.0, "GEMM wrote saved-derivative rows past M"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. matcher cost and the loss at exact ties
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _random_case(B, P, C, seed, nmax=16, counts=None):
    sims = (rng.uniform(seed, "s", B * P * C).reshape(B, P, C) * 1.2 - 0.6).astype(np.float32)
    x0 = rng.uniform(seed, "b", B * P, 0) * 0.7; y0 = rng.uniform(seed, "b", B * P, 1) * 0.7
    w = 0.03 + rng.uniform(seed, "b", B * P, 2) * 0.25; h = 0.03 + rng.uniform(seed, "b", B * P, 3) * 0.25
    pb = np.stack([x0, y0, x0 + w, y0 + h], -1).reshape(B, P, 4).astype(np.float32)
    labels, tbs = [], []
    for b in range(B):
        n = counts[b] if counts is not None else 1 + int(rng.randint(seed, f"n{b}", 1, nmax)[0])
        tx = rng.uniform(seed, f"t{b}", n, 0) * 0.6; ty = rng.uniform(seed, f"t{b}", n, 1) * 0.6
        tw = 0.02 + rng.uniform(seed, f"t{b}", n, 2) * 0.35; th = 0.02 + rng.uniform(seed, f"t{b}", n, 3) * 0.35
        tbs.append(np.stack([tx, ty, tx + tw, ty + th], -1).astype(np.float32))
        labels.append(rng.randint(seed, f"l{b}", n, C))
    return sims, pb, labels, tbs


@pytest.mark.parametrize("B,P,C,counts", [(4, 576, 10, None), (3, 2304, 10, None), (2, 3600, 10, None), (5, 36, 4, None), (2, 36, 4, [36, 36]), (1, 24, 3, [24])],
                         ids=["576", "2304", "3600", "36", "n_eq_P_36", "n_eq_P_24"])
def test_match_cost_matches_oracle(B, P, C, counts):
    """match_cost_kernel (owl_match_cost) on its own: costT[b][j][p] against the oracle's match_one cost (L1 + -softmax[label] + -GIoU), on the
    random cases of the loss tests and with n = Nmax = P."""
    from oracle import owl_oracle as O
    from owl_vit_object_detection_amd.matcher import PackedTargets
    sims, pb, labels, tbs = _random_case(B, P, C, seed=B * 1000 + P, counts=counts)
    tg = PackedTargets([torch.from_numpy(l) for l in labels], [torch.from_numpy(t) for t in tbs], DEV, C)
    costT = torch.full((B, tg.Nmax, P), 123.0, device=DEV)
    _lib.call("owl_match_cost", ops.stream(), torch.from_numpy(sims).to(DEV), torch.from_numpy(pb).to(DEV), tg.labels, tg.boxes, tg.counts, costT,
              B, P, C, tg.Nmax, 1.0, 1.0, 1.0)
    got = costT.cpu()
    for b in range(B):
        n = len(labels[b])
        Cref, _, _, _ = O.match_one(torch.from_numpy(sims[b]), torch.from_numpy(pb[b]), torch.from_numpy(labels[b]).long(), torch.from_numpy(tbs[b]), C)
        report(f"match cost image {b}", got[b, :n], Cref.t(), 1e-6, 1e-6)
        assert bool((got[b, n:] == 123.0).all()), "cost rows past the image's count written"


def _tie_case():
    """Two images of crafted (prediction, target) pairs, one pair per cell of a 3 x 2 grid in the top half, coordinates multiples of 1/128 (exact
    in f32), the other predictions tiny boxes in a band far below every target: the assignment is unambiguous.  Image 1 swaps the roles of
    prediction and target."""
    u = 1.0 / 128
    pairs = [  # (prediction, target) inside a 20 x 30 (in 1/64) cell
        ([2, 2, 14, 12], [2, 2, 14, 12]),           # prediction == target
        ([2, 2, 16, 14], [2, 2, 12, 10]),           # two shared edges (x0, y0)
        ([4, 6, 12, 20], [2, 6, 16, 28]),           # nested, one shared edge (y0): enclosing min and intersection max tie
        ([2, 4, 8, 20], [8, 4, 18, 20]),            # edge to edge: intersection width exactly 0, y extents equal
        ([1, 3, 6, 18], [10, 6, 19, 22]),           # disjoint in x only
        ([3, 3, 18, 26], [3, 8, 12, 26]),           # prediction contains target: shared x0 and y1
    ]
    cells = [(0, 0), (22, 0), (44, 0), (0, 32), (22, 32), (44, 32)]
    P, C = 48, 6
    imgs = []
    for img in range(2):
        pb = np.zeros((P, 4), np.float32)
        for k in range(P):                          # far filler: 2 x 2 boxes on a lattice in y in [104, 118] / 128
            x0, y0 = (k % 24) * 5 + 2, 104 + 12 * (k // 24)
            pb[k] = np.array([x0, y0, x0 + 2, y0 + 2]) * u
        tb = np.zeros((len(pairs), 4), np.float32)
        slots = [5, 11, 17, 29, 30, 41]             # prediction index of each pair
        for k, ((a, t), (cx, cy)) in enumerate(zip(pairs, cells)):
            if img == 1:
                a, t = t, a
            pb[slots[k]] = (np.array(a, np.float64) + [cx, cy, cx, cy]) * u
            tb[k] = (np.array(t, np.float64) + [cx, cy, cx, cy]) * u
        labels = np.array([k % C for k in range(len(pairs))], np.int64) if img == 0 else np.array([(k + 2) % C for k in range(len(pairs))], np.int64)
        sims = np.asarray(rng.uniform(17 + img, "tie", P * C).reshape(P, C) * 1.2 - 0.6, np.float32)
        for k, s in enumerate(slots):               # each pair's prediction prefers its target's class
            sims[s, labels[k]] = 0.55
        # exact 0.0 and +-1.0 entries: on matched rows (the label's own column included) and on background rows
        sims[slots[0], :] = 0.0
        sims[slots[1], labels[1]] = 1.0
        sims[slots[2], (labels[2] + 1) % C] = -1.0
        sims[slots[3], labels[3]] = 0.0
        sims[0, 0] = 1.0; sims[1, 1] = -1.0; sims[2, :] = 0.0; sims[3, 3] = 0.0
        imgs.append((sims, pb, labels, tb))
    return imgs, P, C


@pytest.mark.parametrize("scaled", [False, True])
def test_push_pull_loss_exact_ties_match_oracle(scaled):
    """box_loss_kernel's hand-written L1 / GIoU gradient where random boxes never go: equal coordinates (sign(0) = 0; a max / min tie splits the
    gradient 0.5 / 0.5 as torch does), an intersection of width exactly 0 (torch passes the gradient through clamp(min=0) at 0), disjoint in x,
    nested and containing boxes with shared edges; class_loss_kernel at sims exactly 0.0 and +-1.0 (|s| at 0, the BCE logs clamped at -100).
    Assignments and target classes bit-exact, losses and gradients against the oracle (torch autograd) at the tolerances of the loss tests."""
    from oracle import owl_oracle as O
    from owl_vit_object_detection_amd.losses import PushPullLoss
    imgs, P, C = _tie_case()
    sims = np.stack([i[0] for i in imgs]); pb = np.stack([i[1] for i in imgs])
    labels = [i[2] for i in imgs]; tbs = [i[3] for i in imgs]
    scales = np.array([3.0, 4.5, 3.5, 5.0, 4.0, 3.2], np.float32)[:C] if scaled else None
    det = []
    so = torch.from_numpy(sims).requires_grad_(True); bo = torch.from_numpy(pb).requires_grad_(True)
    lo = O.push_pull_loss(so, [torch.from_numpy(l) for l in labels], bo, [torch.from_numpy(t) for t in tbs], C,
                          None if scales is None else torch.from_numpy(scales), det)
    sum(lo.values()).backward()
    sg = torch.from_numpy(sims).to(DEV).requires_grad_(True); bg = torch.from_numpy(pb).to(DEV).requires_grad_(True)
    crit = PushPullLoss(C, scales)
    lg = crit(sg, [torch.from_numpy(l).to(DEV) for l in labels], bg, [torch.from_numpy(t).to(DEV) for t in tbs])
    (lg["loss_ce"] + lg["loss_bg"] + lg["loss_bbox"] + lg["loss_giou"]).backward()
    slots = [5, 11, 17, 29, 30, 41]
    for b in range(2):
        n = len(labels[b])
        assert np.array_equal(det[b]["pred_idx"].numpy(), np.array(slots)), "crafted case is not the intended assignment"
        assert np.array_equal(crit.last["pred_idx"][b, :n].cpu().numpy(), det[b]["pred_idx"].numpy()), b
        assert np.array_equal(crit.last["tgt_idx"][b, :n].cpu().numpy(), det[b]["tgt_idx"].numpy()), b
        assert np.array_equal(crit.last["target_classes"][b].cpu().numpy(), det[b]["target_classes"].numpy()), b
    for k in ("loss_ce", "loss_bg", "loss_bbox", "loss_giou"):
        assert float(lg[k]) == pytest.approx(float(lo[k]), rel=1e-4, abs=1e-6), k
    np.testing.assert_allclose(sg.grad.cpu().numpy(), so.grad.numpy(), rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(bg.grad.cpu().numpy(), bo.grad.numpy(), rtol=1e-3, atol=1e-7)
    # the crafted rows carry gradient where the ties are (a test that compared zeros with zeros would prove nothing)
    assert float(bo.grad[:, slots].abs().sum()) > 0
