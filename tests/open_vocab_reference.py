"""Float64 reference, derived error bound, inputs and an f32 simulation for the open-vocabulary class head: csrc/open_vocab.hip
(logit_rowstats_kernel, class_logits_kernel behind owl_class_logits_fwd).  Checker side; device-agnostic; nothing here imports the package's ops.

Reference (float64 on the kernel's exact inputs: f32 values, bf16 features upcast; eps6 = the f32 nearest 1e-6, as the kernel holds it)
---------
`exact_logits(e, Q, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask)`  HF modeling_owlvit.py OwlViTClassPredictionHead.forward restated:
    e^ = e / (|e| + eps6), q^ = Q / (|Q| + eps6), cos = e^ . q^, shift = f . w_shift + b_shift, x = f . w_scale + b_scale, scale = elu(x) + 1,
    logit = (cos + shift) scale, finfo(f32).min where mask == 0; score = sigmoid(logit), 0 where masked.  Q is [B, Q, Dt] or [Q, Dt] (shared bank),
    mask [B, Q], [Q] or None.  tests/test_open_vocab_reference.py holds it to HF's own module in float64 (1e-12) and to fixture F15.

Bound (elementwise, derived from the kernel's evaluation order, no fitted constant; F, gamma, _mul, _rnd as in heads_reference.py, whose ASSUMPTIONS
H1 -- sqrtf, the f32 division, expf and here expm1f within 2 ulp = 4 F -- and H2 -- the MFMA rounds every product and add, n_dot = 64 ceil(Dt / 128) + 3
roundings on a product's path -- are taken over; the file is compiled with contraction off, so every written operation rounds once)
 q^ (class_logits_kernel's table loop): lane l adds fl(v v) for k = l, l + 64, ...: ceil(Dt / 64) adds, six butterfly levels, the product's rounding:
   n_q = ceil(Dt / 64) + 7;  n~ = sqrtf: r_n = (1 + 4 F) / sqrt(1 - gamma(n_q)) - 1;  d~ = fl(n~ + eps6): E_d = n r_n + F (d + n r_n);
   inv~ = 1 / d~: r_inv = (1 + 4 F) / (1 - E_d / d) - 1;  q^~ = fl(q inv~): r_q = (1 + r_inv)(1 + F) - 1, relative to every element of q^.
 1 / (|e| + eps6): heads_reference's row norm, n_ss = 16 ceil(Dt / 128) + 5 (the same chain: class_sims_wide_kernel's), r_inv_e likewise.
 acc (Dt / 2 MFMAs in the source's order on e and q^~): E_acc = (gamma(n_dot)(1 + r_q) + r_q) sum_k |e_k q^_k| + T.
 cos = fl(acc~ inv_e~): product rule + one rounding.
 shift, x (logit_rowstats_kernel): lane l runs 8 fmaf per 8-element chunk l, l + 64, ...: 8 ceil(D / 512) roundings, six butterfly levels, the bias
   add: E = gamma(8 ceil(D / 512) + 6) sum |f w| and one rounding.  elu: slope <= 1 on x <= 0 and 1 above: E_elu = E_x exp(E_x) + 4 F |elu| + T
   (expm1f, H1; exact on x > 0, where the term is not charged); + 1: one rounding.
 logit = fl(fl(cos + shift) scale): the add, the multiply: one rounding each.  Masked entries are bit tests: -FLT_MAX and +0.
 score = 1 / (1 + expf(-logit)): heads_reference's sigmoid: r_e = exp(E_logit)(1 + 4 F) - 1, r_s = (1 + 4 F) / ((1 - (1 - s) r_e)(1 - F)) - 1
   relative to s, + T (expf overflows from logit = -88.7 down and the kernel returns 0 where the exact value is below T).

`emulate_logits(..., hooks)` runs the kernel in f32 in the order the source writes it and plants errors; CPU test only, NEVER a reference on the GPU.
"""
import math

import torch

from tests.gemm_reference import F, TINY, bits, check, gamma as gam, ratios  # noqa: F401
from tests.layernorm_reference import _mul, _rnd

EPS6 = float(torch.tensor(1e-6, dtype=torch.float32))
FMIN = float(torch.finfo(torch.float32).min)
ULP2 = 4.0 * F


def cdiv(a, b):
    return (a + b - 1) // b


def n_dot(Dt):
    return 64 * cdiv(Dt, 128) + 3


def n_ss(Dt):
    return 16 * cdiv(Dt, 128) + 5


def n_q(Dt):
    return cdiv(Dt, 64) + 7


def n_row(D):
    return 8 * cdiv(D, 512) + 6


def launch_shape(P):
    """(waves per workgroup, workgroups per image) of owl_class_logits_fwd (open_vocab.hip class_logits_shape)."""
    tiles = cdiv(P, 32)
    groups = cdiv(tiles, 8)
    return cdiv(tiles, groups), groups


def _banks(Q, B):
    Q = Q.double()
    return Q if Q.dim() == 3 else Q[None].expand(B, -1, -1)


def _masks(mask, B, nq, device):
    if mask is None:
        return torch.ones(B, nq, dtype=torch.bool, device=device)
    m = mask != 0
    return m if m.dim() == 2 else m[None].expand(B, -1)


def exact_logits(e, Q, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask=None):
    """float64 reference (module docstring) -> dict: logits, scores [B, P, Q] (masked: FMIN / 0), live [B, 1, Q] bool, and what the bound reads."""
    Dt = e.shape[-1]
    ed = e.double()[:B * P].view(B, P, Dt)
    Qd = _banks(Q, B)
    f = feats.double()[:B * P]
    ne = ed.norm(dim=-1, keepdim=True)
    inv_e = 1.0 / (ne + EPS6)
    nq = Qd.norm(dim=-1, keepdim=True)
    qhat = Qd / (nq + EPS6)
    acc = torch.einsum("bpk,bqk->bpq", ed, qhat)
    acc_abs = torch.einsum("bpk,bqk->bpq", ed.abs(), qhat.abs())
    cos = acc * inv_e
    shift = (f @ w_shift.double().reshape(-1) + float(b_shift)).view(B, P, 1)
    shift_abs = (f.abs() @ w_shift.double().reshape(-1).abs()).view(B, P, 1)
    x = (f @ w_scale.double().reshape(-1) + float(b_scale)).view(B, P, 1)
    x_abs = (f.abs() @ w_scale.double().reshape(-1).abs()).view(B, P, 1)
    elu = torch.where(x > 0, x, torch.expm1(x))
    scale = elu + 1.0
    pre = cos + shift
    lg = pre * scale
    live = _masks(mask, B, Qd.shape[1], lg.device)[:, None, :]
    logits = torch.where(live, lg, torch.full_like(lg, FMIN))
    scores = torch.where(live, torch.sigmoid(lg), torch.zeros_like(lg))
    return dict(logits=logits, scores=scores, live=live, raw=lg, cos=cos, acc=acc, acc_abs=acc_abs, ne=ne, inv_e=inv_e, nq=nq, shift=shift, shift_abs=shift_abs,
                x=x, x_abs=x_abs, elu=elu, scale=scale, pre=pre, Dt=Dt, D=f.shape[-1])


def bounds(r):
    """-> {"logits", "scores"}: tolerances [B, P, Q] of the unmasked entries (module docstring); also "cos", "shift", "scale" for diagnostics."""
    Dt, D = r["Dt"], r["D"]
    # q^: relative error of every element
    nq = r["nq"]
    r_n = (1.0 + ULP2) / math.sqrt(1.0 - gam(n_q(Dt))) - 1.0
    d = nq + EPS6
    E_d = nq * r_n + F * (d + nq * r_n)
    r_inv = (1.0 + ULP2) / (1.0 - E_d / d) - 1.0
    r_q = ((1.0 + r_inv) * (1.0 + F) - 1.0).transpose(1, 2)          # [B, 1, Q]
    # 1 / (|e| + eps6)
    ne = r["ne"]
    r_s = (1.0 + ULP2) / math.sqrt(1.0 - gam(n_ss(Dt))) - 1.0
    de = ne + EPS6
    E_de = ne * r_s + F * (de + ne * r_s)
    r_inv_e = (1.0 + ULP2) / (1.0 - E_de / de) - 1.0
    E_inv = r["inv_e"] * r_inv_e
    E_acc = (gam(n_dot(Dt)) * (1.0 + r_q) + r_q) * r["acc_abs"] + TINY
    E_cos = _rnd(r["cos"], _mul(r["acc"], E_acc, r["inv_e"], E_inv)) + TINY
    g = gam(n_row(D))
    E_shift = _rnd(r["shift"], g * r["shift_abs"]) + TINY
    E_x = _rnd(r["x"], g * r["x_abs"]) + TINY
    E_elu = E_x * torch.exp(E_x) + torch.where(r["x"] > E_x, torch.zeros_like(E_x), ULP2 * r["elu"].abs()) + TINY
    E_scale = _rnd(r["scale"], E_elu)
    E_pre = _rnd(r["pre"], E_cos + E_shift)
    E_lg = _rnd(r["raw"], _mul(r["pre"], E_pre, r["scale"], E_scale)) + TINY
    s = torch.sigmoid(r["raw"])
    r_e = torch.exp(E_lg) * (1.0 + ULP2) - 1.0
    den = (1.0 - (1.0 - s) * r_e) * (1.0 - F)
    r_sig = torch.where(den > 0, (1.0 + ULP2) / den - 1.0, torch.full_like(den, float("inf")))
    E_sc = torch.minimum(s * r_sig, torch.ones_like(s)) + TINY
    return dict(logits=E_lg, scores=E_sc, cos=E_cos, shift=E_shift, scale=E_scale)


def check_logits(name, logits, scores, r, fails=None):
    """logits (and scores, or None) [B, P, Q] on any device against exact_logits' record: unmasked entries inside the bound, masked ones exactly
    finfo.min / +0.  -> worst err / tol of the logits and of the scores."""
    b = bounds(r)
    live = r["live"].expand_as(r["raw"])
    lg = logits.detach().double().cpu()          # (the record is made on the CPU)
    big = torch.full_like(b["logits"], float("inf"))
    worst = [check(name + " logits", torch.where(live, lg, r["raw"]), r["raw"], torch.where(live, b["logits"], big), fails)]
    dead = ~live
    msgs = []
    if bool(dead.any()) and not bool((lg[dead] == FMIN).all()):
        msgs.append(f"{name}: a masked logit is not finfo(f32).min")
    if scores is not None:
        sc = scores.detach().double().cpu()
        worst.append(check(name + " scores", torch.where(live, sc, r["scores"]), r["scores"], torch.where(live, b["scores"], big), fails))
        if bool(dead.any()) and not bool((bits(scores.float().cpu())[dead.cpu()] == 0).all()):
            msgs.append(f"{name}: a masked score is not +0")
    for m in msgs:
        if fails is None:
            raise AssertionError(m)
        fails.append(m)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (B, P, Q, Dt, D): the smallest shapes that reach each way the kernel can go wrong -- P = 4: a tile larger than an image; 36: the image boundary
# inside a 32-row tile; 576: whole tiles (18 = three workgroups of six waves); Q = 1 / 31 / 32 / 33 / 70: one partial query block, a block's edge from
# both sides, three blocks with the last partial; Dt = 192: the Dt % 128 == 64 half-chunk; D = 128 / 768 / 1024: a quarter, one and a half, two
# rounds of the row pre-pass's 512-element stride.
GPU_CASES = [(1, 4, 1, 64, 128), (3, 36, 33, 192, 128), (1, 36, 31, 64, 128), (3, 4, 32, 192, 128), (1, 576, 70, 512, 768), (3, 36, 70, 768, 1024),
             (3, 576, 33, 64, 128)]


def make_inputs(B, P, Q, Dt, D, seed=0, shared=False, masked=True):
    """Seeded CPU inputs: e f32 [B P, Dt] with row norms over 2^-3 .. 2^3; a bank f32 [B, Q, Dt] ([Q, Dt] when shared) whose row norms run over
    1e-3 .. 10 (where the epsilon's placement shows) with one all-zero row when Q >= 3; feats bf16 [B P, D]; head weights of trained-like size:
    shift ~ 0.3 (the size of a cosine), x = w_scale . f + b_scale ~ N(0.1, 1): both ELU branches; mask uint8 [B, Q] with about a fifth masked, the
    zero row among them on image 0, and never a whole image."""
    g = torch.Generator(device="cpu").manual_seed(1000003 * seed + 7919 * B + 104729 * P + 1299709 * Q + 31 * Dt + D)
    rows = B * P
    e = 0.7 * torch.randn(rows, Dt, generator=g) * torch.exp2(torch.randint(-3, 4, (rows, 1), generator=g).float())
    nb = 1 if shared else B
    bank = torch.randn(nb, Q, Dt, generator=g)
    scale = torch.logspace(-3, 1, 9)[(torch.arange(nb * Q) * 5) % 9].view(nb, Q, 1)
    bank = bank / bank.norm(dim=-1, keepdim=True) * scale
    if Q >= 3:
        bank[:, Q // 2] = 0.0
    feats = torch.randn(rows, D, generator=g).to(torch.bfloat16)
    w_shift = (0.3 / math.sqrt(D)) * torch.randn(D, generator=g)
    w_scale = (1.0 / math.sqrt(D)) * torch.randn(D, generator=g)
    b_shift, b_scale = torch.tensor([0.05]), torch.tensor([0.1])
    mask = None
    if masked:
        mask = (torch.rand(B, Q, generator=g) > 0.2).to(torch.uint8)
        mask[:, 0] = 1
        if Q >= 3:
            mask[0, Q // 2] = 0
    return dict(e=e, queries=bank[0] if shared else bank, feats=feats, w_shift=w_shift, b_shift=b_shift, w_scale=w_scale, b_scale=b_scale, mask=mask)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
HOOKS = ("wrapper_eps", "eps_in_root", "exp_scale", "scale_before_shift", "mask_zero", "mask_neginf", "bank0", "mask0", "row_neighbour")


def _wave_sum32(s):
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    return s[..., 0]


def _emulate_qhat(q, hooks):
    """[n, Dt] f32 -> the table rows: lane-strided sum of squares, wave_sum, 1 / (sqrtf + eps6), multiply."""
    n, Dt = q.shape
    v = q.view(n, Dt // 64, 64)
    s = torch.zeros(n, 64)
    for i in range(Dt // 64):
        s = s + v[:, i] * v[:, i]
    s = _wave_sum32(s)
    eps = torch.tensor(EPS6)
    if "wrapper_eps" in hooks:          # the reference wrapper's q / |q| + 1e-6 (ref src/models.py:31-33)
        return q / torch.sqrt(s)[:, None] + eps
    if "eps_in_root" in hooks:
        return q * (1.0 / torch.sqrt(s + eps))[:, None]
    return q * (1.0 / (torch.sqrt(s) + eps))[:, None]


def _columns(Dt):
    """k of lane half 0 / 1 for every MFMA in issue order; None where the half-chunk lies past Dt (it feeds zeros)."""
    out = []
    for blk in range(2 * cdiv(Dt, 128)):
        c0 = (blk >> 1) << 7
        for s in range(8):
            for c in range(4):
                ks = []
                for hi in (0, 1):
                    act = c0 + hi * 64 < Dt
                    ks.append(c0 + hi * 64 + (blk & 1) * 32 + s * 4 + c if act else None)
                out.append(tuple(ks))
    return out


def emulate_logits(e, Q, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask=None, hooks=(), scores=True):
    """owl_class_logits_fwd in f32, in the source's order -> (logits, scores) [B, P, Q] f32.  hooks: HOOKS (the planted errors)."""
    e = e.float()[:B * P]
    Dt = e.shape[1]
    f = feats.float()[:B * P]
    D = f.shape[1]
    nb = Q.shape[0] if Q.dim() == 3 else 1
    nq = Q.shape[-2]
    # pre-pass: lane l, chunks l, l + 64, ...: eight FMAs each, then the butterfly
    nch = cdiv(D // 8, 64)
    fp = torch.zeros(B * P, nch * 512); fp[:, :D] = f
    wp = torch.zeros(2, nch * 512); wp[0, :D] = w_shift.float().reshape(-1); wp[1, :D] = w_scale.float().reshape(-1)
    fp = fp.view(-1, nch, 64, 8); wp = wp.view(2, nch, 64, 8)
    sums = []
    for t in range(2):
        s = torch.zeros(B * P, 64)
        for i in range(nch):
            for j in range(8):
                s = (fp[:, i, :, j].double() * wp[t, i, :, j].double() + s.double()).float()
        sums.append(_wave_sum32(s))
    shift = sums[0] + b_shift.float().reshape(())
    x = sums[1] + b_scale.float().reshape(())
    scale = torch.exp(x) if "exp_scale" in hooks else torch.where(x > 0, x, torch.expm1(x)) + 1.0
    if "row_neighbour" in hooks:
        shift, scale = torch.roll(shift, -1), torch.roll(scale, -1)
    # row norm: each lane half owns 64 consecutive columns of every 128-chunk
    nc = cdiv(Dt, 128)
    ep = torch.zeros(B * P, nc * 128); ep[:, :Dt] = e
    ev = ep.view(-1, nc, 2, 16, 4)
    ss = torch.zeros(B * P, 2)
    for c in range(nc):
        for s in range(16):
            a = ev[:, c, :, s]
            ss = ss + (((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]) + a[..., 3] * a[..., 3])
    inv = 1.0 / (torch.sqrt(ss[:, 0] + ss[:, 1]) + torch.tensor(EPS6))
    cols = _columns(Dt)
    logits = torch.empty(B, P, nq)
    m = None if mask is None else (mask != 0)
    for b in range(B):
        qb = Q if Q.dim() == 2 else Q[0 if "bank0" in hooks else b]
        qh = _emulate_qhat(qb.float().contiguous(), hooks)
        eb = e[b * P:(b + 1) * P]
        acc = torch.zeros(P, nq)
        for k0, k1 in cols:
            for k in (k0, k1):
                if k is not None:
                    acc = acc + eb[:, k, None] * qh[None, :, k]
        cosv = acc * inv[b * P:(b + 1) * P, None]
        sh, sc = shift[b * P:(b + 1) * P, None], scale[b * P:(b + 1) * P, None]
        logits[b] = cosv * sc + sh if "scale_before_shift" in hooks else (cosv + sh) * sc
    sc_out = 1.0 / (1.0 + torch.exp(-logits)) if scores else None
    if m is not None:
        mm = (m if m.dim() == 2 else m[None].expand(B, -1))
        if "mask0" in hooks:
            mm = mm[:1].expand(B, -1)
        dead = ~mm[:, None, :].expand(B, P, nq)
        fill = 0.0 if "mask_zero" in hooks else (float("-inf") if "mask_neginf" in hooks else FMIN)
        logits = torch.where(dead, torch.full_like(logits, fill), logits)
        if scores:
            sc_out = torch.where(dead, torch.zeros_like(sc_out), sc_out)
    return logits, sc_out
