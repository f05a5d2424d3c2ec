"""Float64 reference, derived error bounds, inputs and an f32 simulation for the open-vocabulary class head's backward: csrc/open_vocab_bwd.hip
(ovb_qhat_kernel, ovb_rows_kernel, ovb_dq_kernel, ovb_dq_finish_kernel behind owl_class_logits_bwd).  Checker side; device-agnostic; nothing here
imports the package's ops.

Reference (float64 on the kernel's exact inputs: f32 values, the (shift, scale) the forward saved; eps6 = the f32 nearest 1e-6, as the kernel holds it)
---------
`exact_bwd(g, e, Q, shift, scale, w_shift, w_scale, B, P, mask)`: the adjoint of HF's OwlViTClassPredictionHead.forward in closed form.  With g SELECTED
to 0 where mask == 0 (torch.where: Inf / NaN there changes nothing), e^ = e / (|e| + eps6), q^ = Q / (|Q| + eps6):
    dpre = g scale;  dshift = sum_q dpre;  dscale = sum_q g (e^ . q^ + shift);  ds = dscale (scale > 1 ? 1 : scale)   (ELU' from the saved scale)
    dfeats = dshift w_shift + ds w_scale;  de^ = sum_q dpre q^;  dq^_{b,q} = sum_{r in image b} dpre e^_r (summed over the images for a shared bank)
    dx = (dx^ - u (x^ . dx^)) / (|x| + eps6), u = x / |x| and u = 0 for an all-zero row (torch's gradient of the norm at 0), x in {e, q}.
tests/test_open_vocab_bwd_reference.py holds it to torch autograd of HF's own module in float64 (1e-12).  The record is written in the kernel's
factoring (T = sum_q g q^, c = e^ . T, a = inv scale, coef = c / |e|, de = a (T - coef e)): the same function, the quantities the bound reads.

Bound (elementwise, derived from the kernel's evaluation order, no fitted constant; F, U, gamma, _mul, _rnd, _store_bf16 as in gemm_reference.py /
layernorm_reference.py; open_vocab_reference.py's ASSUMPTIONS are taken over: H1 -- sqrtf and the f32 division within 2 ulp = 4 F -- and H2 -- the f32
MFMA rounds every product and every add; a 32x32x2 instruction is charged TWO adds, so a chain of n products is n + 3 roundings.  The file is compiled
with contraction off: every written operation rounds once)
 q^, |q|, 1 / (|q| + eps6) (ovb_qhat_kernel = the forward's table loop): open_vocab_reference's n_q, r_n, r_inv, r_q.
 T[r, k] (ovb_rows_kernel: Qp = 32 ceil(Q / 32) products in ascending q): E_T = sum_q |g| |q^| (gamma(Qp + 3)(1 + r_q) + r_q) + T.
 row reductions |e|^2 and e . T: the product, a lane's <= ceil(Dt / 128) tiles, five xor steps, three adds over the waves: n_red = ceil(Dt / 128) + 9.
   |e|~ relative r_s = (1 + 4 F) / sqrt(1 - gamma(n_red)) - 1, inv~ as in the forward; et~: (1 + gamma) sum |e| E_T + gamma sum |e T|.
 gs: lane-strided over Q, six butterfly levels: gamma(ceil(Q / 64) + 6) sum |g|.
 c = fl(inv et); dshift = fl(scale gs); dscale = fl(c + fl(shift gs)); ds = fl(dscale f), f exact; dfeats = fl(fl(dshift w_shift) + fl(ds w_scale)).
 a = fl(inv scale); coef = c~ / |e|~ (H1; exactly 0 for an all-zero row); de = bf16(fl(a fl(T~ - fl(coef e)))).
 dq^: the A operand fl(g a~) carries a's error and one rounding; a chunk of `chunk` rows is chunk + 3 roundings, the slabs are then added in index
   order (S per image, B S for a shared bank; split(P, Q) = ovb_split): n_dq = chunk + 3 + slabs + 1.
 dot = q^~ . dq^~: lane-strided + butterfly, n_q; u = q / |q|~ (H1); dq = fl(fl(dq^~ - fl(u dot)) inv~).

`emulate_bwd(..., hooks)` runs the kernels in f32 in the order the source writes them and plants errors; CPU test only, NEVER a reference on the GPU.
"""
import math

import torch

from tests.gemm_reference import F, TINY, U, bits, check, gamma as gam, ratios  # noqa: F401
from tests.layernorm_reference import _mul, _rnd
from tests import open_vocab_reference as FWD
from tests.open_vocab_reference import EPS6, FMIN, ULP2, cdiv, n_q, _banks, _masks, _wave_sum32

# the issue's cases: a ragged last row tile, both sides of a 32-query block, image boundaries inside a row tile, the LDS ceiling of the forward's
# table (Dt = 768 / 1024 beside D = 1024), the query-index range
GPU_CASES = [(1, 4, 1, 64, 128), (3, 36, 33, 192, 128), (1, 36, 31, 64, 128), (3, 4, 32, 192, 128), (2, 70, 70, 512, 768), (3, 36, 70, 768, 1024),
             (1, 4, 4096, 64, 128)]


def split(P, Q):
    """(slabs per image, rows per slab) of the dq^ partial sums (open_vocab_bwd.hip ovb_split): a function of (P, Q) alone."""
    nqb = cdiv(Q, 32)
    s0 = 1 if nqb >= 64 else 64 // nqb
    chunk = cdiv(cdiv(P, s0), 32) * 32
    return cdiv(P, chunk), chunk


def n_red(Dt):
    return cdiv(Dt, 128) + 9


def _store_bf16(ref, E):
    return E + U * (ref.abs() + E) + TINY


def exact_bwd(g, e, Q, shift, scale, w_shift, w_scale, B, P, mask=None, eps=EPS6):
    """float64 reference (module docstring) -> dict: de [B P, Dt], dfeats [B P, D], dq (Q's shape), and what the bound reads.  eps: the kernel's f32
    1e-6 (the comparison with HF in float64 passes HF's literal: an all-zero row's gradient is 1 / eps-scaled)."""
    EPS6 = eps
    Dt = e.shape[-1]
    shared = Q.dim() == 2
    ed = e.double()[:B * P].view(B, P, Dt)
    Qd = Q.double()[None] if shared else Q.double()          # [nb, Q, Dt]
    nQ = Qd.shape[1]
    live = _masks(mask, B, nQ, g.device)[:, None, :]          # [B, 1, Q]
    gm = torch.where(live, g.double().view(B, P, nQ), torch.zeros((), dtype=torch.float64))
    shift = shift.double().reshape(B, P, 1)
    scale = scale.double().reshape(B, P, 1)
    ws, wc = w_shift.double().reshape(-1), w_scale.double().reshape(-1)
    ne = ed.norm(dim=-1, keepdim=True)
    inv_e = 1.0 / (ne + EPS6)
    nq = Qd.norm(dim=-1, keepdim=True)
    inv_q = 1.0 / (nq + EPS6)
    qhat = Qd * inv_q
    qb = qhat.expand(B, -1, -1)
    T = torch.einsum("bpq,bqk->bpk", gm, qb)
    gs = gm.sum(-1, keepdim=True)
    gs_abs = gm.abs().sum(-1, keepdim=True)
    et = (ed * T).sum(-1, keepdim=True)
    c = inv_e * et
    dshift = scale * gs
    dscale = c + shift * gs
    fac = torch.where(scale > 1.0, torch.ones_like(scale), scale)
    ds = dscale * fac
    dfeats = dshift * ws + ds * wc
    a = inv_e * scale
    coef = torch.where(ne > 0, c / ne.clamp_min(1e-300), torch.zeros_like(c))
    inner = T - coef * ed
    de = a * inner
    ga = gm * a
    dqh_img = torch.einsum("bpq,bpk->bqk", ga, ed)
    dqh = dqh_img.sum(0, keepdim=True) if shared else dqh_img
    dot = (qhat * dqh).sum(-1, keepdim=True)
    u = torch.where(nq > 0, Qd / nq.clamp_min(1e-300), torch.zeros_like(Qd))
    diff = dqh - u * dot
    dq = diff * inv_q
    return dict(de=de.reshape(B * P, Dt), dfeats=dfeats.reshape(B * P, -1), dq=dq[0] if shared else dq, shared=shared, B=B, P=P, Q=nQ, Dt=Dt, D=ws.numel(),
                live=live, gm=gm, ed=ed, ne=ne, inv_e=inv_e, nq=nq, inv_q=inv_q, qhat=qhat, T=T, gs=gs, gs_abs=gs_abs, et=et, c=c, shift=shift, scale=scale,
                dshift=dshift, dscale=dscale, fac=fac, ds=ds, ws=ws, wc=wc, a=a, coef=coef, inner=inner, ga=ga, dqh=dqh, dot=dot, u=u, diff=diff,
                de3=de, dfeats3=dfeats, dq3=dq)


def bounds(r):
    """-> {"de" [B P, Dt], "dfeats" [B P, D], "dq" (dq's shape)}: elementwise tolerances (module docstring)."""
    B, P, Q, Dt = r["B"], r["P"], r["Q"], r["Dt"]
    Qp = cdiv(Q, 32) * 32
    # q^
    nq = r["nq"]
    r_n = (1.0 + ULP2) / math.sqrt(1.0 - gam(n_q(Dt))) - 1.0
    d = nq + EPS6
    E_d = nq * r_n + F * (d + nq * r_n)
    r_invq = (1.0 + ULP2) / (1.0 - E_d / d) - 1.0
    r_q = (1.0 + r_invq) * (1.0 + F) - 1.0                    # [nb, Q, 1]
    qhat, gm, ed = r["qhat"], r["gm"], r["ed"]
    E_T = torch.einsum("bpq,bqk->bpk", gm.abs(), (qhat.abs() * (gam(Qp + 3) * (1.0 + r_q) + r_q)).expand(B, -1, -1)) + TINY
    # |e|, 1 / (|e| + eps6)
    nr = n_red(Dt)
    ne = r["ne"]
    r_s = (1.0 + ULP2) / math.sqrt(1.0 - gam(nr)) - 1.0
    de_ = ne + EPS6
    E_de = ne * r_s + F * (de_ + ne * r_s)
    r_inv_e = (1.0 + ULP2) / (1.0 - E_de / de_) - 1.0
    E_inv = r["inv_e"] * r_inv_e
    E_et = (1.0 + gam(nr)) * (ed.abs() * E_T).sum(-1, keepdim=True) + gam(nr) * (ed * r["T"]).abs().sum(-1, keepdim=True) + TINY
    E_c = _rnd(r["c"], _mul(r["inv_e"], E_inv, r["et"], E_et)) + TINY
    E_gs = gam(cdiv(Q, 64) + 6) * r["gs_abs"] + TINY
    E_dsh = _rnd(r["dshift"], r["scale"].abs() * E_gs) + TINY
    sg = r["shift"] * r["gs"]
    E_sg = _rnd(sg, r["shift"].abs() * E_gs) + TINY
    E_dscale = _rnd(r["dscale"], E_c + E_sg)
    E_ds = _rnd(r["ds"], r["fac"].abs() * E_dscale) + TINY
    t1, t2 = r["dshift"] * r["ws"], r["ds"] * r["wc"]
    E_df = _rnd(r["dfeats3"], _rnd(t1, r["ws"].abs() * E_dsh) + TINY + _rnd(t2, r["wc"].abs() * E_ds) + TINY) + TINY
    E_a = _rnd(r["a"], r["scale"].abs() * E_inv) + TINY
    r_div = (1.0 + ULP2) / (1.0 - r_s) - 1.0
    E_coef = torch.where(ne > 0, E_c / ne.clamp_min(1e-300) * (1.0 + r_div) + r["coef"].abs() * r_div, torch.zeros_like(ne)) + TINY
    ce = r["coef"] * ed
    E_ce = _rnd(ce, ed.abs() * E_coef) + TINY
    E_inner = _rnd(r["inner"], E_T + E_ce)
    E_pre = _rnd(r["de3"], _mul(r["a"], E_a, r["inner"], E_inner)) + TINY
    E_de = _store_bf16(r["de3"], E_pre)
    # dq
    S, chunk = split(P, Q)
    n_dq = chunk + 3 + S * (B if r["shared"] else 1) + 1
    ga = r["ga"]
    E_ga = gm.abs() * E_a * (1.0 + F) + F * ga.abs() + TINY
    term = torch.einsum("bpq,bpk->bqk", E_ga, ed.abs())
    abs_ = torch.einsum("bpq,bpk->bqk", ga.abs(), ed.abs())
    if r["shared"]:
        term, abs_ = term.sum(0, keepdim=True), abs_.sum(0, keepdim=True)
    dqh = r["dqh"]
    E_dqh = (1.0 + gam(n_dq)) * term + gam(n_dq) * abs_ + TINY
    nk = n_q(Dt)
    E_dot = (1.0 + gam(nk)) * _mul(qhat, qhat.abs() * r_q, dqh, E_dqh).sum(-1, keepdim=True) + gam(nk) * (qhat * dqh).abs().sum(-1, keepdim=True) + TINY
    r_u = (1.0 + ULP2) / (1.0 - r_n) - 1.0
    u = r["u"]
    E_ud = _rnd(u * r["dot"], _mul(u, u.abs() * r_u, r["dot"], E_dot)) + TINY
    E_diff = _rnd(r["diff"], E_dqh + E_ud)
    E_dq = _rnd(r["dq3"], _mul(r["diff"], E_diff, r["inv_q"], r["inv_q"] * r_invq)) + TINY
    return dict(de=E_de.reshape(B * P, Dt), dfeats=E_df.reshape(B * P, -1), dq=E_dq[0] if r["shared"] else E_dq)


def check_bwd(name, de, dfeats, dq, r, fails=None, b=None):
    """de bf16 / f32 [>= B P, Dt], dfeats [>= B P, D] or None, dq or None on any device against exact_bwd's record: every element inside its bound,
    nothing excluded.  -> {output: worst err / tol}."""
    b = bounds(r) if b is None else b
    rows = r["B"] * r["P"]
    worst = {"de": check(name + " de", de.detach().double().cpu()[:rows], r["de"], b["de"], fails)}
    if dfeats is not None:
        worst["dfeats"] = check(name + " dfeats", dfeats.detach().double().cpu()[:rows], r["dfeats"], b["dfeats"], fails)
    if dq is not None:
        worst["dq"] = check(name + " dq", dq.detach().double().cpu(), r["dq"], b["dq"], fails)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(B, P, Q, Dt, D, seed=0, shared=False, shared_mask=False, zero_row=False, underflow=False, poison=False):
    """The forward checker's inputs (open_vocab_reference.make_inputs: row norms of e over 2^-3 .. 2^3, query norms over 1e-3 .. 10 with one all-zero
    -- padded -- query, about a fifth of the queries masked) plus what the backward reads: rowstats f32 [B P, 2] = (shift, scale) computed in f32 from
    the same features and head, and the upstream g = 0.1 randn [B, P, Q].  zero_row: row 1 of e is all zero.  underflow: the last row's s is -120, its
    scale exactly 0.  poison: Inf and NaN alternate at the masked entries of g."""
    i = FWD.make_inputs(B, P, Q, Dt, D, seed=seed, shared=shared, masked=True)
    gen = torch.Generator(device="cpu").manual_seed(977 * seed + 13 * B + 17 * P + 19 * Q + Dt + D + 5)
    rows = B * P
    if shared_mask:
        i["mask"] = i["mask"][0].contiguous()
    f = i["feats"].float()
    shift = f @ i["w_shift"] + i["b_shift"]
    x = f @ i["w_scale"] + i["b_scale"]
    if underflow:
        x[rows - 1] = -120.0
    scale = torch.where(x > 0, x, torch.expm1(x)) + 1.0
    if underflow:
        assert float(scale[rows - 1]) == 0.0
    if zero_row:
        i["e"][min(1, rows - 1)] = 0.0
    g = 0.1 * torch.randn(B, P, Q, generator=gen)
    if poison:
        dead = ~_masks(i["mask"], B, Q, g.device)[:, None, :].expand(B, P, Q)
        bad = torch.where(torch.arange(B * P * Q).view(B, P, Q) % 2 == 0, torch.tensor(float("inf")), torch.tensor(float("nan")))
        g = torch.where(dead, bad, g)
    i.update(rowstats=torch.stack([shift, scale], 1).contiguous(), g=g, x=x)
    return i


def exact_of(i, B, P):
    return exact_bwd(i["g"], i["e"], i["queries"], i["rowstats"][:, 0], i["rowstats"][:, 1], i["w_shift"], i["w_scale"], B, P, i["mask"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
HOOKS = ("unit_jacobian", "elu_one", "mask_multiply", "no_shift", "logit_over_scale", "bank0", "dq_image0", "row_neighbour", "bf16_acc")


def _bf(x):
    return x.to(torch.bfloat16).float()


def _row_reduce(x):
    """[rows, Dt] products -> their sum in ovb_rows_kernel's order: wave w adds its 32-column tiles w, w + 4, ... in a lane, five xor steps over the 32
    lanes, the four waves in index order."""
    rows, Dt = x.shape
    xt = x.view(rows, Dt // 32, 32)
    part = torch.zeros(rows, 4, 32)
    for t in range(Dt // 32):
        part[:, t % 4] = part[:, t % 4] + xt[:, t]
    lane = torch.arange(32)
    for o in (16, 8, 4, 2, 1):
        part = part + part[..., lane ^ o]
    p = part[..., 0]
    return ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]


def _lane_sum(x):
    """[n, L] -> lane-strided sums (lane l adds elements l, l + 64, ... in order), then the 64-lane butterfly."""
    n, L = x.shape
    nch = cdiv(L, 64)
    xp = torch.zeros(n, nch * 64); xp[:, :L] = x
    xp = xp.view(n, nch, 64)
    s = torch.zeros(n, 64)
    for c in range(nch):
        s = s + xp[:, c]
    return _wave_sum32(s)


def emulate_bwd(g, e, Q, shift, scale, w_shift, w_scale, B, P, mask=None, hooks=()):
    """owl_class_logits_bwd in f32, in the source's order -> (de bf16-rounded f32 [B P, Dt], dfeats [B P, D], dq).  hooks: HOOKS (the planted errors)."""
    e = e.float()[:B * P]
    Dt = e.shape[1]
    shared = Q.dim() == 2
    Qf = (Q[None] if shared else Q).float()
    nb, nQ = Qf.shape[0], Qf.shape[1]
    eps = torch.tensor(EPS6)
    live = _masks(mask, B, nQ, g.device)[:, None, :].expand(B, P, nQ)
    g = g.float().view(B, P, nQ)
    gm = g * live.float() if "mask_multiply" in hooks else torch.where(live, g, torch.zeros(()))
    shift, scale = shift.float().reshape(-1), scale.float().reshape(-1)
    if "row_neighbour" in hooks:
        shift, scale = torch.roll(shift, -1), torch.roll(scale, -1)
    rnd = _bf if "bf16_acc" in hooks else (lambda t: t)
    # q^
    qn = torch.sqrt(_lane_sum((Qf * Qf).view(nb * nQ, Dt))).view(nb, nQ, 1)
    qinv = 1.0 / qn if "unit_jacobian" in hooks else 1.0 / (qn + eps)
    qinv = torch.where(torch.isinf(qinv), 1.0 / eps, qinv)
    qhat = Qf * qinv
    bank = lambda b: 0 if (shared or "bank0" in hooks) else b
    # row pass
    T = torch.zeros(B, P, Dt)
    for b in range(B):
        acc = torch.zeros(P, Dt)
        for q in range(nQ):
            acc = rnd(acc + gm[b, :, q, None] * qhat[bank(b), q][None, :])
        T[b] = acc
    T = T.view(B * P, Dt)
    gs = _lane_sum(gm.reshape(B * P, nQ))
    ss = _row_reduce(e * e)
    et = _row_reduce(e * T)
    nrm = torch.sqrt(ss)
    inv = 1.0 / nrm if "unit_jacobian" in hooks else 1.0 / (nrm + eps)
    inv = torch.where(torch.isinf(inv), 1.0 / eps, inv)
    c = inv * et
    dshift = scale * gs
    if "logit_over_scale" in hooks:          # the cosine term recovered from the forward's logits
        cosv = torch.stack([(e.view(B, P, Dt)[b] * inv.view(B, P, 1)[b]) @ qhat[bank(b)].t() for b in range(B)])
        lg = (cosv + shift.view(B, P, 1)) * scale.view(B, P, 1)
        dscale = (gm * (lg / scale.view(B, P, 1))).sum(-1).view(-1)
    elif "no_shift" in hooks:
        dscale = c
    else:
        dscale = c + shift * gs
    fac = torch.ones_like(scale) if "elu_one" in hooks else torch.where(scale > 1.0, torch.ones_like(scale), scale)
    ds = dscale * fac
    a = inv * scale
    coef = torch.where(nrm > 0, c / nrm, torch.zeros_like(c))
    de = _bf(a[:, None] * (T - coef[:, None] * e))
    dfeats = dshift[:, None] * w_shift.float().reshape(1, -1) + ds[:, None] * w_scale.float().reshape(1, -1)
    # dq^: slabs of `chunk` rows, added in index order
    S, chunk = split(P, nQ)
    ev, av = e.view(B, P, Dt), a.view(B, P)
    dqh = torch.zeros(nb, nQ, Dt)
    for b in range(B):
        if shared and "dq_image0" in hooks and b > 0:
            break
        for s in range(S):
            acc = torch.zeros(nQ, Dt)
            for p in range(s * chunk, min(P, (s + 1) * chunk)):
                acc = rnd(acc + (gm[b, p] * av[b, p])[:, None] * ev[b, p][None, :])
            dqh[0 if shared else b] = dqh[0 if shared else b] + acc
    dot = _lane_sum((qhat * dqh).view(nb * nQ, Dt)).view(nb, nQ, 1)
    u = torch.where(qn > 0, Qf / qn, torch.zeros_like(Qf))
    dq = (dqh - u * dot) * qinv
    return de, dfeats, dq[0] if shared else dq
