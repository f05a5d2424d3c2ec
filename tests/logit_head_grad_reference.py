"""Float64 reference, derived error bounds and a simulation for the gradients of HF's logit shift and scale: csrc/open_vocab_bwd.hip
(ovb_rows_kernel's `rowgrad` store, ovb_head_part_kernel, ovb_head_finish_kernel behind owl_class_logits_bwd_head).  Checker side; device-agnostic;
nothing here imports the package's ops.  tests/open_vocab_bwd_reference.py (R) is imported, not edited: its exact_bwd is the closed form this extends.

Reference (float64 on the kernel's exact inputs: the record of R.exact_bwd plus the bf16 features the forward read)
---------
`exact_head(r, feats)`: with dshift_r = scale_r gs_r and ds_r = (c_r + shift_r gs_r) ELU'(scale_r) of R.exact_bwd, r over all B P rows,
    dw_shift[c] = sum_r dshift_r feats[r, c]    db_shift = sum_r dshift_r    dw_scale[c] = sum_r ds_r feats[r, c]    db_scale = sum_r ds_r.
tests/test_logit_head_grad_reference.py holds it to torch autograd of HF's own OwlViTClassPredictionHead in float64 (1e-12).

Bound (elementwise, as (value, error) pairs along the kernels' operation sequence; no fitted constant; F, TINY, _rnd as in R)
 rowgrad: the row pass stores the f32 registers it multiplies into dfeats: (dshift~, E_dsh), (ds~, E_ds) are R.bounds' own pairs, restated in
   `row_scalar_bounds` (R.bounds returns the outputs' bounds only).  The store adds no rounding.
 ovb_head_part_kernel accumulates in FLOAT64: a bf16 feature (8 significand bits) times an f32 row scalar (24) is exact in f64 (53), so a term
   g~_r f_rc carries E_g |f_rc| and nothing else.  A thread adds its ceil(min(P, CHUNK) / 16) rows in ascending order, the 16 row lanes are then added
   in index order: n_chunk = ceil(min(P, CHUNK) / 16) + 16 f64 adds.  ovb_head_finish_kernel adds an image's S = ceil(P / CHUNK) partials in chunk
   order, then the B images' sums in image order, and rounds ONCE to f32:
       E = (1 + gamma64(n)) sum_r E_g |f_rc| + gamma64(n) sum_r |g_r f_rc|,  n = n_chunk + S + B,  gamma64(n) = n 2^-53 / (1 - n 2^-53)
       E_out = E + F (|ref| + E) + TINY;   the two bias gradients: the same with f = 1.
   The f64 chain lengths therefore enter at 2^-53 each: the bound is the inherited one plus half an f32 ulp at every batch size, which is why the
   kernel accumulates in f64 (its header says the same).

`emulate_head(..., hooks)` runs the row scalars in f32 and the reduction in f64 in the order the source writes them and plants errors; CPU test only,
NEVER a reference on the GPU.
"""
import torch

from tests import open_vocab_bwd_reference as R
from tests.gemm_reference import F, TINY, check, gamma as gam
from tests.layernorm_reference import _mul, _rnd
from tests.open_vocab_reference import EPS6, ULP2, cdiv, _masks

CHUNK = 256              # rows of one partial (open_vocab_bwd.hip OVB_HEAD_CHUNK): a constant, so a function of (P, D) alone
U64 = 2.0 ** -53
KEYS = ("dw_shift", "dw_scale", "db_shift", "db_scale")

# P spans three row chunks, the last one ragged (600 = 256 + 256 + 88); two images, so that image-major partial order shows
CHUNK_CASE = (2, 600, 5, 64, 128)
GPU_CASES = list(R.GPU_CASES) + [(2, 576, 31, 64, 128), CHUNK_CASE]


def gamma64(n):
    return n * U64 / (1.0 - n * U64)


def n_sum64(B, P):
    """f64 adds between a term and the output: a thread's rows, the 16 row lanes, an image's S partials, the B images."""
    return cdiv(min(P, CHUNK), 16) + 16 + cdiv(P, CHUNK) + B


def exact_head(r, feats):
    """R.exact_bwd's record + feats [>= B P, D] (bf16 / any float) -> dict dw_shift [D], dw_scale [D], db_shift [], db_scale [] in float64, and
    what the bound reads."""
    rows = r["B"] * r["P"]
    f = feats.double()[:rows]
    dsh, ds = r["dshift"].reshape(rows), r["ds"].reshape(rows)
    return dict(dw_shift=dsh @ f, dw_scale=ds @ f, db_shift=dsh.sum(), db_scale=ds.sum(), f=f, dsh=dsh, ds=ds)


def exact_head_of(i, B, P):
    """(R.exact_bwd's record, exact_head's) of R.make_inputs' dict."""
    r = R.exact_of(i, B, P)
    return r, exact_head(r, i["feats"])


def row_scalar_bounds(r):
    """-> (E_dsh, E_ds) [B P]: the bounds of the row pass's dshift and ds, R.bounds' chain up to those two registers (R's module docstring)."""
    B, P, Q, Dt = r["B"], r["P"], r["Q"], r["Dt"]
    Qp = cdiv(Q, 32) * 32
    nq = r["nq"]
    r_n = (1.0 + ULP2) / (1.0 - gam(R.n_q(Dt))) ** 0.5 - 1.0
    d = nq + EPS6
    E_d = nq * r_n + F * (d + nq * r_n)
    r_invq = (1.0 + ULP2) / (1.0 - E_d / d) - 1.0
    r_q = (1.0 + r_invq) * (1.0 + F) - 1.0
    qhat, gm, ed = r["qhat"], r["gm"], r["ed"]
    E_T = torch.einsum("bpq,bqk->bpk", gm.abs(), (qhat.abs() * (gam(Qp + 3) * (1.0 + r_q) + r_q)).expand(B, -1, -1)) + TINY
    nr = R.n_red(Dt)
    ne = r["ne"]
    r_s = (1.0 + ULP2) / (1.0 - gam(nr)) ** 0.5 - 1.0
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
    return E_dsh.reshape(B * P), E_ds.reshape(B * P)


def bounds(r, h):
    """-> {key: elementwise tolerance} of the four gradients (module docstring)."""
    E_dsh, E_ds = row_scalar_bounds(r)
    g64 = gamma64(n_sum64(r["B"], r["P"]))
    absf = h["f"].abs()
    out = {}
    for key, g, E_g in (("shift", h["dsh"], E_dsh), ("scale", h["ds"], E_ds)):
        E_w = (1.0 + g64) * (E_g @ absf) + g64 * (g.abs() @ absf)
        E_b = (1.0 + g64) * E_g.sum() + g64 * g.abs().sum()
        out["dw_" + key] = _rnd(h["dw_" + key], E_w) + TINY
        out["db_" + key] = _rnd(h["db_" + key], E_b) + TINY
    return out


def split_head(dhead, D):
    """f32 [2 D + 2] laid out w_shift | w_scale | b_shift | b_scale -> the four tensors by KEYS."""
    return dict(dw_shift=dhead[:D], dw_scale=dhead[D:2 * D], db_shift=dhead[2 * D], db_scale=dhead[2 * D + 1])


def check_head(name, dhead, r, h, fails=None, b=None):
    """dhead f32 [2 D + 2] on any device against exact_head's record: every element inside its bound, nothing excluded.  -> {key: worst err / tol}."""
    b = bounds(r, h) if b is None else b
    got = split_head(dhead.detach().double().cpu(), r["D"])
    return {k: check(f"{name} {k}", got[k].reshape(-1), h[k].reshape(-1), b[k].reshape(-1), fails) for k in KEYS}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# simulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
HOOKS = ("dscale_for_ds", "swapped", "db_shift_gs", "image0", "row_neighbour", "rows_past", "bf16_acc", "ragged_chunk_dropped")


def emulate_rowgrad(g, e, Q, shift, scale, B, P, mask=None, hooks=()):
    """ovb_rows_kernel's row scalars in f32, in the source's order -> (dshift, ds, gs) f32 [B P]."""
    e = e.float()[:B * P]
    Dt = e.shape[1]
    shared = Q.dim() == 2
    Qf = (Q[None] if shared else Q).float()
    nb, nQ = Qf.shape[0], Qf.shape[1]
    eps = torch.tensor(EPS6)
    live = _masks(mask, B, nQ, g.device)[:, None, :].expand(B, P, nQ)
    gm = torch.where(live, g.float().view(B, P, nQ), torch.zeros(()))
    shift, scale = shift.float().reshape(-1), scale.float().reshape(-1)
    qn = torch.sqrt(R._lane_sum((Qf * Qf).view(nb * nQ, Dt))).view(nb, nQ, 1)
    qinv = 1.0 / (qn + eps)
    qhat = Qf * qinv
    T = torch.zeros(B, P, Dt)
    for b in range(B):
        acc = torch.zeros(P, Dt)
        for q in range(nQ):
            acc = acc + gm[b, :, q, None] * qhat[0 if shared else b, q][None, :]
        T[b] = acc
    T = T.view(B * P, Dt)
    gs = R._lane_sum(gm.reshape(B * P, nQ))
    ss = R._row_reduce(e * e)
    et = R._row_reduce(e * T)
    inv = 1.0 / (torch.sqrt(ss) + eps)
    c = inv * et
    dshift = scale * gs
    dscale = c + shift * gs
    ds = dscale if "dscale_for_ds" in hooks else dscale * torch.where(scale > 1.0, torch.ones_like(scale), scale)
    return dshift, ds, gs


def _seq(x, rnd):
    """[n, ...] -> the sum over dim 0 in ascending order, `rnd` after every add."""
    acc = torch.zeros_like(x[0])
    for k in range(x.shape[0]):
        acc = rnd(acc + x[k])
    return acc


def emulate_head(g, e, Q, shift, scale, feats, B, P, mask=None, hooks=()):
    """owl_class_logits_bwd_head's four gradients: the row scalars in f32, the reduction in f64 in the kernels' order, one rounding to f32
    -> f32 [2 D + 2] laid out w_shift | w_scale | b_shift | b_scale.  hooks: HOOKS (the planted errors)."""
    dshift, ds, gs = emulate_rowgrad(g, e, Q, shift, scale, B, P, mask, hooks)
    rows = B * P
    f = feats.float()[:rows].double()
    D = f.shape[1]
    if "row_neighbour" in hooks:
        dshift, ds = torch.roll(dshift, -1), torch.roll(ds, -1)
    rg = torch.stack([dshift, ds], 1).double()               # rowgrad [B P, 2], widened as the kernel widens it
    if "rows_past" in hooks:                                  # one row past B P joins the last chunk (what lies there: the first row again)
        f, rg = torch.cat([f, f[:1]]), torch.cat([rg, rg[:1]])
    rnd = (lambda t: t.to(torch.bfloat16).double()) if "bf16_acc" in hooks else (lambda t: t)
    S = cdiv(P, CHUNK)
    images = []
    for b in range(B):
        if "image0" in hooks and b > 0:
            break
        parts = []
        for s in range(S):
            pbeg, pend = s * CHUNK, min(P, (s + 1) * CHUNK)
            if "ragged_chunk_dropped" in hooks and pend - pbeg < CHUNK:
                continue
            lo, hi = b * P + pbeg, b * P + pend
            if "rows_past" in hooks and b == B - 1 and s == S - 1:
                hi += 1
            n = hi - lo
            npad = cdiv(n, 16) * 16
            ff, gg = torch.zeros(npad, D, dtype=torch.float64), torch.zeros(npad, 2, dtype=torch.float64)
            ff[:n], gg[:n] = f[lo:hi], rg[lo:hi]
            # term [which, row, D] and the scalars themselves; thread (row lane rl) owns rows rl, rl + 16, ...
            term = (gg.t()[:, :, None] * ff[None]).view(2, npad // 16, 16, D)
            cols = _seq(_seq(term.permute(1, 2, 0, 3), rnd), rnd)                   # over a thread's rows, then over the 16 row lanes -> [2, D]
            scal = _seq(_seq(gg.view(npad // 16, 16, 2), rnd), rnd)                # -> [2]
            parts.append(torch.cat([cols[0], cols[1], scal]))
        images.append(_seq(torch.stack(parts), rnd) if parts else torch.zeros(2 * D + 2, dtype=torch.float64))          # an image's chunks, ascending
    tot = _seq(torch.stack(images), rnd)                                                                                 # then the images, ascending
    out = tot.float()
    if "swapped" in hooks:
        out = torch.cat([out[D:2 * D], out[:D], out[2 * D + 1:], out[2 * D:2 * D + 1]])
    if "db_shift_gs" in hooks:
        out[2 * D] = gs.double().sum().float()
    return out


def emulate_head_of(i, B, P, hooks=()):
    return emulate_head(i["g"], i["e"], i["queries"], i["rowstats"][:, 0], i["rowstats"][:, 1], i["feats"], B, P, i["mask"], hooks=hooks)
