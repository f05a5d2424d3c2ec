"""Float64 references, derived error bounds, input profiles and an f32 simulation for the detection heads: csrc/heads.hip (qhat_kernel,
class_sims_kernel, box_final_rows_kernel<1/2>), csrc/class_head_wide.hip (qhat_wide_kernel, class_sims_wide_kernel, class_sims_wide_bwd_kernel<NT>,
qhat_wide_bwd_kernel) and csrc/backward.hip (class_sims_bwd_kernel, class_sims_bwd_pf_kernel<2/3>, qhat_bwd_kernel, box_final_bwd_kernel and the two
slab reduces of gemm.hip behind it).  Checker side; device-agnostic: every function works on whatever device its inputs live on, and nothing here
imports the package's Python ops.

Reference (float64 on the kernel's exact inputs: f32 values, bf16 values upcast; eps6 = the f32 nearest 1e-6, as the kernels hold it)
---------
`exact_qhat(Q)`   n = |Q_j|, qhat = Q / n + eps6 (ref src/models.py:31-33: the eps is added to the quotient, reproduced literally).
`exact_sims(e, qhat, C)`   inv = 1 / (|e| + eps6), all 3C products p = inv (e . qhat_j), sims = max of each triple, argmax = the FIRST maximal prompt
    (torch's rule and the kernel's strict `>`, heads.hip:119-121), margin = best - second best per (row, class).  qhat is an INPUT: any f32 table.
`exact_sims_bwd(dsims, e, qhat, given_sims, given_argmax, given_inv, wide)`   the closed form at the values the kernel is GIVEN, |e| formed in
    float64 from e:  de = inv sum_c g_c qhat_j*(c) - (sum_c g_c s_c) inv e / |e|  (backward.hip:397-398); the second term is 0 on an all-zero row
    (the norm's subgradient at 0 is 0).  G = bf16(fl32(dsims inv)) at the routed column, +0 elsewhere (a bit test: one f32 multiply).  `wide` only
    changes the column of class c's prompt p: 3 c + p narrow, 32 (c / 10) + 3 (c % 10) + p wide (class_head_wide.hip:6-9).
`exact_qhat_bwd(dqhat, Q, old)`   dQ = old + (dqhat - (dqhat . Qn) Qn) / |Q|, Qn = Q / |Q| (backward.hip:539).
`exact_box_final(h, w2, b2, box_bias, P)`   x = h W2^T + b2 + box_bias[r % P], sig = sigmoid(x), boxes = (cx - w/2, cy - h/2, cx + w/2, cy + h/2).
`exact_box_final_bwd(dboxes, given_sig, h1, u1, w2, old)`   dlin = (g0 + g2, g1 + g3, (g2 - g0) / 2, (g3 - g1) / 2), dpre = dlin s (1 - s),
    du1 = (dpre W2) gelu'(u1), dW2 = old + dpre^T h1, db2 = old + sum dpre, colsum = old + sum_rows du1 (du1 BEFORE its bf16 rounding, as the kernel adds it).
A wide column carries the bits of the narrow call on its block (test_wide_columns_are_the_narrow_kernels_bits), so the same reference serves both.
tests/test_heads_reference.py shows every closed form equal to float64 autograd of the reference expression at exact statistics.

Bounds (elementwise, derived, no fitted constant)
-------------------------------------------------
u, f, T, gamma(n) are gemm_reference.py:18-20; _V (one rounding per WRITTEN operation, for code whose contraction is left to the compiler), mul and
rnd are layernorm_reference.py:20,303-326.
 ASSUMPTION H1: sqrtf, the f32 division, expf are within 2 ulp = 4 f (relative) of the exact result.  This ROCm tree documents no accuracy for the
   device libm (layernorm_reference.py Assumption 1 searched it), so the 2 ulp budget the issue sets for that event is used (`ULP2`).
 ASSUMPTION H2: v_mfma_f32_32x32x2_f32 rounds every product and every add to nearest; the order of the two products inside one instruction is not
   documented.  The INSTRUCTIONS are issued in the order the source writes them (heads.hip:91-94: one per k of a lane's float4, lanes hi = 0 / 1
   supplying the two products), Dt / 2 of them in a row into one accumulator (64 per 128-chunk, a masked half-chunk adding exact zeros), so, as
   gemm_reference.py:24-27 counts its MFMAs, a product passes its own rounding, at most 2 adds inside its instruction and one add per later
   instruction:   n_dot = 64 ceil(Dt / 128) + 3   (`n_dot(Dt)`),  |acc~ - acc| <= gamma(n_dot) sum_k |e_k qhat_k|.  This is half the
   order-independent gamma(Dt + 1), which the first draft used and which excused more than 1 % of the `trained` arg-max pairs at Dt = 768.
   The wide backward's product over the routed tile (class_head_wide.hip:206-243) has C live terms among exact zeros: n = C + 1, any order.
 qhat (heads.hip:17-21): lane l adds v v for k = l, l + 64, ...: ceil(Dt / 64) adds, six butterfly levels (common.h:142-146), the products rounded
   (one rounding per written operation): n_q = ceil(Dt / 64) + 6 + 1.  n~ = sqrtf: r_n = (1 + 4 f) / sqrt(1 - gamma(n_q)) - 1 (both sides);
   q / n~: r = (1 + 4 f) / (1 - r_n) - 1; + eps6: one rounding.   qnorm: n r_n.
 row norm of class_sims_kernel (heads.hip:87-90,105-106; contraction OFF, so the count is exact): a lane owns 64 consecutive columns of each 128-chunk:
   per float4 four rounded squares, three adds, one accumulate; 16 float4 per chunk; the two halves meet in one add:
       n_ss = 1 + 3 + 16 ceil(Dt / 128) + 1      (`n_ss(Dt)`; longest path of one element; the simulation runs the same chain)
   nrm~ = sqrtf(ss~): r_s = (1 + 4 f) / sqrt(1 - gamma(n_ss)) - 1;  d~ = fl(nrm~ + eps6): E_d = nrm r_s + f (d + nrm r_s);
   inv~ = 1 / d~: r_inv = (1 + 4 f) / (1 - E_d / d) - 1.
 sims (heads.hip:91-94,117): acc by the MFMA: E_acc = gamma(n_dot) sum |e qhat| + T;  v = fl(acc~ inv~): mul + one rounding.  The max of 3: the
   error of a maximum is at most the largest of the three errors: tol = max_p E_v.  argmax: where the reference margin exceeds E_best + E_second the
   prompt must be the reference's; elsewhere any prompt p with p_best - p_p <= E_best + E_p is accepted (`check_argmax`).
 class head backward (backward.hip:415-449,494-524; class_head_wide.hip:185-197,256).  gs = wave_sum(fl(ds s)): n_gs = ceil(C / 64) + 6 + 1.
   The kernels RECOVER |e| from the given inv~: t = fl(1 / inv~) = (|e| + eps6)(1 + d), |d| <= r_t = (1 + 4 f) / (1 - r_inv) - 1 (the given inv's own
   forward error and the division);  nrm~ = fl(t - eps6): E_nrm = (|e| + eps6) r_t + f (|e| + .): relative to |e| that is AMPLIFIED by
   (|e| + eps6) / |e|: rel_n = E_nrm / (|e| - E_nrm), infinite once E_nrm >= |e| (|e| below about 3e-12: no profile goes there).
   coef = fl(fl(gs inv) / nrm~): E_coef = (E_a / |e|)(1 + rel_n) + |coef| rel_n, + 4 f.  On an all-zero row e = 0 multiplies it: the term is 0
   and so is its bound, PROVIDED coef is finite -- a NaN there is outside every bound.
   de: t0 = fl(coef e_k); the C routed terms g_c q (g_c = fl(ds inv): one rounding, the product one, the add one; wide: the MFMA over C live
   products, then fl(inv acc)): n = C + 3 on sum |g q| + |t0| covers both forms.  de is rounded once to bf16: tol = E + u (|ref| + E) + T.
   G, e_bf16: bit tests.
 qhat backward (backward.hip:540-550): _V through ss, dt (n_q each), n = sqrtf, qn = q / n, (dt / n) qn, the difference, / n, + old.
 box_final (heads.hip:198-224; contraction off): 8 NC fmaf + 6 levels: E_v = gamma(8 NC + 6) sum |h w|; two bias adds; e = expf(-x):
   r_e = exp(E_x) (1 + 4 f) - 1; 1 + e: f; 1 / .: 4 f: r_s = (1 + 4 f) / ((1 - (1 - s) r_e)(1 - f)) - 1 (gemm_reference.py:38), RELATIVE to s: a
   saturated width of 1e-4 is held to a few f of itself, not to 1e-6 absolute.  + T: expf overflows to inf from x = -88.7 on and the kernel
   returns 0 where the exact value is below T.  boxes: fl(cx -+ 0.5 w): E_cx + 0.5 E_w and one rounding.
 box_final backward (backward.hip:620-685): _V through dlin, dpre = (dlin s)(1 - s), dh1 (4 products, 3 adds), o = dh1 dgelu_erf_f(u1) with
   gemm_reference.dgelu_eval as the evaluation error of dgelu_erf_f (its Assumption on A&S 7.1.26 included); du1 = bf16(o).
   Row reductions, adds counted as the source orders them: inside a block rows in order: rpb adds (rpb = clamp(ceil(rows / 512), 8, 64));
   db2: each row sits in one thread (rpb <= 64 < 256): wave_sum (6) + four waves in order (3); owl_slab_reduce_impl (gemm.hip):
   nblk >= 128 (and n / 4 <= 8192: always here) -> tall_reduce_kernel: lane g adds slabs g, g + 8, ... in order (ceil(nblk / 8)), then old + the 8
   lane sums in order (8); else slab_reduce_kernel: old + slab 0 + slab 1 ... in order (nblk):   `n_reduce(nblk)`
       tol = gamma(n) (sum_rows (|term| + E_term) + |old|) + sum_rows E_term + T,   n = rpb + n_reduce (dW2, colsum), 9 + n_reduce (db2).

Profiles (`make_inputs` class head, `make_box_inputs` box head) -- tests/test_heads_reference.py asserts that each reaches what it names
--------
 randn      e = 0.7 randn, Q = randn: what every earlier test runs.
 trained    e rows with norms 2^-6 .. 2^6, three channels 16 x larger; a class's prompts = one direction + 10 % noise: cosine >= 0.98, small margins.
 ties       class c % 3 == 0: three identical prompts (argmax 0); == 1: prompts 1 and 2 identical (never 2); == 2: prompts that differ only in
            columns where every e is exactly 0: the three products are bit-identical by construction (argmax 0).
 tiny       rows of norm 1e-3 / 1e-5 / 1e-7 in turn, every seventh row exactly zero.
 aligned    randn inputs, dsims = a sims + 1e-3 noise.
 saturated  (box head) pre-activations +-(8 .. 40), every fifth row -(90 .. 100) (expf overflows); dboxes with g2 ~ g0, g3 ~ g1 (g.z - g.x cancels).

`emulate_*` simulate the kernels in f32 in the order the source writes it and take `hooks` that plant errors; CPU test only, NEVER a reference on the GPU.
"""
import math

import torch

from tests.gemm_reference import F, TINY, U, bf16_round, bits, check, dgelu_erf_f32, dgelu_eval, gamma as gam, gelu_d1, ratios, untouched  # noqa: F401
from tests.layernorm_reference import _V, _fma32, _mul, _rnd, _wave_sum, padded, store_bf16  # noqa: F401

EPS6 = float(torch.tensor(1e-6, dtype=torch.float32))
ULP2 = 4.0 * F           # ASSUMPTION H1: 2 ulp
INF = float("inf")


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the launchers' choices, recomputed on the host
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sims_waves(rows):                       # heads.hip:132-136
    return min(10, max(4, cdiv(cdiv(rows, 32), 256)))


def sims_bwd_rpw(rows):                     # backward.hip:561-562
    return min(18, max(2, cdiv(rows, 4096)))


def sims_bwd_kernel(Dt):
    return "pf" if Dt in (512, 768) else "generic"


def _wave_counts(rows, per):
    out = {per} if rows >= per else set()
    if rows % per:
        out.add(rows % per)
    return out


def sims_bwd_exits(rows):
    """how the waves of a launch leave class_sims_bwd_pf_kernel's 4-row rotation (backward.hip:528-536)."""
    return {("cond", "break1", "break2", "break3")[n % 4] for n in _wave_counts(rows, sims_bwd_rpw(rows))}


def sims_bwd_odd_tail(rows):
    """class_sims_bwd_kernel's `if (r < row1)` tail (backward.hip:460): a wave with an odd row count."""
    return any(n % 2 for n in _wave_counts(rows, sims_bwd_rpw(rows)))


def wide_nt(Dt):                            # class_head_wide.hip:287-295
    pw = cdiv(Dt // 32, 4)
    return 1 if pw <= 1 else 2 if pw <= 2 else 4 if pw <= 4 else 6 if pw <= 6 else 8


def wide_blocks(C):
    return cdiv(C, 10)


def wide_qp(C):
    return cdiv(32 * wide_blocks(C), 256) * 256


def box_bwd_rpb(rows):                      # backward.hip:692-695
    return min(64, max(8, cdiv(rows, 512)))


def box_bwd_blocks(rows):
    return cdiv(rows, box_bwd_rpb(rows))


def box_bwd_forms(rows):
    """(rpb, rows of the last block, tall reduce, a block whose row count is no multiple of 4)."""
    rpb = box_bwd_rpb(rows)
    counts = _wave_counts(rows, rpb)
    return {"rpb": rpb, "ragged": bool(rows % rpb), "tall": box_bwd_blocks(rows) >= 128, "nr_mod4": any(n % 4 for n in counts)}


def n_reduce(nblk):
    return cdiv(nblk, 8) + 8 if nblk >= 128 else nblk


def n_q(Dt):
    return cdiv(Dt, 64) + 6 + 1


def n_dot(Dt):
    return 64 * cdiv(Dt, 128) + 3


def n_ss(Dt):
    return 1 + 3 + 16 * cdiv(Dt, 128) + 1


def prompt_cols(C, wide, device=None):
    """[C] column of class c's first prompt in the query table / in G."""
    c = torch.arange(C, device=device)
    return 32 * (c // 10) + 3 * (c % 10) if wide else 3 * c


def table_rows(C, wide):
    return 32 * wide_blocks(C) if wide else 32


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def exact_qhat(Q):
    q = Q.double()
    ss = (q * q).sum(-1, keepdim=True)
    n = ss.sqrt()
    qn = q / n
    return {"q": q, "ss": ss, "n": n[:, 0], "qn": qn, "qhat": qn + EPS6}


def to_table(qhat_rows, C, wide):
    """[3C, Dt] -> the [32 (nblk), Dt] table the kernels read: zero rows at 30 / 31 and past the last class."""
    t = torch.zeros(table_rows(C, wide), qhat_rows.shape[1], dtype=qhat_rows.dtype, device=qhat_rows.device)
    j = torch.arange(3 * C, device=qhat_rows.device)
    t[(32 * (j // 30) + j % 30) if wide else j] = qhat_rows
    return t


def exact_sims(e, qhat, C, wide=False):
    ed, qd = e.double(), qhat.double()
    rows = ed.shape[0]
    cols = (prompt_cols(C, wide, ed.device)[:, None] + torch.arange(3, device=ed.device)).reshape(-1)
    qd = qd[cols]
    nrm = (ed * ed).sum(-1).sqrt()
    inv = 1.0 / (nrm + EPS6)
    dots = ed @ qd.t()
    prods = dots * inv[:, None]
    p3 = prods.view(rows, C, 3)
    best, arg = p3[..., 0], torch.zeros(rows, C, dtype=torch.long, device=ed.device)
    for p in (1, 2):
        better = p3[..., p] > best
        best, arg = torch.where(better, p3[..., p], best), torch.where(better, torch.full_like(arg, p), arg)
    others = p3.clone()
    others.scatter_(2, arg[..., None], -INF)
    second, arg2 = others.max(-1)
    return {"nrm": nrm, "inv": inv, "dots": dots, "dots_abs": ed.abs() @ qd.abs().t(), "prods": prods, "sims": best, "argmax": arg,
            "second": arg2, "margin": best - second, "Dt": ed.shape[1], "C": C}


def exact_sims_bwd(dsims, e, qhat, given_sims, given_argmax, given_inv, wide=False):
    ds, ed, qd = dsims.double(), e.double(), qhat.double()
    rows, C = ds.shape
    inv, sm, am = given_inv.double(), given_sims.double(), given_argmax.long()
    j = prompt_cols(C, wide, ed.device)[None] + am
    nrm = (ed * ed).sum(-1).sqrt()
    gs = (ds * sm).sum(-1)
    coef = torch.where(nrm > 0, gs * inv / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(nrm))
    gq, gq_abs = torch.zeros_like(ed), torch.zeros_like(ed)
    for c in range(C):
        t = (ds[:, c] * inv)[:, None] * qd[j[:, c]]
        gq, gq_abs = gq + t, gq_abs + t.abs()
    W = wide_qp(C) if wide else 32
    g32 = (dsims.float() * given_inv.float()[:, None]).bfloat16()
    G = torch.zeros(rows, W, dtype=torch.bfloat16, device=ed.device)
    G.scatter_(1, j, g32)
    return {"de": gq - coef[:, None] * ed, "G": G, "e_bf16": e.float().bfloat16(), "gq_abs": gq_abs, "coef": coef, "nrm": nrm, "inv": inv,
            "gs": gs, "gs_abs": (ds * sm).abs().sum(-1), "e": ed, "C": C}


def exact_qhat_bwd(dqhat, Q, old):
    q, dh = Q.double(), dqhat.double()
    n = (q * q).sum(-1, keepdim=True).sqrt()
    qn = q / n
    return {"dq": old.double() + (dh - (dh * qn).sum(-1, keepdim=True) * qn) / n, "q": q, "dh": dh, "old": old.double()}


def _corners(s):
    return torch.stack([s[:, 0] - 0.5 * s[:, 2], s[:, 1] - 0.5 * s[:, 3], s[:, 0] + 0.5 * s[:, 2], s[:, 1] + 0.5 * s[:, 3]], -1)


def exact_box_final(h, w2, b2, box_bias, P):
    hd, wd = h.double(), w2.double()
    rows = hd.shape[0]
    bb = box_bias.double()[torch.arange(rows, device=hd.device) % P]
    v = hd @ wd.t()
    x = v + b2.double() + bb
    s = torch.sigmoid(x)
    return {"v": v, "v_abs": hd.abs() @ wd.abs().t(), "x1": v + b2.double(), "x": x, "sig": s, "boxes": _corners(s), "D": hd.shape[1]}


def exact_box_final_bwd(dboxes, given_sig, h1, u1, w2, old=None):
    g, s, h, u, w = dboxes.double(), given_sig.double(), h1.double(), u1.double(), w2.double()
    dlin = torch.stack([g[:, 0] + g[:, 2], g[:, 1] + g[:, 3], 0.5 * (g[:, 2] - g[:, 0]), 0.5 * (g[:, 3] - g[:, 1])], -1)
    dpre = dlin * s * (1.0 - s)
    du1 = (dpre @ w) * gelu_d1(u)
    old = old or {}
    o = lambda k: old[k].double() if k in old else 0.0
    return {"du1": du1, "dW2": o("dW2") + dpre.t() @ h, "db2": o("db2") + dpre.sum(0), "colsum": o("colsum") + du1.sum(0), "dpre": dpre,
            "in": {"g": g, "s": s, "h": h, "u": u, "w": w}}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _sqrt_rel(g):
    return (1.0 + ULP2) / math.sqrt(1.0 - g) - 1.0


def _div(a, b):
    """_V of a / b, the division within 2 ulp (H1)."""
    r = a.v / b.v
    E = (a.E + r.abs() * b.E) / (b.v.abs() - b.E)
    return _V(r, E + ULP2 * (r.abs() + E) + TINY)


def bounds_qhat(r):
    Dt = r["q"].shape[1]
    r_n = _sqrt_rel(gam(n_q(Dt)))
    r_div = (1.0 + ULP2) / (1.0 - r_n) - 1.0
    return {"qnorm": r["n"] * r_n + TINY, "qhat": _rnd(r["qhat"], r["qn"].abs() * r_div) + TINY}


def inv_rel(nrm, Dt):
    """relative forward error of the saved 1 / (|e| + eps6)."""
    r_s = _sqrt_rel(gam(n_ss(Dt)))
    d = nrm + EPS6
    E_d = _rnd(d, nrm * r_s)
    return (1.0 + ULP2) / (1.0 - E_d / d) - 1.0


def bounds_sims(r):
    """-> {"inv": [rows], "prods": [rows, 3C] (every product before the max), "sims": [rows, C]}."""
    rows, C = r["sims"].shape
    E_inv = r["inv"] * inv_rel(r["nrm"], r["Dt"]) + TINY
    E_dot = gam(n_dot(r["Dt"])) * r["dots_abs"] + TINY
    E_p = _rnd(r["prods"], _mul(r["dots"], E_dot, r["inv"][:, None], E_inv[:, None])) + TINY
    return {"inv": E_inv, "prods": E_p, "sims": E_p.view(rows, C, 3).amax(-1)}


def check_argmax(name, got, r, E_p, fails=None, tie_kind=None):
    """arg-max rule of the docstring.  tie_kind [C] (profile `ties`): 1 / 3 = bit-identical triple: the first prompt outright; 2 = prompts 1 and 2
    bit-identical: never 2.  An all-zero row of e likewise gives three exact zeros: prompt 0 outright.  Returns the share of (row, class) pairs excused from equality."""
    rows, C = got.shape
    g = got.long()
    p3, E3 = r["prods"].view(rows, C, 3), E_p.view(rows, C, 3)
    a, b = r["argmax"][..., None], r["second"][..., None]
    strict = r["margin"] > (E3.gather(2, a) + E3.gather(2, b))[..., 0]
    inr = g < 3
    gi = g.clamp(max=2)[..., None]
    near = ((p3.gather(2, a) - p3.gather(2, gi)) <= (E3.gather(2, a) + E3.gather(2, gi)))[..., 0]
    ok = inr & ((g == r["argmax"]) | (~strict & near))
    zero = (r["dots_abs"].view(rows, C, 3) == 0).all(-1)          # every product of the three dots is exactly 0 (an all-zero e row): three +0, so
    ok = ok & (~zero | (g == 0))                                  # the first prompt outright, by bit-identity -- not an excused pair
    strict = strict | zero
    if tie_kind is not None:
        tk = tie_kind.to(g.device)[None].expand(rows, C)
        ok = ok & torch.where((tk == 1) | (tk == 3), g == 0, torch.ones_like(ok)) & torch.where(tk == 2, g != 2, torch.ones_like(ok))
    nb = int((~ok).sum())
    if nb:
        msg = f"{name}: {nb}/{ok.numel()} arg-max prompts are neither the reference's nor within the bound of it; first at {(~ok).nonzero()[:6].tolist()}"
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return float((~strict).double().mean())


def bounds_sims_bwd(x, Dt):
    """x = exact_sims_bwd(...).  -> {"de": tol [rows, Dt]}."""
    C, e, nrm, inv, coef = x["C"], x["e"], x["nrm"], x["inv"], x["coef"]
    E_gs = gam(cdiv(C, 64) + 6 + 1) * x["gs_abs"] + TINY
    r_t = (1.0 + ULP2) / (1.0 - inv_rel(nrm, Dt)) - 1.0
    E_t = (nrm + EPS6) * r_t
    E_nrm = E_t + F * (nrm + E_t)
    rel_n = torch.where(nrm > E_nrm, E_nrm / (nrm - E_nrm).clamp(min=TINY), torch.full_like(nrm, INF))
    a = x["gs"] * inv
    E_a = _rnd(a, inv * E_gs)
    safe = torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    E_c = (E_a / safe) * (1.0 + rel_n) + coef.abs() * rel_n
    E_c = E_c + ULP2 * (coef.abs() + E_c) + TINY
    t0 = coef[:, None] * e
    E_t0 = torch.where(e == 0, torch.zeros_like(e), _rnd(t0, e.abs() * E_c[:, None]))
    E = E_t0 + gam(C + 3) * (x["gq_abs"] + t0.abs() + E_t0) + TINY
    return {"de": store_bf16(x["de"], E), "de_f32": E}


def bounds_qhat_bwd(x):
    q, dh = _V(x["q"]), _V(x["dh"])
    Dt = x["q"].shape[1]
    ns = n_q(Dt) - 1
    ss, dt = (q * q).mean(ns, 1), (q * dh).mean(ns, 1)
    nv = ss.v.sqrt()
    n = _V(nv, nv * ((1.0 + ULP2) / torch.sqrt(1.0 - ss.E / ss.v) - 1.0) + TINY)
    one = lambda t: _V(t.v.expand_as(q.v), t.E.expand_as(q.v))
    qn = _div(q, one(n))
    t = dh - _div(one(dt), one(n)) * qn
    return {"dq": (_div(t, one(n)) + _V(x["old"])).E + TINY}


def bounds_box_final(r):
    NC = 1 if r["D"] <= 512 else 2
    E_v = gam(8 * NC + 6) * r["v_abs"] + TINY
    E_x = _rnd(r["x"], _rnd(r["x1"], E_v))
    s = r["sig"]
    r_e = torch.expm1(E_x + math.log1p(ULP2))
    r_s = (1.0 + ULP2) / ((1.0 - (1.0 - s) * r_e).clamp(min=TINY) * (1.0 - F)) - 1.0
    E_s = s * r_s + TINY
    b = r["boxes"]
    E_b = torch.stack([E_s[:, 0] + 0.5 * E_s[:, 2], E_s[:, 1] + 0.5 * E_s[:, 3], E_s[:, 0] + 0.5 * E_s[:, 2], E_s[:, 1] + 0.5 * E_s[:, 3]], -1)
    return {"sig": E_s, "boxes": _rnd(b, E_b) + TINY}


def bounds_box_final_bwd(x, old=None):
    i = x["in"]
    rows, D = i["h"].shape
    G, S = [_V(i["g"][:, k:k + 1]) for k in range(4)], [_V(i["s"][:, k:k + 1]) for k in range(4)]
    half = lambda t: _V(0.5 * t.v, 0.5 * t.E)
    dl = [G[0] + G[2], G[1] + G[3], half(G[2] - G[0]), half(G[3] - G[1])]
    one = _V(torch.ones_like(S[0].v))
    dp = [(dl[k] * S[k]) * (one - S[k]) for k in range(4)]
    Wk = [_V(i["w"][k:k + 1]) for k in range(4)]
    dh1 = ((dp[0] * Wk[0] + dp[1] * Wk[1]) + dp[2] * Wk[2]) + dp[3] * Wk[3]
    o = dh1 * _V(gelu_d1(i["u"]), dgelu_eval(i["u"]))
    H = _V(i["h"])
    rpb, nr = box_bwd_rpb(rows), n_reduce(box_bwd_blocks(rows))
    old = old or {}

    def red(t, n, key):
        ov = old[key].double().abs() if key in old else 0.0
        return gam(n) * ((t.v.abs() + t.E).sum(0) + ov) + t.E.sum(0) + TINY

    tW = [dp[k] * H for k in range(4)]
    ow = old.get("dW2")
    dW2 = torch.stack([gam(rpb + nr) * ((tW[k].v.abs() + tW[k].E).sum(0) + (ow[k].double().abs() if ow is not None else 0.0)) + tW[k].E.sum(0) + TINY
                       for k in range(4)])
    dpv = _V(torch.cat([t.v for t in dp], 1), torch.cat([t.E for t in dp], 1))
    return {"du1": store_bf16(x["du1"], o.E), "dW2": dW2, "db2": red(dpv, 9 + nr, "db2"), "colsum": red(o, rpb + nr, "colsum")}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input profiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILES = ("randn", "trained", "ties", "tiny", "aligned")
BOX_PROFILES = ("randn", "saturated")
TIE_COLS = (5, 6, 7)           # the columns in which the prompts of an "orthogonal" class differ, and every e of `ties` is exactly 0
NARROW_C = (1, 3, 10)
WIDE_C = (11, 80, 81, 384)


def _gen(seed, *dims):
    return torch.Generator(device="cpu").manual_seed(seed * 1000003 + sum(d * m for d, m in zip(dims, (10007, 101, 7, 3))))


def qhat_f32(Q):
    """the f32 nearest to the exact qhat: an input table for the class-sims kernels (NOT the qhat kernels' reference: that is exact_qhat)."""
    return exact_qhat(Q)["qhat"].float()


def make_inputs(profile, rows, Dt, C, seed, wide=False):
    """Seeded class-head inputs on the CPU: e [rows, Dt] f32, Q [3C, Dt] f32, qhat = the [32 (nblk), Dt] f32 table the class-sims kernels are given,
    tie_kind [C] (see check_argmax; zeros outside `ties`)."""
    g = _gen(seed, rows, Dt, C)
    e = 0.7 * torch.randn(rows, Dt, generator=g)
    Q = torch.randn(3 * C, Dt, generator=g)
    tie_kind = torch.zeros(C, dtype=torch.long)
    if profile == "trained":
        e = e / e.norm(dim=-1, keepdim=True) * 2.0 ** (12.0 * torch.rand(rows, 1, generator=g) - 6.0)
        idx = torch.randperm(Dt, generator=g)[:3]
        e[:, idx] = e[:, idx] * 16.0
        base = torch.randn(C, 1, Dt, generator=g)
        Q = (base + 0.1 * torch.randn(C, 3, Dt, generator=g)).reshape(3 * C, Dt)
    elif profile == "tiny":
        scale = torch.tensor([1e-3, 1e-5, 1e-7])[torch.arange(rows) % 3][:, None]
        e = e / e.norm(dim=-1, keepdim=True) * scale
        e[0::7] = 0.0
    elif profile == "ties":
        e[:, list(TIE_COLS)] = 0.0
    elif profile not in ("randn", "aligned"):
        raise ValueError(profile)
    qh = qhat_f32(Q)
    if profile == "ties":
        qh = qh.view(C, 3, Dt).clone()
        for c in range(C):
            kind = c % 3
            if kind == 0:
                qh[c, 1:] = qh[c, 0]
                tie_kind[c] = 1
            elif kind == 1:
                qh[c, 2] = qh[c, 1]
                tie_kind[c] = 2
            else:
                keep = qh[c, :, list(TIE_COLS)].clone()
                qh[c, 1:] = qh[c, 0]
                qh[c, :, list(TIE_COLS)] = keep + torch.tensor([0.0, 0.25, -0.25])[:, None]
                tie_kind[c] = 3
        qh = qh.reshape(3 * C, Dt)
    return {"e": e.float().contiguous(), "Q": Q.float().contiguous(), "qhat": to_table(qh, C, wide), "tie_kind": tie_kind}


def make_dsims(profile, sims, seed):
    rows, C = sims.shape
    g = _gen(seed, rows, C, 17)
    n = torch.randn(rows, C, generator=g)
    if profile == "aligned":
        return (torch.randn(rows, 1, generator=g) * sims.float().cpu() + 1e-3 * n).float()
    return n.float()


def poison_rows(t, pad, kind, like=None):
    """t with `pad` more rows: NaN, or finite values built to hurt: 1e30 with alternating sign (an f32 sum of their squares overflows, a product
    with anything of size 1 swamps every valid term); bf16 / integer tensors take their largest finite / in-range value."""
    if kind == "nan" and t.dtype.is_floating_point:
        return padded(t, pad, float("nan"))
    out = padded(t, pad, 0)
    if t.dtype == torch.uint8:
        out[t.shape[0]:] = 2
    else:
        v = torch.full(out[t.shape[0]:].shape, 1e30, dtype=torch.float32)
        v.view(-1)[1::2] = -1e30
        out[t.shape[0]:] = v.to(t.dtype)
    return out


def make_box_inputs(profile, rows, D, seed, P=None):
    """Box-head inputs on the CPU: h / h1 / u1 (float32 holding bf16 values), w2 [4, D], b2 [4], box_bias [P, 4], dboxes [rows, 4], sig [rows, 4] (the
    f32 nearest sigmoid of the profile's pre-activations: what the backward is given), x [rows, 4] the pre-activations the forward reaches."""
    g = _gen(seed, rows, D)
    P = rows if P is None else P
    u1 = bf16_round(2.0 * torch.randn(rows, D, generator=g))
    h1 = bf16_round(torch.nn.functional.gelu(u1))
    w2 = 0.1 * torch.randn(4, D, generator=g)
    b2 = torch.randn(4, generator=g)
    dboxes = torch.randn(rows, 4, generator=g)
    v = h1.double() @ w2.double().t()
    if profile == "randn":
        bb = 0.5 * torch.randn(P, 4, generator=g)
    elif profile == "saturated":
        assert P == rows, "the saturated profile sets one box bias per row"
        sign = torch.where(torch.rand(rows, 4, generator=g) < 0.5, -1.0, 1.0)
        target = sign * (8.0 + 32.0 * torch.rand(rows, 4, generator=g))
        target[4::5] = -(90.0 + 10.0 * torch.rand(target[4::5].shape, generator=g))
        bb = (target.double() - v - b2.double()).float()
        dboxes[:, 2] = dboxes[:, 0] * (1.0 + 1e-6 * torch.randn(rows, generator=g))
        dboxes[:, 3] = dboxes[:, 1] * (1.0 + 1e-6 * torch.randn(rows, generator=g))
    else:
        raise ValueError(profile)
    x = v + b2.double() + bb.double()[torch.arange(rows) % P]
    sig = torch.sigmoid(x).float()
    sig = torch.where(sig < TINY, torch.zeros_like(sig), sig)          # 1 / (1 + inf) = 0: what the forward stores once expf has overflowed
    return {"h1": h1, "u1": u1, "w2": w2.float(), "b2": b2.float(), "box_bias": bb.float().contiguous(), "dboxes": dboxes.float(), "x": x,
            "sig": sig, "P": P}


def box_old(D):
    return {"dW2": torch.linspace(-0.5, 0.75, 4 * D).view(4, D).clone(), "db2": torch.tensor([1.0, -0.25, 0.5, 2.0]), "colsum": torch.full((D,), 2.0)}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
E6 = torch.tensor(1e-6, dtype=torch.float32)


def _lane_strided_sum(v):
    """sum over the last axis as qhat_kernel forms it: lane l adds k = l, l + 64, ... in order, then the six butterfly levels."""
    R_, Dt = v.shape
    buf = torch.zeros(R_, cdiv(Dt, 64) * 64, dtype=torch.float32)
    buf[:, :Dt] = v
    s = torch.zeros(R_, 64, dtype=torch.float32)
    for i in range(buf.shape[1] // 64):
        s = s + buf[:, 64 * i:64 * i + 64]
    return _wave_sum(s, [0])[:, :1]


def emulate_qhat(Q, C=None, wide=False, hooks=()):
    """qhat_kernel / qhat_wide_kernel -> (table [32 (nblk), Dt], qnorm [3C]).  hook "eps_inside": Q / (n + 1e-6)."""
    Q = Q.float()
    n = torch.sqrt(_lane_strided_sum(Q * Q))
    qh = Q / (n + E6) if "eps_inside" in hooks else Q / n + E6
    C = Q.shape[0] // 3 if C is None else C
    return (to_table(qh, C, wide) if Q.shape[0] == 3 * C else torch.cat([qh, torch.zeros(32 - Q.shape[0], Q.shape[1])])), n[:, 0]


def emulate_sims(e, qhat, C, wide=False, pad=3, hooks=(), sentinel=7.0):
    """class_sims_kernel (per query block: class_sims_wide_kernel) -> sims, argmax, inv [rows + pad, .] buffers that start at `sentinel`.
    hooks: "drop_half", "masked_live", "clamp_store", "ge_max", "col_off", "inv_neighbor", "wide_pad_class"."""
    e, qhat = e.float(), qhat.float()
    R_, Dt = e.shape
    live = Dt - 64 if "drop_half" in hooks else Dt
    nb = wide_blocks(C) if wide else 1
    ss = [torch.zeros(R_), torch.zeros(R_)]
    acc = torch.zeros(R_, 32 * nb)
    for c0 in range(0, Dt, 128):
        for hi in (0, 1):
            k0 = c0 + 64 * hi
            if k0 >= live:
                if "masked_live" in hooks and k0 >= Dt:
                    k0 = 0                                   # the address the masked lanes read (kbase returns 0): taken as live
                else:
                    continue
            blk = e[:, k0:k0 + 64]
            for q4 in range(16):
                a = blk[:, 4 * q4:4 * q4 + 4]
                sq = a * a
                ss[hi] = ss[hi] + (((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3])
            acc = acc + blk @ qhat[:, k0:k0 + 64].t()
    inv = 1.0 / (torch.sqrt(ss[0] + ss[1]) + E6)
    used = torch.roll(inv, -1) if "inv_neighbor" in hooks else inv
    v = acc * used[:, None]
    cols = prompt_cols(C, wide) + (1 if "col_off" in hooks else 0)
    v0, v1, v2 = v[:, cols], v[:, cols + 1], v[:, cols + 2]
    best, arg = v0, torch.zeros(R_, C, dtype=torch.uint8)
    for p, vp in ((1, v1), (2, v2)):
        better = (vp >= best) if "ge_max" in hooks else (vp > best)
        best, arg = torch.where(better, vp, best), torch.where(better, torch.full_like(arg, p), arg)
    out = {"sims": torch.full((R_ + pad, C), sentinel), "argmax": torch.full((R_ + pad, C), 7, dtype=torch.uint8), "inv": torch.full((R_ + pad,), sentinel)}
    out["sims"][:R_], out["argmax"][:R_], out["inv"][:R_] = best, arg, inv
    if "clamp_store" in hooks:
        out["sims"][R_], out["argmax"][R_], out["inv"][R_] = best[-1], arg[-1], inv[-1]
    if "wide_pad_class" in hooks:                            # class C of the last block written at its real address orow * C + C (= [orow + 1, 0]) with what
        idx = (torch.arange(R_) + 1) * C                     # the zero prompt rows give (0, prompt 0), landing after the owner's store
        out["sims"].view(-1)[idx] = 0.0
        out["argmax"].view(-1)[idx] = 0
    return out


def _gs(ds, sm):
    """wave_sum over the classes, lane c (+ 64 i) holding class c."""
    R_, C = ds.shape
    p = ds * sm
    s = torch.zeros(R_, 64)
    for i in range(cdiv(C, 64)):
        blk = p[:, 64 * i:64 * i + 64]
        s[:, :blk.shape[1]] = s[:, :blk.shape[1]] + blk
    return _wave_sum(s, [0])[:, 0]


def emulate_sims_bwd(dsims, sims, am, inv, e, qhat, wide=False, pad=3, hooks=None, fixed=True, sentinel=7.0):
    """class_sims_bwd_kernel / _pf_kernel (one arithmetic) or class_sims_wide_bwd_kernel -> de, G, e_bf16 (float32 holding bf16 values) in buffers of
    rows + pad rows that start at `sentinel`.  fixed=False: coef_e without the select (the defect).  hooks (dict): "coef_sign", "stale_last": True
    (the last row reads row r - 4's e), "G_second": [rows, C] prompt to route to, "skip_chunk2" (wide)."""
    hooks = hooks or {}
    ds, sm, inv, e, qhat = dsims.float(), sims.float(), inv.float(), e.float(), qhat.float()
    R_, C = ds.shape
    Dt = e.shape[1]
    j = prompt_cols(C, wide)[None] + am.long()
    nrm = 1.0 / inv - E6
    coef = _gs(ds, sm) * inv / nrm
    if fixed:
        coef = torch.where(nrm > 0, coef, torch.zeros_like(coef))
    if "coef_sign" in hooks:
        coef = -coef
    eu = e.clone()
    if hooks.get("stale_last"):
        eu[R_ - 1] = e[R_ - 5]
    W = wide_qp(C) if wide else 32
    if wide:
        A = torch.zeros(R_, W)
        A.scatter_(1, j, ds)
        acc = torch.zeros(R_, Dt)
        for q0 in range(0, 32 * wide_blocks(C), 256):
            if "skip_chunk2" in hooks and q0 == 256:
                continue
            q1 = min(q0 + 256, 32 * wide_blocks(C))
            acc = acc + A[:, q0:q1] @ qhat[q0:q1]
        d = inv[:, None] * acc - coef[:, None] * eu
    else:
        d = -coef[:, None] * eu
        for c in range(C):
            d = d + (ds[:, c] * inv)[:, None] * qhat[j[:, c]]
    jg = prompt_cols(C, wide)[None] + hooks["G_second"].long() if "G_second" in hooks else j
    G = torch.zeros(R_, W)
    G.scatter_(1, jg, bf16_round(ds * inv[:, None]))
    out = {"de": torch.full((R_ + pad, Dt), sentinel), "G": torch.full((R_ + pad, W), sentinel), "e_bf16": torch.full((R_ + pad, Dt), sentinel)}
    out["de"][:R_], out["G"][:R_], out["e_bf16"][:R_] = bf16_round(d), G, bf16_round(e)
    out["de_f32"] = d
    if "skip_chunk2" in hooks:
        out["G"][:R_, 256:512] = sentinel
    return out


def emulate_qhat_bwd(dqhat, Q, old, hooks=()):
    """qhat_bwd_kernel.  hook "no_projection": dQ = dqhat / n."""
    q, dh = Q.float(), dqhat.float()
    ss, dt = _lane_strided_sum(q * q), _lane_strided_sum(q * dh)
    n = torch.sqrt(ss)
    qn = q / n
    t = dh if "no_projection" in hooks else dh - (dt / n) * qn
    return old.float() + t / n


def emulate_box_final(h, w2, b2, box_bias, P, hooks=()):
    """box_final_rows_kernel -> sig, boxes.  hook "no_box_bias"."""
    h, w2 = h.float(), w2.float()
    R_, D = h.shape
    NC = 1 if D <= 512 else 2
    buf_h, buf_w = torch.zeros(R_, 512 * NC), torch.zeros(4, 512 * NC)
    buf_h[:, :D], buf_w[:, :D] = h, w2
    hh, ww = buf_h.view(R_, NC, 64, 8), buf_w.view(4, NC, 64, 8)
    a = torch.zeros(R_, 4, 64)
    for c in range(NC):
        for k in range(8):
            a = _fma32(hh[:, None, c, :, k], ww[None, :, c, :, k], a)
    v = torch.stack([_wave_sum(a[:, o], [0])[:, 0] for o in range(4)], -1)
    bb = box_bias.float()[torch.arange(R_) % P]
    x = v + b2.float() if "no_box_bias" in hooks else (v + b2.float()) + bb
    s = 1.0 / (1.0 + torch.exp(-x))
    half = torch.tensor(0.5)
    return {"sig": s, "boxes": torch.stack([s[:, 0] - half * s[:, 2], s[:, 1] - half * s[:, 3], s[:, 0] + half * s[:, 2], s[:, 1] + half * s[:, 3]], -1)}


def _slab_reduce(part, old):
    """owl_slab_reduce_impl with accumulate on part [nblk, n]."""
    nblk = part.shape[0]
    if nblk >= 128:
        a = torch.zeros(8, part.shape[1])
        for g in range(8):
            for s in range(g, nblk, 8):
                a[g] = a[g] + part[s]
        r = old.float().clone()
        for g in range(8):
            r = r + a[g]
        return r
    r = old.float().clone()
    for s in range(nblk):
        r = r + part[s]
    return r


def emulate_box_final_bwd(dboxes, sig, h1, u1, w2, old, hooks=None):
    """box_final_bwd_kernel + the slab reduces -> du1 (bf16 values), dW2, db2, colsum.  hooks (dict): "dW2_drop_last_row": block, "db2_drop_wave": block (rpb <= 64: wave 0 holds every row of a block, so its loss is the block's db2),
    "no_dgelu_group": thread t (columns 4 t .. 4 t + 3), "sig_from": tensor used in place of sig."""
    hooks = hooks or {}
    g, s, h, u, w = dboxes.float(), (hooks["sig_from"] if "sig_from" in hooks else sig).float(), h1.float(), u1.float(), w2.float()
    R_, D = h.shape
    half = torch.tensor(0.5)
    dl = torch.stack([g[:, 0] + g[:, 2], g[:, 1] + g[:, 3], half * (g[:, 2] - g[:, 0]), half * (g[:, 3] - g[:, 1])], -1)
    dp = dl * s * (1.0 - s)
    dh1 = ((dp[:, 0:1] * w[0:1] + dp[:, 1:2] * w[1:2]) + dp[:, 2:3] * w[2:3]) + dp[:, 3:4] * w[3:4]
    dg = dgelu_erf_f32(u)
    if "no_dgelu_group" in hooks:
        t = hooks["no_dgelu_group"]
        dg[:, 4 * t:4 * t + 4] = 1.0
    o = dh1 * dg
    rpb, nblk = box_bwd_rpb(R_), box_bwd_blocks(R_)

    def blocks(t):
        buf = torch.zeros(nblk * rpb, t.shape[1])
        buf[:R_] = t
        return buf.view(nblk, rpb, -1)

    tw = blocks((dp[:, :, None] * h[:, None, :]).reshape(R_, 4 * D)).clone()
    if "dW2_drop_last_row" in hooks:
        b = hooks["dW2_drop_last_row"]
        tw[b, min(rpb, R_ - b * rpb) - 1] = 0.0
    to, tb = blocks(o), blocks(dp)
    pw, po = torch.zeros(nblk, 4 * D), torch.zeros(nblk, D)
    for i in range(rpb):
        pw, po = pw + tw[:, i], po + to[:, i]
    lanes = torch.zeros(nblk, 4, 64)
    lanes[:, :, :rpb] = tb.transpose(1, 2)
    pb = torch.stack([_wave_sum(lanes[:, k], [0])[:, 0] for k in range(4)], -1)     # wave 0; waves 1-3 hold no rows (rpb <= 64): + 0 three times
    if "db2_drop_wave" in hooks:
        pb[hooks["db2_drop_wave"]] = 0.0
    return {"du1": bf16_round(o), "dW2": _slab_reduce(pw, old["dW2"].reshape(-1)).view(4, D), "db2": _slab_reduce(pb, old["db2"]),
            "colsum": _slab_reduce(po, old["colsum"])}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case sets of the GPU test (smallest shapes per launcher form; the CPU test checks that they reach every form)
# ---------------------------------------------------------------------------------------------------------------------------------------------
SIMS_FWD_ROWS = (1, 31, 33, 127, 300)
SIMS_FWD_DT = (64, 192, 512, 768)
SIMS_FWD_TALL = (32801, 64)        # the smallest row count with nw = 5 whose last workgroup holds fewer than 5 waves of rows: 1026 = 205 * 5 + 1 waves
# (rows, Dt): rpw 2 with an odd tail (break1 / the generic odd-row tail), rpw 2, 3 (break3), 4 (cond), 5 (break1), 18 (break2) + ragged last waves
SIMS_BWD = ((1, 64), (33, 192), (300, 64), (33, 512), (300, 768), (8193, 64), (8193, 512), (8194, 768), (12289, 512), (16385, 512),
            (69633, 512), (69633, 64))
WIDE_ROWS = (1, 33, 300)
WIDE_DT = (512, 768)
WIDE_NT_DT = (96, 128, 256, 512, 768, 1024)
QHAT_NQ = (3, 30, 32)
BOX_BWD = ((1, 8), (7, 128), (9, 516), (2304, 768), (9, 1024), (4097, 128), (32257, 8), (300, 516), (300, 1024))
BOX_FWD = tuple((rows, D) for rows in (1, 4097) for D in (512, 520, 768))


def sims_fwd_cases():
    """(rows, Dt, C, profile): every row count and width on randn; every profile and narrow class count at 33 and 300 rows."""
    out = [(rows, Dt, 10, "randn") for rows in SIMS_FWD_ROWS for Dt in SIMS_FWD_DT]
    out += [(rows, Dt, C, p) for rows, Dt in ((33, 192), (300, 512)) for C in NARROW_C for p in PROFILES if (rows, Dt, C, p) not in out]
    out.append(SIMS_FWD_TALL + (3, "trained"))
    return out


def sims_bwd_cases():
    out = []
    for i, (rows, Dt) in enumerate(SIMS_BWD):
        if rows > 1000:
            out.append((rows, Dt, 3, ("trained", "tiny", "aligned")[i % 3]))
        else:
            out += [(rows, Dt, NARROW_C[(i + k) % 3], p) for k, p in enumerate(PROFILES)]
    return out


def wide_cases():
    out = [(rows, Dt, C, PROFILES[(i + k + n) % 5]) for i, rows in enumerate(WIDE_ROWS) for k, Dt in enumerate(WIDE_DT) for n, C in enumerate(WIDE_C)]
    out += [(33, Dt, 11, "tiny" if Dt % 64 == 0 else "aligned") for Dt in WIDE_NT_DT]
    out += [(300, 512, 81, p) for p in PROFILES if (300, 512, 81, p) not in out]
    return out
