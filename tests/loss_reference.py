"""Float64 references, derived error bounds and input builders for the criterion of csrc/loss.hip: match_cost_kernel, hungarian_kernel, spread_kernel,
class_loss_kernel, box_loss_kernel, loss_reduce_kernel and loss_bwd_kernel.  Checker side, CPU only: nothing here imports the package.

References (float64, on the kernel's exact f32 inputs), one per stage; each takes the DISCRETE decisions (assignment, post-spreading labels) as inputs
----------
`cost_stage(sims, boxes, labels, tgt)`          cost[p, j] = |box_p - tgt_j|_1 - softmax(sims_p)[label_j] - GIoU(box_p, tgt_j)  (ref src/matcher.py:107-130).
`class_stage(sims, tc, bg, scales)`             loss_ce / loss_bg of one image and d(loss of the row's kind) / d sims  (ref src/losses.py:16-40).
`box_stage(boxes, tgt, pred_idx, tgt_idx)`      loss_bbox / loss_giou of one image and their gradients wrt the predicted boxes  (ref src/losses.py:42-69).
`mean_stage(per_image)`                         the batch mean of the four per-image terms.
`combine_stage(g, tc, bg, dsims, dl1, dgiou, B)`   d_sims = g[kind(row)] dsims / B,  d_boxes = (g[2] dl1 + g[3] dgiou) / B.
`criterion(...)`                                the five chained: what PushPullLoss returns and leaves in .grad, with the bounds carried through.
The VALUES are the oracle's own functions (oracle/owl_oracle.py: generalized_box_iou, softmax / cdist, and class_loss with a dtype-generic one-hot:
`class_loss_any_dtype`) run in double under torch autograd.
They carry torch's conventions, which the kernel restates by hand: the 0.5 / 0.5 split of a max / min tie, pass-through of clamp(min=0) at exactly 0,
sign(0) = 0, logs clamped at -100, the BCE-backward clamp at 1e-12.

Bounds (elementwise, derived, no fitted constant)
------
Every stage is ALSO written out once more as the kernel's own operation sequence over `EV` pairs (value, error): float64 values, and a first-order
bound on what a correct f32 evaluation of that sequence may differ from them:
    z = fl(x op y):   e_z = |dz/dx| e_x + |dz/dy| e_y + f |z| + d          f = 2^-24 (gemm_reference.F), d = 2^-149 (one subnormal step)
with the partial derivatives at the float64 values, so the cancellation in 1 - exp(-l) at small l (e_om ~ 4 f against om ~ l) and the division by
(1 - a) a near |s| = 1 widen the bound where they should and nowhere else.  Multiplications by 0, +-1, 0.5 and selections are exact and add nothing.
 ASSUMPTION L1: expf, logf, log1pf are within 2 ulp (`LIBM` = 4 f relative), the budget heads_reference.py (H1) uses for the device libm.
 ASSUMPTION L2: the f32 division is correctly rounded (hipcc's default; tests/test_loss_gpu.py::test_box_ops_free_functions pins IoU bit for bit on it).
 loss.hip is compiled with -ffp-contract=off (csrc/build.sh), so one rounding per written operation is exact, not a guess.
 The tolerance of an element is  e + |v - ref|:  the EV error plus the distance of the EV value to the autograd value.  The second term is the f32
   constant 1e-12f against torch's double 1e-12 in the BCE-backward clamp (4e-9 relative, where the clamp acts) and float64 noise elsewhere;
   tests/test_loss_reference.py holds it below 1e-8 relative, so a kernel formula that is not the autograd's cannot hide in it.
 Sums (`_sum`): |err| <= gamma(depth) sum (|t| + e_t) + sum e_t -- u times the sum of magnitudes times the depth of the reduction:
   class loss   C adds in a row, ceil(P / 1024) rows per thread, 6 butterfly levels, 16 wave partials, the division:   C + ceil(P / 1024) + 23
   box losses   4 (L1) or 1 (GIoU) adds per pair, ceil(n / 256) pairs per thread, 6 levels, 4 partials, times fl(1 / n):  ceil(n / 256) + 16
   batch mean   B adds and the division:  B + 1
   softmax denominator of the matching cost:  C adds.

Builders -- tests/test_loss_reference.py asserts that each does what it claims
--------
`contention_cost(n, P, seed)`    -(i + 1)(j + 1) / (n P) + 1e-3 noise (+ 1.0 on columns >= 120 when P > 120): every target wants the same predictions,
    in the same order; augmentations scan >= n / 2 rows and re-route chains >= n / 4 long (`sap_trace` measures it).
`spread_case(P, pattern)`        disjoint lattice filler boxes and chains of near-duplicates (neighbours IoU 0.887, second neighbours 0.786):
    "forward"   one chain over `edge_rows(P)` (rows 0, P - 1, both sides of every 32-row, 2048-row and 4096-row edge in reach, 2111 / 2112), seed at row 0:
                every chain row ends with the seed's label;
    "overwrite" the same chain, seeds A (label 1) at its first row, B (label 2) at its second, and a third (label 3) at row P - 1: B takes A's label and
                spreads it on; every chain row ends 1;
    "mixed"     a backward chain P - 1 -> b1 -> b2 (b1 relabelled, b2 stays background: rows behind the cursor are not revisited); at large P also
                2300 -> 2200 -> 2100; zero-area boxes (one of them a seed: IoU NaN or 0, nothing spreads); a pair whose f32 IoU is exactly float32(0.85)
                (stays background) and its one-ulp-above twin (relabelled);
    "background" no positive at all: nothing changes.
`make_sims(profile, ...)`        uniform | trained_like (one column per row within 4 ulp of +-1, the rest 1e-4 .. 1e-2) | tiny (1e-20 and subnormals) |
                                 exact (0, +-1, +-0.5, +-0.25).
`make_case(profile, B, P, C, seed, counts, spread)`   sims of the profile, random boxes, targets = jittered copies of chosen predictions (some sharing a
    coordinate exactly: max / min ties); with `spread`, two near-duplicates per target among the first k, so positives outnumber matches.
`sap_trace(cost)`   the shortest-augmenting-path loop of oracle/lsap.c restated, reporting rows scanned and chain length per augmentation.  It exists
    ONLY to prove what the cost builders claim; the assignment oracle stays oracle/lsap.c.
"""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import owl_oracle as O
from tests.gemm_reference import F, check, gamma, ratios  # noqa: F401

F64 = torch.float64
LIBM = 4.0 * F                 # ASSUMPTION L1
DEN = 2.0 ** -149
EPS32 = float(np.float32(1e-12))
THR32 = float(np.float32(0.85))
PROFILES = ("uniform", "trained_like", "tiny", "exact")


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (value, error) arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------------
class EV:
    """float64 value v and a bound e on |f32 evaluation - v|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=F64)

    def __getitem__(self, i):
        return EV(self.v[i], self.e[i])


def _ev(x):
    return x if isinstance(x, EV) else EV(x)


def _rnd(v, e):
    return EV(v, e + F * v.abs() + DEN)


def add(a, b):
    a, b = _ev(a), _ev(b)
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    a, b = _ev(a), _ev(b)
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b):
    a, b = _ev(a), _ev(b)
    return _rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e)


def div(a, b):
    a, b = _ev(a), _ev(b)
    v = a.v / b.v
    return _rnd(v, (a.e + v.abs() * b.e) / b.v.abs())


def scaled(a, k):
    """a * k for k in {0, +-1, +-0.5} (tensor or number): exact."""
    k = torch.as_tensor(k, dtype=F64)
    return EV(a.v * k, a.e * k.abs())


def pick(mask, a, b):
    a, b = _ev(a), _ev(b)
    return EV(torch.where(mask, a.v, b.v), torch.where(mask, a.e, b.e))


def vmax(a, b):
    a, b = _ev(a), _ev(b)
    return EV(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e))


def vmin(a, b):
    a, b = _ev(a), _ev(b)
    return EV(torch.minimum(a.v, b.v), torch.maximum(a.e, b.e))


def vabs(a):
    return EV(a.v.abs(), a.e)


def vexp(a):
    v = torch.exp(a.v)
    return EV(v, v * a.e + LIBM * v + DEN)


def log_clamped(a, log1p_of_minus=False):
    """max(logf(a), -100) or max(log1pf(-a), -100) of an EXACT input a >= 0."""
    v = (torch.log1p(-a) if log1p_of_minus else torch.log(a)).clamp(min=-100.0)
    return EV(v, torch.where(v > -100.0, LIBM * v.abs() + DEN, torch.zeros_like(v)))


def _sum(t, depth, dim=None):
    """A sum of EV terms whose longest chain of f32 adds is `depth`."""
    mag = t.v.abs() + t.e
    if dim is None:
        return EV(t.v.sum(), gamma(depth) * mag.sum() + t.e.sum())
    return EV(t.v.sum(dim), gamma(depth) * mag.sum(dim) + t.e.sum(dim))


def tol_of(ev, ref):
    return ev.e + (ev.v - ref).abs()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stage 1: matching cost
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _giou_ev(a, t):
    """giou_pair of loss.hip on EV-able coordinate tuples (x0, y0, x1, y1); returns (giou, parts)."""
    ax, ay, az, aw = a
    tx, ty, tz, tw = t
    area_a = mul(sub(az, ax), sub(aw, ay))
    area_b = mul(sub(tz, tx), sub(tw, ty))
    ltx, lty, rbx, rby = vmax(ax, tx), vmax(ay, ty), vmin(az, tz), vmin(aw, tw)
    dw, dh = sub(rbx, ltx), sub(rby, lty)
    w, h = vmax(dw, 0.0), vmax(dh, 0.0)
    inter = mul(w, h)
    uni = sub(add(area_a, area_b), inter)
    iou = div(inter, uni)
    cx0, cy0, cx1, cy1 = vmin(ax, tx), vmin(ay, ty), vmax(az, tz), vmax(aw, tw)
    dcw, dch = sub(cx1, cx0), sub(cy1, cy0)
    cw, ch = vmax(dcw, 0.0), vmax(dch, 0.0)
    area_c = mul(cw, ch)
    giou = sub(iou, div(sub(area_c, uni), area_c))
    return giou, dict(w=w, h=h, inter=inter, uni=uni, cw=cw, ch=ch, area_c=area_c, dw=dw, dh=dh, dcw=dcw, dch=dch)


def cost_stage(sims, boxes, labels, tgt):
    """sims [P, C], boxes [P, 4], labels [n] i64, tgt [n, 4] (f32 tensors) -> dict(ref [P, n] f64, tol)."""
    sd, bd, td = sims.double(), boxes.double(), tgt.double()
    ref = torch.cdist(bd, td, p=1) - sd.softmax(-1)[:, labels] - O.generalized_box_iou(bd, td)
    C = sd.shape[1]
    mx = sd.max(-1, keepdim=True).values
    e = vexp(sub(EV(sd), EV(mx)))
    den = _sum(e, C, dim=1)
    prob = div(e[:, labels], EV(den.v[:, None], den.e[:, None]))
    a = tuple(EV(bd[:, None, k]) for k in range(4))
    t = tuple(EV(td[None, :, k]) for k in range(4))
    l1 = None
    for k in range(4):
        d = vabs(sub(a[k], t[k]))
        l1 = d if l1 is None else add(l1, d)
    g, _ = _giou_ev(a, t)
    ev = add(add(mul(1.0, l1), mul(1.0, scaled(prob, -1.0))), mul(1.0, scaled(g, -1.0)))
    return dict(ref=ref, ev=ev, tol=tol_of(ev, ref))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stage 2: class loss and its gradient (one image)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def class_loss_any_dtype(sims, tc, bg, scales):
    """oracle.class_loss (ref src/losses.py:16-40) with the one-hot target in the dtype of `sims` instead of .float(), which binary_cross_entropy
    refuses against double inputs.  tests/test_loss_reference.py holds it to the oracle's bits in f32."""
    a = torch.abs(sims)
    pos = tc != bg
    pos_t = Fn.one_hot(tc[pos], bg).to(sims.dtype)
    pos_l = Fn.binary_cross_entropy(a[pos], pos_t, weight=scales, reduction="none")
    neg_l = Fn.binary_cross_entropy(a[~pos], torch.zeros_like(a[~pos]), weight=scales, reduction="none")
    pos_l = (torch.pow(1 - torch.exp(-pos_l), 2) * pos_l).sum(dim=1).mean()
    neg_l = (torch.pow(1 - torch.exp(-neg_l), 2) * neg_l).sum(dim=1).mean()
    return pos_l, neg_l


def class_stage(sims, tc, bg, scales=None):
    """sims [P, C] f32, tc [P] i64 (post-spreading), scales [C] f32 or None ->
    dict(loss = (ref [2], tol [2]) for (loss_ce, loss_bg), dsims = (ref [P, C], tol), ev_loss, ev_dsims)."""
    P, C = sims.shape
    sd = sims.double().requires_grad_(True)
    wd = None if scales is None else scales.double()
    pos_l, neg_l = class_loss_any_dtype(sd, tc, bg, wd)
    ref_d, = torch.autograd.grad(pos_l + neg_l, sd)
    ref_l = torch.stack([pos_l.detach(), neg_l.detach()])

    s = sims.double()
    a = s.abs()
    pos = tc != bg
    y = torch.zeros(P, C, dtype=torch.bool)
    y[pos, tc[pos]] = True
    w = torch.ones(C, dtype=F64) if wd is None else wd
    npos = float(pos.sum())
    nbg = float(P) - npos
    inner = pick(y, log_clamped(a), log_clamped(a, True))          # y la + (1 - y) l1a: a selection
    l = mul(EV(-w), inner)
    em = vexp(scaled(l, -1.0))
    om = sub(1.0, em)
    om2 = mul(om, om)
    t = mul(om2, l)
    depth = C + cdiv(P, 1024) + 23
    posf = pos[:, None].expand(P, C)
    zero = EV(torch.zeros(P, C, dtype=F64))
    lp = div(_sum(pick(posf, t, zero), depth), npos)
    lb = div(_sum(pick(~posf, t, zero), depth), nbg)
    ev_l = EV(torch.stack([lp.v, lb.v]), torch.stack([lp.e, lb.e]))
    dF = add(mul(mul(scaled(om, 2.0), em), l), om2)
    yv = y.double()
    dl = div(mul(EV(w), sub(EV(a), EV(yv))), vmax(mul(sub(1.0, EV(a)), EV(a)), EPS32))
    inv_rows = div(1.0, torch.where(pos, torch.tensor(npos, dtype=F64), torch.tensor(nbg, dtype=F64))[:, None])
    ev_d = mul(scaled(mul(dF, dl), torch.sign(s)), inv_rows)
    return dict(loss=(ref_l, tol_of(ev_l, ref_l)), dsims=(ref_d, tol_of(ev_d, ref_d)), ev_loss=ev_l, ev_dsims=ev_d)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stage 3: box losses on the matched pairs and their gradients (one image)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _w_gt(a, b):
    """d max(a, b) / da of torch: 1, 0.5 at a tie, 0."""
    return torch.where(a > b, 1.0, torch.where(a == b, 0.5, 0.0)).double()


def box_stage(boxes, tgt, pred_idx, tgt_idx):
    """boxes [P, 4], tgt [n, 4] f32; pred_idx, tgt_idx [n] i64 ->
    dict(loss = (ref [2], tol) for (loss_bbox, loss_giou), dl1 / dgiou = (ref [P, 4], tol), ev_*).  Rows no pair names hold exact zeros, tol 0."""
    P, n = boxes.shape[0], pred_idx.shape[0]
    bd = boxes.double().requires_grad_(True)
    src, tg = bd[pred_idx], tgt.double()[tgt_idx]
    l1_ref = Fn.l1_loss(src, tg, reduction="none").sum() / n
    g_ref = (1 - torch.diag(O.generalized_box_iou(src, tg))).sum() / n
    dl1_ref, = torch.autograd.grad(l1_ref, bd, retain_graph=True)
    dg_ref, = torch.autograd.grad(g_ref, bd)
    ref_l = torch.stack([l1_ref.detach(), g_ref.detach()])

    A, T = boxes.double()[pred_idx], tgt.double()[tgt_idx]
    a = tuple(EV(A[:, k]) for k in range(4))
    t = tuple(EV(T[:, k]) for k in range(4))
    invn = div(1.0, float(n))
    depth = cdiv(n, 256) + 16
    l1 = None
    for k in range(4):
        d = vabs(sub(a[k], t[k]))
        l1 = d if l1 is None else add(l1, d)
    giou, q = _giou_ev(a, t)
    ev_l1 = mul(_sum(l1, depth), invn)
    ev_g = mul(_sum(sub(1.0, giou), depth), invn)
    ev_l = EV(torch.stack([ev_l1.v, ev_g.v]), torch.stack([ev_l1.e, ev_g.e]))
    # gradients, as box_loss_kernel writes them
    d1 = [scaled(invn, torch.sign(A[:, k] - T[:, k])) for k in range(4)]
    on = lambda x: (x.v >= 0).double()                                  # noqa: E731  (the sign of an f32 difference is the exact one)
    dw_on, dh_on, dcw_on, dch_on = on(q["dw"]), on(q["dh"]), on(q["dcw"]), on(q["dch"])
    gt, lt = _w_gt, lambda x, y: _w_gt(y, x)                            # noqa: E731
    d_inter = [scaled(q["h"], -dw_on * gt(A[:, 0], T[:, 0])), scaled(q["w"], -dh_on * gt(A[:, 1], T[:, 1])),
               scaled(q["h"], dw_on * lt(A[:, 2], T[:, 2])), scaled(q["w"], dh_on * lt(A[:, 3], T[:, 3]))]
    hh, ww = sub(a[3], a[1]), sub(a[2], a[0])
    d_area_a = [scaled(hh, -1.0), scaled(ww, -1.0), hh, ww]
    d_area_c = [scaled(q["ch"], -dcw_on * lt(A[:, 0], T[:, 0])), scaled(q["cw"], -dch_on * lt(A[:, 1], T[:, 1])),
                scaled(q["ch"], dcw_on * gt(A[:, 2], T[:, 2])), scaled(q["cw"], dch_on * gt(A[:, 3], T[:, 3]))]
    uni, inter, area_c = q["uni"], q["inter"], q["area_c"]
    d2 = []
    for k in range(4):
        d_uni = sub(d_area_a[k], d_inter[k])
        d_iou = div(sub(mul(d_inter[k], uni), mul(inter, d_uni)), mul(uni, uni))
        d_ratio = div(sub(mul(d_uni, area_c), mul(uni, d_area_c[k])), mul(area_c, area_c))
        d2.append(mul(scaled(add(d_iou, d_ratio), -1.0), invn))

    def scatter(cols):
        v = torch.zeros(P, 4, dtype=F64); e = torch.zeros(P, 4, dtype=F64)
        v[pred_idx] = torch.stack([c.v.expand(n) for c in cols], 1)
        e[pred_idx] = torch.stack([c.e.expand(n) for c in cols], 1)
        return EV(v, e)

    ev_d1, ev_d2 = scatter(d1), scatter(d2)
    return dict(loss=(ref_l, tol_of(ev_l, ref_l)), dl1=(dl1_ref, tol_of(ev_d1, dl1_ref)), dgiou=(dg_ref, tol_of(ev_d2, dg_ref)),
                ev_loss=ev_l, ev_dl1=ev_d1, ev_dgiou=ev_d2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stages 4 and 5: batch mean, backward combine
# ---------------------------------------------------------------------------------------------------------------------------------------------
def mean_stage(per_image):
    """per_image: EV [B, 4] (or an exact tensor) -> EV [4]."""
    per_image = _ev(per_image)
    B = per_image.v.shape[0]
    return div(_sum(per_image, B, dim=0), float(B))


def combine_stage(g, tc, bg, dsims, dl1, dgiou, B):
    """g [4] f32 upstream gradients; tc [R] labels; dsims EV [R, C]; dl1, dgiou EV [R, 4] -> (EV d_sims [R, C], EV d_boxes [R, 4])."""
    g = g.double()
    invB = div(1.0, float(B))
    gk = mul(EV(torch.where(tc != bg, g[0], g[1])[:, None]), invB)
    d_sims = mul(gk, _ev(dsims))
    g2, g3 = mul(EV(g[2]), invB), mul(EV(g[3]), invB)
    d_boxes = add(mul(g2, _ev(dl1)), mul(g3, _ev(dgiou)))
    return d_sims, d_boxes


def criterion(sims, boxes, tcs, pred_idx, tgt_idx, tgt_boxes, bg, scales, g):
    """The whole criterion at given decisions.  sims [B, P, C], boxes [B, P, 4] f32; tcs [B, P]; pred_idx / tgt_idx / tgt_boxes: per-image lists;
    g [4] f32.  Returns name -> (ref, tol) for per_image [B, 4], losses [4], grad_sims [B, P, C], grad_boxes [B, P, 4].  The values of the two
    gradients are float64 autograd of sum_k g_k loss_k through the oracle's functions."""
    B, P, C = sims.shape
    sd = sims.double().requires_grad_(True)
    bd = boxes.double().requires_grad_(True)
    wd = None if scales is None else scales.double()
    rows = []
    for b in range(B):
        src, tg = bd[b][pred_idx[b]], tgt_boxes[b].double()[tgt_idx[b]]
        n = pred_idx[b].shape[0]
        ce, bgl = class_loss_any_dtype(sd[b], tcs[b], bg, wd)
        rows.append(torch.stack([ce, bgl, Fn.l1_loss(src, tg, reduction="none").sum() / n,
                                 (1 - torch.diag(O.generalized_box_iou(src, tg))).sum() / n]))
    per_ref = torch.stack(rows)
    loss_ref = per_ref.sum(0) / B
    (loss_ref * g.double()).sum().backward()
    cs = [class_stage(sims[b], tcs[b], bg, scales) for b in range(B)]
    bs = [box_stage(boxes[b], tgt_boxes[b], pred_idx[b], tgt_idx[b]) for b in range(B)]
    cat = lambda evs, d: EV(d([e.v for e in evs]), d([e.e for e in evs]))                    # noqa: E731
    per = cat([cat([c["ev_loss"], x["ev_loss"]], torch.cat) for c, x in zip(cs, bs)], torch.stack)
    ds, db = combine_stage(g, tcs.reshape(-1), bg, cat([c["ev_dsims"] for c in cs], torch.cat), cat([x["ev_dl1"] for x in bs], torch.cat),
                           cat([x["ev_dgiou"] for x in bs], torch.cat), B)
    per_ref = per_ref.detach()
    loss_ref = loss_ref.detach()
    return dict(per_image=(per_ref, tol_of(per, per_ref)), losses=(loss_ref, tol_of(mean_stage(per), loss_ref)),
                grad_sims=(sd.grad, tol_of(EV(ds.v.view(B, P, C), ds.e.view(B, P, C)), sd.grad)),
                grad_boxes=(bd.grad, tol_of(EV(db.v.view(B, P, 4), db.e.view(B, P, 4)), bd.grad)))


def decisions(cost, labels, boxes, bg):
    """The oracle's decisions for one image from ITS cost matrix [P, n]: (pred_idx, tgt_idx, matched labels [P], post-spreading labels [P])."""
    i, j = O.linear_sum_assignment(np.asarray(cost, dtype=np.float64))
    i, j = torch.as_tensor(i), torch.as_tensor(j)
    tc = torch.full((cost.shape[0],), bg, dtype=torch.int64)
    tc[i] = labels[j]
    return i, j, tc, O.spread_labels(boxes, tc, bg)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------------------
def contention_cost(n, P, seed=0):
    """[n, P] f32 (the solver's transposed layout: row = target)."""
    rs = np.random.RandomState(seed)
    i, j = np.arange(n, dtype=np.float64)[:, None], np.arange(P, dtype=np.float64)[None, :]
    c = -(i + 1) * (j + 1) / (n * P) + 1e-3 * rs.rand(n, P)
    if P > 120:
        c[:, 120:] += 1.0
    return c.astype(np.float32)


def sap_trace(costT):
    """oracle/lsap.c's loop on costT [n, P] (n <= P), float64.  Returns (col4row [n], [(rows scanned, chain length) per augmentation])."""
    c = np.asarray(costT, dtype=np.float64)
    n, P = c.shape
    u, v = np.zeros(n), np.zeros(P)
    path = np.full(P, -1, np.int64); row4col = np.full(P, -1, np.int64); col4row = np.full(n, -1, np.int64)
    trace = []
    for cur in range(n):
        remaining = np.arange(P - 1, -1, -1)
        nrem = P
        spc = np.full(P, np.inf)
        SR = np.zeros(n, bool); SC = np.zeros(P, bool)
        i, min_val, sink = cur, 0.0, -1
        while sink == -1:
            SR[i] = True
            rem = remaining[:nrem]
            r = min_val + c[i, rem] - u[i] - v[rem]
            better = r < spc[rem]
            path[rem[better]] = i
            spc[rem[better]] = r[better]
            vals = spc[rem]
            lowest = vals.min()
            eq = np.nonzero(vals == lowest)[0]
            free = eq[row4col[rem[eq]] == -1]
            index = int(free[-1]) if free.size else int(eq[0])
            min_val = lowest
            j = int(rem[index])
            if row4col[j] == -1:
                sink = j
            else:
                i = int(row4col[j])
            SC[j] = True
            nrem -= 1
            remaining[index] = remaining[nrem]
        u[cur] += min_val
        others = SR.copy(); others[cur] = False
        u[others] += min_val - spc[col4row[others]]
        v[SC] -= min_val - spc[SC]
        j, chain = sink, 0
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            chain += 1
            if i == cur:
                break
        trace.append((int(SR.sum()), chain))
    return col4row, trace


def edge_rows(P):
    want = {0, 1, 30, 31, 32, 33, 63, 64, 65, 2046, 2047, 2048, 2049, 2111, 2112, 4094, 4095, 4096, 4097, P - 2, P - 1}
    return sorted(r for r in want if 0 <= r < P)


SPREAD_PATTERNS = ("forward", "overwrite", "mixed", "background")
SPREAD_BG = 7
_DX = 0.06           # shift between chain neighbours of unit boxes: IoU (1 - d) / (1 + d) = 0.887; second neighbours 0.786


def spread_case(P, pattern):
    """-> dict(boxes [P, 4] f32, tc [P] i64, expect {row: final label} for every row the pattern speaks about, changed = rows whose label changes)."""
    G = int(math.ceil(math.sqrt(P)))
    r = np.arange(P)
    x0 = 10.0 + (r % G) / G
    y0 = 10.0 + (r // G) / G
    boxes = np.stack([x0, y0, x0 + 0.5 / G, y0 + 0.5 / G], -1).astype(np.float32)
    tc = np.full(P, SPREAD_BG, np.int64)
    expect = {}

    def chain(rows, y):
        for k, row in enumerate(rows):
            boxes[row] = (20.0 + k * _DX, y, 21.0 + k * _DX, y + 1.0)

    E = edge_rows(P)
    if pattern == "forward":
        chain(E, 20.0)
        tc[E[0]] = 1
        expect = {row: 1 for row in E}
    elif pattern == "overwrite":
        chain(E, 20.0)
        tc[E[0]], tc[E[1]], tc[E[-1]] = 1, 2, 3
        expect = {row: 1 for row in E}
    elif pattern == "mixed":
        b1, b2 = (P // 2 + 3, 5)
        chain([P - 1, b1, b2], 30.0)
        tc[P - 1] = 2
        expect.update({P - 1: 2, b1: 2, b2: SPREAD_BG})
        if P > 2300:
            chain([2300, 2200, 2100], 40.0)
            tc[2300] = 3
            expect.update({2300: 3, 2200: 3, 2100: SPREAD_BG})
        # zero-area boxes: a seed (IoU with itself 0 / 0) and two background rows, one of them on top of the seed
        boxes[8] = (50.0, 50.0, 50.0, 51.0); boxes[9] = (50.0, 50.0, 50.0, 51.0); boxes[11] = (60.0, 60.0, 60.0, 60.0)
        tc[8] = 4
        expect.update({8: 4, 9: SPREAD_BG, 11: SPREAD_BG})
        # IoU exactly float32(0.85) with the unit box at the origin, and one ulp above it (along the other axis, so the two do not meet above 0.85)
        above = float(np.nextafter(np.float32(0.85), np.float32(1)))
        boxes[12] = (0.0, 0.0, 1.0, 1.0); boxes[13] = (0.0, 0.0, THR32, 1.0); boxes[14] = (0.0, 0.0, 1.0, above)
        tc[12] = 5
        expect.update({12: 5, 13: SPREAD_BG, 14: 5})
    elif pattern != "background":
        raise ValueError(pattern)
    changed = sum(1 for row, lab in expect.items() if lab != tc[row])
    return dict(boxes=torch.from_numpy(boxes), tc=torch.from_numpy(tc), expect=expect, changed=changed)


def make_sims(profile, B, P, C, seed):
    rs = np.random.RandomState(seed)
    sign = np.where(rs.rand(B, P, C) < 0.5, -1.0, 1.0)
    if profile == "uniform":
        s = rs.rand(B, P, C) * 1.2 - 0.6
    elif profile == "trained_like":
        s = sign * 10.0 ** (-4.0 + 2.0 * rs.rand(B, P, C))
        hot = (np.arange(P)[None, :] + np.arange(B)[:, None]) % C
        k = 1 + (np.arange(B * P).reshape(B, P) % 4)
        np.put_along_axis(s, hot[..., None], (np.take_along_axis(sign, hot[..., None], -1)[..., 0] * (1.0 - k * 2.0 ** -24))[..., None], -1)
    elif profile == "tiny":
        mags = np.array([1e-20, 1e-40, 1.4e-45, 3e-39, 1e-30, 1e-12, 1e-7, 2.0 ** -126])
        s = sign * mags[rs.randint(0, len(mags), (B, P, C))]
    elif profile == "exact":
        vals = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 0.0])
        s = vals[rs.randint(0, len(vals), (B, P, C))]
    else:
        raise ValueError(profile)
    return torch.from_numpy(s.astype(np.float32))


def make_case(profile, B, P, C, seed, counts, spread=0):
    """-> dict(sims [B, P, C], boxes [B, P, 4], labels [n_b] list, tgt [n_b, 4] list).  Target j of image b is a jittered copy of prediction row
    rows_b[j] (every fourth shares x0 and y1 with it exactly); the first `spread` targets' predictions have two near-duplicate neighbours."""
    rs = np.random.RandomState(seed + 7919)
    sims = make_sims(profile, B, P, C, seed)
    x0, y0 = rs.rand(B, P) * 0.7, rs.rand(B, P) * 0.7
    w, h = 0.03 + rs.rand(B, P) * 0.25, 0.03 + rs.rand(B, P) * 0.25
    boxes = np.stack([x0, y0, x0 + w, y0 + h], -1).astype(np.float32)
    labels, tgt = [], []
    for b in range(B):
        n = counts[b]
        rows = np.sort(rs.choice(np.arange(0, P - 2, 3), n, replace=False))
        for j in range(min(spread, n)):
            for d in (1, 2):
                wh = boxes[b, rows[j], 2:] - boxes[b, rows[j], :2]
                boxes[b, rows[j] + d] = boxes[b, rows[j]] + np.float32(0.01 * d) * np.concatenate([wh, wh])      # IoU 0.96 / 0.92 with the original
        t = boxes[b, rows] + (rs.rand(n, 4).astype(np.float32) - 0.5) * np.float32(0.02)
        t[::4, 0] = boxes[b, rows[::4], 0]
        t[::4, 3] = boxes[b, rows[::4], 3]
        lab = (rows + b) % C                                   # trained_like: the prediction's hot column ...
        lab[1::2] = (lab[1::2] + 1) % C                        # ... and, for every other target, its neighbour
        labels.append(torch.from_numpy(lab.astype(np.int64)))
        tgt.append(torch.from_numpy(t.astype(np.float32)))
    return dict(sims=sims, boxes=torch.from_numpy(boxes), labels=labels, tgt=tgt)


def edge_pairs():
    """Hand-placed matched pairs for box_stage: (boxes [6, 4], tgt [6, 4], pred_idx = tgt_idx = 0..5): identical boxes (every max / min ties), a shared
    x0 and y1, intersection width exactly 0 (touching: clamp(min=0) passes the gradient through), disjoint, nested, plain overlap."""
    tgt = torch.tensor([[0.25, 0.25, 0.5, 0.75], [0.125, 0.25, 0.5, 0.625], [0.5, 0.25, 0.75, 0.5], [0.0625, 0.125, 0.25, 0.375],
                        [0.25, 0.25, 0.75, 0.75], [0.3, 0.1, 0.6, 0.7]], dtype=torch.float32)
    boxes = torch.tensor([[0.25, 0.25, 0.5, 0.75], [0.125, 0.3, 0.45, 0.625], [0.25, 0.125, 0.5, 0.375], [0.5, 0.5, 0.75, 0.875],
                          [0.375, 0.3, 0.5, 0.6], [0.2, 0.3, 0.5, 0.9]], dtype=torch.float32)
    idx = torch.arange(6)
    return boxes, tgt, idx, idx.clone()
