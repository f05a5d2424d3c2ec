"""Float64 references, derived error bounds and input builders for the open-vocabulary criterion of csrc/open_vocab_loss.hip: ovl_cost_kernel,
ovl_focal_kernel (forward and backward), ovl_pairs_kernel, ovl_reduce_kernel and ovl_boxes_bwd_kernel.  Checker side, CPU only: nothing here imports
the package.  The `EV` arithmetic, `tol_of`, `LIBM` and `decisions` are tests/loss_reference.py's.

Contract restated: transformers' DeformableDetrHungarianMatcher + DeformableDetrImageLoss(losses=["labels", "boxes"]) + sigmoid_focal_loss on
(logits, corners_to_center(pred_boxes)), targets in centre form (tests/test_open_vocab_loss_reference.py pins the restatement to live transformers and
to the recorded fixture tests/golden/f17_open_vocab_loss.npz).  A masked query's logit is -FLT_MAX: HF's term there is exactly 0 with gradient 0, which
is what selecting the column out gives for ANY bits.

References (float64, on the kernel's exact f32 inputs), one per stage; each takes the DISCRETE decisions (assignment, target classes) as inputs
----------
`cost_double / cost_stage`      cost[p, j] = w_bbox L1(centre) + w_class (pos - neg) + w_giou (-GIoU(corners)).
`class_double / class_stage`    the focal element of every (row, query), selected to 0 under the mask, its sum and d element / d logit.
`box_stage`                     sum L1(centre forms), sum (1 - GIoU) over the matched pairs of one image and their gradients wrt the CORNER boxes.
`reduce_stage`                  the three sums / num_boxes.
`backward_stage`                dlogits = (g_ce / num_boxes) d element, dboxes = (g_bbox dl1 + g_giou dgiou) / num_boxes.
`criterion`                     all chained; the VALUES are torch autograd in double through `loss_double`.
The GIoU is taken on the corners as given (HF converts centre -> corners -> the same numbers to 1e-16; at an exact max / min tie of two corners torch
splits the gradient 0.5 / 0.5, which the round trip in double would break -- the fixture has no ties, the GPU cases do).

Bounds (elementwise, derived, no fitted constant)
------
Every stage is also written as the kernel's own operation sequence over EV pairs: one rounding per written f32 operation (the file is compiled with
-ffp-contract=off), expf / logf / log1pf within LIBM (ASSUMPTION L1), a correctly rounded division (L2).  Sums are f64 in the kernel: their error is
the sum of the element errors, 2^-53 per add, and the ONE final rounding to f32.  Two places need more than the first-order rule:
 * logf(x + 1e-8f) in the cost, where x = 1 - sigmoid carries an absolute error of an f32 ulp of 1 against a value that can be 1e-8: `vlog_floor`
   bounds the logarithm over the whole interval [max(v - e, floor), v + e], floor = 1e-8f (1 - F): x >= 0 exactly in f32, so the argument never
   falls below fl(1e-8f).  HF's formula has this cancellation by construction; the bound is wide exactly there.  The class LOSS does not: it
   evaluates 1 - p_t as sigmoid(z), the form the bound counts.  Where expf(-x) < F / 2 (x > 17.4) the f32 chain is exact -- 1 + e = 1, p = 1,
   1 - p = 0 -- and the bound says so: it is wide only for x between about 13 and 17.4.
 * sign(cx_a - cx_t) of the L1 gradient: the centre (x0 + x1) / 2 is rounded, so where |difference| <= its error the f32 sign is not determined and
   the bound admits either (`sgn_ev`); an exact zero is exact in f32 too (equal sums round equally).

Builders -- tests/test_open_vocab_loss_reference.py asserts that each does what it claims
--------
`make_logits(profile, B, P, Q, seed)`  uniform (+-8) | saturated (+-40, +-100 among uniform) | zero | tiny (1e-20, subnormals) | mixed.
`make_case(...)`   logits of a profile, -FLT_MAX or NaN under the mask, random boxes, targets = jittered copies of chosen predictions (every fourth shares
                   x0 and y1 with it exactly), labels among the image's live queries.
`fixture_inputs()` the fixture's case: three images with 1 / 3 / 5 targets, Q = 5, two padded queries on image 1, no ties, matched logits raised: margin.
`GPU_CASES`        the shapes tests/test_open_vocab_loss_gpu.py runs; `planted(...)` the wrong formulas the bounds must catch on them.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from tests import loss_reference as LR
from tests.gemm_reference import F, check, ratios  # noqa: F401
from tests.loss_reference import DEN, EV, LIBM, add, decisions, div, mul, pick, scaled, sub, tol_of, vabs, vexp  # noqa: F401

F64 = torch.float64
FMIN = float(torch.finfo(torch.float32).min)
EPS8 = float(np.float32(1e-8))
U64 = 2.0 ** -53
CHUNK, MAX_PARTS = 256 * 8, 1024          # ovl_focal_kernel's chunk of units and the cap on its workgroups


def f32(x):
    return float(np.float32(x))


def n_parts(B, P, Q):
    """Workgroups (= f64 partials) of the class kernel: a function of the shape alone."""
    units = B * P * (Q // 4 if Q % 4 == 0 else Q)
    return min((units + CHUNK - 1) // CHUNK, MAX_PARTS)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 restatement of transformers' formulas
# ---------------------------------------------------------------------------------------------------------------------------------------------
def corners_to_center(b):
    x0, y0, x1, y1 = b.unbind(-1)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1)


def center_to_corners(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou(a, b):
    """HF's generalized_box_iou elementwise over broadcastable corner boxes [..., 4] (torch.max / min / clamp: torch's tie and clamp gradients)."""
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a + area_b - inter
    iou = inter / union
    whc = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    area = whc[..., 0] * whc[..., 1]
    return iou - (area - union) / area


def label_ok(labels, live_row, Q):
    ok = (labels >= 0) & (labels < Q)
    if live_row is not None:
        ok = ok & live_row[labels.clamp(0, Q - 1)]
    return ok


def cost_double(logits, boxes, labels, tgt, live_row=None, alpha=0.25, wc=1.0, wb=5.0, wg=2.0, variant=None):
    """logits [P, Q], boxes [P, 4] corners, tgt [n, 4] corners (any float dtype) -> cost [P, n] f64, DeformableDetrHungarianMatcher's."""
    x, bd, td = logits.double(), boxes.double(), tgt.double()
    Q = x.shape[1]
    ok = label_ok(labels, live_row, Q)
    cols = labels.clamp(0, Q - 1)
    xs = x[:, cols]
    xs = torch.where(ok[None, :].expand_as(xs), xs, torch.zeros_like(xs))
    if variant == "softmax":
        xm = x if live_row is None else torch.where(live_row[None, :].expand_as(x), x, torch.full_like(x, FMIN))
        p = xm.softmax(-1)[:, cols]
    else:
        p = xs.sigmoid()
    neg = (1 - alpha) * (p ** 2) * (-(1 - p + 1e-8).log())
    pos = alpha * ((1 - p) ** 2) * (-(p + 1e-8).log())
    cls = torch.where(ok[None, :].expand_as(xs), pos - neg, torch.zeros_like(xs))
    l1 = torch.cdist(bd, td, p=1) if variant == "l1_corners" else torch.cdist(corners_to_center(bd), corners_to_center(td), p=1)
    g = giou(bd[:, None, :], td[None, :, :])
    return wb * l1 + wc * cls + wg * (g if variant == "plus_giou" else -g)


def focal_double(x, t, alpha, variant=None):
    """transformers' sigmoid_focal_loss element (before its mean / sum / num_boxes), gamma = 2."""
    prob = x.sigmoid()
    ce = Fn.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = prob * t + (1 - prob) * (1 - t)
    loss = ce * ((1 - p_t) if variant == "gamma1" else (1 - p_t) ** 2)
    if alpha >= 0:
        a_t = (1 - alpha) * t + alpha * (1 - t) if variant == "alpha_swapped" else alpha * t + (1 - alpha) * (1 - t)
        loss = a_t * loss
    return loss


def class_double(x, tc, live, alpha, variant=None):
    """x [R, Q] f64 (may require grad), tc [R] i64 (background = Q), live [R, Q] bool -> the element of every (row, query), 0 where masked."""
    R, Q = x.shape
    onehot = torch.zeros(R, Q + 1, dtype=x.dtype)
    onehot.scatter_(1, tc.clamp(0, Q)[:, None], 1.0)
    if variant == "bg_spill":
        onehot[:, Q - 1] = torch.maximum(onehot[:, Q - 1], onehot[:, Q])
    t = onehot[:, :Q]
    if variant == "mask_multiplied":
        return focal_double(x, t, alpha) * live.to(x.dtype)
    xs = torch.where(live, x, torch.zeros_like(x))
    return torch.where(live, focal_double(xs, t, alpha, variant), torch.zeros_like(xs))


def _live(mask, B, P, Q):
    if mask is None:
        return torch.ones(B, P, Q, dtype=torch.bool)
    m = mask.bool()
    return (m if m.shape[0] == B else m.expand(B, Q))[:, None, :].expand(B, P, Q)


def loss_double(logits, boxes, mask, tcs, pred_idx, tgt_idx, tgts, alpha, num_boxes, variant=None):
    """The three losses in double (differentiable wrt logits [B, P, Q] and corner boxes [B, P, 4], both f64).  tgts: per-image corner boxes."""
    B, P, Q = logits.shape
    live = _live(mask, B, P, Q)
    el = class_double(logits.reshape(B * P, Q), tcs.reshape(-1), live.reshape(B * P, Q), alpha, variant).view(B, P, Q)
    l1s, gis = [], []
    for b in range(B):
        src, tg = boxes[b][pred_idx[b]], tgts[b].double()[tgt_idx[b]]
        if variant == "l1_corners":
            l1s.append(Fn.l1_loss(src, tg, reduction="none").sum())
        else:
            l1s.append(Fn.l1_loss(corners_to_center(src), corners_to_center(tg), reduction="none").sum())
        gis.append((1 + giou(src, tg)).sum() if variant == "plus_giou" else (1 - giou(src, tg)).sum())
    if variant == "per_image":
        ns = [max(1, int(p.shape[0])) for p in pred_idx]
        return (sum(el[b].sum() / ns[b] for b in range(B)) / B, sum(l1s[b] / ns[b] for b in range(B)) / B, sum(gis[b] / ns[b] for b in range(B)) / B)
    ce = el.sum() / num_boxes
    if variant == "mean_q":
        ce = ce / Q
    return ce, sum(l1s) / num_boxes, sum(gis) / num_boxes


# ---------------------------------------------------------------------------------------------------------------------------------------------
# EV helpers this criterion adds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def vlog_floor(a, floor):
    """logf of an EV whose f32 value is known to be >= floor > 0: the logarithm's range over [max(v - e, floor), v + e], plus the libm budget."""
    v = torch.log(a.v)
    up = torch.log1p(a.e / a.v)
    lo = a.v - a.e
    lo = torch.where(lo > floor, lo, torch.full_like(lo, floor))
    lo = torch.minimum(lo, a.v)
    down = torch.log(a.v / lo)
    dev = torch.maximum(up, down)
    return EV(v, dev + LIBM * (v.abs() + dev) + DEN)


def vlog1p(a):
    """log1pf of an EV >= 0 (d/dx = 1 / (1 + x) <= 1 / (1 + max(v - e, 0)))."""
    v = torch.log1p(a.v)
    return EV(v, a.e / (1.0 + (a.v - a.e).clamp(min=0.0)) + LIBM * v.abs() + DEN)


def sgn_ev(d):
    """sign of an f32 difference whose operands were rounded: exact where |v| > e or v == 0, undetermined (either sign, or 0) otherwise."""
    s = torch.sign(d.v)
    loose = (d.v.abs() <= d.e) & (d.v != 0)
    return EV(s, torch.where(loose, torch.full_like(s, 2.0), torch.zeros_like(s)))


def _center_ev(x0, x1):
    return scaled(add(x0, x1), 0.5), sub(x1, x0)


def _l1_center_ev(a, t):
    """|cx - tcx| + |cy - tcy| + |w - tw| + |h - th| left to right, on coordinate tuples; also the four differences."""
    acx, aw = _center_ev(a[0], a[2])
    acy, ah = _center_ev(a[1], a[3])
    tcx, tw = _center_ev(t[0], t[2])
    tcy, th = _center_ev(t[1], t[3])
    d = [sub(acx, tcx), sub(acy, tcy), sub(aw, tw), sub(ah, th)]
    l1 = add(add(add(vabs(d[0]), vabs(d[1])), vabs(d[2])), vabs(d[3]))
    return l1, d


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stage 1: matching cost
# ---------------------------------------------------------------------------------------------------------------------------------------------
def cost_stage(logits, boxes, labels, tgt, live_row=None, alpha=0.25, wc=1.0, wb=5.0, wg=2.0):
    """logits [P, Q], boxes [P, 4], tgt [n, 4] f32; labels [n] i64; live_row [Q] bool or None -> dict(ref [P, n] f64, ev, tol)."""
    a32 = f32(alpha)
    ref = cost_double(logits, boxes, labels, tgt, live_row, a32, f32(wc), f32(wb), f32(wg))
    x, bd, td = logits.double(), boxes.double(), tgt.double()
    Q = x.shape[1]
    ok = label_ok(labels, live_row, Q)[None, :].expand(x.shape[0], labels.shape[0])
    xs = x[:, labels.clamp(0, Q - 1)]
    xs = torch.where(ok, xs, torch.zeros_like(xs))
    ex = vexp(EV(-xs))
    pr = div(1.0, add(1.0, ex))
    om = sub(1.0, pr)
    # expf(-x) below half an ulp of 1: 1 + e rounds to 1, 1 / 1 = 1 and 1 - 1 = 0 exactly -- the f32 values are known, not merely bounded
    sat = (ex.v + ex.e) < 0.5 * F
    pr = pick(sat, EV(pr.v, (1.0 - pr.v).abs()), pr)
    om = pick(sat, EV(om.v, om.v.abs()), om)
    floor = EPS8 * (1.0 - F)
    pos = mul(mul(a32, mul(om, om)), scaled(vlog_floor(add(pr, EPS8), floor), -1.0))
    neg = mul(mul(sub(1.0, a32), mul(pr, pr)), scaled(vlog_floor(add(om, EPS8), floor), -1.0))
    cls = pick(ok, sub(pos, neg), EV(torch.zeros_like(xs)))
    a = tuple(EV(bd[:, None, k]) for k in range(4))
    t = tuple(EV(td[None, :, k]) for k in range(4))
    l1, _ = _l1_center_ev(a, t)
    g, _ = LR._giou_ev(a, t)
    ev = add(add(mul(f32(wb), l1), mul(f32(wc), cls)), mul(f32(wg), scaled(g, -1.0)))
    return dict(ref=ref, ev=ev, tol=tol_of(ev, ref))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stage 2: the focal element and its derivative (ovl_focal)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def class_stage(logits, tc, live, alpha=0.25):
    """logits [R, Q] f32, tc [R] i64 (background = Q), live [R, Q] bool -> dict(el = (ref, ev), del_ = (ref, ev), total = (ref f64 scalar, ev))."""
    R, Q = logits.shape
    a32 = f32(alpha)
    xd = logits.double().requires_grad_(True)
    el_ref = class_double(xd, tc, live, a32)
    d_ref, = torch.autograd.grad(el_ref.sum(), xd)
    el_ref = el_ref.detach()

    x = torch.where(live, logits.double(), torch.zeros(R, Q, dtype=F64))
    t = tc[:, None] == torch.arange(Q)[None, :]
    z = torch.where(t, -x, x)
    nn = z >= 0
    e = vexp(EV(-z.abs()))
    d = add(1.0, e)
    l = vlog1p(e)
    sp = add(EV(z.clamp(min=0.0)), l)
    one = EV(torch.ones_like(z))
    s = div(pick(nn, one, e), d)
    m = mul(s, s)
    at = pick(t, EV(torch.full_like(z, a32)), sub(1.0, EV(torch.full_like(z, a32))))
    v = mul(sp, m)
    c = div(pick(nn, e, one), d)
    k = add(mul(scaled(c, 2.0), sp), s)
    gz = mul(m, k)
    if a32 >= 0:
        v, gz = mul(at, v), mul(at, gz)
    gz = scaled(gz, torch.where(t, -1.0, 1.0))
    zero = EV(torch.zeros_like(z))
    ev_el, ev_d = pick(live, v, zero), pick(live, gz, zero)
    n = R * Q
    tot = EV(ev_el.v.sum(), ev_el.e.sum() + n * U64 * (ev_el.v.abs() + ev_el.e).sum())
    return dict(el=(el_ref, ev_el), del_=(d_ref, ev_d), total=(el_ref.sum(), tot))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stage 3: matched pairs of one image (ovl_pairs_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def box_stage(boxes, tgt, pred_idx, tgt_idx):
    """boxes [P, 4], tgt [n, 4] corners f32; pred_idx, tgt_idx [n] i64 -> dict(sums = (ref [2] f64, ev [2]) for (sum L1, sum 1 - GIoU),
    dl1 / dgiou = (ref [P, 4], ev)): unscaled; rows no pair names hold exact zeros."""
    P, n = boxes.shape[0], int(pred_idx.shape[0])
    zero = torch.zeros(P, 4, dtype=F64)
    if n == 0:
        z2 = torch.zeros(2, dtype=F64)
        return dict(sums=(z2, EV(z2)), dl1=(zero, EV(zero)), dgiou=(zero, EV(zero)))
    bd = boxes.double().requires_grad_(True)
    src, tg = bd[pred_idx], tgt.double()[tgt_idx]
    l1_ref = Fn.l1_loss(corners_to_center(src), corners_to_center(tg), reduction="none").sum()
    g_ref = (1 - giou(src, tg)).sum()
    dl1_ref, = torch.autograd.grad(l1_ref, bd, retain_graph=True)
    dg_ref, = torch.autograd.grad(g_ref, bd)
    ref = torch.stack([l1_ref.detach(), g_ref.detach()])

    A, T = boxes.double()[pred_idx], tgt.double()[tgt_idx]
    a = tuple(EV(A[:, k]) for k in range(4))
    t = tuple(EV(T[:, k]) for k in range(4))
    l1, dd = _l1_center_ev(a, t)
    gi, q = LR._giou_ev(a, t)
    og = sub(1.0, gi)

    def total(x):
        return EV(x.v.sum(), x.e.sum() + n * U64 * (x.v.abs() + x.e).sum())

    s1, s2 = total(l1), total(og)
    ev_s = EV(torch.stack([s1.v, s2.v]), torch.stack([s1.e, s2.e]))
    sx, sy, sw, sh = scaled(sgn_ev(dd[0]), 0.5), scaled(sgn_ev(dd[1]), 0.5), sgn_ev(dd[2]), sgn_ev(dd[3])
    ex = lambda p, q_, sign: EV(p.v + sign * q_.v, p.e + q_.e)                       # noqa: E731  (multiples of 0.5: exact)
    d1 = [ex(sx, sw, -1.0), ex(sy, sh, -1.0), ex(sx, sw, 1.0), ex(sy, sh, 1.0)]
    on = lambda x: (x.v >= 0).double()                                                # noqa: E731  (the sign of a difference of exact inputs is exact)
    dw_on, dh_on, dcw_on, dch_on = on(q["dw"]), on(q["dh"]), on(q["dcw"]), on(q["dch"])
    gt, lt = LR._w_gt, lambda x, y: LR._w_gt(y, x)                                    # noqa: E731
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
        d2.append(scaled(add(d_iou, d_ratio), -1.0))

    def scatter(cols):
        v = torch.zeros(P, 4, dtype=F64); e = torch.zeros(P, 4, dtype=F64)
        v[pred_idx] = torch.stack([c_.v.expand(n) for c_ in cols], 1)
        e[pred_idx] = torch.stack([c_.e.expand(n) for c_ in cols], 1)
        return EV(v, e)

    return dict(sums=(ref, ev_s), dl1=(dl1_ref, scatter(d1)), dgiou=(dg_ref, scatter(d2)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stages 4 and 5: reduce, backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
def reduce_stage(sums, num_boxes):
    """sums: EV [3] of f64 sums -> EV [3]: (float)(sum / num_boxes), the one f32 rounding."""
    v = sums.v / num_boxes
    return EV(v, sums.e / num_boxes + 2 * U64 * v.abs() + F * v.abs() + DEN)


def backward_stage(g3, del_, dl1, dgiou, num_boxes):
    """g3 [3] f32; del_ EV [.., Q]; dl1, dgiou EV [.., 4] -> (EV dlogits, EV dboxes), as ovl_focal_kernel<BWD> and ovl_boxes_bwd_kernel write them."""
    g = g3.double()
    inv = EV(torch.tensor(1.0 / num_boxes, dtype=F64), torch.tensor(F / num_boxes + U64 / num_boxes + DEN, dtype=F64))
    gs, gb, gg = mul(EV(g[0]), inv), mul(EV(g[1]), inv), mul(EV(g[2]), inv)
    return mul(gs, del_), add(mul(gb, dl1), mul(gg, dgiou))


def criterion(logits, boxes, mask, tcs, pred_idx, tgt_idx, tgts, alpha, num_boxes, g3):
    """The whole criterion at given decisions.  logits [B, P, Q], boxes [B, P, 4] f32; mask [nm, Q] bool or None; tcs [B, P]; pred_idx / tgt_idx / tgts:
    per-image lists; g3 [3] f32.  Returns name -> (ref, tol) for losses [3], dlogits [B, P, Q], dboxes [B, P, 4]."""
    B, P, Q = logits.shape
    a32 = f32(alpha)
    ld = logits.double()
    ld = torch.where(_live(mask, B, P, Q), ld, torch.zeros_like(ld)).requires_grad_(True)          # (NaN under the mask must not reach autograd)
    bd = boxes.double().requires_grad_(True)
    ce, l1, gi = loss_double(ld, bd, mask, tcs, pred_idx, tgt_idx, tgts, a32, num_boxes)
    loss_ref = torch.stack([ce, l1, gi])
    (loss_ref * g3.double()).sum().backward()
    live = _live(mask, B, P, Q).reshape(B * P, Q)
    cs = class_stage(logits.reshape(B * P, Q), tcs.reshape(-1), live, alpha)
    bs = [box_stage(boxes[b], tgts[b], pred_idx[b], tgt_idx[b]) for b in range(B)]
    bsum = EV(sum(x["sums"][1].v for x in bs), sum(x["sums"][1].e for x in bs))
    sums = EV(torch.cat([cs["total"][1].v.reshape(1), bsum.v]), torch.cat([cs["total"][1].e.reshape(1), bsum.e]))
    ev_loss = reduce_stage(sums, num_boxes)
    cat = lambda key: EV(torch.stack([x[key][1].v for x in bs]), torch.stack([x[key][1].e for x in bs]))          # noqa: E731
    dlg, dbx = backward_stage(g3, cs["del_"][1], cat("dl1"), cat("dgiou"), num_boxes)
    dlg = EV(dlg.v.view(B, P, Q), dlg.e.view(B, P, Q))
    loss_ref = loss_ref.detach()
    return dict(losses=(loss_ref, tol_of(ev_loss, loss_ref)), dlogits=(ld.grad, tol_of(dlg, ld.grad)), dboxes=(bd.grad, tol_of(dbx, bd.grad)))


def decide(cost, labels, Q):
    """The oracle's decisions for one image from a cost matrix [P, n]: (pred_idx, tgt_idx, target classes [P] with background Q)."""
    P, n = cost.shape
    if n == 0:
        e = torch.zeros(0, dtype=torch.int64)
        return e, e.clone(), torch.full((P,), Q, dtype=torch.int64)
    i, j, tc, _ = decisions(cost, labels, torch.zeros(P, 4), Q)
    return i, j, tc


# ---------------------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILES = ("uniform", "saturated", "zero", "tiny", "mixed")


def make_logits(profile, B, P, Q, seed):
    rs = np.random.RandomState(seed)
    uni = rs.rand(B, P, Q) * 16.0 - 8.0
    sign = np.where(rs.rand(B, P, Q) < 0.5, -1.0, 1.0)
    sat = sign * np.array([40.0, 100.0])[rs.randint(0, 2, (B, P, Q))]
    tiny = sign * np.array([1e-20, 1e-40, 1.4e-45, 1e-7, 2.0 ** -126])[rs.randint(0, 5, (B, P, Q))]
    pickk = rs.randint(0, 4, (B, P, Q))
    if profile == "uniform":
        x = uni
    elif profile == "saturated":
        x = np.where(pickk < 2, sat, uni)
    elif profile == "zero":
        x = np.zeros((B, P, Q))
    elif profile == "tiny":
        x = tiny
    elif profile == "mixed":
        x = np.choose(pickk, [uni, sat, tiny, np.zeros((B, P, Q))])
    else:
        raise ValueError(profile)
    return torch.from_numpy(x.astype(np.float32))


def make_mask(kind, B, Q, seed):
    """None | 'shared' [1, Q] | 'per_image' [B, Q]: about a third of the queries masked, query 0 always live, image 0 of a per-image mask all live."""
    if kind is None:
        return None
    rs = np.random.RandomState(seed + 101)
    m = rs.rand(1 if kind == "shared" else B, Q) > 0.35
    m[:, 0] = True
    if kind == "per_image":
        m[0, :] = True
    return torch.from_numpy(m)


def make_case(B, P, Q, counts, mask_kind, profile, fill, seed, jitter=0.02, ties=True):
    """-> dict(logits [B, P, Q] with `fill` (FMIN or nan) under the mask, boxes [B, P, 4], mask, labels / tgt per-image lists (corners), counts)."""
    rs = np.random.RandomState(seed + 7919)
    logits = make_logits(profile, B, P, Q, seed)
    mask = make_mask(mask_kind, B, Q, seed)
    if mask is not None:
        live = _live(mask, B, P, Q)
        logits = torch.where(live, logits, torch.full_like(logits, fill))
    x0, y0 = rs.rand(B, P) * 0.7, rs.rand(B, P) * 0.7
    w, h = 0.03 + rs.rand(B, P) * 0.25, 0.03 + rs.rand(B, P) * 0.25
    boxes = np.stack([x0, y0, x0 + w, y0 + h], -1).astype(np.float32)
    labels, tgt = [], []
    for b in range(B):
        n = counts[b]
        rows = np.sort(rs.choice(P, n, replace=False))
        t = boxes[b, rows] + (rs.rand(n, 4).astype(np.float32) - 0.5) * np.float32(jitter)
        if ties:
            t[::4, 0] = boxes[b, rows[::4], 0]
            t[::4, 3] = boxes[b, rows[::4], 3]
        lv = np.arange(Q) if mask is None else np.nonzero(mask[b if mask.shape[0] == B else 0].numpy())[0]
        labels.append(torch.from_numpy(lv[rs.randint(0, len(lv), n)].astype(np.int64)))
        tgt.append(torch.from_numpy(t.astype(np.float32).reshape(n, 4)))
    return dict(logits=logits, boxes=torch.from_numpy(boxes), mask=mask, labels=labels, tgt=tgt, counts=list(counts), rows=None)


def fixture_inputs():
    """The fixture's inputs: B = 3 images of P = 36 patches with 1 / 3 / 5 targets, Q = 5, queries 3 and 4 of image 1 padded (masked, -FLT_MAX); no exact
    ties; the logit of (matched prediction, its label) raised to +4 and that row's others lowered to -4, jitter 0.01: the assignment has margin."""
    B, P, Q, counts = 3, 36, 5, [1, 3, 5]
    rs = np.random.RandomState(1717)
    logits = (rs.rand(B, P, Q) * 4.0 - 4.0).astype(np.float32)
    mask = np.ones((B, Q), dtype=bool)
    mask[1, 3:] = False
    x0, y0 = rs.rand(B, P) * 0.7, rs.rand(B, P) * 0.7
    w, h = 0.03 + rs.rand(B, P) * 0.25, 0.03 + rs.rand(B, P) * 0.25
    boxes = np.stack([x0, y0, x0 + w, y0 + h], -1).astype(np.float32)
    labels, tgt = [], []
    for b in range(B):
        n = counts[b]
        rows = np.sort(rs.choice(P, n, replace=False))
        t = boxes[b, rows] + (rs.rand(n, 4).astype(np.float32) - 0.5) * np.float32(0.01)
        lv = np.nonzero(mask[b])[0]
        lab = lv[rs.randint(0, len(lv), n)]
        logits[b, rows, :] = -4.0 - rs.rand(n, Q).astype(np.float32)
        logits[b, rows, lab] = 4.0 + rs.rand(n).astype(np.float32)
        labels.append(torch.from_numpy(lab.astype(np.int64)))
        tgt.append(torch.from_numpy(t.astype(np.float32)))
    logits[~np.broadcast_to(mask[:, None, :], logits.shape)] = FMIN
    return dict(logits=torch.from_numpy(logits), boxes=torch.from_numpy(boxes), mask=torch.from_numpy(mask), labels=labels, tgt=tgt, counts=counts)


# name -> make_case arguments: P = 4 / 36 / 576, B = 1 / 3 / 5, Q = 1 / 3 / 31 / 32 / 33 / 70 / 260 (the scalar and the 16-byte path, both sides of a
# 32-query tile, several chunks), counts with 0, 1 and Nmax = P at P = 4, every mask kind, every profile, both fills.  "stride" is the one shape at which
# a workgroup of the class kernel walks more than one chunk (B P Q > 1024 chunks of 2048 scalar units).
GPU_CASES = {
    "p4_full": dict(B=1, P=4, Q=3, counts=[4], mask_kind=None, profile="uniform", fill=FMIN, seed=1),
    "q1_zero": dict(B=1, P=36, Q=1, counts=[2], mask_kind=None, profile="zero", fill=FMIN, seed=2),
    "q31_empty": dict(B=3, P=36, Q=31, counts=[0, 1, 5], mask_kind="per_image", profile="uniform", fill=FMIN, seed=3),
    "q32_sat_nan": dict(B=3, P=36, Q=32, counts=[3, 2, 1], mask_kind="shared", profile="saturated", fill=float("nan"), seed=4),
    "q33_nan": dict(B=5, P=576, Q=33, counts=[1, 3, 5, 0, 7], mask_kind="per_image", profile="mixed", fill=float("nan"), seed=5),
    "q70_tiny": dict(B=3, P=576, Q=70, counts=[2, 9, 4], mask_kind=None, profile="tiny", fill=FMIN, seed=6),
    "q260_sat": dict(B=5, P=576, Q=260, counts=[6, 1, 3, 12, 2], mask_kind="per_image", profile="saturated", fill=FMIN, seed=7),
    "stride": dict(B=5, P=576, Q=729, counts=[2, 0, 1, 3, 1], mask_kind="shared", profile="uniform", fill=FMIN, seed=8),
}


def gpu_case(name):
    return make_case(**GPU_CASES[name])


PLANTED = ("alpha_swapped", "gamma1", "softmax", "l1_corners", "plus_giou", "mean_q", "per_image", "bg_spill", "mask_multiplied")


def oracle_decisions(case, alpha=0.25, wc=1.0, wb=5.0, wg=2.0):
    """(tcs [B, P], pred_idx list, tgt_idx list) of the float64 cost under the oracle's LSAP."""
    B, P, Q = case["logits"].shape
    tcs, pi, ti = [], [], []
    for b in range(B):
        live_row = None if case["mask"] is None else case["mask"][b if case["mask"].shape[0] == B else 0]
        c = cost_double(case["logits"][b], case["boxes"][b], case["labels"][b], case["tgt"][b], live_row, alpha, wc, wb, wg)
        i, j, tc = decide(c.numpy(), case["labels"][b], Q)
        pi.append(i); ti.append(j); tcs.append(tc)
    return torch.stack(tcs), pi, ti


def planted(case, variant, dec, num_boxes, g3):
    """What a kernel with the planted error would return, in double: name -> tensor for the outputs the error touches."""
    B, P, Q = case["logits"].shape
    tcs, pi, ti = dec
    if variant == "softmax":
        b = max(range(B), key=lambda i: case["counts"][i])
        live_row = None if case["mask"] is None else case["mask"][b if case["mask"].shape[0] == B else 0]
        return {("cost", b): cost_double(case["logits"][b], case["boxes"][b], case["labels"][b], case["tgt"][b], live_row, variant=variant)}
    ld = case["logits"].double()
    if variant != "mask_multiplied":
        ld = torch.where(_live(case["mask"], B, P, Q), ld, torch.zeros_like(ld))
    ce, l1, gi = loss_double(ld, case["boxes"].double(), case["mask"], tcs, pi, ti, case["tgt"], 0.25, num_boxes, variant)
    return {"losses": torch.stack([ce, l1, gi])}
