"""Float64 reference, derived decision margin and input builders for the inference post-process of csrc/postprocess.hip: pp_sort_kernel, pp_mask_kernel
and pp_scan_kernel behind owl_postprocess (ref src/models.py:122-146 + torchvision.ops.batched_nms).  Checker side, CPU only: nothing here imports the
package, and nothing here calls oracle/owl_oracle.py -- the oracle is one of the things this file judges.

Reference, stage by stage (`reference(boxes, sims, conf, thr, route)`)
---------
`select(sims, conf)`     score_p = max_c sims[p][c] with torch's NaN rule (a NaN anywhere in the row makes the maximum NaN), class_p = the FIRST column that
                         holds the maximum (-0.0 == +0.0, so a [-0.0, +0.0] row answers column 0 and the score keeps that column's bits); a row passes iff
                         score_p > float32(conf), strictly (NaN never passes).  Passing rows are ordered by score descending, then patch index ascending,
                         with -0.0 == +0.0: what a stable descending sort gives.
`route_taken(route, n)`  "per_class" | "coordinate_offset" as asked, or torchvision's own choice for n boxes past the threshold: per class iff
                         boxes.numel() = 4 n > 20000 on a GPU ("torchvision_gpu") / > 4000 on the CPU ("torchvision_cpu"), else the coordinate offset.
`shift(boxes, cls)`      boxes + f32(class) * (boxes.max() + 1): the f32 add, f32 multiply and f32 add torch performs.  This is INPUT rounding -- part of
                         the contract, not of the evaluation -- so it is done in f32 and the IoU below starts from its result.
`exact_nms(boxes, group, thr)`   greedy NMS over the sorted list: box j is suppressed iff a kept box i < j of the same group has IoU(i, j) > float32(thr),
                         the IoU  inter / (area_i + area_j - inter)  (sides of the intersection clamped at 0) evaluated in float64 on those f32
                         coordinates.  Row by row: no n x n array is ever made (n = 8192 would need 512 MB for each).

Decision margin (per pair, derived, no fitted constant)
---------------
Every same-group pair also gets a first-order bound on how far ANY correct f32 evaluation of that formula may land from the float64 value, by the
(value, error) propagation of tests/loss_reference.py:
    z = fl(x op y):   e_z = |dz/dx| e_x + |dz/dy| e_y + f |z| + d          f = 2^-24 (gemm_reference.F), d = 2^-149 (one subnormal step)
over the sequence  w, h, inter = w h, area_i, area_j, area_i + area_j - inter, inter / union:
    sides       x2 - x1 of f32 inputs: e = f |v| (a difference of two floats has no subnormal step to lose).  A side v <= 0 clamps to EXACTLY 0, e = 0:
                rounding is monotone, so fl(v) <= 0 whenever v <= 0.
    products    inter, area_i, area_j: the rule above.  A product with an exactly-zero factor (v = 0, e = 0) is exactly 0.
    union       the three-term sum in ANY association: every partial sum is at most |area_i| + |area_j| + |inter| in magnitude, so
                e = e_ai + e_aj + e_inter + f (|area_i| + |area_j| + |inter|) + f |union| + 2 d  covers (a_i + a_j) - inter and a_i + (a_j - inter) alike.
    quotient    correctly rounded (hipcc's default, and IEEE on the CPU): e = (e_inter + |iou| e_union) / |union| + f |iou| + d; 0 / x with an exactly-zero
                numerator is exactly 0, and 0 / 0 is NaN: neither exceeds a threshold >= 0.
postprocess.hip is compiled with -ffp-contract=off (csrc/build.sh), so one rounding per written operation is what the device does; torchvision's CPU and
GPU kernels and the oracle are sequences of the same operations.  A pair is UNDECIDED when |iou64 - float32(thr)| <= e (or when the bound cannot be
formed: a zero union under a non-zero numerator).  `exact_nms` returns the count over ALL same-group pairs, kept or not.

WHAT THE COUNT PROVES: with 0 undecided pairs, every correct f32 evaluation of the formula -- in any operation order -- takes the float64 decision at
every pair, so it must return exactly the reference's list.  That pins torchvision's two kernels, the oracle and the device kernel at once without
restating anyone's operation order.  Cases built to sit on the threshold (an IoU of exactly 0.5 at thr 0.5, duplicates at thr 1.0, fixture F6's last case)
are undecided by construction: they are compared with the oracle and with hand-written expectations only.

Builders -- tests/test_postprocess_reference.py asserts that each does what it claims
--------
`random_case(P, C, seed, n, cluster)`   the generator of tests/test_postprocess_gpu.py with box sides scaled by min(1, sqrt(576 / P)) (a constant number
    of overlapping neighbours per box), and EXACTLY n rows past CONF = 0.125; when 0 < n < P one dropped row has its maximum equal to CONF and one kept row
    sits one ulp above it.
`lattice_case(P, C, pairs, chains)`     disjoint lattice filler boxes (as loss_reference.spread_case) with scores strictly decreasing in a designed order, so
    sorted position k is patch `perm[k]`; `pairs` (a, b): the box at sorted position a suppresses the one at b (unit boxes 0.25 apart: IoU 0.6); `chains`
    (a, b, c): a suppresses b, b alone would suppress c, a does not reach c (IoU 1/3): c is kept.  Thr 0.5.  -> expected kept positions.
`far_case(n, seed)`                     base boxes of side 2 at coordinates up to 8000, each repeated 10 times with N(0, 0.35) jitter, classes 60..90, exactly n
    rows past the threshold; thr FAR_THR = 0.47 (the shifted coordinates lie on a 1/16 grid: IoUs are small rationals, 0.5 among them).  The two routes'
    lists differ.
`score_profile(name)` / `box_profile(name)`   the named edge inputs at P <= 200 (see SCORE_PROFILES / BOX_PROFILES), each with its hand-written expectation.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests.gemm_reference import F

DEN = 2.0 ** -149
CONF = 0.125
FAR_THR = 0.47
ROUTES = ("per_class", "coordinate_offset", "torchvision_gpu", "torchvision_cpu")
f32 = np.float32

Result = namedtuple("Result", "boxes classes scores patch n undecided route")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# selection, route, shift
# ---------------------------------------------------------------------------------------------------------------------------------------------
def select(sims, conf):
    """-> (patch [n] i64 in sorted order, classes [n] i64, scores [n] f32 with the input's bits)."""
    s = np.asarray(sims, f32)
    P, C = s.shape
    nan = np.isnan(s)
    nanrow = nan.any(1)
    top = np.where(nan, -np.inf, s.astype(np.float64)).max(1)           # float64 holds every f32 exactly; -0.0 == +0.0 in the compare below
    cls = (s.astype(np.float64) == top[:, None]).argmax(1)              # first column equal to the maximum
    score = s[np.arange(P), cls]                                        # that column's bits
    passed = ~nanrow & (score.astype(np.float64) > float(f32(conf)))
    idx = np.nonzero(passed)[0]
    key = -(score[idx].astype(np.float64) + 0.0)                        # -0.0 + 0.0 = +0.0: one key for both zeros
    order = np.lexsort((idx, key))
    idx = idx[order]
    return idx.astype(np.int64), cls[idx].astype(np.int64), score[idx]


def route_taken(route, n):
    if route == "torchvision_gpu":
        return "per_class" if 4 * n > 20000 else "coordinate_offset"
    if route == "torchvision_cpu":
        return "per_class" if 4 * n > 4000 else "coordinate_offset"
    assert route in ("per_class", "coordinate_offset"), route
    return route


def shift(boxes, cls, max_coord=None):
    """boxes + f32(class) * (max + 1) in f32; `max_coord` overrides boxes.max() (to show that another image's maximum gives another list)."""
    b = np.asarray(boxes, f32)
    m = f32(b.max() if max_coord is None else max_coord)
    step = f32(m + f32(1))
    off = (np.asarray(cls).astype(f32) * step).astype(f32)
    return (b + off[:, None]).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact NMS with the per-pair margin
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _rnd(v, prop, den=DEN):
    """Error after rounding v whose propagated error is prop; an exact zero (v == 0, prop == 0) stays exact."""
    return np.where((v == 0) & (prop == 0), 0.0, prop + F * np.abs(v) + den)


def pair_iou(bi, bj):
    """bi [4], bj [m, 4] float64 views of f32 coordinates -> (iou64 [m], e [m], sure_zero [m]): the float64 IoU, the bound on an f32 evaluation of it, and
    where the f32 result is exactly 0 or NaN whatever the order (an exactly-zero intersection)."""
    dxi, dyi = bi[2] - bi[0], bi[3] - bi[1]
    dxj, dyj = bj[:, 2] - bj[:, 0], bj[:, 3] - bj[:, 1]
    ai, aj = dxi * dyi, dxj * dyj
    e_ai = _rnd(ai, np.abs(dxi) * F * np.abs(dyi) + np.abs(dyi) * F * np.abs(dxi))
    e_aj = _rnd(aj, np.abs(dxj) * F * np.abs(dyj) + np.abs(dyj) * F * np.abs(dxj))
    wv = np.minimum(bi[2], bj[:, 2]) - np.maximum(bi[0], bj[:, 0])
    hv = np.minimum(bi[3], bj[:, 3]) - np.maximum(bi[1], bj[:, 1])
    w, h = np.maximum(wv, 0.0), np.maximum(hv, 0.0)
    e_w, e_h = F * w, F * h                                             # 0 where clamped
    inter = w * h
    e_in = _rnd(inter, w * e_h + h * e_w)
    sure_zero = (inter == 0) & (e_in == 0)
    union = ai + aj - inter
    e_un = e_ai + e_aj + e_in + F * (np.abs(ai) + np.abs(aj) + np.abs(inter)) + F * np.abs(union) + 2 * DEN
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / union
        e = _rnd(iou, (e_in + np.abs(iou) * e_un) / np.abs(union))
    return iou, e, sure_zero


def exact_nms(boxes, group, thr):
    """boxes [n, 4] f32 IN SORTED ORDER, group [n] ints or None (class-agnostic) -> (kept positions i64, undecided pair count)."""
    b = np.asarray(boxes, f32).astype(np.float64)
    n = b.shape[0]
    t = float(f32(thr))
    g = None if group is None else np.asarray(group)
    suppressed = np.zeros(n, bool)
    keep, undecided = [], 0
    for i in range(n):
        if i + 1 < n:
            js = np.arange(i + 1, n) if g is None else i + 1 + np.nonzero(g[i + 1:] == g[i])[0]
            # pairs whose intersection is exactly empty are decided without the rest of the sequence (thr >= 0): this is most of them
            if t >= 0 and js.size:
                bj = b[js]
                meet = (np.minimum(b[i, 2], bj[:, 2]) > np.maximum(b[i, 0], bj[:, 0])) & (np.minimum(b[i, 3], bj[:, 3]) > np.maximum(b[i, 1], bj[:, 1]))
                js = js[meet]
            if js.size:
                iou, e, sure_zero = pair_iou(b[i], b[js])
                hit = iou > t                                            # NaN: False, as in f32
                und = ~(np.abs(iou - t) > e)                            # a NaN bound counts as undecided ...
                if t >= 0:
                    und &= ~sure_zero                                   # ... unless the f32 result is exactly 0 or NaN
                undecided += int(und.sum())
                if not suppressed[i]:
                    suppressed[js[hit]] = True
        if not suppressed[i]:
            keep.append(i)
    return np.asarray(keep, np.int64), undecided


def reference(boxes, sims, conf, thr, route="per_class", top_k=None, max_coord=None):
    """One image ([P, 4], [P, C]) -> Result(boxes, classes, scores, patch, n past the threshold, undecided pairs, route taken)."""
    b = np.asarray(boxes, f32)
    idx, cls, score = select(sims, conf)
    n = len(idx)
    taken = route_taken(route, n)
    if n == 0:
        keep, und = np.zeros(0, np.int64), 0
    elif taken == "per_class":
        keep, und = exact_nms(b[idx], cls, thr)
    else:
        keep, und = exact_nms(shift(b[idx], cls, max_coord), None, thr)
    if top_k is not None:
        keep = keep[:top_k]
    return Result(b[idx[keep]], cls[keep], score[keep], idx[keep], n, und, taken)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------------------
def random_case(P, C, seed, n=None, cluster=False):
    """-> (boxes [P, 4], sims [P, C]) with exactly n (default P) rows past CONF."""
    rng = np.random.default_rng(seed)
    n = P if n is None else n
    k = f32(min(1.0, math.sqrt(576.0 / P)))
    if cluster:
        centers = rng.random((8, 2)).astype(f32) * 0.6 + 0.1
        c = centers[rng.integers(0, 8, P)] + rng.normal(0, 0.01, (P, 2)).astype(f32)
        wh = f32(0.2) + rng.normal(0, 0.01, (P, 2)).astype(f32)
    else:
        c = rng.random((P, 2)).astype(f32) * f32(0.7)
        wh = (rng.random((P, 2)).astype(f32) * f32(0.3) + f32(0.02)) * k
    boxes = np.concatenate([c, c + wh], 1).astype(f32)
    sims = ((rng.random((P, C)).astype(f32) * 2 - 1) * f32(0.12)).astype(f32)       # every entry below CONF
    rows = np.sort(rng.permutation(P)[:n])
    win = rng.integers(0, C, P)
    sims[rows, win[rows]] = (f32(0.13) + rng.random(n).astype(f32) * f32(0.4)).astype(f32)
    if 0 < n < P:
        out = np.setdiff1d(np.arange(P), rows)
        sims[out[0], win[out[0]]] = f32(CONF)                                       # equal to the threshold: dropped
        sims[rows[n // 2], win[rows[n // 2]]] = np.nextafter(f32(CONF), f32(1))     # one ulp above: kept
    return boxes, sims


_D = 0.25           # unit boxes _D apart: IoU (1 - _D) / (1 + _D) = 0.6; 2 _D apart: 1 / 3


def lattice_case(P, C=3, pairs=(), chains=(), seed=0):
    """-> dict(boxes, sims, perm [P] (sorted position -> patch), kept = expected kept sorted positions); conf CONF, thr 0.5, n = P."""
    G = int(math.ceil(math.sqrt(P)))
    perm = np.random.default_rng(seed).permutation(P)
    pos = np.arange(P)
    x0, y0 = 10.0 + (pos % G) / G, 10.0 + (pos // G) / G
    bpos = np.stack([x0, y0, x0 + 0.5 / G, y0 + 0.5 / G], -1).astype(f32)           # by sorted position
    cpos = pos % C
    gone = []
    for k, grp in enumerate(list(pairs) + list(chains)):
        for m, a in enumerate(grp):
            bpos[a] = (20.0 + m * _D, 20.0 + 3 * k, 21.0 + m * _D, 21.0 + 3 * k)
            cpos[a] = cpos[grp[0]]
        gone.append(grp[1])
    score = (f32(0.9) - pos.astype(f32) * f32(2.0 ** -14)).astype(f32)               # strictly decreasing: 2^-14 apart, an ulp is 2^-24
    boxes, sims = np.zeros((P, 4), f32), np.full((P, C), f32(-1), f32)
    boxes[perm] = bpos
    sims[perm, cpos] = score
    return dict(boxes=boxes, sims=sims, perm=perm, kept=np.setdiff1d(pos, gone), conf=CONF, thr=0.5)


def far_case(n, seed=0, extra=64):
    """-> (boxes [n + extra, 4], sims [n + extra, 91]): exactly n rows past CONF; thr FAR_THR."""
    rng = np.random.default_rng(seed)
    P = n + extra
    nb = -(-P // 10)
    base = rng.random((nb, 2)) * 7998.0
    c = np.repeat(base, 10, 0)[:P] + rng.normal(0, 0.35, (P, 2))
    boxes = np.concatenate([c, c + 2.0], 1).astype(f32)
    cls = np.repeat(rng.integers(60, 91, nb), 10)[:P]
    sims = np.full((P, 91), f32(-1), f32)
    rows = np.sort(rng.permutation(P)[:n])
    sims[np.arange(P), cls] = f32(0.01)
    sims[rows, cls[rows]] = (f32(0.2) + rng.random(n).astype(f32) * f32(0.7)).astype(f32)
    return boxes, sims


def wide_case(P, C, seed=0):
    """Random boxes, winners spread over the whole class axis: column C - 1 and (C > 256) columns above 255 among them.  All rows pass CONF."""
    rng = np.random.default_rng(seed)
    boxes, _ = random_case(P, 1, seed, cluster=True)
    sims = ((rng.random((P, C)).astype(f32) * 2 - 1) * f32(0.12)).astype(f32)
    cands = np.asarray(sorted({0, min(C - 1, 255), min(C - 1, 256), min(C - 1, 257), C // 2, C - 1}))     # few distinct classes: boxes do meet in one
    win = cands[rng.integers(0, len(cands), P)]
    sims[np.arange(P), win] =(f32(0.2) + rng.random(P).astype(f32) * f32(0.7)).astype(f32)
    return boxes, sims, win


SCORE_PROFILES = ("all_equal", "signed_zeros", "all_negative", "inf_subnormal", "nan", "conf_edge", "zero_columns")
_SUB = f32(2.0 ** -149)


def score_profile(name, P=96):
    """-> dict(boxes, sims, conf, thr, patch = expected SELECTION in sorted order (before NMS; the boxes are a disjoint lattice, so NMS keeps all))."""
    lat = lattice_case(P, 1)
    boxes = lat["boxes"]
    r = np.arange(P)
    if name == "all_equal":                     # one score everywhere: patch order
        sims, conf, exp = np.full((P, 3), f32(0.5), f32), 0.0, r
    elif name == "signed_zeros":                # -0.0 == +0.0: patch order whatever the sign; conf = -1 as the `dup` case of test_postprocess_gpu.py runs
        sims = np.where(((r * 7) % 3 == 0)[:, None], f32(-0.0), f32(0.0)) * np.ones((P, 1), f32)
        sims[:3, 0] = (-0.0, 0.0, -0.0)         # the issue's example
        conf, exp = -1.0, r
    elif name == "zero_columns":                # a row's own columns hold both zeros: first column wins and its bits are the score
        sims = np.zeros((P, 2), f32)
        sims[::2, 0] = -0.0
        sims[1::3, 1] = -0.0
        conf, exp = -0.5, r
    elif name == "all_negative":                # C = 1: the negative branch of the device's ordering key
        sims = (-(f32(0.05) + ((r * 37) % P).astype(f32) / f32(P))).astype(f32)[:, None]
        conf, exp = -2.0, np.argsort(((r * 37) % P), kind="stable")
    elif name == "inf_subnormal":
        sims = np.full((P, 2), f32(-1), f32)
        vals = [np.inf, 3.0e38, 1.0, _SUB * 2, _SUB, 0.0, -0.0, -_SUB, -1.0e-38, -3.0e38, -np.inf]
        rows = [(k * 5 + 3) % P for k in range(len(vals))]
        sims[:, 0] = -0.5
        sims[rows, 1] = np.asarray(vals, f32)
        sims[rows, 0] = -np.inf
        conf = -0.75                            # the -0.5 fillers and everything down to -1e-38 stay; -3e38 and -inf go
        top = np.full(P, -0.5)
        top[rows] = np.asarray(vals, f32).astype(np.float64)
        exp = np.asarray([row for v, row in sorted(((top[q], q) for q in range(P) if top[q] > conf), key=lambda t: (-(t[0] + 0.0), t[1]))])
    elif name == "nan":                         # torch.max: a NaN in ANY column makes the row NaN, and NaN > conf is False
        sims = np.tile(np.asarray([0.3, 0.2, 0.1], f32), (P, 1)) - (r / f32(4 * P)).astype(f32)[:, None]
        sims[2, 0] = np.nan                     # column 0
        sims[5, 1] = np.nan                     # a later column, below the row's maximum
        sims[7, 2] = np.nan                     # the last column
        sims[9, :] = np.nan                     # all
        sims[11, 1] = -np.nan                   # sign bit set
        conf, exp = 0.0, np.setdiff1d(r, [2, 5, 7, 9, 11])
    elif name == "conf_edge":
        sims = np.full((P, 2), f32(0.5), f32) - (r / f32(8 * P)).astype(f32)[:, None]
        conf = 0.3
        sims[4, :] = f32(0.3)                   # equal: dropped
        sims[6, :] = np.nextafter(f32(0.3), f32(1))   # one ulp above: kept, last
        sims[8, :] = np.nextafter(f32(0.3), f32(0))   # one ulp below: dropped
        exp = np.concatenate([np.setdiff1d(r, [4, 6, 8]), [6]])
    else:
        raise ValueError(name)
    return dict(boxes=boxes, sims=sims.astype(f32), conf=conf, thr=0.5, patch=np.asarray(exp, np.int64))


BOX_PROFILES = ("zero_area", "duplicates", "inverted", "negative", "pixel", "exact_half", "exact_half_below")


def box_profile(name):
    """-> dict(boxes, sims, conf, thr, patch = expected kept patches in order per route, or None where only the float64 reference speaks;
    decided = whether 0 undecided pairs is claimed)."""
    P = 12
    score = (f32(0.9) - np.arange(P).astype(f32) * f32(0.01)).astype(f32)
    sims = np.full((P, 2), f32(-1), f32)
    sims[:, 1] = score                          # one class, patch order = score order
    boxes = np.stack([np.arange(P) * 3.0, np.zeros(P), np.arange(P) * 3.0 + 1.0, np.ones(P)], -1).astype(f32)      # disjoint unit boxes
    thr, exp, decided = 0.5, np.arange(P), True
    if name == "zero_area":                     # IoU 0 / x or 0 / 0 (NaN): suppresses nothing and is never suppressed
        boxes[1] = (0.5, 0.5, 0.5, 0.9); boxes[2] = (0.5, 0.5, 0.5, 0.9)          # zero width, inside box 0, twice
        boxes[3] = (0.25, 0.25, 0.25, 0.25); boxes[4] = (0.25, 0.25, 0.25, 0.25)  # points
    elif name == "duplicates":                  # IoU exactly 1: the first of each run stays
        boxes[1] = boxes[0]; boxes[2] = boxes[0]; boxes[7] = boxes[5]
        exp = np.setdiff1d(exp, [1, 2, 7])
    elif name == "inverted":                    # x2 < x1: a negative side clamps the intersection to 0; two doubly-inverted twins have area > 0, inter 0
        boxes[1] = (1.0, 0.0, 0.0, 1.0); boxes[2] = (1.0, 1.0, 0.0, 0.0); boxes[3] = (1.0, 1.0, 0.0, 0.0)
        # every intersection with or between them clamps to exactly 0 (the twins: w = min(0, 0) - max(1, 1) = -1), so IoU is 0 / 2: all 12 stay
    elif name == "negative":                    # every coordinate negative: the shifted route's max + 1 with max < 0
        boxes = (boxes - f32(100.0)).astype(f32)
        boxes[1] = boxes[0] + f32(0.25) * np.asarray([1, 0, 1, 0], f32)           # IoU 0.6 with box 0
        sims[:, 0], sims[:, 1] = score, -1
        sims[6:, 0], sims[6:, 1] = -1, score[6:]                                   # two classes
        exp = np.setdiff1d(exp, [1])
    elif name == "pixel":                       # pixel scale
        boxes = (boxes * f32(1.0e4)).astype(f32)
        boxes[1] = boxes[0] + f32(2500.0) * np.asarray([1, 0, 1, 0], f32)
        exp = np.setdiff1d(exp, [1])
    elif name in ("exact_half", "exact_half_below"):       # [0,0,2,2] / [0,0,2,1]: IoU 0.5 in f32 and in f64 -- kept at thr 0.5, gone one ulp below
        boxes[0] = (0, 0, 2, 2); boxes[1] = (0, 0, 2, 1)
        decided = False
        if name == "exact_half_below":
            thr, exp = float(np.nextafter(f32(0.5), f32(0))), np.setdiff1d(exp, [1])
    else:
        raise ValueError(name)
    return dict(boxes=boxes, sims=sims, conf=0.0, thr=thr, patch=None if exp is None else np.asarray(exp, np.int64), decided=decided)


def batch_case(P=200):
    """Four images for one call, n = (0, P, 1, 70); image 1 lives in the unit square, image 3 at coordinates up to 5000: with the other's maximum as the
    coordinate offset's step either list changes (the CPU test shows it).  thr 0.45 / conf CONF."""
    b0, s0 = random_case(P, 6, 40, n=0)
    b1, s1 = random_case(P, 6, 41, n=P)
    b2, s2 = random_case(P, 6, 42, n=1)
    b3, s3 = random_case(P, 6, 43, n=70, cluster=True)
    b3 = (b3 * f32(5000.0)).astype(f32)
    return np.stack([b0, b1, b2, b3]), np.stack([s0, s1, s2, s3])


TEMPLATE_P = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)     # both sides of every sort template and of the scan's word split
TEMPLATE_THR = 0.45
N_VALID = (0, 1, 63, 64, 65, 128, 200)                                               # at P = 200
SCAN_P = 8192
SCAN_SCENES = {     # name: (pairs, chains) of sorted positions on the P = n = 8192 lattice; a position appears once per scene
    "edges_a": (((0, 8191), (63, 64), (4095, 4096)), ()),
    "edges_b": (((4096, 4097), (4031, 8191)), ()),
    "chains": ((), ((4095, 4096, 4160), (4100, 4101, 8190))),       # across the word split, and its mirror entirely above it
}
BASIC = ("per_class", "coordinate_offset")


def template_case(P, half, routes=BASIC):
    return cached_reference("random", P, 3, 1000 + P, (P + 1) // 2 if half else P, TEMPLATE_THR, tuple(routes))


@functools.lru_cache(maxsize=None)
def cached_reference(kind, *args):
    """The named case and its reference, made once per process: (inputs dict, {route: Result})."""
    if kind == "random":
        P, C, seed, n, thr, routes = args
        boxes, sims = random_case(P, C, seed, n=n)
        case = dict(boxes=boxes, sims=sims, conf=CONF, thr=thr)
    elif kind == "lattice":
        P, pairs, chains, routes = args
        case = lattice_case(P, 3, pairs, chains)
    elif kind == "far":
        n, seed, routes = args
        boxes, sims = far_case(n, seed)
        case = dict(boxes=boxes, sims=sims, conf=CONF, thr=FAR_THR)
    else:
        raise ValueError(kind)
    return case, {r: reference(case["boxes"], case["sims"], case["conf"], case["thr"], r) for r in routes}
