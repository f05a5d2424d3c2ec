"""Float64 reference, derived decision margin and named cases for the merge of sliced inference, csrc/slice_merge.hip: sm_sort_kernel, sm_mask_kernel and
sm_scan_kernel behind owl_slice_merge.  Checker side, CPU only: nothing here imports the package.  The IoU half, the rounding model and the greedy loop are
those of tests/postprocess_reference.py, imported and not edited.

Reference, stage by stage (`reference(case, metric)` -> one `Merged` per source image)
---------
`live(case, g)`          candidate c = local_slice * K + rank of source image g (slices slice_offsets[g] .. slice_offsets[g + 1]) is live iff
                         rank < counts[slice] and its score is not NaN.  Live candidates are ordered by score descending, then c ascending, with -0.0 == +0.0.
`map_boxes(b, xform)`    x = f32(ox + f32(bx * sx)), y = f32(oy + f32(by * sy)) for both corners, xform row (sx, ox, sy, oy) of the candidate's slice: the f32
                         multiply and the f32 add the device performs (-ffp-contract=off).  This is INPUT rounding -- part of the contract, as the
                         coordinate-offset route's shift is -- so it is done in numpy f32 and the overlap below starts from its result.  No clipping.
`merge_nms(boxes, group, thr, metric)`   greedy suppression over the sorted list: j goes iff a kept i < j of the same group has ovr(i, j) > float32(thr), with
                         "iou"  ovr = inter / (area_i + area_j - inter)       (postprocess_reference.exact_nms itself)
                         "ios"  ovr = inter / min(area_i, area_j)             (intersection over the smaller area)
                         evaluated in float64 on the f32 mapped coordinates.

Decision margin of IoS (per pair, derived like `pair_iou`'s: one rounding per written operation, f = 2^-24, d = 2^-149)
---------------
    sides, inter, area_i, area_j     exactly as in pair_iou (a clamped side is exactly 0; a product with an exactly-zero factor is exactly 0)
    den = fminf(area_i, area_j)      a selection, no rounding: |min(a, b) - min(a', b')| <= max(|a - a'|, |b - b'|), so e_den = max(e_ai, e_aj)
    quotient                         correctly rounded: e = (e_inter + |ios| e_den) / |den| + f |ios| + d; 0 / x with an exactly-zero numerator is exactly
                                     0 (or -0), and 0 / 0 is NaN: neither exceeds a threshold >= 0
A pair is UNDECIDED when |ovr64 - float32(thr)| <= e (or the bound cannot be formed).  With 0 undecided pairs every correct f32 evaluation of the formula
takes the float64 decision at every pair and must return exactly the reference's list.

Planted errors (`reference(case, metric, plant=...)`): "iou_for_ios" the other metric | "class_agnostic" classes ignored | "no_offset" ox = oy = 0 |
"xform0" row 0 of xform for every slice | "swap_sxsy" sx and sy exchanged | "tie_last" score ties broken by the LAST index | "add_first" f32(f32(ox + bx) * sx).
tests/test_slice_merge_reference.py shows that each changes the list of the case named in `PLANTS`.

Cases (`case(name)`, names in `CASES`): every one has 0 undecided pairs under both metrics (asserted by the CPU test).  Slots past a slice's count hold a box
(0, 0, 1, 1) of class 0 with score 2.0: read by mistake they would head every list.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests.postprocess_reference import DEN, F, _rnd, exact_nms, lattice_case, pair_iou, random_case

f32 = np.float32
METRICS = ("iou", "ios")
Merged = namedtuple("Merged", "boxes classes scores src n undecided")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the map, the order, the overlap
# ---------------------------------------------------------------------------------------------------------------------------------------------
def map_boxes(b, xf, plant=None):
    """b [n, 4] f32 slice-local boxes, xf [n, 4] f32 rows (sx, ox, sy, oy) -> [n, 4] f32 in the source image."""
    b, xf = np.asarray(b, f32), np.asarray(xf, f32)
    sx, ox, sy, oy = xf[:, 0:1], xf[:, 1:2], xf[:, 2:3], xf[:, 3:4]
    if plant == "swap_sxsy":
        sx, sy = sy, sx
    if plant == "no_offset":
        ox, oy = np.zeros_like(ox), np.zeros_like(oy)
    xs, ys = b[:, 0::2], b[:, 1::2]
    if plant == "add_first":
        mx, my = ((ox + xs).astype(f32) * sx).astype(f32), ((oy + ys).astype(f32) * sy).astype(f32)
    else:
        mx, my = (ox + (xs * sx).astype(f32)).astype(f32), (oy + (ys * sy).astype(f32)).astype(f32)
    out = np.empty_like(b)
    out[:, 0::2], out[:, 1::2] = mx, my
    return out


def live(case, g, plant=None):
    """-> (c [n] i64 in sorted order, flat input index [n]) of source image g."""
    K = case["K"]
    s0, s1 = int(case["slice_offsets"][g]), int(case["slice_offsets"][g + 1])
    c = np.arange((s1 - s0) * K, dtype=np.int64)
    sl, rank = s0 + c // K, c % K
    score = np.asarray(case["scores"], f32)[sl, rank] if c.size else np.zeros(0, f32)
    ok = (rank < np.asarray(case["counts"])[sl]) & ~np.isnan(score) if c.size else np.zeros(0, bool)
    c, score = c[ok], score[ok]
    key = -(score.astype(np.float64) + 0.0)                               # -0.0 + 0.0 = +0.0: one key for both zeros
    order = np.lexsort((-c if plant == "tie_last" else c, key))
    c = c[order]
    return c, (s0 + c // K) * K + c % K


def pair_ios(bi, bj):
    """bi [4], bj [m, 4] float64 views of f32 coordinates -> (ios64 [m], e [m], sure_zero [m]); see the module docstring."""
    dxi, dyi = bi[2] - bi[0], bi[3] - bi[1]
    dxj, dyj = bj[:, 2] - bj[:, 0], bj[:, 3] - bj[:, 1]
    ai, aj = dxi * dyi, dxj * dyj
    e_ai = _rnd(ai, np.abs(dxi) * F * np.abs(dyi) + np.abs(dyi) * F * np.abs(dxi))
    e_aj = _rnd(aj, np.abs(dxj) * F * np.abs(dyj) + np.abs(dyj) * F * np.abs(dxj))
    wv = np.minimum(bi[2], bj[:, 2]) - np.maximum(bi[0], bj[:, 0])
    hv = np.minimum(bi[3], bj[:, 3]) - np.maximum(bi[1], bj[:, 1])
    w, h = np.maximum(wv, 0.0), np.maximum(hv, 0.0)
    e_w, e_h = F * w, F * h
    inter = w * h
    e_in = _rnd(inter, w * e_h + h * e_w)
    sure_zero = (inter == 0) & (e_in == 0)
    den = np.minimum(ai, aj)
    e_den = np.maximum(e_ai, e_aj)
    with np.errstate(divide="ignore", invalid="ignore"):
        ios = inter / den
        e = _rnd(ios, (e_in + np.abs(ios) * e_den) / np.abs(den))
    return ios, e, sure_zero


def merge_nms(boxes, group, thr, metric):
    """boxes [n, 4] f32 IN SORTED ORDER, group [n] ints or None -> (kept positions i64, undecided pair count).  "iou" IS postprocess_reference.exact_nms;
    "ios" is the same loop over pair_ios."""
    if metric == "iou":
        return exact_nms(boxes, group, thr)
    assert metric == "ios", metric
    b = np.asarray(boxes, f32).astype(np.float64)
    n = b.shape[0]
    t = float(f32(thr))
    g = None if group is None else np.asarray(group)
    suppressed = np.zeros(n, bool)
    keep, undecided = [], 0
    for i in range(n):
        if i + 1 < n:
            js = np.arange(i + 1, n) if g is None else i + 1 + np.nonzero(g[i + 1:] == g[i])[0]
            if t >= 0 and js.size:                                        # an exactly empty intersection is decided at once (thr >= 0)
                bj = b[js]
                meet = (np.minimum(b[i, 2], bj[:, 2]) > np.maximum(b[i, 0], bj[:, 0])) & (np.minimum(b[i, 3], bj[:, 3]) > np.maximum(b[i, 1], bj[:, 1]))
                js = js[meet]
            if js.size:
                ovr, e, sure_zero = pair_ios(b[i], b[js])
                hit = ovr > t
                und = ~(np.abs(ovr - t) > e)
                if t >= 0:
                    und &= ~sure_zero
                undecided += int(und.sum())
                if not suppressed[i]:
                    suppressed[js[hit]] = True
        if not suppressed[i]:
            keep.append(i)
    return np.asarray(keep, np.int64), undecided


def reference(case, metric, plant=None, class_aware=None, max_out=None):
    """-> [Merged(boxes f32 [k, 4] in the source image, classes i64, scores f32 with the input's bits, src i64 = c, n live, undecided pairs)] per source image."""
    aware = case.get("class_aware", True) if class_aware is None else class_aware
    if plant == "class_agnostic":
        aware = False
    if plant == "iou_for_ios":
        metric = "iou" if metric == "ios" else "ios"
    max_out = case.get("max_out") if max_out is None else max_out
    K = case["K"]
    fb = np.asarray(case["boxes"], f32).reshape(-1, 4)
    fs = np.asarray(case["scores"], f32).reshape(-1)
    fc = np.asarray(case["classes"], np.int64).reshape(-1)
    xf = np.asarray(case["xform"], f32)
    out = []
    for g in range(len(case["slice_offsets"]) - 1):
        c, flat = live(case, g, plant)
        rows = xf[np.zeros_like(flat) if plant == "xform0" else flat // K]
        mapped = map_boxes(fb[flat], rows, plant) if c.size else np.zeros((0, 4), f32)
        keep, und = merge_nms(mapped, fc[flat] if aware else None, case["thr"], metric) if c.size else (np.zeros(0, np.int64), 0)
        if max_out is not None:
            keep = keep[:max_out]
        out.append(Merged(mapped[keep], fc[flat][keep], fs[flat][keep], c[keep], len(c), und))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pack(per_slice, xform, slice_offsets, thr, K=None, **extra):
    """per_slice: [(boxes [n, 4], scores [n], classes [n])] -> the padded arrays of one owl_slice_merge call; the slots past a count are poisoned."""
    T = len(per_slice)
    K = max([len(s[1]) for s in per_slice] + [1]) if K is None else K
    boxes = np.tile(np.asarray([0, 0, 1, 1], f32), (T, K, 1))
    scores = np.full((T, K), f32(2.0), f32)
    classes = np.zeros((T, K), np.int64)
    counts = np.zeros(T, np.int32)
    for t, (b, s, c) in enumerate(per_slice):
        n = len(s)
        counts[t] = n
        boxes[t, :n], scores[t, :n], classes[t, :n] = np.asarray(b, f32).reshape(n, 4), np.asarray(s, f32), np.asarray(c, np.int64)
    xform = np.ascontiguousarray(xform, f32).reshape(T, 4)
    return dict(boxes=boxes, scores=scores, classes=classes, counts=counts, xform=xform, slice_offsets=np.asarray(slice_offsets, np.int32), K=K, thr=thr, **extra)


def plan_xform(H, W, s, overlap, full_image=True):
    """The xform rows of the issue's grid rule, restated: windows (p, p + s) every s - int(s * overlap), the last flush with the axis; + the whole image."""
    def starts(n):
        if n <= s:
            return [(0, n)]
        step, out, p = s - int(s * overlap), [], 0
        while p + s < n:
            out.append((p, p + s))
            p += step
        return out + [(n - s, n)]
    boxes = [(l, u, r, lo) for (u, lo) in starts(H) for (l, r) in starts(W)]
    if full_image and len(boxes) > 1:
        boxes.append((0, 0, W, H))
    return np.asarray([((r - l) / W, l / W, (lo - u) / H, u / H) for (l, u, r, lo) in boxes], np.float64).astype(f32)


def rand_xform(S, seed):
    rng = np.random.default_rng(seed)
    xf = np.empty((S, 4), f32)
    xf[:, 0::2] = (rng.random((S, 2)) * 0.4 + 0.2).astype(f32)
    xf[:, 1::2] = (rng.random((S, 2)) * 0.4).astype(f32)
    return xf


def to_local(full, xf):
    """Full-image boxes [n, 4] -> slice-local f32 boxes under rows xf [n, 4]: (v - o) / s in f32 (any f32 value will do: the map's own result is the input)."""
    full, xf = np.asarray(full, f32), np.asarray(xf, f32)
    out = np.empty_like(full)
    out[:, 0::2] = ((full[:, 0::2] - xf[:, 1:2]) / xf[:, 0:1]).astype(f32)
    out[:, 1::2] = ((full[:, 1::2] - xf[:, 3:4]) / xf[:, 2:3]).astype(f32)
    return out


def spread(full, scores, classes, xform, K=None, assign=None):
    """n candidates in full-image coordinates dealt to the S slices of `xform` (candidate i -> slice assign[i], default i % S) -> per_slice list."""
    S = len(xform)
    n = len(scores)
    assign = np.arange(n) % S if assign is None else np.asarray(assign)
    per = []
    for t in range(S):
        m = np.flatnonzero(assign == t)
        per.append((to_local(full[m], np.tile(xform[t], (len(m), 1))), np.asarray(scores)[m], np.asarray(classes)[m]))
    return per


def random_candidates(n, C, seed, cluster):
    boxes, sims = random_case(n, C, seed, cluster=cluster)
    return boxes, sims.max(1), sims.argmax(1)


def lattice():
    """Image 128 x 128, windows of 64 without overlap + the whole image: sx in {0.5, 1}, ox in {0, 0.5}; every coordinate dyadic, every map exact.  thr 0.5.
    slice 4 (whole image): A = (0.25, 0.25, 0.75, 0.75) class 1 score 0.9; U = (20.75, 20.5, 21.75, 21.5) class 2 score 0.8; V = U's twin of class 0, 0.55
    slice 0 (ox = oy = 0): a = local (0.5, 0.5, 0.75, 0.75) -> (0.25, 0.25, 0.375, 0.375) class 1 score 0.7: wholly inside A, IoS 1, IoU 1 / 16
                           b = the same box, class 2, score 0.6: another class, stays under either metric (class-aware)
    slice 3 (ox = oy = 0.5): u = local (40, 40, 42, 42) -> (20.5, 20.5, 21.5, 21.5) class 2 score 0.5: a unit box a quarter from U, IoU 0.6, IoS 0.75
    slices 1, 2: one far box each."""
    xf = plan_xform(128, 128, 64, 0.0)
    assert xf.tolist() == [[0.5, 0, 0.5, 0], [0.5, 0.5, 0.5, 0], [0.5, 0, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5], [1, 0, 1, 0]]
    per = [([(0.5, 0.5, 0.75, 0.75), (0.5, 0.5, 0.75, 0.75)], [0.7, 0.6], [1, 2]),
           ([(8, 8, 9, 9)], [0.3], [1]),
           ([(8, 8, 9, 9)], [0.2], [1]),
           ([(40, 40, 42, 42)], [0.5], [2]),
           ([(0.25, 0.25, 0.75, 0.75), (20.75, 20.5, 21.75, 21.5), (20.75, 20.5, 21.75, 21.5)], [0.9, 0.8, 0.55], [1, 2, 0])]
    case = pack(per, xf, [0, 5], 0.5)
    K = case["K"]                                # 3: c = slice * 3 + rank
    A, U, V, a, b, u, f1, f2 = 4 * K, 4 * K + 1, 4 * K + 2, 0, 1, 3 * K, K, 2 * K
    case["expect"] = {"iou": [A, U, a, b, V, f1, f2], "ios": [A, U, b, V, f1, f2], "iou_agnostic": [A, U, a, f1, f2], "ios_agnostic": [A, U, f1, f2]}
    return case


def _random(S, K, seed, cluster, thr=0.45, xform=None, n=None, C=3, **extra):
    xform = rand_xform(S, seed + 7) if xform is None else xform
    n = S * K if n is None else n
    full, score, cls = random_candidates(n, C, seed, cluster)
    return pack(spread(full, score, cls, xform), xform, [0, S], thr, K=K, **extra)


def ties():
    """Four score levels over 120 clustered candidates in 6 slices: inside a level the order is by c, and which of two overlapping equals stays depends on it."""
    xf = rand_xform(6, 5)
    full, score, cls = random_candidates(120, 2, 77, True)
    score = (f32(0.25) * (1 + (np.arange(120) * 7) % 4)).astype(f32)
    return pack(spread(full, score, cls, xf), xf, [0, 6], 0.45)


def empties(which):
    xf = rand_xform(4, 9)
    full, score, cls = random_candidates(40, 3, 81, True)
    per = spread(full, score, cls, xf)
    if which == "one":
        per[2] = (np.zeros((0, 4), f32), np.zeros(0, f32), np.zeros(0, np.int64))
        return pack(per, xf, [0, 4], 0.45)
    return pack([(np.zeros((0, 4), f32), np.zeros(0, f32), np.zeros(0, np.int64))] * 4, xf, [0, 4], 0.45, K=5)


def k_one():
    xf = plan_xform(200, 300, 96, 0.2)
    full, score, cls = random_candidates(13, 2, 91, True)
    return pack(spread(full, score, cls, xf), xf, [0, 13], 0.45, K=1)


def nan_and_zeros():
    """A NaN score (dropped) and NaN with the sign bit; then -0.0 / +0.0 scores (what a negative confidence threshold upstream lets through): equal in the order,
    so c decides, and the emitted scores keep their sign bits."""
    xf = rand_xform(3, 13)
    full, score, cls = random_candidates(30, 2, 93, True)
    score = score.copy()
    score[4], score[11] = np.nan, -np.nan
    score[5:11] = np.asarray([-0.0, 0.0, -0.0, 0.0, 0.0, -0.0], f32)
    score[20:24] = np.asarray([-0.5, -0.0, -1.0, 0.0], f32)
    for i in (5, 6, 7, 8, 9, 10, 21, 23):                                 # the zeros stand apart from everything: all eight are kept, whatever their order
        full[i] = (3 + i, 3, 3.5 + i, 3.5)
    return pack(spread(full, score, cls, xf), xf, [0, 3], 0.45)


def ragged():
    """Two source images in one call: 1 slice and 6 slices (5 windows + the whole image)."""
    xf = np.concatenate([plan_xform(96, 96, 96, 0.2), plan_xform(96, 330, 96, 0.2)])
    assert len(xf) == 7
    f0, s0, c0 = random_candidates(50, 3, 101, True)
    f1, s1, c1 = random_candidates(180, 3, 102, True)
    per = spread(f0, s0, c0, xf[:1]) + spread(f1, s1, c1, xf[1:])
    return pack(per, xf, [0, 1, 7], 0.45)


SCAN_N = 8192
SCAN_PAIRS = ((0, 8191), (63, 64), (4095, 4096))


def scan_edges():
    """N = 8192 live candidates (64 slices x 128) on postprocess_reference.lattice_case: suppressing pairs at sorted positions (0, 8191), (63, 64) and
    (4095, 4096); dyadic xforms (sx in {0.5, 1}, ox in {0, 0.5})."""
    lat = lattice_case(SCAN_N, 3, SCAN_PAIRS)
    S, K = 64, 128
    xf = np.asarray([((0.5, 0.5 * (t & 1), 0.5, 0.5 * ((t >> 1) & 1)) if t % 3 else (1, 0, 1, 0)) for t in range(S)], f32)
    score, cls = lat["sims"].max(1), lat["sims"].argmax(1)
    case = pack(spread(lat["boxes"], score, cls, xf, assign=np.arange(SCAN_N) // K), xf, [0, S], 0.5, K=K)
    case["expect_src"] = lat["perm"][lat["kept"]]                   # candidate c = patch index: slice c // K, rank c % K
    return case


_SIZES = {63: (3, 21), 64: (2, 32), 65: (5, 13), 1023: (3, 341), 1024: (4, 256), 1025: (5, 205), 4095: (13, 315), 4096: (16, 256), 4097: (17, 241)}

_BUILDERS = {
    "lattice": lattice,
    "cluster_1": lambda: _random(1, 150, 201, True, xform=plan_xform(96, 96, 96, 0.2)),
    "cluster_2": lambda: _random(2, 100, 202, True, xform=plan_xform(96, 160, 96, 0.25, full_image=False)),
    "cluster_13": lambda: _random(13, 20, 203, True, xform=plan_xform(200, 300, 96, 0.2)),
    "agnostic": lambda: _random(13, 20, 203, True, xform=plan_xform(200, 300, 96, 0.2), class_aware=False),
    "ties": ties,
    "empty_slice": lambda: empties("one"),
    "all_empty": lambda: empties("all"),
    "k_one": k_one,
    "nan_zeros": nan_and_zeros,
    "ragged": ragged,
    "max_out": lambda: _random(6, 30, 204, True, max_out=9),
    "scan_edges": scan_edges,
}
for _n, (_s, _k) in _SIZES.items():
    _BUILDERS[f"n_{_n}"] = functools.partial(_random, _s, _k, 300 + _n, False)
CASES = tuple(_BUILDERS)

# planted error -> (case, metric) whose list it changes
PLANTS = {"iou_for_ios": ("lattice", "ios"), "class_agnostic": ("lattice", "ios"), "no_offset": ("cluster_13", "ios"), "xform0": ("cluster_13", "ios"),
          "swap_sxsy": ("cluster_13", "iou"), "tie_last": ("ties", "ios"), "add_first": ("cluster_13", "ios")}


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def cached_reference(name, metric, plant=None):
    """The named case's reference, made once per process and never modified."""
    return reference(case(name), metric, plant)


def n_max(c):
    return int(np.diff(c["slice_offsets"]).max()) * c["K"]
