"""Plain numpy f64 restatement of the COCO bbox evaluation protocol (pycocotools `COCOeval`: evaluateImg -> accumulate -> summarize), the
contract `metrics.MeanAveragePrecision` is held to.  Test infrastructure only: written as the loops of the protocol, slow on purpose, never
imported by the package.

An "image" is a dict: det_boxes [n,4] f32 pixel xyxy, det_scores [n] f32, det_labels [n] int, gt_boxes [g,4] f32 pixel xyxy, gt_labels [g] int.

`accumulate_records` is `accumulate` from the records on (hand-built records need no boxes).  `match_cases()` / `accumulate_cases()` are the named edge
cases of tests/test_metrics_edges_gpu.py, aimed at the forms of csrc/metrics.hip (line numbers in `aims` are that file's); tests/test_metrics.py
shows that every planted protocol mistake changes an output of one of them, profiles/eval_map_edges.md has the table.
"""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RNG = np.array([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]], dtype=np.float64)
MAX_DETS = np.array([1, 10, 100], dtype=np.int32)
EPS = float(np.spacing(1))
T, R, A, M = 10, 101, 4, 3


def _xywh64(boxes_xyxy_f32):
    """pixel xyxy f32 -> xywh: the subtraction in f32, everything afterwards in f64"""
    b = np.asarray(boxes_xyxy_f32, dtype=np.float32).reshape(-1, 4)
    w = (b[:, 2] - b[:, 0]).astype(np.float32)
    h = (b[:, 3] - b[:, 1]).astype(np.float32)
    return np.stack([b[:, 0], b[:, 1], w, h], axis=1).astype(np.float64)


def _iou(d, g):
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    i = iw * ih
    return i / (d[2] * d[3] + g[2] * g[3] - i)


def match_image(img, n_classes):
    """-> per detection (in the order given): label (-1: not a record), rank, matched [n,A,T] bool, ignored [n,A,T] bool; and npig [C,A]."""
    scores = np.asarray(img["det_scores"], dtype=np.float32).reshape(-1)
    dlab = np.asarray(img["det_labels"], dtype=np.int64).reshape(-1)
    glab = np.asarray(img["gt_labels"], dtype=np.int64).reshape(-1)
    dbox = _xywh64(img["det_boxes"])
    gbox = _xywh64(img["gt_boxes"])
    n = len(scores)
    label = np.full(n, -1, dtype=np.int64)
    rank = np.zeros(n, dtype=np.int32)
    matched = np.zeros((n, A, T), dtype=bool)
    ignored = np.zeros((n, A, T), dtype=bool)
    npig = np.zeros((n_classes, A), dtype=np.int32)
    for c in range(n_classes):
        didx = np.nonzero(dlab == c)[0]
        didx = didx[np.argsort(-scores[didx].astype(np.float64), kind="stable")][:int(MAX_DETS[-1])]
        gidx = np.nonzero(glab == c)[0]
        for r, d in enumerate(didx):
            label[d] = c
            rank[d] = r
        for a in range(A):
            lo, hi = AREA_RNG[a]
            g_ig = np.array([bool(gbox[g, 2] * gbox[g, 3] < lo or gbox[g, 2] * gbox[g, 3] > hi) for g in gidx], dtype=bool)
            order = np.argsort(g_ig, kind="stable")
            gs = gidx[order]
            gs_ig = g_ig[order]
            npig[c, a] = int((~g_ig).sum())
            for t in range(T):
                taken = np.zeros(len(gs), dtype=bool)
                for d in didx:
                    best = min(IOU_THRS[t], 1 - 1e-10)
                    m = -1
                    for p, g in enumerate(gs):
                        if taken[p]:
                            continue
                        if m > -1 and not gs_ig[m] and gs_ig[p]:
                            break
                        iou = _iou(dbox[d], gbox[g])
                        if iou < best:
                            continue
                        best = iou
                        m = p
                    if m > -1:
                        taken[m] = True
                        matched[d, a, t] = True
                        ignored[d, a, t] = gs_ig[m]
                    else:
                        area = dbox[d, 2] * dbox[d, 3]
                        ignored[d, a, t] = bool(area < lo or area > hi)
    return label, rank, matched, ignored, npig


def accumulate(images, n_classes):
    """-> precision [T,R,C,A,M], recall [T,C,A,M] (f64, -1 where there is no non-ignored ground truth), over the images in the order given"""
    recs = [match_image(img, n_classes) for img in images]
    if not recs:
        return -np.ones((T, R, n_classes, A, M)), -np.ones((T, n_classes, A, M))
    score = np.concatenate([np.asarray(img["det_scores"], dtype=np.float32).reshape(-1) for img in images])
    return accumulate_records(np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs]), score, np.concatenate([r[2] for r in recs]),
                              np.concatenate([r[3] for r in recs]), np.sum([r[4] for r in recs], axis=0), n_classes)


def accumulate_records(label, rank, score, matched, ignored, npig, n_classes):
    """The records of match_image, concatenated over the images in the order given (label [N], -1: not a record; rank [N]; score [N];
    matched / ignored [N,A,T] bool), and npig [C,A] summed over the images -> precision [T,R,C,A,M], recall [T,C,A,M] as `accumulate`."""
    label, rank = np.asarray(label, dtype=np.int64).reshape(-1), np.asarray(rank, dtype=np.int32).reshape(-1)
    score = np.asarray(score, dtype=np.float32).reshape(-1).astype(np.float64)
    matched, ignored = np.asarray(matched, dtype=bool).reshape(-1, A, T), np.asarray(ignored, dtype=bool).reshape(-1, A, T)
    npig_all = np.asarray(npig).reshape(n_classes, A)
    precision = -np.ones((T, R, n_classes, A, M))
    recall = -np.ones((T, n_classes, A, M))
    for k in range(n_classes):
        for a in range(A):
            npig = int(npig_all[k, a])
            if npig == 0:
                continue
            for mi, md in enumerate(MAX_DETS):
                sel = np.nonzero((label == k) & (rank < md))[0]
                sel = sel[np.argsort(-score[sel], kind="stable")]
                for t in range(T):
                    mt, ig = matched[sel, a, t], ignored[sel, a, t]
                    tp = np.cumsum(mt & ~ig).astype(np.float64)
                    fp = np.cumsum(~mt & ~ig).astype(np.float64)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + EPS)
                    recall[t, k, a, mi] = rc[-1] if nd else 0.0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, REC_THRS, side="left")
                    for r, pi in enumerate(inds):
                        precision[t, r, k, a, mi] = pr[pi] if pi < nd else 0.0
    return precision, recall


def _mean(x):
    x = np.asarray(x, dtype=np.float64)
    x = x[x > -1]
    return float(x.mean()) if x.size else -1.0


def summarize(precision, recall):
    n_classes = precision.shape[2]
    out = {
        "map": _mean(precision[:, :, :, 0, 2]),
        "map_50": _mean(precision[0, :, :, 0, 2]),
        "map_75": _mean(precision[5, :, :, 0, 2]),
        "map_small": _mean(precision[:, :, :, 1, 2]),
        "map_medium": _mean(precision[:, :, :, 2, 2]),
        "map_large": _mean(precision[:, :, :, 3, 2]),
        "mar_1": _mean(recall[:, :, 0, 0]),
        "mar_10": _mean(recall[:, :, 0, 1]),
        "mar_100": _mean(recall[:, :, 0, 2]),
        "mar_small": _mean(recall[:, :, 1, 2]),
        "mar_medium": _mean(recall[:, :, 2, 2]),
        "mar_large": _mean(recall[:, :, 3, 2]),
        "map_per_class": np.array([_mean(precision[:, :, k, 0, 2]) for k in range(n_classes)]),
        "mar_100_per_class": np.array([_mean(recall[:, k, 0, 2]) for k in range(n_classes)]),
        "classes": np.arange(n_classes, dtype=np.int32),
    }
    return out


def evaluate(images, n_classes=None):
    if n_classes is None:
        n_classes = 1 + max([-1] + [int(np.max(img[k])) for img in images for k in ("det_labels", "gt_labels") if len(img[k])])
    precision, recall = accumulate(images, n_classes)
    return summarize(precision, recall)


def image(det_boxes=(), det_scores=(), det_labels=(), gt_boxes=(), gt_labels=()):
    return dict(det_boxes=np.asarray(det_boxes, dtype=np.float32).reshape(-1, 4), det_scores=np.asarray(det_scores, dtype=np.float32).reshape(-1),
                det_labels=np.asarray(det_labels, dtype=np.int64).reshape(-1), gt_boxes=np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4),
                gt_labels=np.asarray(gt_labels, dtype=np.int64).reshape(-1))


def random_eval_set(seed, n_images=40, n_classes=10, n_det=200, tie_scores=False):
    """Seeded eval-like set: 1-16 ground truths per image of size 200-640, detections jittered around them (plus strays), so that all three
    size ranges occur and nothing is degenerate."""
    rng = np.random.RandomState(seed)
    images = []
    for _ in range(n_images):
        W, H = rng.randint(200, 641, size=2)
        g = rng.randint(1, 17)
        side = np.exp(rng.uniform(np.log(8.0), np.log(300.0), size=(g, 2)))
        cx, cy = rng.uniform(0, W, size=g), rng.uniform(0, H, size=g)
        gt = np.stack([np.clip(cx - side[:, 0] / 2, 0, W - 2), np.clip(cy - side[:, 1] / 2, 0, H - 2), np.clip(cx + side[:, 0] / 2, 0, W), np.clip(cy + side[:, 1] / 2, 0, H)], 1)
        gt[:, 2] = np.maximum(gt[:, 2], gt[:, 0] + 1.0)
        gt[:, 3] = np.maximum(gt[:, 3], gt[:, 1] + 1.0)
        gl = rng.randint(0, n_classes, size=g)
        src = rng.randint(0, g, size=n_det)
        wh = np.stack([gt[src, 2] - gt[src, 0], gt[src, 3] - gt[src, 1]], 1)
        jit = rng.normal(0, 0.12, size=(n_det, 4)) * np.concatenate([wh, wh], 1)
        det = gt[src] + jit
        stray = rng.uniform(size=n_det) < 0.3
        det[stray] = np.stack([rng.uniform(0, W / 2, stray.sum()), rng.uniform(0, H / 2, stray.sum()), rng.uniform(W / 2, W, stray.sum()), rng.uniform(H / 2, H, stray.sum())], 1)
        det[:, 2] = np.maximum(det[:, 2], det[:, 0] + 1.0)
        det[:, 3] = np.maximum(det[:, 3], det[:, 1] + 1.0)
        dl = np.where(rng.uniform(size=n_det) < 0.6, gl[src], rng.randint(0, n_classes, size=n_det))
        sc = rng.uniform(0.01, 1.0, size=n_det)
        if tie_scores:
            sc = np.round(sc * 8) / 8
        images.append(image(det, sc, dl, gt, gl))
    return images


# ---- named edge cases (tests/test_metrics_edges_gpu.py runs them on the device, tests/test_metrics.py shows that each planted mistake changes one) ----
# A match case is a dict: images (what the restatement is fed), n_classes, aims (the kernel form it is aimed at), and optionally `batched`, the
# padded arrays MeanAveragePrecision.update_batched is given instead of update(images): boxes [B,K,4], labels [B,K], scores [B,K], counts [B],
# gt_boxes [B,G,4], gt_labels [B,G], gt_counts [B], width / height [B] f32 or None.  Everything is seeded and built from numpy alone.
_GT3 = np.array([[20, 20, 80, 90], [150, 40, 300, 260], [10, 200, 40, 230]], dtype=np.float32)
DET_NS = (1, 63, 64, 65, 99, 100, 101, 129)


def _interleaved_image(rng, n, scores):
    """Class 1 owns n of the 2n + 7 slots, class 0 the others, shuffled: a class-1 lane's position depends on the ballot of the lanes below it.
    scores: "distinct" | "equal" | "straddle" (distinct, but ranks 99 and 100 of class 1 share a score: exactly one of the two is a record)."""
    k = 2 * n + 7
    lab = np.array([1] * n + [0] * (n + 7), dtype=np.int64)
    rng.shuffle(lab)
    det = _GT3[rng.randint(0, 3, size=k)] + rng.normal(0, 6, size=(k, 4)).astype(np.float32)
    det[:, 2:] = np.maximum(det[:, 2:], det[:, :2] + 1)
    sc = np.linspace(0.05, 0.95, k).astype(np.float32)[rng.permutation(k)]
    if scores == "equal":
        sc[:] = 0.5
    if scores == "straddle":
        mine = np.nonzero(lab == 1)[0]
        by_score = mine[np.argsort(-sc[mine].astype(np.float64), kind="stable")]
        sc[by_score[100]] = sc[by_score[99]]
    return image(det, sc, lab, _GT3, [1, 1, 0])


def _gt_image(rng, gt_count, owned, sizes=(20.0, 50.0, 120.0), with_pairs=True):
    """gt_count ground truths of which class 1 owns `owned` (the others are class 0), on a grid of cells 400 px apart.  The q-th ground truth of
    class 1 has side sizes[q % len(sizes)]: with three sizes, ignored and non-ignored alternate with period 3 in every area range, so the pattern
    runs across the 64-lane boundary out of step with it.  Two pairs (40x80 / 40x20 in one cell) have IoU exactly 0.5 with a 40x40 detection:
    which of them the detection takes depends on their order.  Detections sit on the ground truths next to the boundaries, each twice."""
    mine = np.sort(rng.choice(gt_count, size=owned, replace=False))
    gl = np.zeros(gt_count, dtype=np.int64)
    gl[mine] = 1
    cell = np.stack([(np.arange(gt_count) % 16) * 400.0, (np.arange(gt_count) // 16) * 400.0], 1)
    side = np.full(gt_count, 30.0)
    side[mine] = np.asarray(sizes)[np.arange(owned) % len(sizes)]
    gt = np.concatenate([cell, cell + side[:, None]], 1)
    det, sc, dl = [], [], []
    pairs = [(q0, q1, flip) for q0, q1, flip in ((62, 64, False), (0, owned - 1, True), (1, 63, True)) if with_pairs and 0 <= q0 < q1 < owned]
    paired = set()
    for q0, q1, flip in pairs:
        if q0 in paired or q1 in paired:
            continue
        paired.update((q0, q1))
        o = cell[mine[q0]]
        tall, flat = [o[0], o[1], o[0] + 40, o[1] + 80], [o[0], o[1], o[0] + 40, o[1] + 20]
        gt[mine[q0]], gt[mine[q1]] = (flat, tall) if flip else (tall, flat)
        det += [[o[0], o[1], o[0] + 40, o[1] + 40], tall, flat]
        sc += [0.99 - 0.001 * q0, 0.6 - 0.001 * q0, 0.5 - 0.001 * q0]
        dl += [1, 1, 1]
    for q in (0, 1, 62, 63, 64, 65, 127, 128, 254, 255):
        if q < owned and q not in paired:
            b = gt[mine[q]]
            det += [b + np.array([1, 0, 1, 0]), b + np.array([0, 2, 0, 2])]
            sc += [0.9 - 0.002 * q, 0.3 + 0.001 * q]
            dl += [1, 1]
    others = np.nonzero(gl == 0)[0][:2]
    for j in others:
        det.append(gt[j] + np.array([1, 1, 0, 0]))
        sc.append(0.7)
        dl.append(0)
    return image(det, sc, dl, gt, gl)


def _nudge(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def _area_edge_images():
    """Boxes of 32x32, 96x96, 1024x1, 1x1024 and 9216x1 px and their neighbours one f32 step either side (the stepped side starts at x0 = 0 or
    y0 = 0, so the f32 subtraction gives it back exactly).  Image 0: every one as a ground truth with a detection on it (IoU 1); image 1: the same
    detections with no ground truth near them (one far away keeps npig > 0): unmatched, their own area decides `ignored`."""
    boxes = []
    for i, (w, h) in enumerate(((32, 32), (96, 96), (1024, 1), (9216, 1))):
        for step in (None, False, True):
            boxes.append([0.0, 200.0 * len(boxes), w if step is None else _nudge(w, step), 200.0 * len(boxes) + h])
    for step in (None, False, True):
        x = 10000.0 + 8.0 * len(boxes)
        boxes.append([x, 0.0, x + 1.0, 1024.0 if step is None else _nudge(1024.0, step)])
    boxes = np.array(boxes, dtype=np.float32)
    n = len(boxes)
    sc = np.linspace(0.9, 0.2, n)
    far = [[20000, 20000, 20050, 20050]]
    return [image(boxes, sc, [0] * n, boxes, [0] * n), image(boxes, sc, [0] * n, far, [0])]


def _chain_images():
    up = lambda v: _nudge(v, True)
    imgs = {
        # a 40x40 detection has IoU exactly 0.5 with both ground truths: the later one is taken, so the second detection (on the 40x80) finds it taken
        "equal_iou_later_wins": image([[0, 0, 40, 40], [0, 0, 40, 80], [0, 0, 40, 20]], [0.9, 0.8, 0.7], [0] * 3, [[0, 0, 40, 20], [0, 0, 40, 80]], [0, 0]),
        "equal_iou_later_wins_swapped": image([[0, 0, 40, 40], [0, 0, 40, 80], [0, 0, 40, 20]], [0.9, 0.8, 0.7], [0] * 3, [[0, 0, 40, 80], [0, 0, 40, 20]], [0, 0]),
        # small range: the 30x30 ground truth (IoU 0.833) is not ignored, the 40x30 (IoU 0.9) is: up to 0.80 the non-ignored match stands,
        # at 0.85 / 0.90 only the ignored one passes and the detection is ignored, at 0.95 nothing passes and its own area (1080) ignores it
        "ignored_gt_has_higher_iou": image([[0, 0, 36, 30]], [0.9], [0], [[0, 0, 40, 30], [0, 0, 30, 30]], [0, 0]),
        # the same with the non-ignored IoU one f32 step under 0.5: the ignored 30x61 takes the detection at 0.5 already
        "non_ignored_iou_just_under": image([[0, 0, 30, up(60.0)], [100, 0, 130, 60]], [0.9, 0.8], [0, 0], [[0, 0, 30, 61], [0, 0, 30, 30], [100, 0, 130, 61], [100, 0, 130, 30]], [0] * 4),
        # boxes that share an edge (iw == 0), a corner, and zero-width boxes on top of each other (iw == 0 and no area at all)
        "touching": image([[10, 0, 20, 10], [20, 10, 30, 20], [50, 50, 50, 90], [0, 0, 10, 10]], [0.9, 0.8, 0.7, 0.6], [0] * 4, [[0, 0, 10, 10], [10, 10, 20, 20], [50, 50, 50, 90]], [0] * 3),
        "iou_one": image([[3, 5, 43, 75], [100, 100, 300, 250]], [0.9, 0.8], [0, 0], [[3, 5, 43, 75], [100, 100, 300, 250]], [0, 0]),
        # the first detection (IoU 0.6) takes the ground truth up to 0.60 and leaves it free above: the second (IoU 1) is matched from 0.65 on only
        "taken_per_threshold": image([[0, 0, 100, 60], [0, 0, 100, 100], [0, 0, 100, 96]], [0.9, 0.8, 0.7], [0] * 3, [[0, 0, 100, 100]], [0]),
        # x1 < x0 (and y1 < y0): negative width, no overlap with anything, area negative or (both negative) positive
        "negative_width": image([[60, 0, 10, 100], [60, 80, 10, 20], [0, 0, 100, 100], [0, 90, 100, 10]], [0.9, 0.8, 0.7, 0.6], [0] * 4, [[0, 0, 100, 100]], [0]),
    }
    return imgs


def _padding_case():
    """K = 12 detection and G = 6 ground-truth slots; behind the counts: labels that look valid, NaN boxes, NaN scores.  Counts -3 and K + 5 / G + 5
    are clamped; labels -1, C and 2^40 inside the counts are no records."""
    rng = np.random.RandomState(21)
    B, K, G, C = 4, 12, 6, 3
    gt = np.tile(np.array([[10, 10, 60, 60], [100, 20, 180, 140], [30, 150, 50, 170], [200, 200, 330, 330], [5, 5, 25, 30], [90, 90, 140, 150]], dtype=np.float32), (B, 1, 1))
    gl = rng.randint(0, C, size=(B, G)).astype(np.int64)
    boxes = gt[:, rng.randint(0, G, size=K)] + rng.normal(0, 3, size=(B, K, 4)).astype(np.float32)
    boxes[..., 2:] = np.maximum(boxes[..., 2:], boxes[..., :2] + 1)
    labels = rng.randint(0, C, size=(B, K)).astype(np.int64)
    scores = rng.uniform(0.05, 0.95, size=(B, K)).astype(np.float32)
    labels[0, 1], labels[0, 3], labels[0, 4] = -1, C, 2 ** 40
    gl[0, 1], gl[3, 2], gl[3, 4] = -1, C, 2 ** 40
    counts = np.array([7, -3, K + 5, 5], dtype=np.int32)
    gt_counts = np.array([4, 3, -3, G + 5], dtype=np.int32)
    for b in range(B):
        boxes[b, max(counts[b], 0):] = np.nan
        scores[b, max(counts[b], 0):] = np.nan
        gt[b, max(gt_counts[b], 0):] = np.nan
    return dict(boxes=boxes, labels=labels, scores=scores, counts=counts, gt_boxes=gt, gt_labels=gl, gt_counts=gt_counts, width=None, height=None), C


# (size S, a, b, g) f32, 2a <= b <= g: fl(fl(b*S) - fl(a*S)) is exactly half of fl(g*S), but the single-rounding fl(b*S - fl(a*S)) is one step less
_SCALE_HITS = ((333, 0.19827918708324432, 0.6114735007286072, 0.8263887166976929), (375, 0.148982435464859, 0.48004913330078125, 0.6621334552764893),
               (500, 0.15364906191825867, 0.47968193888664246, 0.6520658135414124), (427, 0.20649388432502747, 0.6616021394729614, 0.9102165699005127),
               (500, 0.24831050634384155, 0.516347348690033, 0.5360737442970276), (480, 0.2663053870201111, 0.5571921467781067, 0.581773579120636))


def _scale_case():
    """Normalised boxes scaled in the kernel.  Image i: a ground truth [0, 0, 0.5, g] and a detection [0, a, 0.5, b] whose height, computed as the
    kernel must (two f32 products, then an f32 subtraction), is exactly half the ground truth's: IoU exactly 0.5, matched at the first threshold.
    A fused multiply-subtract gives the height one step less and loses the match.  The x axis uses the same numbers on a second pair."""
    B = len(_SCALE_HITS)
    boxes, gt = np.zeros((B, 4, 4), dtype=np.float32), np.zeros((B, 2, 4), dtype=np.float32)
    for i in range(B):
        (_, xa, xb, xg), (_, ya, yb, yg) = _SCALE_HITS[i], _SCALE_HITS[B - 1 - i]          # width = size i, height = size B - 1 - i
        gt[i] = [[0, 0, 0.5, yg], [0, 0, xg, 0.25]]
        boxes[i] = [[0, ya, 0.5, yb], [xa, 0, xb, 0.25], [0.125, 0.25, 0.5, 0.75], [0.3, 0.3, 0.31, 0.31]]
    size = np.array([s for s, _, _, _ in _SCALE_HITS], dtype=np.float32)
    return dict(boxes=boxes, labels=np.tile(np.array([0, 1, 0, 1], dtype=np.int64), (B, 1)), scores=np.tile(np.array([0.9, 0.8, 0.7, 0.6], dtype=np.float32), (B, 1)),
                counts=None, gt_boxes=gt, gt_labels=np.tile(np.array([0, 1], dtype=np.int64), (B, 1)), gt_counts=None, width=size, height=size[::-1].copy()), 2


def batched_images(bt, fused=False):
    """The images a padded batch stands for: the first clamp(count) slots of each row, boxes scaled by f32 products.  fused=True is the planted
    mistake of a contracted multiply-subtract: each image also carries det_wh / gt_wh = fl(b*s - fl(a*s)) (planted code reads them, match_image does not)."""
    B, K, G = bt["boxes"].shape[0], bt["boxes"].shape[1], bt["gt_boxes"].shape[1]
    out = []
    for b in range(B):
        n = K if bt["counts"] is None else min(max(int(bt["counts"][b]), 0), K)
        g = G if bt["gt_counts"] is None else min(max(int(bt["gt_counts"][b]), 0), G)
        s = np.ones(4, dtype=np.float32) if bt["width"] is None else np.array([bt["width"][b], bt["height"][b]] * 2, dtype=np.float32)
        im = image((bt["boxes"][b, :n] * s).astype(np.float32), bt["scores"][b, :n], bt["labels"][b, :n], (bt["gt_boxes"][b, :g] * s).astype(np.float32), bt["gt_labels"][b, :g])
        if fused:
            for key, raw, px in (("det_wh", bt["boxes"][b, :n], im["det_boxes"]), ("gt_wh", bt["gt_boxes"][b, :g], im["gt_boxes"])):
                im[key] = (raw[:, 2:].astype(np.float64) * s[2:].astype(np.float64) - px[:, :2].astype(np.float64)).astype(np.float32)
        out.append(im)
    return out


_match_cases = None


def match_cases():
    """name -> case, built once"""
    global _match_cases
    if _match_cases is not None:
        return _match_cases
    cases = {}

    def add(name, images, n_classes, aims, batched=None):
        cases[name] = dict(images=images, n_classes=n_classes, aims=aims, batched=batched)

    rng = np.random.RandomState(100)
    add("det_distinct", [_interleaved_image(rng, n, "distinct") for n in DET_NS], 2, "detection compaction (ballot prefix, :63-73), rank loop, cut at 100 (:84-92)")
    add("det_equal", [_interleaved_image(rng, n, "equal") for n in DET_NS], 2, "rank at equal scores = slot order through the compaction; cut at 100 by slot")
    add("det_straddle", [_interleaved_image(rng, n, "straddle") for n in (101, 129)], 2, "tie across rank 99 / 100: one of two equal scores is a record")
    for gc, owned in ((63, 0), (63, 1), (64, 64), (65, 64), (65, 65), (256, 65), (256, 255), (256, 256)):
        add(f"gt_{gc}_own{owned}", [_gt_image(rng, gc, owned)], 2, "ground-truth compaction (:104-114), two-pass order per range (:119-138)" + (", g_ord byte = 255" if owned == 256 else ""))
    add("gt_all_or_none_ignored", [_gt_image(rng, 65, 65, sizes=(50.0,), with_pairs=False), _gt_image(rng, 64, 1, sizes=(50.0,))], 2, "npig == 0 in small / large, nothing ignored in all / medium")
    add("area_edges", _area_edge_images(), 1, "area < lo || area > hi on ground truths (:130) and on unmatched detections (:181), edges belong to both ranges")
    chain_aims = {"equal_iou_later_wins": "`!(iou < best)` moves the match to the later ground truth (:176)", "equal_iou_later_wins_swapped": "the same, ground truths in the other order",
                  "ignored_gt_has_higher_iou": "the chain stops at the first ignored position once a non-ignored match stands (:165)",
                  "non_ignored_iou_just_under": "that stop not taken: the non-ignored IoU is one f32 step under 0.5 (:165,:176)", "touching": "iw > 0 && ih > 0 (:172): 0 / 0 is never formed",
                  "iou_one": "IoU exactly 1 against min(thr, 1 - 1e-10) (:150)", "taken_per_threshold": "one `taken` byte per (position, lane) (:145,:180)",
                  "negative_width": "negative width / height: no overlap, area out of range (:169-172,:181)"}
    for name, im in _chain_images().items():
        add("chain_" + name, [im], 1, chain_aims[name])
    bt, C = _padding_case()
    add("padding", batched_images(bt), C, "nslots / ngslots clamps (:48,:102), the no-record block (:50-58)", bt)
    bt, C = _scale_case()
    add("scale_unfused", batched_images(bt), C, "x1 * sx - x0 * sx as two products and a subtraction (:97-98,:110-111): -ffp-contract=off", bt)
    _match_cases = cases
    return cases


# An accumulate case is hand-built records, already in the order owl_map_accumulate is given them (class ascending, then the order given):
# label [N], rank [N], score [N] (descending within a class), matched / ignored [N,A,T], npig [C,A], n_classes, aims.
ACC_NS = (0, 1, 63, 64, 65, 128, 129, 200)
ACC_NPIG = (1, 3, 7, 10, 20, 100, 101)


def _pattern(p, n, rng):
    """-> matched [n], ignored [n] of one (area range, threshold)"""
    i = np.arange(n)
    z, o = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    if p == 0:
        return o, z                                    # all true positives
    if p == 1:
        return z, z                                    # all false positives
    if p == 2:
        return i % 2 == 0, o                           # all ignored (matched or not)
    if p == 3:
        return i == n - 1, z                           # the only true positive is the last record
    if p == 4:
        return i == 0, z                               # ... the first
    if p == 5:
        return (i > 0) & (i % 3 != 0), z               # the first record is no true positive
    if p == 6:
        return i >= (2 * n) // 3, z                    # false positives, then true positives: the maximum is carried from the last chunk to the first
    if p == 7:
        return i < n // 3, z                           # the reverse
    if p == 8:
        return rng.uniform(size=n) < 0.5, rng.uniform(size=n) < 0.3
    return rng.uniform(size=n) < 0.15, i % 64 == 63    # sparse true positives; the ignored records end every chunk


def _acc_ranks(n, rng, mixed):
    if not mixed:
        return np.zeros(n, dtype=np.int32)
    rank = rng.choice(np.array([0, 0, 0, 1, 5, 9, 10, 57, 99, 100], dtype=np.int32), size=n)
    edge = np.arange(n)
    rank[(edge % 64 == 63) & (edge % 128 < 64)] = 10       # excluded records on the chunk boundaries
    rank[(edge % 64 == 0) & (edge > 0)] = 100
    rank[(edge % 128 == 127)] = 1
    return rank


def _acc_case(seed, ns, npigs, mixed_ranks, aims, shift=0):
    rng = np.random.RandomState(seed)
    C = len(ns)
    label = np.concatenate([np.full(n, k, dtype=np.int64) for k, n in enumerate(ns)])
    N = len(label)
    matched, ignored = np.zeros((N, A, T), dtype=bool), np.zeros((N, A, T), dtype=bool)
    rank = np.concatenate([_acc_ranks(n, rng, mixed_ranks) for n in ns]).astype(np.int32)
    npig = np.zeros((C, A), dtype=np.int32)
    s0 = 0
    for k, n in enumerate(ns):
        for a in range(A):
            for t in range(T):
                matched[s0:s0 + n, a, t], ignored[s0:s0 + n, a, t] = _pattern((a * 3 + t + k + shift) % 10, n, rng)
            want = npigs[(k + a) % len(npigs)]
            most = int((matched[s0:s0 + n, a] & ~ignored[s0:s0 + n, a]).sum(axis=0).max()) if n else 0
            npig[k, a] = want if want == 0 or want >= most else most + want
        s0 += n
    score = np.linspace(0.99, 0.01, max(N, 1)).astype(np.float32)[:N]
    return dict(label=label, rank=rank, score=score, matched=matched, ignored=ignored, npig=npig, n_classes=C, aims=aims)


def _recall_case():
    """Class k has npig = ACC_NPIG[k] true positives (recall runs through every j / npig) separated by 0-2 false positives, then a tail of false
    positives; k / 10, k / 20, k / 100 coincide with a recall threshold for some k and lie one step under it for others, k / 7 and k / 101 only at 1."""
    rng = np.random.RandomState(33)
    label, matched = [], []
    for k, npg in enumerate(ACC_NPIG):
        m = []
        for _ in range(npg):
            m += [False] * int(rng.randint(0, 3)) + [True]
        m += [False] * 5
        label.append(np.full(len(m), k, dtype=np.int64))
        matched.append(np.array(m, dtype=bool))
    label, m = np.concatenate(label), np.concatenate(matched)
    N = len(label)
    matched = np.repeat(m[:, None, None], A * T, axis=1).reshape(N, A, T).copy()
    ignored = np.zeros((N, A, T), dtype=bool)
    for t in range(1, T):           # threshold t loses every (t+1)-th true positive: recall stops short of 1 at other fractions
        tp = np.nonzero(m)[0]
        matched[tp[::t + 1], :, t] = False
    ignored[:, 1, :] = (np.arange(N) % 5 == 2)[:, None]
    npig = np.repeat(np.array(ACC_NPIG, dtype=np.int32)[:, None], A, axis=1)
    score = np.linspace(0.99, 0.01, N).astype(np.float32)
    return dict(label=label, rank=np.zeros(N, dtype=np.int32), score=score, matched=matched, ignored=ignored, npig=npig, n_classes=len(ACC_NPIG),
                aims="thr_reached / searchsorted 'left' on recall values on and one step under a recall threshold (:191-198,:262-265)")


_accumulate_cases = None


def accumulate_cases():
    global _accumulate_cases
    if _accumulate_cases is None:
        ns = ACC_NS[1:4] + (0,) + ACC_NS[4:] + (7, 0)          # an empty segment between two full ones, and at the end
        _accumulate_cases = {
            "acc_patterns": _acc_case(41, ns, ACC_NPIG, False, "pass-1 counts (:223-233), backward walk in chunks of 64 with the carried maximum (:238-268), zero fill (:237)"),
            "acc_patterns_ranks": _acc_case(42, ns, ACC_NPIG, True, "rank < maxDet per column (:226,:244), excluded records on chunk boundaries", shift=4),
            "acc_no_records_and_no_ground_truth": _acc_case(43, (0, 65, 0, 64, 129), (5, 0, 3, 0), True, "n == 0 with npig > 0 (recall 0, precision 0), npig == 0 (-1 everywhere) (:211-215,:235-237)", shift=7),
            "acc_recall_steps": _recall_case(),
        }
    return _accumulate_cases
