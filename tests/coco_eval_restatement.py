"""Plain numpy f64 restatement of the COCO bbox evaluation protocol (pycocotools `COCOeval`: evaluateImg -> accumulate -> summarize), the
contract `metrics.MeanAveragePrecision` is held to.  Test infrastructure only: written as the loops of the protocol, slow on purpose, never
imported by the package.

An "image" is a dict: det_boxes [n,4] f32 pixel xyxy, det_scores [n] f32, det_labels [n] int, gt_boxes [g,4] f32 pixel xyxy, gt_labels [g] int.
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
    precision = -np.ones((T, R, n_classes, A, M))
    recall = -np.ones((T, n_classes, A, M))
    if not recs:
        return precision, recall
    score = np.concatenate([np.asarray(img["det_scores"], dtype=np.float32).reshape(-1) for img in images]).astype(np.float64)
    label = np.concatenate([r[0] for r in recs])
    rank = np.concatenate([r[1] for r in recs])
    matched = np.concatenate([r[2] for r in recs])
    ignored = np.concatenate([r[3] for r in recs])
    npig_all = np.sum([r[4] for r in recs], axis=0)
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
