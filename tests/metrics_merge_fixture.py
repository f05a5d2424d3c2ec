"""The eval set of tests/test_metrics_merge.py and tests/test_metrics_merge_gpu.py: 7 images, 3 classes, built deterministically with the package's
counter-based rng (numpy only; the worker processes of the GPU test rebuild exactly the same arrays).

What it holds, and why:
* 0-8 detections and 0-5 ground truths per image; image 3 has no detections, image 5 no ground truths;
* scores on 5 levels (0.2, 0.4, 0.6, 0.8, 1.0 as f32): ties across images are certain;
* class 2 occurs in the even images only: under two shards rank 1 (images 1, 3, 5) infers 2 classes, rank 0 infers 3;
* two pairs of duplicate boxes in different images, same class and score.  Pair A: a true positive in image 6 (it is a copy of a ground truth there)
  and a false positive in image 1 (no ground truth near it).  In image order the false positive comes first; any order that puts a shard holding
  image 6 before a shard holding image 1 (rank-major concatenation for 2 and for 3 shards) flips them and changes the precision of class 0.
  Pair B: the same with images 2 (true positive) and 5 (false positive), class 1;
* integer boxes whose IoU with a ground truth is exactly 0.5 and 0.75 (restated from tests/test_metrics_gpu.py: [0,0,10,5] on [0,0,10,10],
  [0,0,20,15] on [0,0,20,20]), in images 0 and 4.
"""
import numpy as np

from owl_vit_object_detection_amd import rng
from tests import coco_eval_restatement as R

N_IMAGES, N_CLASSES, SEED = 7, 3, 11
LEVELS = np.array([0.2, 0.4, 0.6, 0.8, 1.0], dtype=np.float32)
PAIR_A = ([300.0, 300.0, 340.0, 350.0], 0, LEVELS[3])     # box, class, score: image 1 (false positive) and image 6 (true positive)
PAIR_B = ([320.0, 40.0, 420.0, 160.0], 1, LEVELS[2])      # image 5 (false positive) and image 2 (true positive)


def _boxes(stream, n):
    side = np.array([12.0, 50.0, 150.0])[rng.randint(SEED, stream + ".size", n, 3)][:, None] * (0.8 + 0.4 * rng.uniform(SEED, stream + ".wh", 2 * n).reshape(n, 2))
    xy = np.floor(rng.uniform(SEED, stream + ".xy", 2 * n).reshape(n, 2) * 250.0)
    return np.concatenate([xy, xy + np.floor(side) + 1.0], axis=1).astype(np.float32)


def images():
    n_det = rng.randint(SEED, "n_det", N_IMAGES, 6) + 1          # 1..6 random ones; the constructed ones come on top (at most 8)
    n_gt = rng.randint(SEED, "n_gt", N_IMAGES, 3) + 1            # 1..3 (at most 5 with the constructed ones)
    n_det[3], n_gt[5] = 0, 0
    out = []
    for i in range(N_IMAGES):
        classes = 3 if i % 2 == 0 else 2
        s = f"img{i}"
        g, d = int(n_gt[i]), int(n_det[i])
        gt, gl = _boxes(s + ".gt", g), rng.randint(SEED, s + ".gl", g, classes)
        # detections: copies of the image's ground truths shifted by a few pixels (or strays where there is none), mostly of the right class
        det = _boxes(s + ".det", d)
        dl = rng.randint(SEED, s + ".dl", d, classes)
        if g and d:
            src = rng.randint(SEED, s + ".src", d, g)
            near = rng.uniform(SEED, s + ".near", d) < 0.7
            shift = np.floor(rng.uniform(SEED, s + ".shift", 4 * d).reshape(d, 4) * 7.0) - 3.0
            det[near] = (gt[src] + shift)[near]
            det[:, 2:] = np.maximum(det[:, 2:], det[:, :2] + 1.0)
            dl[near] = gl[src][near]
        sc = LEVELS[rng.randint(SEED, s + ".score", d, len(LEVELS))]
        extra_det, extra_sc, extra_dl, extra_gt, extra_gl = [], [], [], [], []
        if i in (1, 6):
            extra_det.append(PAIR_A[0]); extra_dl.append(PAIR_A[1]); extra_sc.append(PAIR_A[2])
            if i == 6:
                extra_gt.append(PAIR_A[0]); extra_gl.append(PAIR_A[1])
        if i in (2, 5):
            extra_det.append(PAIR_B[0]); extra_dl.append(PAIR_B[1]); extra_sc.append(PAIR_B[2])
            if i == 2:
                extra_gt.append(PAIR_B[0]); extra_gl.append(PAIR_B[1])
        if i == 0:      # IoU exactly 0.5
            extra_det.append([400.0, 400.0, 410.0, 405.0]); extra_dl.append(0); extra_sc.append(LEVELS[3])
            extra_gt.append([400.0, 400.0, 410.0, 410.0]); extra_gl.append(0)
        if i == 4:      # IoU exactly 0.75
            extra_det.append([400.0, 400.0, 420.0, 415.0]); extra_dl.append(1); extra_sc.append(LEVELS[2])
            extra_gt.append([400.0, 400.0, 420.0, 420.0]); extra_gl.append(1)
        out.append(R.image(np.concatenate([det, np.asarray(extra_det, np.float32).reshape(-1, 4)]), np.concatenate([sc, np.asarray(extra_sc, np.float32)]),
                           np.concatenate([dl, np.asarray(extra_dl, np.int64)]), np.concatenate([gt, np.asarray(extra_gt, np.float32).reshape(-1, 4)]),
                           np.concatenate([gl, np.asarray(extra_gl, np.int64)])))
    return out


def rank_major(world, n=N_IMAGES):
    """the image order a gather without keys leaves behind: shard 0's images, then shard 1's, ..."""
    return [i for r in range(world) for i in range(r, n, world)]
