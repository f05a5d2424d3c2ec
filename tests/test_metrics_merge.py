"""mAP under data parallel, the parts that need no GPU: the explicit order of the records (metrics.record_order), the shard of an eval set
(ddp.eval_indices / ddp.EvalSampler), the ragged gather (ddp.all_gather_ragged) over two gloo ranks on host tensors, and -- with the numpy
restatement alone -- that the fixture of the GPU tests has a cross-image score tie that matters.  Everything is compared exactly."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import coco_eval_restatement as R
from tests import metrics_merge_fixture as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tied_records(seed):
    """heavy ties: 9 images with up to 6 slots each, 3 classes, scores on 4 levels; records of an image arrive together, ranks follow slot order per class"""
    rng = np.random.RandomState(seed)
    score, label, key, rank = [], [], [], []
    for img in range(9):
        n = rng.randint(0, 7)
        sc = np.sort(rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), size=n))[::-1]       # an image's list is sorted by descending score
        lb = rng.randint(0, 3, size=n)
        rk = np.zeros(n, np.int32)
        for c in range(3):
            rk[lb == c] = np.arange((lb == c).sum())
        score.append(sc); label.append(lb); key.append(np.full(n, img, np.int64)); rank.append(rk)
    return np.concatenate(score).astype(np.float32), np.concatenate(label).astype(np.int64), np.concatenate(key), np.concatenate(rank)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_record_order_is_the_lexicographic_order_of_the_four_keys(seed):
    from owl_vit_object_detection_amd.metrics import record_order
    score, label, key, rank = _tied_records(seed)
    assert len(score) > 20 and len(np.unique(score)) <= 4
    rng = np.random.RandomState(100 + seed)
    for shuffle in (False, True):          # in arrival order, and with the records (and the image keys) scrambled
        p = rng.permutation(len(score)) if shuffle else np.arange(len(score))
        k = (rng.permutation(9)[key] if shuffle else key)[p]
        s, l, r = score[p], label[p], rank[p]
        got = record_order(torch.from_numpy(s), torch.from_numpy(l), torch.from_numpy(k), torch.from_numpy(r)).numpy()
        want = np.lexsort((r, k, -s.astype(np.float64), l))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_record_order_with_arrival_keys_is_the_two_stable_sorts(seed):
    """With image keys = arrival index the order is what two stable sorts (by descending score, then by class) give: ties broken by arrival."""
    from owl_vit_object_detection_amd.metrics import record_order
    score, label, key, rank = _tied_records(seed)
    by_score = np.argsort(-score.astype(np.float64), kind="stable")
    want = by_score[np.argsort(label[by_score], kind="stable")]
    got = record_order(torch.from_numpy(score), torch.from_numpy(label), torch.from_numpy(key), torch.from_numpy(rank)).numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [0, 1, 7, 8])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_eval_shards_partition_the_set_and_default_keys_are_global_indices(n, world):
    from owl_vit_object_detection_amd import ddp
    shards = [list(ddp.eval_indices(n, r, world)) for r in range(world)]
    assert sorted(i for s in shards for i in s) == list(range(n))
    assert max(len(s) for s in shards) - min(len(s) for s in shards) <= 1
    for r, s in enumerate(shards):
        assert s == [i_local * world + r for i_local in range(len(s))]          # the metric's default image key of shard position i_local


def test_eval_sampler_walks_the_same_indices():
    from owl_vit_object_detection_amd import ddp
    assert list(ddp.eval_indices(7)) == list(range(7))                          # no process group: one shard
    for dataset in (7, list(range(7))):
        s = ddp.EvalSampler(dataset)
        assert isinstance(s, torch.utils.data.Sampler) and list(s) == list(range(7)) and len(s) == 7
    s.rank, s.world = 1, 3
    assert list(s) == [1, 4] and len(s) == 2
    with pytest.raises(ValueError):
        ddp.eval_indices(7, 3, 3)


def test_fixture_has_a_cross_image_tie_that_matters():
    """The restatement alone: the fixture is what its docstring says, and evaluating the images in the order a rank-major gather leaves (2 and 3 shards)
    changes the precision array -- otherwise the GPU tests' negative control would prove nothing."""
    images = F.images()
    assert len(images) == 7
    assert [len(im["det_scores"]) for im in images][3] == 0 and len(images[5]["gt_labels"]) == 0
    assert all(len(im["det_scores"]) <= 8 and len(im["gt_labels"]) <= 5 for im in images)
    labels = np.concatenate([np.concatenate([im["det_labels"], im["gt_labels"]]) for im in images])
    assert set(labels) == {0, 1, 2}
    assert max(max(im["det_labels"].max(initial=-1), im["gt_labels"].max(initial=-1)) for im in images[1::2]) == 1      # the odd images infer 2 classes
    assert set(np.concatenate([im["det_scores"] for im in images])) <= set(F.LEVELS)
    # the duplicate pairs: true positive in one image, false positive in the other (IoU threshold 0.5, all areas)
    for (box, cls, sc), tp_img, fp_img in ((F.PAIR_A, 6, 1), (F.PAIR_B, 2, 5)):
        for img, want in ((tp_img, True), (fp_img, False)):
            im = images[img]
            d = [j for j in range(len(im["det_scores"])) if np.array_equal(im["det_boxes"][j], np.asarray(box, np.float32))]
            assert len(d) == 1 and im["det_labels"][d[0]] == cls and im["det_scores"][d[0]] == sc
            assert bool(R.match_image(im, 3)[2][d[0], 0, 0]) is want
    # IoU exactly on 0.5 and on 0.75: matched at that threshold, not at the next
    for img, t in ((0, 0), (4, 5)):
        m = R.match_image(images[img], 3)[2]
        d = len(images[img]["det_scores"]) - 1
        assert m[d, 0, t] and not m[d, 0, t + 1]
    precision, recall = R.accumulate(images, 3)
    assert (precision > 0).any() and (precision[precision > -1] < 1).any()
    for world in (2, 3):
        p, r = R.accumulate([images[i] for i in F.rank_major(world)], 3)
        assert np.array_equal(r, recall)                  # the recall does not depend on the order
        assert not np.array_equal(p, precision), world


_GATHER_WORKER = r'''
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from owl_vit_object_detection_amd import ddp
rank, world, _ = ddp.init_from_env("gloo")
torch.set_num_threads(1)

def rows(r, n):      # the dtypes and trailing shapes of the metric's record tuple: score, label, rank, mask, key
    base = torch.arange(n, dtype=torch.int64) + 100 * r
    return [base.to(torch.float32) * 0.25, -base - 1, base.to(torch.int32) + 7, (base[:, None] * 4 + torch.arange(4)).to(torch.int32), base * (2 ** 40)]

for case, counts in enumerate(([0, 5], [3, 3])):
    out, got_counts = ddp.all_gather_ragged(rows(rank, counts[rank]), None)
    assert got_counts == counts, got_counts
    np.savez(os.path.join({out!r}, f"case{{case}}_rank{{rank}}.npz"), *[t.numpy() for t in out])
dist.barrier(); dist.destroy_process_group()
'''


@pytest.mark.timeout(300)
def test_ragged_gather_over_two_gloo_ranks_on_host_tensors(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GATHER_WORKER.format(root=ROOT, out=str(tmp_path)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "OWL_FORCE_DIST")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script)], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]

    def rows(r, n):
        base = np.arange(n, dtype=np.int64) + 100 * r
        return [base.astype(np.float32) * 0.25, -base - 1, base.astype(np.int32) + 7, (base[:, None] * 4 + np.arange(4)).astype(np.int32), base * (2 ** 40)]

    for case, counts in enumerate(([0, 5], [3, 3])):
        want = [np.concatenate(x) for x in zip(rows(0, counts[0]), rows(1, counts[1]))]
        for rank in (0, 1):
            got = np.load(tmp_path / f"case{case}_rank{rank}.npz")
            got = [got[f"arr_{i}"] for i in range(5)]
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
