"""mAP under data parallel on the device: the merged state of several shards (metrics.MeanAveragePrecision.merge_state in one process, the gather
inside compute() over real ranks) gives the BITS of one metric fed the whole eval set in order.  No tolerance anywhere: the merged path runs the
same owl_map_accumulate on the same ordered input.  The eval set is tests/metrics_merge_fixture.py (ties in score across images that matter: a
rank-major concatenation without image keys provably changes the precision, test_metrics_merge.py::test_fixture_has_a_cross_image_tie_that_matters)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import coco_eval_restatement as R
from tests import metrics_merge_fixture as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")


def _metric(n_classes=F.N_CLASSES, **kw):
    from owl_vit_object_detection_amd.metrics import MeanAveragePrecision
    return MeanAveragePrecision(iou_type="bbox", class_metrics=True, n_classes=n_classes, **kw).to("cuda")


def _dicts(images):
    preds = [{"boxes": torch.from_numpy(im["det_boxes"]).cuda(), "scores": torch.from_numpy(im["det_scores"]).cuda(), "labels": torch.from_numpy(im["det_labels"]).cuda()} for im in images]
    targets = [{"boxes": torch.from_numpy(im["gt_boxes"]).cuda(), "labels": torch.from_numpy(im["gt_labels"]).cuda()} for im in images]
    return preds, targets


def _results(m):
    """-> (precision, recall, compute()) of a metric"""
    precision, recall = m.evaluate()
    return precision, recall, m.compute()


def _assert_same_bits(got, want):
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert set(got[2]) == set(want[2])
    for k in want[2]:
        assert got[2][k].dtype == want[2][k].dtype and torch.equal(got[2][k], want[2][k]), k


@pytest.fixture(scope="module")
def images():
    return F.images()


@pytest.fixture(scope="module")
def single(images):
    """One metric fed all 7 images in order (one shard, default keys): the reference of every test here, held to the restatement once."""
    m = _metric()
    m.update(*_dicts(images))
    res = _results(m)
    rp, rr = R.accumulate(images, F.N_CLASSES)
    assert np.array_equal(res[0].cpu().numpy(), rp) and np.array_equal(res[1].cpu().numpy(), rr)
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_in_process_shards_merge_to_the_bits_of_one_metric(images, single, world):
    shards = [_metric(shard=(r, world)) for r in range(world)]
    for r, m in enumerate(shards):
        m.update(*_dicts(images[r::world]))
    merged = shards[0]
    for m in shards[1:]:
        merged.merge_state(m)
    res = _results(merged)
    _assert_same_bits(res, single)
    rp, rr = R.accumulate(images, F.N_CLASSES)
    assert np.array_equal(res[0].cpu().numpy(), rp) and np.array_equal(res[1].cpu().numpy(), rr)
    assert torch.equal(merged.image_keys().sort().values, torch.arange(len(images), device="cuda"))
    # negative control: the same records concatenated rank-major without keys (arrival order = what a naive gather leaves) are another precision
    naive = _metric()
    naive.update(*_dicts([images[i] for i in F.rank_major(world)]))
    precision, recall = naive.evaluate()
    assert torch.equal(recall, single[1])
    assert not torch.equal(precision, single[0])
    # the merged state is left intact, and takes further merges: the same answer again
    _assert_same_bits(_results(merged), single)


def test_explicit_image_ids_in_scrambled_arrival_order(images, single):
    order = [6, 2, 5, 0, 3, 1, 4]
    m = _metric()
    m.update(*_dicts([images[i] for i in order[:3]]), image_ids=order[:3])                                      # a list
    m.update(*_dicts([images[i] for i in order[3:]]), image_ids=torch.tensor(order[3:], dtype=torch.int32).cuda())      # a device tensor
    assert m.image_keys().tolist() == order
    _assert_same_bits(_results(m), single)
    # sparse ids in the same relative order are the same result
    sparse = _metric()
    sparse.update(*_dicts([images[i] for i in order]), image_ids=torch.tensor([1000 * i + 17 for i in order]))
    _assert_same_bits(_results(sparse), single)
    with pytest.raises(ValueError, match="non-negative"):
        _metric().update(*_dicts(images[:2]), image_ids=[0, -1])
    with pytest.raises(ValueError, match="image_ids"):
        _metric().update(*_dicts(images[:2]), image_ids=[0, 1, 2])


def test_duplicate_image_key_is_refused(images):
    a, b = _metric(shard=(0, 2)), _metric(shard=(0, 2))          # two shards that both believe they are rank 0: image 0 and image 2 twice
    a.update(*_dicts(images[0::2]))
    b.update(*_dicts(images[0:2]))
    a.merge_state(b)
    with pytest.raises(ValueError, match=r"more than once.*\[0, 2\]"):
        a.compute()
    c, d = _metric(shard=(0, 2)), _metric(shard=(1, 2))          # the same explicit id from two shards
    c.update(*_dicts(images[:2]), image_ids=[4, 9])
    d.update(*_dicts(images[2:4]), image_ids=[9, 5])
    c.merge_state(d)
    with pytest.raises(ValueError, match=r"more than once.*\[9\]"):
        c.evaluate()
    neg = _metric()
    neg.update(*_dicts(images[:2]), image_ids=torch.tensor([3, -2]).cuda())          # device ids are not read back in update: refused in compute()
    with pytest.raises(ValueError, match="non-negative"):
        neg.compute()


def test_update_and_update_batched_agree_on_keys_and_results(images, single):
    B, K, G = len(images), max(len(im["det_scores"]) for im in images), max(len(im["gt_labels"]) for im in images)
    boxes, scores, labels = np.zeros((B, K, 4), np.float32), np.zeros((B, K), np.float32), np.full((B, K), -1, np.int64)
    gtb, gtl = np.zeros((B, G, 4), np.float32), np.full((B, G), -1, np.int64)
    counts, gcounts = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, im in enumerate(images):
        n, g = len(im["det_scores"]), len(im["gt_labels"])
        boxes[b, :n], scores[b, :n], labels[b, :n], counts[b] = im["det_boxes"], im["det_scores"], im["det_labels"], n
        gtb[b, :g], gtl[b, :g], gcounts[b] = im["gt_boxes"], im["gt_labels"], g
    batch = [torch.from_numpy(a).cuda() for a in (boxes, labels, scores, counts, gtb, gtl, gcounts)]
    ids = torch.arange(B, dtype=torch.int64, device="cuda") * 3 + 1
    for shard, image_ids in (((1, 3), None), ((0, 1), ids)):          # the default keys of shard (1, 3) ARE ids
        mb, mu = _metric(shard=shard), _metric(shard=shard)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")          # neither the default keys nor explicit device ids synchronise
        try:
            mb.update_batched(*batch, image_ids=image_ids)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        mu.update(*_dicts(images), image_ids=image_ids)
        assert torch.equal(mb.image_keys(), ids) and torch.equal(mu.image_keys(), ids)
        for x, y in zip(mb._state()[0], mu._state()[0]):          # score, label, rank, mask and the per-record key
            assert x.dtype == y.dtype and torch.equal(x, y)
        _assert_same_bits(_results(mb), single)
        _assert_same_bits(_results(mu), single)
    # two updates continue the count: image i of the metric has key i * world + rank
    m = _metric(shard=(2, 4))
    m.update(*_dicts(images[:3])); m.update(*_dicts(images[3:]))
    assert m.image_keys().tolist() == [4 * i + 2 for i in range(B)]
    m.reset(); m.update(*_dicts(images[:2]))
    assert m.image_keys().tolist() == [2, 6]


def test_update_metrics_passes_image_ids_through(images, single):
    from owl_vit_object_detection_amd.train_util import update_metrics
    order = [6, 2, 5, 0, 3, 1, 4]
    K, G = 8, 5
    m = _metric()
    for i in order:          # one image per call, normalised boxes, ground truth on the host as the loader delivers it
        im = images[i]
        n, g = len(im["det_scores"]), len(im["gt_labels"])
        pb, pc, ps = torch.zeros(1, K, 4), torch.full((1, K), -1, dtype=torch.int64), torch.zeros(1, K)
        gb, gl = torch.zeros(1, G, 4), torch.full((1, G), -1, dtype=torch.int64)
        pb[0, :n], pc[0, :n], ps[0, :n] = torch.from_numpy(im["det_boxes"]) / 512.0, torch.from_numpy(im["det_labels"]), torch.from_numpy(im["det_scores"])
        gb[0, :g], gl[0, :g] = torch.from_numpy(im["gt_boxes"]) / 512.0, torch.from_numpy(im["gt_labels"])
        update_metrics(m, {"width": 512.0, "height": 512.0}, pb.cuda(), pc.cuda(), ps.cuda(), gb, gl, image_ids=torch.tensor([i]))
    assert m.image_keys().tolist() == order
    _assert_same_bits(_results(m), single)          # (integer pixel coordinates / 512 * 512 are exact in f32)


# ---- real ranks ------------------------------------------------------------------------------------------------------------------------------
_WORKER = r'''
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from owl_vit_object_detection_amd import ddp
from owl_vit_object_detection_amd.metrics import MeanAveragePrecision
from tests import metrics_merge_fixture as F
rank, world, local = ddp.init_from_env({backend!r})
dev = torch.device("cuda", local if {backend!r} == "nccl" else 0)       # (gloo variant: both ranks on the one visible GPU)
torch.cuda.set_device(dev)
images = F.images()
mine = list(ddp.EvalSampler(len(images)))
assert mine == list(ddp.eval_indices(len(images))) == list(range(rank, len(images), world))
if {rank1_empty}:
    mine = list(range(len(images))) if rank == 0 else []

def dicts(idx):
    preds = [dict(boxes=torch.from_numpy(images[i]["det_boxes"]).to(dev), scores=torch.from_numpy(images[i]["det_scores"]).to(dev), labels=torch.from_numpy(images[i]["det_labels"]).to(dev)) for i in idx]
    targets = [dict(boxes=torch.from_numpy(images[i]["gt_boxes"]).to(dev), labels=torch.from_numpy(images[i]["gt_labels"]).to(dev)) for i in idx]
    return preds, targets

metric = MeanAveragePrecision(iou_type="bbox", class_metrics=True, n_classes={n_classes}).to(dev)
local_only = MeanAveragePrecision(iou_type="bbox", class_metrics=True, n_classes=3, sync_on_compute=False).to(dev)
for i0 in range(0, len(mine), 2):                  # batches of 2 (and one of 1)
    metric.update(*dicts(mine[i0:i0 + 2]))
    local_only.update(*dicts(mine[i0:i0 + 2]))
SCALARS = {scalars!r}

def dump(m, name):
    precision, recall = m.evaluate()
    out = m.compute()
    again = m.compute()                             # the local state is left intact
    assert all(torch.equal(out[k], again[k]) for k in out)
    np.save(os.path.join({out!r}, f"{{name}}_precision_{{rank}}.npy"), precision.cpu().numpy())
    np.save(os.path.join({out!r}, f"{{name}}_recall_{{rank}}.npy"), recall.cpu().numpy())
    np.save(os.path.join({out!r}, f"{{name}}_summary_{{rank}}.npy"), torch.cat([torch.stack([out[k] for k in SCALARS]), out["map_per_class"], out["mar_100_per_class"]]).cpu().numpy())

dump(metric, "merged")
dump(local_only, "local")
torch.cuda.synchronize()
dist.barrier(); dist.destroy_process_group()
'''

RUNS = {"uneven-inferred-classes": dict(nproc=2, backend="gloo", n_classes=None, rank1_empty=False),
        "rank1-empty": dict(nproc=2, backend="gloo", n_classes=3, rank1_empty=True),
        "forced-single-rccl-rank": dict(nproc=1, backend="nccl", n_classes=3, rank1_empty=False),
        "two-rccl-ranks": dict(nproc=2, backend="nccl", n_classes=None, rank1_empty=False)}
_done = {}


def _launch(name, tmp_path_factory):
    """Run the worker of RUNS[name] once per session -> {(kind, what, rank): array}"""
    if name in _done:
        return _done[name]
    cfg = RUNS[name]
    out = tmp_path_factory.mktemp(name.replace("-", "_"))
    script = out / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=str(out), backend=cfg["backend"], n_classes=cfg["n_classes"], rank1_empty=cfg["rank1_empty"], scalars=SCALARS))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "OWL_FORCE_DIST"):
        env.pop(k, None)
    if cfg["nproc"] == 1:
        env["OWL_FORCE_DIST"] = "1"
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={cfg['nproc']}", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    _done[name] = {(kind, what, rank): np.load(out / f"{kind}_{what}_{rank}.npy") for kind in ("merged", "local") for what in ("precision", "recall", "summary")
                   for rank in range(cfg["nproc"])}
    return _done[name]


def _arrays(res):
    out = res[2]
    return {"precision": res[0].cpu().numpy(), "recall": res[1].cpu().numpy(),
            "summary": torch.cat([torch.stack([out[k] for k in SCALARS]), out["map_per_class"], out["mar_100_per_class"]]).cpu().numpy()}


@pytest.mark.timeout(400)
@pytest.mark.parametrize("name", ["uneven-inferred-classes", "rank1-empty", "forced-single-rccl-rank", "two-rccl-ranks"])
def test_real_ranks_compute_the_bits_of_one_process(single, tmp_path_factory, name):
    """compute() on every rank gathers the ranks' states: two gloo ranks on the one visible GPU holding 4 and 3 images (class count inferred: rank 1
    sees 2 classes, rank 0 sees 3), rank 1 holding no image at all, one forced rank over the real RCCL backend, and two RCCL ranks where there are two
    GPUs.  Every rank's arrays are bytewise the single process's."""
    if name == "two-rccl-ranks" and torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs; the same worker runs on 2 gloo ranks and on one forced RCCL rank above")
    got = _launch(name, tmp_path_factory)
    want = _arrays(single)
    for rank in range(RUNS[name]["nproc"]):
        for what in ("precision", "recall", "summary"):
            g = got[("merged", what, rank)]
            assert g.dtype == want[what].dtype and g.shape == want[what].shape and g.tobytes() == want[what].tobytes(), (rank, what)


@pytest.mark.timeout(400)
def test_sync_on_compute_false_returns_the_local_shard(images, tmp_path_factory):
    got = _launch("uneven-inferred-classes", tmp_path_factory)
    for rank in (0, 1):
        m = _metric()
        m.update(*_dicts(images[rank::2]))
        want = _arrays(_results(m))
        for what in ("precision", "recall", "summary"):
            assert got[("local", what, rank)].tobytes() == want[what].tobytes(), (rank, what)
    assert got[("local", "precision", 0)].tobytes() != got[("local", "precision", 1)].tobytes()
