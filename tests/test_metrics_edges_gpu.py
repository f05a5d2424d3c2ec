"""The two kernels of csrc/metrics.hip at the named edge cases of tests/coco_eval_restatement.py (`match_cases`, `accumulate_cases`): the shapes
at which map_match_kernel's compactions, rank cut, ground-truth order and matching chain, and map_accumulate_kernel's chunked backward walk and
threshold search change form.  tests/test_metrics.py shows on the CPU that every planted protocol mistake changes an output of one of these cases;
profiles/eval_map_edges.md maps case -> kernel form -> mistakes killed.

Every comparison is exact: the records are integers and bits, precision / recall are IEEE f64 quotients of the same integers on both sides."""
import functools

import numpy as np
import pytest
import torch

from tests import coco_eval_restatement as R
from tests.test_metrics_gpu import _decode, _dicts, _metric

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _match_reference(name):
    """the restatement's records and curves of a match case, computed once: (label, rank, score, matched, ignored) of the records, npig, precision, recall"""
    case = R.match_cases()[name]
    recs = [R.match_image(im, case["n_classes"]) for im in case["images"]]
    label, rank, matched, ignored = (np.concatenate([r[i] for r in recs]) for i in range(4))
    score = np.concatenate([im["det_scores"] for im in case["images"]])
    npig = np.sum([r[4] for r in recs], axis=0)
    precision, recall = R.accumulate_records(label, rank, score, matched, ignored, npig, case["n_classes"])
    keep = label >= 0
    return (label[keep], rank[keep], score[keep], matched[keep], ignored[keep]), npig, precision, recall


def _cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _update(m, case):
    bt = case["batched"]
    if bt is None:
        m.update(*_dicts(case["images"]))
    else:
        m.update_batched(_cuda(bt["boxes"]), _cuda(bt["labels"]), _cuda(bt["scores"]), _cuda(bt["counts"]), _cuda(bt["gt_boxes"]), _cuda(bt["gt_labels"]),
                         _cuda(bt["gt_counts"]), width=_cuda(bt["width"]), height=_cuda(bt["height"]))


@pytest.mark.parametrize("name", list(R.match_cases()))
def test_match_case(name):
    case = R.match_cases()[name]
    (rl, rr, rs, rm, ri), rnpig, rprec, rrec = _match_reference(name)
    m = _metric(case["n_classes"])
    _update(m, case)
    (score, label, rank, mask), npig, C = m.records()
    assert C == case["n_classes"]
    label, rank, score, mask, npig = (x.cpu().numpy() for x in (label, rank, score, mask, npig))
    print(name, "records", len(label), "of", sum(len(im["det_scores"]) for im in case["images"]), "slots; npig", npig.tolist())
    assert np.array_equal(label, rl)
    assert np.array_equal(rank, rr)
    assert np.array_equal(score.view(np.uint32), rs.view(np.uint32))          # bits: a NaN behind a count must not come through as a score
    matched, ignored = _decode(mask)
    assert np.array_equal(matched, rm), np.argwhere(matched != rm)[:8]
    assert np.array_equal(ignored, ri), np.argwhere(ignored != ri)[:8]
    assert (mask >> 20 == 0).all()
    assert np.array_equal(npig, rnpig)
    precision, recall = m.evaluate()
    assert np.array_equal(recall.cpu().numpy(), rrec)
    assert np.array_equal(precision.cpu().numpy(), rprec)


def test_padding_behind_the_counts_changes_no_bit():
    """owl_map_match on the padding case as built (valid-looking labels, NaN boxes and NaN scores behind the counts, counts -3 and K + 5) and with the
    padding wiped clean and the counts clamped: every output array is the same, and every slot behind a count is "no record"."""
    from owl_vit_object_detection_amd import ops
    bt = R.match_cases()["padding"]["batched"]
    C = R.match_cases()["padding"]["n_classes"]
    B, K = bt["labels"].shape
    G = bt["gt_labels"].shape[1]
    clean = {k: (None if v is None else v.copy()) for k, v in bt.items()}
    clean["counts"], clean["gt_counts"] = np.clip(bt["counts"], 0, K), np.clip(bt["gt_counts"], 0, G)
    for b in range(B):
        n, g = clean["counts"][b], clean["gt_counts"][b]
        clean["boxes"][b, n:], clean["scores"][b, n:], clean["labels"][b, n:] = 0, 0, -1
        clean["gt_boxes"][b, g:], clean["gt_labels"][b, g:] = 0, -1
    scale = torch.ones(B, 2, dtype=torch.float32, device="cuda")
    outs = [ops.map_match(_cuda(d["boxes"]), _cuda(d["scores"]), _cuda(d["labels"]), _cuda(d["counts"]), _cuda(d["gt_boxes"]), _cuda(d["gt_labels"]),
                          _cuda(d["gt_counts"]), scale, C) for d in (bt, clean, bt)]
    for x, y, z in zip(*outs):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, z.view(torch.int32) if z.dtype == torch.float32 else z)
    score, label, rank, mask, _ = (x.cpu().numpy() for x in outs[0])
    behind = np.arange(K)[None, :] >= clean["counts"][:, None]
    out_of_range = (bt["labels"] < 0) | (bt["labels"] >= C)
    assert np.array_equal(label == -1, behind | out_of_range)
    assert (score[label == -1] == 0).all() and (rank[label == -1] == 0).all() and (mask[label == -1] == 0).all()


# ---- owl_map_accumulate on hand-built records ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _accumulate_reference(name):
    c = R.accumulate_cases()[name]
    return R.accumulate_records(c["label"], c["rank"], c["score"], c["matched"], c["ignored"], c["npig"], c["n_classes"])


def _device_records(c):
    """-> rank [N] i32, mask [N,4] i32, seg [C+1] i64, npig [C,4] i32 on the device (the records are given in class order, scores descending)"""
    assert np.all(np.diff(c["label"]) >= 0) and all(np.all(np.diff(c["score"][c["label"] == k]) < 0) for k in range(c["n_classes"]))
    bits = np.concatenate([c["matched"], c["ignored"]], axis=2).astype(np.int64)                    # [N,A,20]: bit t matched, bit 10 + t ignored
    mask = (bits << np.arange(20)[None, None, :]).sum(axis=2).astype(np.int32)
    seg = np.searchsorted(c["label"], np.arange(c["n_classes"] + 1)).astype(np.int64)
    return _cuda(c["rank"].astype(np.int32)), _cuda(mask), _cuda(seg), _cuda(c["npig"].astype(np.int32))


@pytest.mark.parametrize("name", list(R.accumulate_cases()))
def test_accumulate_case(name):
    from owl_vit_object_detection_amd import ops
    c = R.accumulate_cases()[name]
    rprec, rrec = _accumulate_reference(name)
    rank, mask, seg, npig = _device_records(c)
    precision, recall = ops.map_accumulate(rank, mask, seg, npig, c["n_classes"])
    again = ops.map_accumulate(rank, mask, seg, npig, c["n_classes"])
    assert torch.equal(precision.view(torch.int64), again[0].view(torch.int64)) and torch.equal(recall.view(torch.int64), again[1].view(torch.int64))
    precision, recall = precision.cpu().numpy(), recall.cpu().numpy()
    print(name, "segments", np.diff(seg.cpu().numpy()).tolist(), "entries that differ", int((precision != rprec).sum()), int((recall != rrec).sum()))
    assert precision.shape == rprec.shape and recall.shape == rrec.shape
    assert np.array_equal(recall, rrec), np.argwhere(recall != rrec)[:8]
    assert np.array_equal(precision, rprec), np.argwhere(precision != rprec)[:8]


def test_accumulate_raw_entry_writes_every_entry_and_nothing_behind_them():
    from owl_vit_object_detection_amd import _lib, ops
    c = R.accumulate_cases()["acc_patterns_ranks"]
    C = c["n_classes"]
    rprec, rrec = _accumulate_reference("acc_patterns_ranks")
    rank, mask, seg, npig = _device_records(c)
    k = ops.map_constants(rank.device)
    n_prec, n_rec, tail = 10 * 101 * C * 4 * 3, 10 * C * 4 * 3, 4096
    runs = []
    for _ in range(2):
        prec = torch.full((n_prec + tail,), float("nan"), dtype=torch.float64, device="cuda")
        rec = torch.full((n_rec + tail,), float("nan"), dtype=torch.float64, device="cuda")
        prec[n_prec:], rec[n_rec:] = -7.0, -7.0
        _lib.call("owl_map_accumulate", ops.stream(), rank, mask, seg, npig, k["rec_thr"], k["max_dets"], k["eps"], prec, rec, rank.shape[0], C)
        torch.cuda.synchronize()
        runs.append((prec.cpu().numpy(), rec.cpu().numpy()))
    (prec, rec), (prec2, rec2) = runs
    assert not np.isnan(prec[:n_prec]).any() and not np.isnan(rec[:n_rec]).any()          # every entry is written
    assert (prec[n_prec:] == -7.0).all() and (rec[n_rec:] == -7.0).all()                   # and nothing behind them
    assert np.array_equal(prec[:n_prec].reshape(rprec.shape), rprec) and np.array_equal(rec[:n_rec].reshape(rrec.shape), rrec)
    assert np.array_equal(prec.view(np.int64), prec2.view(np.int64)) and np.array_equal(rec.view(np.int64), rec2.view(np.int64))
