"""Time the device-resident COCO mAP (metrics.MeanAveragePrecision) at eval-loop shapes and print one JSON line.

  update_batched   one 32-image batch of top-200 detections (the PostProcess(..., top_k=200) layout), HIP events around the Python call: the
                   kernel plus the wrapper's few small torch ops, i.e. device time INCLUDING host launch gaps; `match_kernel_ms` is the
                   events around the one owl_map_match launch alone
  compute          over --images such images (default 5000): HIP events and wall clock around compute() (it synchronises: sorts, one
                   owl_map_accumulate launch, the means)
  restatement      the numpy restatement (tests/coco_eval_restatement.py) on the FIRST --restatement-images images of the same data
                   (it is a slow loop nest; the per-image figure is extrapolated to the full set and labelled as such), with the core count
  forward + PostProcess of the same batch size (owlvit-base-patch16, batch 32, top_k = 200), HIP events: what the metric runs beside
  --shards W       the data-parallel merge beside the single state, same images: W in-process shards (images r::W, shard=(r, W)) merged with
                   merge_state, compute() of the merged state (HIP events + wall clock; four stable sorts over keyed records instead of two), and
                   two real gloo ranks on the one GPU (fresh child processes through torch.distributed.run): wall clock of the collective compute()
                   on rank 0, state staged through host memory

Nothing here is asserted; every figure is the median of 5 windows after warm-up.  The note beside the recorded line: profiles/eval_map.md."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from owl_vit_object_detection_amd import ops
from owl_vit_object_detection_amd.metrics import MeanAveragePrecision
from tests import coco_eval_restatement as R


def events_ms(fn, windows=5, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), out


def padded_batches(images, batch, K, G):
    """restatement-style images -> padded device batches in the PostProcess layout (detections sorted by descending score, -1 label pads)"""
    out = []
    for i0 in range(0, len(images), batch):
        chunk = images[i0:i0 + batch]
        B = len(chunk)
        boxes, scores, labels = np.zeros((B, K, 4), np.float32), np.zeros((B, K), np.float32), np.full((B, K), -1, np.int64)
        gtb, gtl = np.zeros((B, G, 4), np.float32), np.full((B, G), -1, np.int64)
        counts, gcounts = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b, im in enumerate(chunk):
            o = np.argsort(-im["det_scores"], kind="stable")
            im["det_boxes"], im["det_scores"], im["det_labels"] = im["det_boxes"][o], im["det_scores"][o], im["det_labels"][o]
            n, g = len(o), len(im["gt_labels"])
            boxes[b, :n], scores[b, :n], labels[b, :n], counts[b] = im["det_boxes"], im["det_scores"], im["det_labels"], n
            gtb[b, :g], gtl[b, :g], gcounts[b] = im["gt_boxes"], im["gt_labels"], g
        out.append(tuple(torch.from_numpy(a).cuda() for a in (boxes, labels, scores, counts, gtb, gtl, gcounts)))
    return out


def timed_compute(metric):
    """-> (HIP-event median ms, windows, wall-clock median ms, last result) of metric.compute() + synchronise"""
    walls = []

    def compute():
        t = time.perf_counter()
        compute.out = metric.compute()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t)
    ms, windows = events_ms(compute)
    return ms, windows, statistics.median(walls[-5:]) * 1e3, compute.out


def shard_metric(images, args, rank, world, **kw):
    m = MeanAveragePrecision(n_classes=args.classes, shard=(rank, world), **kw).to("cuda")
    for b in padded_batches(images[rank::world], args.batch, 200, 16):
        m.update_batched(*b)
    return m


def gloo_worker(args):
    """one of the two ranks started by shards_mode: its shard of the same images, the collective compute() timed on the wall clock"""
    from owl_vit_object_detection_amd import ddp
    rank, world, _ = ddp.init_from_env("gloo")
    images = R.random_eval_set(0, n_images=args.images, n_classes=args.classes, n_det=200)
    m = MeanAveragePrecision(n_classes=args.classes).to("cuda")          # shard and default image keys from the process group
    for b in padded_batches(images[rank::world], args.batch, 200, 16):
        m.update_batched(*b)
    _, _, wall_ms, out = timed_compute(m)
    if rank == 0:
        print(json.dumps({"gloo_ranks": world, "compute_wall_ms": round(wall_ms, 3), "map": float(out["map"]), "map_50": float(out["map_50"])}))
    torch.distributed.barrier(); torch.distributed.destroy_process_group()


def shards_mode(images, args, single_out):
    world = args.shards
    merged = shard_metric(images, args, 0, world)
    for r in range(1, world):
        merged.merge_state(shard_metric(images, args, r, world))
    ms, windows, wall_ms, out = timed_compute(merged)
    res = {"shards": world, "merged_compute_ms": round(ms, 3), "merged_compute_ms_windows": [round(x, 3) for x in windows], "merged_compute_wall_ms": round(wall_ms, 3),
           "merged_equals_single_bitwise": all(torch.equal(out[k], single_out[k]) for k in out)}
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "OWL_FORCE_DIST")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.abspath(__file__), "--gloo-worker", "--images", str(args.images), "--batch", str(args.batch), "--classes", str(args.classes)],
                       capture_output=True, text=True, env=env, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        res["two_gloo_ranks"] = {"error": r.stderr[-500:]}
    else:
        res["two_gloo_ranks"] = json.loads(lines[-1])
        res["two_gloo_ranks"]["map_equals_single"] = res["two_gloo_ranks"]["map"] == float(single_out["map"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--restatement-images", type=int, default=160)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--shards", type=int, default=0, help="also time the merged compute() of W in-process shards and of two gloo ranks")
    ap.add_argument("--gloo-worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gloo_worker:
        return gloo_worker(args)
    C = args.classes
    images = R.random_eval_set(0, n_images=args.images, n_classes=C, n_det=200)
    batches = padded_batches(images, args.batch, 200, 16)

    metric = MeanAveragePrecision(n_classes=C).to("cuda")
    first = batches[0]
    upd_ms, upd_all = events_ms(lambda: metric.update_batched(*first))
    scale = torch.ones(first[0].shape[0], 2, device="cuda")
    kern_ms, _ = events_ms(lambda: ops.map_match(first[0], first[2], first[1], first[3], first[4], first[5], first[6], scale, C))
    metric.reset()
    t0 = time.perf_counter()
    for b in batches:
        metric.update_batched(*b)
    torch.cuda.synchronize()
    all_updates_s = time.perf_counter() - t0
    cmp_ms, cmp_all, cmp_wall_ms, single_out = timed_compute(metric)
    summary = {k: round(float(v), 6) for k, v in single_out.items() if v.dim() == 0}

    n_ref = min(args.restatement_images, len(images))
    t0 = time.perf_counter()
    ref = R.evaluate(images[:n_ref], C)
    ref_s = time.perf_counter() - t0
    if n_ref == len(images):
        assert abs(ref["map"] - summary["map"]) < 1e-6, (ref["map"], summary["map"])

    fwd_ms = None
    if not args.no_forward:
        from owl_vit_object_detection_amd import synth
        from owl_vit_object_detection_amd.models import PostProcess, load_model
        model = load_model({str(i): i for i in range(C)}, "cuda", arch="owlvit-base-patch16").eval()
        img = torch.from_numpy(synth.make_images(model.cfg, args.batch)).cuda().to(torch.bfloat16)
        pp = PostProcess(0.01, 0.6)

        def fwd():
            with torch.no_grad():
                pb, _, ps, _ = model(img)
                pp(pb, ps, top_k=200)
        fwd_ms, _ = events_ms(fwd)

    line = {
        "what": "device COCO bbox mAP at eval-loop shapes", "device": torch.cuda.get_device_name(0), "images": len(images), "batch": args.batch, "classes": C,
        "detections_per_image": 200, "records": int(sum(int(b[3].sum()) for b in batches)),
        "update_batched_ms_per_batch": round(upd_ms, 4), "update_batched_ms_windows": [round(x, 4) for x in upd_all], "match_kernel_ms_per_batch": round(kern_ms, 4),
        "all_updates_wall_s": round(all_updates_s, 4), "compute_ms": round(cmp_ms, 3), "compute_ms_windows": [round(x, 3) for x in cmp_all],
        "compute_wall_ms": round(cmp_wall_ms, 3),
        "restatement_images": n_ref, "restatement_s": round(ref_s, 3), "restatement_s_extrapolated_to_all_images": round(ref_s / n_ref * len(images), 1),
        "restatement_cpu_cores_used": 1, "cpu_cores_available": len(os.sched_getaffinity(0)),
        "forward_plus_postprocess_ms_per_batch": None if fwd_ms is None else round(fwd_ms, 3), "summary": summary,
        "measured_under": "HIP events, median of 5 windows after 2 warm-up calls; *_wall_* = host perf_counter around a synchronised region",
    }
    if args.shards:
        line["data_parallel_merge"] = shards_mode(images, args, single_out)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
