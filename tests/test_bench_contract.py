"""CPU-side checks of bench.py's bookkeeping (no GPU): the counter-traffic file it quotes as `roofline.traffic` was measured on THESE kernel sources, the
`cpu_baseline` leg produces the fields the contract names, a plain run measures the headline alone (the rest behind --full), and --dump-outputs writes
float32 arrays with a fixed seeded sample of the large ones."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench_mod():
    argv = sys.argv
    sys.argv = ["bench.py"]
    try:
        sys.path.insert(0, ROOT)
        import bench
        return bench
    finally:
        sys.argv = argv


def test_traffic_file_is_bound_to_the_shipped_kernel_sources(bench_mod):
    """`roofline.traffic` is a PMC figure taken in separate rocprofv3 passes (tools/run_profiles_r06.sh) and read from profiles/: bench.py refuses it (traffic =
    null) when the kernel sources changed since.  This test makes that refusal visible BEFORE a round ends: edit a kernel -> re-run the traffic passes."""
    t = json.load(open(os.path.join(ROOT, bench_mod.TRAFFIC_FILE)))
    assert t["kernel_source_digest"] == bench_mod.kernel_source_digest(), (
        f"{bench_mod.TRAFFIC_FILE} was measured on other kernel sources: re-run tools/run_profiles_r06.sh on a GPU box and copy gpurun_out/r6_traffic.json over it")
    assert bench_mod.TRAFFIC_NOTE is None
    for wl in ("owlvit-base-patch16/32", "owlvit-large-patch14/16"):
        assert set(t["workloads"][wl]) == {bench_mod.LABEL_BIAS, bench_mod.LABEL_QGELU, bench_mod.LABEL_ATTN}
        assert all(1e8 < v < 5e9 for v in t["workloads"][wl].values())


def test_cpu_baseline_leg_fields(bench_mod):
    from owl_vit_object_detection_amd.config import get_config
    out = bench_mod.cpu_baseline(get_config("tiny"), 5)
    assert out["kind"] == "port" and out["unit"] == "images/sec" and out["value"] > 0 and 1 <= out["cores"] <= (os.cpu_count() or 1)
    assert "AdamW" in out["sample"] and "median" in out["sample"]


def test_plain_run_is_the_headline_alone_and_full_keeps_the_rest(bench_mod):
    """A plain run times ONE window of exactly --steps steps and measures nothing else; --full brings back the 5 windows, HIP events, CPU baseline and the
    comparison runs, each still switchable off on its own."""
    a = bench_mod.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.steps, a.warmup, a.windows, a.dump_outputs) == (False, 7, 2, 1, None)
    assert a.no_cpu_baseline and a.no_compare and a.no_kernel_events
    f = bench_mod.parse(["--full", "--steps", "7"])
    assert f.full and f.windows == 5 and not (f.no_cpu_baseline or f.no_compare or f.no_kernel_events)
    f = bench_mod.parse(["--full", "--no-cpu-baseline", "--no-compare", "--windows", "2"])
    assert f.no_cpu_baseline and f.no_compare and not f.no_kernel_events and f.windows == 2
    assert bench_mod.parse(["--windows", "3", "--dump-outputs", "d"]).windows == 3 and bench_mod.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_dump_outputs_float32_with_a_fixed_seeded_sample(bench_mod, tmp_path):
    import numpy as np
    import torch
    n_big = bench_mod.DUMP_SAMPLE_ELEMS + 12345
    big = torch.arange(n_big, dtype=torch.float64).reshape(1, -1)          # (a float64 2-D array: flattened, sampled, written as float32)
    small = torch.randn(3, 4, 2, dtype=torch.float32)
    arrays = {"pred_boxes": small, "loss": torch.tensor(1.5, dtype=torch.float32), "params": big, "half": torch.ones(6, dtype=torch.bfloat16)}
    w1 = bench_mod.dump_outputs(str(tmp_path / "a"), arrays)
    w2 = bench_mod.dump_outputs(str(tmp_path / "b"), arrays)
    assert w1 == w2 == {"pred_boxes.npy": [3, 4, 2], "loss.npy": [], "params_sample.npy": [bench_mod.DUMP_SAMPLE_ELEMS], "half.npy": [6]}
    total = 0
    for name in w1:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype == np.float32 and np.array_equal(x, y), name
        total += os.path.getsize(tmp_path / "a" / name)
    assert total <= bench_mod.DUMP_BUDGET_BYTES
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "pred_boxes.npy"), small.numpy())
    s = np.load(tmp_path / "a" / "params_sample.npy")
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < n_big           # ascending, distinct indices of the flattened array (its values ARE the indices)
    idx = np.sort(np.random.default_rng(bench_mod.DUMP_SAMPLE_SEED).choice(n_big, bench_mod.DUMP_SAMPLE_ELEMS, replace=False))
    np.testing.assert_array_equal(s, idx.astype(np.float32))
