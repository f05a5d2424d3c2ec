"""CPU: tests/image_query_reference.py against HF (fixture f14 and, when it imports, live transformers), the order-faithful emulation of
csrc/image_query.hip inside the derived bounds on every profile, every planted error caught, and the caps on what the bounds may leave undecided."""
import os

import numpy as np
import pytest
import torch

from tests import image_query_reference as R

CPU_CASES = [c for c in R.GPU_CASES if c[1] <= 3600]          # (the 8192-patch shape adds no path: it is the GPU file's)


def _refs(N, P, Dt, profile):
    e, boxes, qbox = R.make_case(profile, N, P, Dt)
    return e, boxes, qbox, [R.exact_select(e[n], boxes[n], qbox[n]) for n in range(N)]


@pytest.fixture(scope="module")
def f14(golden_dir):
    return np.load(os.path.join(golden_dir, "f14_image_query.npz"))


def test_restatement_reproduces_fixture_f14(f14):
    """HF's own embed_image_query (recorded by tests/golden/make_golden_image_queries.py): same indices, same embeddings, all 6 decided."""
    ce, boxes = torch.from_numpy(f14["class_embeds"]), torch.from_numpy(f14["boxes"])
    assert ce.shape[0] == 6
    for n in range(6):
        r = R.exact_select(ce[n], boxes[n], None)
        assert r["decided"], (n, float(r["margin_v"].min()), r["margin_best"])
        assert r["best"] == int(f14["box_indices"][n]) and not r["fallback"]
        assert torch.equal(ce[n, r["best"]], torch.from_numpy(f14["query_embeds"][n]))
        out = R.emulate_select(ce[n], boxes[n], None)
        assert out["best"] == r["best"]


def test_restatement_reproduces_live_hf():
    pytest.importorskip("transformers")
    from tests.golden.make_golden_image_queries import hf_case
    case = hf_case(seed=3)
    for n in range(case["class_embeds"].shape[0]):
        r = R.exact_select(torch.from_numpy(case["class_embeds"][n]), torch.from_numpy(case["boxes"][n]), None)
        if r["decided"]:
            assert r["best"] == int(case["box_indices"][n])
        else:          # HF itself runs in f32: inside the bounds its choice is as good as the restatement's
            assert bool((r["sel"] | ~r["decided_mem"])[int(case["box_indices"][n])])


@pytest.mark.parametrize("N,P,Dt,profile", CPU_CASES)
def test_emulation_stays_inside_the_bounds(N, P, Dt, profile):
    e, boxes, qbox, refs = _refs(N, P, Dt, profile)
    worst = dict(v=0.0, mean=0.0, sim=0.0)
    for n in range(min(N, 6)):
        r = R.check_select(f"{profile} ({N}, {P}, {Dt}) exemplar {n}", R.emulate_select(e[n], boxes[n], qbox[n]), refs[n], e[n])
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"emulation {profile} ({N}, {P}, {Dt}): worst err / tol v {worst['v']:.3f} mean {worst['mean']:.3f} sim {worst['sim']:.3f}")


def test_profiles_reach_what_they_name():
    e, boxes, qbox, refs = _refs(3, 36, 64, "touching")
    for r in refs:          # every number of the touching pair is exact: the outcome is a fact of exact arithmetic, whatever the bounds leave open
        assert r["fallback"] and r["nsel"] == 1 and r["best"] == 12 and float(r["v"][12]) == 0.0 and float(r["v"].max()) == 0.0
    for n in range(3):
        out = R.emulate_select(e[n], boxes[n], qbox[n])
        assert out["best"] == 12 and out["nsel"] == 1 and out["flags"] == R.FLAG_FALLBACK
    for r in _refs(3, 36, 64, "disjoint")[3]:
        assert r["fallback"] and r["empty"] and r["best"] == -1 and float(r["v"].max()) < 0 and r["decided"]
    e, boxes, qbox, refs = _refs(5, 577, 512, "ties")
    for n, r in enumerate(refs):
        assert r["nsel"] == 577 and not r["decided"] and r["margin_best"] == 0.0 and r["best"] % 2 == 0          # the minimum is an exact tie: the lower index
        assert torch.equal(e[n, r["best"]], e[n, r["best"] + 1])
    for n, r in enumerate(_refs(5, 577, 512, "near_thr")[3]):
        if n % 5 == 0:          # boxes the bounds cannot place: the accept-either path
            assert int((~r["decided_mem"]).sum()) >= 1 and float(r["margin_v"].min()) <= 8 * R.F
        else:                   # near the threshold, on both sides, and decided
            assert bool(r["decided_mem"].all()) and float(r["margin_v"].min()) <= 100 * R.F and 2 <= r["nsel"] <= 7
    for r in _refs(2, 2304, 512, "offset")[3]:
        assert float(r["sim"].abs().min()) > 1e3 * max(r["margin_best"], 1e-30) or r["margin_best"] < 1.0          # sims far larger than their gaps


HOOK_CASES = [("thr075", "randn", 70, 36, 64), ("argmax", "randn", 70, 36, 64), ("mean_selected", "randn", 70, 36, 64), ("tie_last", "ties", 3, 36, 64),
              ("no_fallback", "touching", 3, 36, 64), ("union_no_inter", "randn", 70, 36, 64), ("f32_accum", "randn", 2, 3600, 768)]


@pytest.mark.parametrize("hook,profile,N,P,Dt", HOOK_CASES)
def test_planted_error_is_caught(hook, profile, N, P, Dt):
    e, boxes, qbox, refs = _refs(N, P, Dt, profile)
    caught = 0
    for n in range(N):
        fails = []
        R.check_select(f"{hook} {n}", R.emulate_select(e[n], boxes[n], qbox[n], hooks=(hook,)), refs[n], e[n], fails)
        caught += bool(fails)
        if hook == "f32_accum":          # must breach the f64 BOUND itself, not merely flip a decision
            assert any(" mean:" in f or " sim:" in f for f in fails), fails
    print(f"planted {hook}: caught on {caught} of {N} exemplars")
    assert caught >= (N if hook in ("tie_last", "no_fallback", "union_no_inter", "f32_accum", "mean_selected") else 1)


@pytest.mark.parametrize("N,P,Dt,profile", [c for c in R.GPU_CASES if c[3] in R.UNDECIDED_CAP])
def test_reference_alone_meets_the_caps(N, P, Dt, profile):
    """A condition, not a measurement: on randn EVERY exemplar is decided (no membership and no argmin left to the bounds); near_thr and offset leave at
    most a quarter undecided."""
    share, m_thr, m_best = R.undecided_share(profile, N, P, Dt)
    print(f"{profile} ({N}, {P}, {Dt}): undecided {share:.2f}, worst threshold margin {m_thr:.3e}, worst argmin margin {m_best:.3e}")
    assert share <= R.UNDECIDED_CAP[profile]


def test_bank_reference_rows():
    g = torch.Generator().manual_seed(2)
    q = torch.randn(5, 64, generator=g)
    old = torch.randn(4, 64, generator=g)
    ref, tol = R.exact_bank(q, [[0], [], [1, 4], [0, 1, 2, 3, 4]], old)
    assert torch.equal(ref[1], old[1].double()) and float(tol[1].max()) == 0.0
    assert torch.allclose(ref[0], q[0].double() / q[0].double().norm())
    assert torch.allclose(torch.linalg.norm(ref[[0, 2, 3]], dim=-1), torch.ones(3, dtype=torch.float64))
