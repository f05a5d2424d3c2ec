"""CPU: the float64 post-process reference of tests/postprocess_reference.py against the oracle and torch, and every claim its builders make.  No GPU:
what is pinned here is the CHECKER -- that the oracle takes the float64 decision at every decided pair on both routes and both dispatch rules, that the
cases compared against float64 have no undecided pair, and that each case really stands on the boundary it names."""
import numpy as np
import pytest
import torch

from oracle import owl_oracle as O
from tests import postprocess_reference as R

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_oracle_is(ref, boxes, sims, conf, thr, route, top_k=None):
    eb, ec, es, ei = O.post_process(boxes, sims, conf, thr, top_k=top_k, route=route)
    assert np.array_equal(ei, ref.patch), (route, len(ei), len(ref.patch))
    assert np.array_equal(ec, ref.classes)
    assert np.array_equal(bits(es), bits(ref.scores)) and np.array_equal(bits(eb), bits(ref.boxes))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the selection against torch itself
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SCORE_PROFILES)
def test_select_follows_torch(name):
    """torch.max(dim) -> strict > -> stable descending sort, on every score profile: values (bits), first arg-max, NaN rows, both zeros."""
    c = R.score_profile(name)
    s = torch.from_numpy(c["sims"])
    v, a = s.max(1)
    sel = torch.nonzero(v > torch.tensor(c["conf"], dtype=torch.float32))[:, 0]
    order = torch.sort(v[sel], descending=True, stable=True)[1]
    idx = sel[order].numpy()
    patch, cls, score = R.select(c["sims"], c["conf"])
    assert np.array_equal(patch, idx) and np.array_equal(patch, c["patch"])
    assert np.array_equal(cls, a[sel][order].numpy())
    assert np.array_equal(bits(score), bits(v[sel][order].numpy()))


def test_oracle_follows_torch_on_signed_zeros_and_nan():
    """The issue's two examples, and the profiles built from them."""
    z = np.asarray([[-0.0], [0.0], [-0.0]], f32)
    box = R.lattice_case(3, 1)["boxes"]
    _, _, es, ei = O.post_process(box, z, -0.5, 0.5)
    assert ei.tolist() == [0, 1, 2] and np.array_equal(bits(es), bits(z[:, 0]))           # patch order, input bits
    n = np.asarray([[0.3, np.nan], [np.nan, 0.2], [0.1, 0.0]], f32)
    v = torch.from_numpy(n).max(1)[0].numpy()
    assert np.isnan(v[0]) and np.isnan(v[1]) and v[2] == f32(0.1)
    _, _, _, ei = O.post_process(box, n, 0.0, 0.5)
    assert ei.tolist() == [2]
    for name in ("signed_zeros", "zero_columns", "nan", "inf_subnormal"):
        c = R.score_profile(name)
        for route in R.BASIC:
            ref = R.reference(c["boxes"], c["sims"], c["conf"], c["thr"], route)
            assert ref.undecided == 0 and np.array_equal(ref.patch, c["patch"])             # the lattice: NMS keeps the whole selection
            assert_oracle_is(ref, c["boxes"], c["sims"], c["conf"], c["thr"], route)


def test_score_profiles_reach_what_they_name():
    z = R.score_profile("signed_zeros")["sims"][:, 0]
    assert np.all(z == 0) and 10 < int(np.signbit(z).sum()) < len(z) - 10 and np.signbit(z[:3]).tolist() == [True, False, True]
    zc = R.score_profile("zero_columns")["sims"]
    assert {(bool(a), bool(b)) for a, b in np.signbit(zc)} == {(True, True), (True, False), (False, True), (False, False)}
    neg = R.score_profile("all_negative")
    assert neg["sims"].shape[1] == 1 and np.all(neg["sims"] < 0) and len(neg["patch"]) == len(neg["sims"])
    inf = R.score_profile("inf_subnormal")
    top = inf["sims"].max(1)
    assert np.isposinf(top).any() and np.isneginf(top).any() and (np.abs(top[top != 0]) < 1.1754944e-38).sum() >= 4
    nan = R.score_profile("nan")["sims"]
    assert np.isnan(nan[2, 0]) and np.isnan(nan[5, 1]) and not np.isnan(nan[5, 0]) and nan[5, 0] > 0 and np.isnan(nan[9]).all() and np.signbit(nan[11, 1])
    ce = R.score_profile("conf_edge")
    assert ce["sims"][4, 0] == f32(ce["conf"]) and ce["sims"][6, 0] == np.nextafter(f32(ce["conf"]), f32(1)) and ce["patch"][-1] == 6 and 4 not in ce["patch"]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the margin
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_margin_covers_f32_evaluations_and_no_more():
    """On random overlapping pairs, the f32 IoU in both association orders lies within the derived bound of the float64 value, and the bound is a few
    units of f32 round-off, not a loose constant."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for scale in (1.0, 1.0e4, 1.0e-3):
        c = rng.random((4000, 2)).astype(f32) * f32(0.5 * scale)
        wh = (rng.random((4000, 2)).astype(f32) * f32(0.5) + f32(0.05)) * f32(scale)
        b = np.concatenate([c, c + wh], 1).astype(f32)
        bi, bj = b[0], b[1:]
        iou, e, _ = R.pair_iou(bi.astype(np.float64), bj.astype(np.float64))
        w = np.maximum(f32(0), np.minimum(bi[2], bj[:, 2]) - np.maximum(bi[0], bj[:, 0]))
        h = np.maximum(f32(0), np.minimum(bi[3], bj[:, 3]) - np.maximum(bi[1], bj[:, 1]))
        inter = w * h
        ai, aj = (bi[2] - bi[0]) * (bi[3] - bi[1]), (bj[:, 2] - bj[:, 0]) * (bj[:, 3] - bj[:, 1])
        for union in ((ai + aj) - inter, ai + (aj - inter)):
            got = (inter / union).astype(np.float64)
            assert got.dtype == np.float64 and inter.dtype == f32
            m = iou > 0
            assert m.sum() > 100 and np.array_equal(got[~m], iou[~m])      # an empty intersection is exactly 0 in f32 too
            worst = max(worst, float(np.max(np.abs(got[m] - iou[m]) / e[m])))
        assert np.all(e[iou > 0] < 16 * R.F), float(e.max())
    assert 0.0 < worst <= 1.0, worst


def test_exact_pair_is_undecided_and_hand_decided():
    """[0,0,2,2] / [0,0,2,1]: IoU exactly 0.5 -- the reference must refuse to speak (1 undecided pair); the oracle keeps it at 0.5 and drops it one ulp below."""
    for name, kept in (("exact_half", 12), ("exact_half_below", 11)):
        c = R.box_profile(name)
        for route in R.BASIC:
            ref = R.reference(c["boxes"], c["sims"], c["conf"], c["thr"], route)
            assert ref.undecided == 1 and not c["decided"]
            _, _, _, ei = O.post_process(c["boxes"], c["sims"], c["conf"], c["thr"], route=route)
            assert np.array_equal(ei, c["patch"]) and len(ei) == kept
    # duplicates at thr 1.0 (HF's detect contract): IoU exactly 1, undecided for the float64 pin, never > 1 in f32
    c = R.box_profile("duplicates")
    ref = R.reference(c["boxes"], c["sims"], c["conf"], 1.0, "per_class")
    assert ref.undecided == 4           # (0, 1), (0, 2), (1, 2), (5, 7)
    assert O.post_process(c["boxes"], c["sims"], c["conf"], 1.0)[3].tolist() == list(range(12))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the oracle equals the float64 reference wherever it is decided
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.BOX_PROFILES)
def test_box_profiles(name):
    c = R.box_profile(name)
    for route in R.ROUTES:
        ref = R.reference(c["boxes"], c["sims"], c["conf"], c["thr"], route)
        assert ref.n == 12
        if c["decided"]:
            assert ref.undecided == 0
        if c["patch"] is not None:
            assert np.array_equal(ref.patch, c["patch"]), (route, ref.patch)
        assert_oracle_is(ref, c["boxes"], c["sims"], c["conf"], c["thr"], route)
    b = c["boxes"]
    if name == "zero_area":
        assert ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) == 0).sum() == 4
    if name == "negative":
        assert b.max() < -1 and len(set(c["sims"].argmax(1))) == 2
    if name == "pixel":
        assert b.max() > 1.0e5
    if name == "inverted":
        assert (b[:, 2] < b[:, 0]).sum() == 3 and (b[:, 3] < b[:, 1]).sum() == 2


@pytest.mark.parametrize("half", (False, True))
@pytest.mark.parametrize("P", R.TEMPLATE_P)
def test_template_cases(P, half):
    case, refs = R.template_case(P, half)
    n = (P + 1) // 2 if half else P
    for route, ref in refs.items():
        assert ref.n == n and ref.undecided == 0
        assert_oracle_is(ref, case["boxes"], case["sims"], case["conf"], case["thr"], route)
    if P >= 63:
        assert len(refs["per_class"].patch) < n            # something is suppressed: the case is not a sort test only
    if half and n < P:
        top = case["sims"].max(1)
        assert (top == f32(R.CONF)).sum() == 1 and (top == np.nextafter(f32(R.CONF), f32(1))).sum() == 1


@pytest.mark.parametrize("n", R.N_VALID)
def test_n_valid_cases(n):
    case, refs = R.cached_reference("random", 200, 3, 2000 + n, n, R.TEMPLATE_THR, R.BASIC)
    top = case["sims"].max(1)
    assert (top > f32(R.CONF)).sum() == n
    if 0 < n < 200:
        drop, keep = np.nonzero(top == f32(R.CONF))[0], np.nonzero(top == np.nextafter(f32(R.CONF), f32(1)))[0]
        assert len(drop) == 1 and len(keep) == 1
        assert drop[0] not in refs["per_class"].patch
    for route, ref in refs.items():
        assert ref.n == n and ref.undecided == 0
        assert_oracle_is(ref, case["boxes"], case["sims"], case["conf"], case["thr"], route)


@pytest.mark.parametrize("scene", sorted(R.SCAN_SCENES))
def test_scan_scenes(scene):
    """Sorted position k holds patch perm[k]; exactly the planted positions go, on both routes, and every pair is decided."""
    pairs, chains = R.SCAN_SCENES[scene]
    case, refs = R.cached_reference("lattice", R.SCAN_P, pairs, chains, R.BASIC)
    patch, _, score = R.select(case["sims"], case["conf"])
    assert np.array_equal(patch, case["perm"]) and np.all(np.diff(score.astype(np.float64)) < 0)
    gone = sorted(g[1] for g in pairs + chains)
    assert np.array_equal(case["kept"], np.setdiff1d(np.arange(R.SCAN_P), gone))
    for g in chains:
        assert g[2] in case["kept"]
        # b alone WOULD have suppressed c: drop a from the scene and c goes
        alone = R.lattice_case(R.SCAN_P, 3, ((g[1], g[2]),), ())
        assert g[2] not in alone["kept"]
        r = R.reference(alone["boxes"], alone["sims"], alone["conf"], alone["thr"], "per_class")
        assert np.array_equal(r.patch, alone["perm"][alone["kept"]])
    for route, ref in refs.items():
        assert ref.n == R.SCAN_P and ref.undecided == 0
        assert np.array_equal(ref.patch, case["perm"][case["kept"]])
        assert_oracle_is(ref, case["boxes"], case["sims"], case["conf"], case["thr"], route)


def test_scan_scenes_cover_the_issue():
    pairs = {p for ps, _ in R.SCAN_SCENES.values() for p in ps}
    assert pairs == {(0, 8191), (63, 64), (4095, 4096), (4096, 4097), (4031, 8191)}
    chains = [c for _, cs in R.SCAN_SCENES.values() for c in cs]
    assert (4095, 4096, 4160) in chains and any(min(c) > 4096 for c in chains)
    for ps, cs in R.SCAN_SCENES.values():
        used = [q for g in ps + cs for q in g]
        assert len(used) == len(set(used))


@pytest.mark.parametrize("n,route,taken", [(1000, "torchvision_cpu", "coordinate_offset"), (1001, "torchvision_cpu", "per_class"),
                                           (5000, "torchvision_gpu", "coordinate_offset"), (5001, "torchvision_gpu", "per_class")])
def test_far_cases_tell_the_routes_apart(n, route, taken):
    case, refs = R.cached_reference("far", n, 0, R.BASIC)
    assert (case["sims"].max(1) > f32(R.CONF)).sum() == n
    assert R.route_taken(route, n) == taken
    a, b = refs["per_class"], refs["coordinate_offset"]
    assert a.n == b.n == n and a.undecided == 0 and b.undecided == 0
    assert len(np.setxor1d(a.patch, b.patch)) >= 10                       # a dispatch test can tell them apart
    assert set(a.classes.tolist()) <= set(range(60, 91)) and case["boxes"].max() > 7000
    for r, ref in refs.items():
        assert_oracle_is(ref, case["boxes"], case["sims"], case["conf"], case["thr"], r)
    assert_oracle_is(refs[taken], case["boxes"], case["sims"], case["conf"], case["thr"], route)


def test_route_taken_is_torchvisions_rule():
    for n in (0, 1, 999, 1000, 1001, 4999, 5000, 5001, 8192):
        assert R.route_taken("torchvision_cpu", n) == ("per_class" if 4 * n > 4000 else "coordinate_offset")
        assert R.route_taken("torchvision_gpu", n) == ("per_class" if 4 * n > 20000 else "coordinate_offset")
        assert R.route_taken("per_class", n) == "per_class" and R.route_taken("coordinate_offset", n) == "coordinate_offset"


@pytest.mark.parametrize("C", (1, 257, 4096))
def test_wide_cases(C):
    boxes, sims, win = R.wide_case(150, C)
    assert win.max() == C - 1 and (C < 257 or (win > 255).any())
    for route in R.BASIC:
        ref = R.reference(boxes, sims, R.CONF, R.TEMPLATE_THR, route)
        assert ref.n == 150 and ref.undecided == 0 and len(ref.patch) < 150
        assert C - 1 in ref.classes and (C < 257 or (ref.classes > 255).sum() >= 2)
        assert_oracle_is(ref, boxes, sims, R.CONF, R.TEMPLATE_THR, route)


def test_batch_case_maxima_matter():
    bb, ss = R.batch_case()
    ns = [R.reference(bb[i], ss[i], R.CONF, R.TEMPLATE_THR, "coordinate_offset") for i in range(4)]
    assert [r.n for r in ns] == [0, 200, 1, 70] and all(r.undecided == 0 for r in ns)
    assert bb[1].max() < 1.5 and 4000 < bb[3].max() < 6000
    for i, j in ((1, 3), (3, 1)):     # with the other image's maximum as the step the float64 list changes (and is still decided)
        other = R.reference(bb[i], ss[i], R.CONF, R.TEMPLATE_THR, "coordinate_offset", max_coord=bb[j].max())
        assert other.undecided == 0 and not np.array_equal(other.patch, ns[i].patch)
    for i in range(4):
        for route in R.BASIC:
            ref = R.reference(bb[i], ss[i], R.CONF, R.TEMPLATE_THR, route)
            assert ref.undecided == 0
            assert_oracle_is(ref, bb[i], ss[i], R.CONF, R.TEMPLATE_THR, route)


def test_existing_generator_is_decided():
    """The generator of tests/test_postprocess_gpu.py at model sizes: 0 undecided pairs, float64 greedy equals the oracle, both routes."""
    from tests.test_postprocess_gpu import _case
    for P, C, conf, thr in ((2304, 10, 0.01, 0.6), (3600, 91, 0.01, 0.6)):
        boxes, sims = _case(P, C, seed=P + C)
        for route in R.BASIC:
            ref = R.reference(boxes, sims, conf, thr, route)
            assert ref.undecided == 0
            assert_oracle_is(ref, boxes, sims, conf, thr, route)


def test_top_k_is_a_prefix():
    case, refs = R.cached_reference("random", 200, 3, 2200, 200, R.TEMPLATE_THR, R.BASIC)
    full = refs["per_class"]
    for k in (1, 7, 8, 9, len(full.patch) - 1, len(full.patch), len(full.patch) + 1, 200):
        ref = R.reference(case["boxes"], case["sims"], case["conf"], case["thr"], "per_class", top_k=k)
        assert np.array_equal(ref.patch, full.patch[:k])
        assert_oracle_is(ref, case["boxes"], case["sims"], case["conf"], case["thr"], "per_class", top_k=k)
