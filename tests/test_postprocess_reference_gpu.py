"""-m gpu: owl_postprocess (csrc/postprocess.hip: pp_sort_kernel, pp_mask_kernel, pp_scan_kernel) against the float64 reference of
tests/postprocess_reference.py and the oracle, at the sort templates' and the scan's word edges, torchvision's dispatch boundaries, the wide class axis,
the score / box edge profiles, top_k, one batched call, a poisoned exact-size workspace and the wrapper's contract.

Everything is exact: patch indices, classes, counts, and the BITS of scores and boxes (they are copies of inputs).  A case is compared against float64 only
when the reference has 0 undecided pairs (asserted); then any correct f32 evaluation must return that list.  Cases on the threshold are compared with the
oracle and with hand-written expectations.  Every call is made twice and must give the same bits.

Findings of the first run on an MI355X (profiles/postprocess_reference.md): with the sort kernel as it was, `signed_zeros`, `zero_columns` (every +0.0 sorted
before every -0.0) and `nan` (a NaN in a later column skipped by `v > best`) failed, as read from the code beforehand; nothing else did."""
import numpy as np
import pytest
import torch

from oracle import owl_oracle as O
from tests import postprocess_reference as R

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def raw(boxes, sims, conf, thr, route, max_out=None):
    """ops.postprocess on [B, P, ...] numpy inputs -> padded numpy outputs (boxes, classes, scores, patch, counts)."""
    from owl_vit_object_detection_amd import ops
    b = torch.from_numpy(np.ascontiguousarray(boxes, f32)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(sims, f32)).cuda()
    if b.dim() == 2:
        b, s = b[None], s[None]
    out = ops.postprocess(b, s, int(max_out or b.shape[1]), float(conf), float(thr), route)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def assert_padded(out, i, k, max_out):
    ob, oc, os_, op, cnt = out
    assert cnt[i] == k and ob.shape[1] == max_out
    assert np.all(oc[i, k:] == -1) and np.all(op[i, k:] == -1) and np.all(bits(os_[i, k:]) == 0) and np.all(bits(ob[i, k:]) == 0)


def assert_is(out, i, patch, classes, scores, boxes, what=""):
    ob, oc, os_, op, cnt = out
    k = len(patch)
    assert cnt[i] == k, (what, int(cnt[i]), k)
    assert np.array_equal(op[i, :k], patch), what
    assert np.array_equal(oc[i, :k], classes), what
    assert np.array_equal(bits(os_[i, :k]), bits(scores)) and np.array_equal(bits(ob[i, :k]), bits(boxes)), what
    assert oc.dtype == np.int64 and op.dtype == np.int64


def run_checked(boxes, sims, conf, thr, route, ref=None, oracle=True, max_out=None):
    """One image: two runs with the same bits; equals `ref` (a Result with 0 undecided pairs) and the oracle.  -> the padded outputs."""
    out = raw(boxes, sims, conf, thr, route, max_out)
    again = raw(boxes, sims, conf, thr, route, max_out)
    for a, b in zip(out, again):
        assert same(a, b)
    mo = max_out or len(boxes)
    if ref is not None:
        assert ref.undecided == 0
        assert_is(out, 0, ref.patch[:mo], ref.classes[:mo], ref.scores[:mo], ref.boxes[:mo], "float64 reference")
    if oracle:
        eb, ec, es, ei = O.post_process(boxes, sims, conf, thr, top_k=mo, route=route)
        assert_is(out, 0, ei, ec, es, eb, "oracle")
    assert_padded(out, 0, int(out[4][0]), mo)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", R.BASIC)
@pytest.mark.parametrize("half", (False, True))
@pytest.mark.parametrize("P", R.TEMPLATE_P)
def test_template_and_word_edges(P, half, route):
    """Both sides of the 1024 / 4096 / 8192-key sort templates (the p + 1 == P end-of-list rule at P = NP) and of the scan's 64-bit words and remv0 / remv1
    split, with every row past the threshold and with half of them."""
    case, refs = R.template_case(P, half, (route,))
    assert refs[route].n == ((P + 1) // 2 if half else P)
    run_checked(case["boxes"], case["sims"], case["conf"], case["thr"], route, refs[route])


@pytest.mark.parametrize("route", R.BASIC)
@pytest.mark.parametrize("n", R.N_VALID)
def test_n_valid_edges(n, route):
    """Exactly n of 200 rows past the threshold; the row equal to it is dropped and its one-ulp twin kept (the CPU test shows both are there)."""
    case, refs = R.cached_reference("random", 200, 3, 2000 + n, n, R.TEMPLATE_THR, R.BASIC)
    out = run_checked(case["boxes"], case["sims"], case["conf"], case["thr"], route, refs[route])
    if 0 < n < 200:
        top = case["sims"].max(1)
        kept = set(out[3][0, :out[4][0]].tolist())
        assert int(np.nonzero(top == f32(R.CONF))[0][0]) not in kept
    assert refs[route].n == n


@pytest.mark.parametrize("route", R.BASIC)
@pytest.mark.parametrize("scene", sorted(R.SCAN_SCENES))
def test_scan_lanes(scene, route):
    """P = n = 8192 on the lattice: suppressing pairs at sorted positions (0, 8191), (63, 64), (4095, 4096), (4096, 4097), (4031, 8191); the chain 4095 ->
    4096 -/-> 4160 across the removed set's word split and its mirror above it: exactly the planted positions go."""
    pairs, chains = R.SCAN_SCENES[scene]
    case, refs = R.cached_reference("lattice", R.SCAN_P, pairs, chains, R.BASIC)
    out = run_checked(case["boxes"], case["sims"], case["conf"], case["thr"], route, refs[route])
    assert np.array_equal(out[3][0, :out[4][0]], case["perm"][case["kept"]])


@pytest.mark.parametrize("n,route,taken", [(1000, "torchvision_cpu", "coordinate_offset"), (1001, "torchvision_cpu", "per_class"),
                                           (5000, "torchvision_gpu", "coordinate_offset"), (5001, "torchvision_gpu", "per_class")])
def test_torchvision_dispatch(n, route, taken):
    """numel = 4 n on either side of 4000 (CPU rule) and 20000 (GPU rule): the result is the float64 list of the route torchvision takes at that n; the
    other route's list differs by >= 10 entries (tests/test_postprocess_reference.py)."""
    case, refs = R.cached_reference("far", n, 0, R.BASIC)
    other = refs["per_class" if taken == "coordinate_offset" else "coordinate_offset"]
    assert not np.array_equal(other.patch, refs[taken].patch)
    run_checked(case["boxes"], case["sims"], case["conf"], case["thr"], route, refs[taken])
    run_checked(case["boxes"], case["sims"], case["conf"], case["thr"], taken, refs[taken], oracle=False)


@pytest.mark.parametrize("route", R.BASIC)
@pytest.mark.parametrize("C", (1, 257, 4096))
def test_wide_class_axis(C, route):
    """detect's query axis: winners above 255 and at C - 1 in the key's 16-bit class field; the shifted route's offset at class 4095."""
    boxes, sims, _ = R.wide_case(150, C)
    ref = R.reference(boxes, sims, R.CONF, R.TEMPLATE_THR, route)
    out = run_checked(boxes, sims, R.CONF, R.TEMPLATE_THR, route, ref)
    assert out[1][0, :out[4][0]].max() == C - 1


@pytest.mark.parametrize("route", R.BASIC)
@pytest.mark.parametrize("name", R.SCORE_PROFILES)
def test_score_profiles(name, route):
    """all equal | -0.0 / +0.0 across rows (conf = -1) and inside a row | all negative, C = 1 | +-inf and subnormals | NaN in column 0, in a later column,
    everywhere | equal to conf and one ulp either side -- against the hand-written selection, the float64 reference and the oracle."""
    c = R.score_profile(name)
    ref = R.reference(c["boxes"], c["sims"], c["conf"], c["thr"], route)
    assert np.array_equal(ref.patch, c["patch"])
    out = run_checked(c["boxes"], c["sims"], c["conf"], c["thr"], route, ref)
    assert np.array_equal(out[3][0, :out[4][0]], c["patch"])
    # conf = +inf: nothing passes, nothing is written
    out = run_checked(c["boxes"], c["sims"], np.inf, c["thr"], route, R.reference(c["boxes"], c["sims"], np.inf, c["thr"], route))
    assert out[4][0] == 0


@pytest.mark.parametrize("route", R.BASIC)
@pytest.mark.parametrize("name", R.BOX_PROFILES)
def test_box_profiles(name, route):
    """zero area | duplicates | inverted | all negative | pixel scale | the exact 0.5 pair at thr 0.5 and one ulp below."""
    c = R.box_profile(name)
    ref = R.reference(c["boxes"], c["sims"], c["conf"], c["thr"], route)
    out = run_checked(c["boxes"], c["sims"], c["conf"], c["thr"], route, ref if c["decided"] else None)
    if c["patch"] is not None:
        assert np.array_equal(out[3][0, :out[4][0]], c["patch"])


def test_top_k_prefix_and_padding():
    case, refs = R.cached_reference("random", 200, 3, 2200, 200, R.TEMPLATE_THR, R.BASIC)
    for route in R.BASIC:
        full = refs[route]
        kept = len(full.patch)
        assert 9 < kept - 1 and kept + 1 < 200
        for k in (1, 7, 8, 9, kept - 1, kept, kept + 1, 200):
            out = run_checked(case["boxes"], case["sims"], case["conf"], case["thr"], route, full, oracle=(k in (1, 8, kept)), max_out=k)
            assert out[4][0] == min(k, kept)


def test_batch_is_per_image():
    """B = 4 in one call, n = (0, P, 1, 70), per-image maxima ~1 and ~5000 on the coordinate-offset route (another image's max_coord would change the float64
    list: CPU test): each image equals its reference and its own single-image run bit for bit, at either batch position."""
    bb, ss = R.batch_case()
    for route in R.BASIC:
        refs = [R.reference(bb[i], ss[i], R.CONF, R.TEMPLATE_THR, route) for i in range(4)]
        assert [r.n for r in refs] == [0, 200, 1, 70]
        out = raw(bb, ss, R.CONF, R.TEMPLATE_THR, route)
        perm = [3, 0, 1, 2]
        moved = raw(bb[perm], ss[perm], R.CONF, R.TEMPLATE_THR, route)
        for i, r in enumerate(refs):
            assert r.undecided == 0
            assert_is(out, i, r.patch, r.classes, r.scores, r.boxes, f"image {i}")
            assert_padded(out, i, len(r.patch), 200)
            single = raw(bb[i], ss[i], R.CONF, R.TEMPLATE_THR, route)
            j = perm.index(i)
            for a, b, c in zip(out, single, moved):
                assert same(a[i], b[0]) and same(a[i], c[j])
    # the wrapper's batched surface: padded to the longest list, counts in last_counts
    from owl_vit_object_detection_amd.postprocess import PostProcess
    pp = PostProcess(R.CONF, R.TEMPLATE_THR, nms_route="coordinate_offset")
    ob, oc, os_ = pp(torch.from_numpy(bb).cuda(), torch.from_numpy(ss).cuda())
    cnt = pp.last_counts.cpu().numpy()
    assert cnt.tolist() == [len(r.patch) for r in refs] and ob.shape == (4, cnt.max(), 4) and oc.shape == os_.shape == (4, cnt.max())
    assert np.array_equal(pp.last_patch_idx[3, :cnt[3]].cpu().numpy(), refs[3].patch) and np.all(oc[2, 1:].cpu().numpy() == -1)


def test_workspace_and_guards():
    """Through the C ABI: a workspace of exactly owl_postprocess_workspace bytes, poisoned with 0xFF and then left dirty by a larger-n run; outputs inside
    sentinel-filled buffers.  Same results, tail and guards untouched."""
    from owl_vit_object_detection_amd import _lib, ops
    P, G, TAIL = 200, 64, 4096
    big, refs_big = R.cached_reference("random", P, 3, 2200, 200, R.TEMPLATE_THR, R.BASIC)
    small, refs_small = R.cached_reference("random", P, 3, 2065, 65, R.TEMPLATE_THR, R.BASIC)
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_postprocess_workspace", 1, P, nbytes)
    nbytes = int(nbytes.item())
    ws = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(case, route, fill):
        if fill is not None:
            ws[:nbytes] = fill
        b = torch.from_numpy(case["boxes"]).cuda()
        s = torch.from_numpy(case["sims"]).cuda()
        ob = torch.full((G + P * 4 + G,), -7.0, device="cuda")
        os_ = torch.full((G + P + G,), -7.0, device="cuda")
        oc = torch.full((G + P + G,), -7, dtype=torch.int64, device="cuda")
        op = torch.full((G + P + G,), -7, dtype=torch.int64, device="cuda")
        cnt = torch.full((G + 1 + G,), -7, dtype=torch.int32, device="cuda")
        _lib.call("owl_postprocess", ops.stream(), b, s, ws, nbytes, ob[G:], os_[G:], oc[G:], op[G:], cnt[G:], 1, P, 3, P,
                  float(case["conf"]), float(case["thr"]), ops.NMS_ROUTES[route])
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all()), "workspace tail written"
        k = int(cnt[G])
        for t, w in ((ob, 4), (os_, 1), (oc, 1), (op, 1)):      # the C entry writes k rows and nothing else: no padding, no guard
            assert bool((t[:G] == -7).all()) and bool((t[G + k * w:] == -7).all())
        assert bool((cnt[:G] == -7).all()) and bool((cnt[G + 1:] == -7).all())
        return (ob[G:G + 4 * k].reshape(1, k, 4).cpu().numpy(), oc[G:G + k][None].cpu().numpy(), os_[G:G + k][None].cpu().numpy(),
                op[G:G + k][None].cpu().numpy(), np.asarray([k], np.int32))

    for route in R.BASIC:
        r = refs_small[route]
        for fill in (0xFF, 0x00):
            assert_is(call(small, route, fill), 0, r.patch, r.classes, r.scores, r.boxes, f"fill {fill:#x}")
        assert_is(call(big, route, None), 0, refs_big[route].patch, refs_big[route].classes, refs_big[route].scores, refs_big[route].boxes, "larger n")
        assert_is(call(small, route, None), 0, r.patch, r.classes, r.scores, r.boxes, "after a larger-n run")
    with pytest.raises(_lib.OwlLibError, match="workspace"):
        _lib.call("owl_postprocess", ops.stream(), ws, ws, ws, nbytes - 1, ws, ws, ws, ws, ws, 1, P, 3, P, 0.0, 0.5, 0)


def test_hf_contract_threshold_one():
    """model.detect's documented post-process, PostProcess(confidence_threshold=t, iou_threshold=1.0), at P = 576 with 4096 queries as the class axis: every row
    past t is kept, exact duplicates included (their f32 IoU is exactly 1, never > 1); masked scores of exactly 0 are dropped at any t >= 0."""
    rng = np.random.default_rng(7)
    P, C = 576, 4096
    boxes, _ = R.random_case(P, 1, 7, cluster=True)
    boxes[1::4] = boxes[0:-1:4]                                              # exact duplicates ...
    sims = (rng.random((P, C)).astype(f32) * f32(0.2)).astype(f32)
    sims[rng.random((P, C)) < 0.5] = 0.0                                      # masked queries
    win = rng.integers(0, C, P)
    win[:8] = (4095, 4095, 256, 256, 0, 0, 4094, 4094)
    sims[np.arange(P), win] = (f32(0.3) + rng.random(P).astype(f32) * f32(0.6)).astype(f32)
    sims[1::4] = sims[0:-1:4]                                                # ... with the same scores and classes
    sims[10::16] = 0.0                                                       # rows masked everywhere
    sims[11::32] = -0.0
    for t in (0.0, 0.25):
        patch, cls, score = R.select(sims, t)
        assert len(patch) == P - len(sims[10::16]) - len(sims[11::32]) and (cls == 4095).any()
        for route in R.BASIC + ("torchvision_gpu",):
            out = run_checked(boxes, sims, t, 1.0, route)
            assert_is(out, 0, patch, cls, score, boxes[patch], "every row past the threshold")


def test_wrapper_contract():
    from owl_vit_object_detection_amd import _lib
    from owl_vit_object_detection_amd.postprocess import PostProcess
    boxes, sims = R.random_case(200, 3, 2200)
    b = torch.from_numpy(boxes).bfloat16().float().cuda()                    # bf16-representable values
    s = torch.from_numpy(sims).bfloat16().float().cuda()
    pp = PostProcess(R.CONF, R.TEMPLATE_THR, nms_route="per_class")
    want = [t.clone() for t in pp(b[None], s[None])] + [pp.last_patch_idx.clone()]
    assert want[0].shape[0] == 1 and 0 < want[0].shape[1] < 200
    wide_b = torch.zeros(200, 8, device="cuda"); wide_b[:, ::2] = b
    wide_s = torch.zeros(3, 200, device="cuda"); wide_s[:] = s.t()
    for name, (xb, xs) in dict(bf16=(b[None].bfloat16(), s[None].bfloat16()), strided=(wide_b[:, ::2][None], wide_s.t()[None]), two_d=(b, s)).items():
        assert name != "strided" or not (xb.is_contiguous() or xs.is_contiguous())
        got = list(pp(xb, xs)) + [pp.last_patch_idx]
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g.view(torch.uint8), w.view(torch.uint8)), name
    with pytest.raises(_lib.OwlLibError, match="8192"):
        pp(torch.zeros(1, 8193, 4, device="cuda"), torch.zeros(1, 8193, 2, device="cuda"))
    with pytest.raises(_lib.OwlLibError, match="65536"):
        pp(torch.zeros(1, 4, 4, device="cuda"), torch.zeros(1, 4, 65536, device="cuda"))
