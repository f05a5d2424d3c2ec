"""-m gpu: owl_class_logits_fwd (csrc/open_vocab.hip) on a real MI355X, kernel level.

Random e, features, banks and head weights (tests/open_vocab_reference.make_inputs) on the shapes of R.GPU_CASES, everything against the float64
reference inside the derived bound (no fitted tolerance); each case prints its worst err / tol, profiles/open_vocab_reference.md records them.  The
bitwise properties -- an image's block wherever it stands in a batch, a query's column wherever it stands in a bank, a shared bank against its
copies, masked entries, all-zero rows, two runs, guard rows and columns -- are torch.equal, no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402
from tests import open_vocab_reference as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = -12345.0


def _dev(i):
    return {k: (None if v is None else v.to(DEV)) for k, v in i.items()}


def _run(i, B, P, masked=True, scores=True, queries=None, mask=None):
    """ops.class_logits on device copies of make_inputs' tensors -> (logits, scores, rowstats) on the CPU."""
    d = _dev(i)
    q = d["queries"] if queries is None else queries.to(DEV)
    m = (d["mask"] if masked else None) if mask is None else mask.to(DEV)
    lg, sc, rs = ops.class_logits(d["e"], q, d["feats"], d["w_shift"], d["b_shift"], d["w_scale"], d["b_scale"], B, P, mask=m, scores=scores)
    torch.cuda.synchronize()
    return lg.cpu(), (None if sc is None else sc.cpu()), rs.cpu()


@pytest.fixture(scope="module")
def cases():
    """Inputs and float64 references, made once and shared."""
    out = {}
    for c in R.GPU_CASES:
        i = R.make_inputs(*c, seed=0)
        out[c] = (i, R.exact_logits(i["e"], i["queries"], i["feats"], i["w_shift"], i["b_shift"], i["w_scale"], i["b_scale"], c[0], c[1], i["mask"]))
    return out


@pytest.mark.parametrize("case", R.GPU_CASES)
def test_against_float64_inside_the_derived_bound(cases, case):
    B, P, Q, Dt, D = case
    i, r = cases[case]
    d = _dev(i)
    # guard rows and columns: the outputs are the interior of sentinel-filled buffers ([B, P + 2, Q] would break the layout, so: one buffer per output
    # with a guard image in front and behind, and the rowstats scratch with guard rows)
    lg_buf = torch.full((B + 2, P, Q), SENT, device=DEV)
    sc_buf = torch.full((B + 2, P, Q), SENT, device=DEV)
    rs_buf = torch.full((B * P + 2, 2), SENT, device=DEV)
    lg, sc, rs = ops.class_logits(d["e"], d["queries"], d["feats"], d["w_shift"], d["b_shift"], d["w_scale"], d["b_scale"], B, P, mask=d["mask"],
                                  rowstats=rs_buf[1:-1], logits=lg_buf[1:-1], scores=sc_buf[1:-1])
    torch.cuda.synchronize()
    assert bool((lg_buf[0] == SENT).all()) and bool((lg_buf[-1] == SENT).all()) and bool((sc_buf[0] == SENT).all()) and bool((sc_buf[-1] == SENT).all())
    assert bool((rs_buf[0] == SENT).all()) and bool((rs_buf[-1] == SENT).all())
    fails = []
    worst = R.check_logits(f"class_logits {case}", lg, sc, r, fails)
    b = R.bounds(r)
    ws = R.check(f"shift {case}", rs[:, 0].cpu().view(B, P, 1), r["shift"], b["shift"], fails)
    wc = R.check(f"scale {case}", rs[:, 1].cpu().view(B, P, 1), r["scale"], b["scale"], fails)
    print(f"class_logits B={B} P={P} Q={Q} Dt={Dt} D={D}: err / tol logits {worst[0]:.3f} scores {worst[1]:.3f} shift {ws:.3f} scale {wc:.3f}")
    assert not fails, "\n".join(fails[:8])
    assert not bool(torch.isnan(lg).any()) and not bool(torch.isnan(sc).any())
    # (h) two runs give equal bits; the score output is optional and changes nothing
    lg2, sc2, rs2 = _run(i, B, P)
    assert torch.equal(lg.cpu(), lg2) and torch.equal(sc.cpu(), sc2) and torch.equal(rs.cpu(), rs2)
    lg3, none, _ = _run(i, B, P, scores=False)
    assert none is None and torch.equal(lg3, lg2)


def test_guard_columns_between_rows_stay_untouched():
    """(i) columns: Q = 33 written into rows of a wider buffer is not possible through the contiguous [B, P, Q] contract, so the guard is the element
    after each row's last query seen through a flat view: logits of B = 1, P = 36, Q = 33 sit in a flat buffer with a sentinel tail of 31 floats (the
    rest of the last 32-column tile), and a run with Q = 32 into the same storage leaves the 33rd column of the earlier layout alone."""
    B, P, Q, Dt, D = 1, 36, 33, 192, 128
    i = _dev(R.make_inputs(B, P, Q, Dt, D, seed=1))
    flat = torch.full((B * P * Q + 31,), SENT, device=DEV)
    ops.class_logits(i["e"], i["queries"], i["feats"], i["w_shift"], i["b_shift"], i["w_scale"], i["b_scale"], B, P, mask=i["mask"],
                     logits=flat[:B * P * Q].view(B, P, Q))
    torch.cuda.synchronize()
    assert bool((flat[B * P * Q:] == SENT).all()) and not bool((flat[:B * P * Q] == SENT).any())
    # P = 4 inside a 32-row tile: 28 rows of the tile do not exist
    i4 = _dev(R.make_inputs(1, 4, 70, 64, 128, seed=1))
    flat = torch.full((4 * 70 + 70 * 28,), SENT, device=DEV)
    ops.class_logits(i4["e"], i4["queries"], i4["feats"], i4["w_shift"], i4["b_shift"], i4["w_scale"], i4["b_scale"], 1, 4, logits=flat[:280].view(1, 4, 70))
    torch.cuda.synchronize()
    assert bool((flat[280:] == SENT).all()) and not bool((flat[:280] == SENT).any())


@pytest.mark.parametrize("case", [(3, 36, 33, 192, 128), (3, 4, 32, 192, 128), (3, 576, 33, 64, 128)])
def test_an_images_block_does_not_depend_on_the_batch(cases, case):
    """(a) image b alone (B = 1) and at every position of a batch: the same bits, scores and row statistics included."""
    B, P, Q, Dt, D = case
    i, _ = cases[case]
    lg, sc, rs = _run(i, B, P)
    for b in range(B):
        one = dict(i, e=i["e"][b * P:(b + 1) * P], feats=i["feats"][b * P:(b + 1) * P], queries=i["queries"][b:b + 1], mask=i["mask"][b:b + 1])
        l1, s1, r1 = _run(one, 1, P)
        assert torch.equal(l1[0], lg[b]) and torch.equal(s1[0], sc[b]) and torch.equal(r1, rs[b * P:(b + 1) * P]), b
    # ... and permuted: the batch in reverse order
    rev = dict(i, e=i["e"].view(B, P, Dt).flip(0).reshape(B * P, Dt).contiguous(), feats=i["feats"].view(B, P, D).flip(0).reshape(B * P, D).contiguous(),
               queries=i["queries"].flip(0).contiguous(), mask=i["mask"].flip(0).contiguous())
    lr, sr, _ = _run(rev, B, P)
    assert torch.equal(lr.flip(0), lg) and torch.equal(sr.flip(0), sc)


def test_a_querys_column_does_not_depend_on_the_bank():
    """(b) a query alone in a bank of one, and at any column of a bank of 70 (block 0, the block edge, the last partial block): the same bits."""
    B, P, Q, Dt, D = 3, 36, 70, 192, 128
    i = R.make_inputs(B, P, Q, Dt, D, seed=2)
    lg, sc, _ = _run(i, B, P, masked=False)
    for col in (0, 5, 31, 32, 33, 63, 64, 69):
        l1, s1, _ = _run(i, B, P, masked=False, queries=i["queries"][:, col:col + 1].contiguous())
        assert torch.equal(l1[..., 0], lg[..., col]) and torch.equal(s1[..., 0], sc[..., col]), col
    # moved to another column: the bank rolled by 37
    lr, _, _ = _run(i, B, P, masked=False, queries=torch.roll(i["queries"], 37, dims=1).contiguous())
    assert torch.equal(torch.roll(lr, -37, dims=2), lg)


@pytest.mark.parametrize("case", [(3, 36, 33, 192, 128), (3, 576, 33, 64, 128)])
def test_a_shared_bank_is_the_bank_repeated(case):
    """(c) queries [Q, Dt] against the same bank repeated B times; a shared [Q] mask likewise."""
    B, P, Q, Dt, D = case
    i = R.make_inputs(B, P, Q, Dt, D, seed=3, shared=True)
    m1 = i["mask"][0].contiguous()
    a = _run(i, B, P, mask=m1)
    b = _run(i, B, P, queries=i["queries"][None].repeat(B, 1, 1).contiguous(), mask=m1[None].repeat(B, 1).contiguous())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    r = R.exact_logits(i["e"], i["queries"], i["feats"], i["w_shift"], i["b_shift"], i["w_scale"], i["b_scale"], B, P, m1)
    fails = []
    R.check_logits(f"shared bank {case}", a[0], a[1], r, fails)
    assert not fails, "\n".join(fails[:8])


def test_masks_and_zero_rows(cases):
    """(d) masked entries exactly finfo.min / +0; (e) unmasked entries carry the bits of the run without a mask; (f) an image with every query masked;
    (g) an all-zero query row gives shift * scale exactly, and no NaN anywhere."""
    case = (3, 36, 33, 192, 128)
    B, P, Q, Dt, D = case
    i, _ = cases[case]
    lg0, sc0, rs = _run(i, B, P, masked=False)
    mask = i["mask"].clone()
    mask[1] = 0                                   # (f)
    lg, sc, _ = _run(i, B, P, mask=mask)
    dead = (mask == 0)[:, None, :].expand(B, P, Q)
    assert bool(dead[1].all()) and bool(dead[0].any()) and not bool(dead[0].all())
    assert torch.equal(lg[dead], torch.full_like(lg[dead], R.FMIN))                                    # (d)
    assert torch.equal(R.bits(sc[dead]), torch.zeros_like(R.bits(sc[dead])))
    assert torch.equal(R.bits(lg[~dead]), R.bits(lg0[~dead])) and torch.equal(R.bits(sc[~dead]), R.bits(sc0[~dead]))          # (e)
    assert not bool(torch.isnan(lg0).any()) and not bool(torch.isnan(sc0).any()) and not bool(torch.isinf(lg0).any())
    z = Q // 2                                    # (g) make_inputs' all-zero row
    assert not bool(i["queries"][:, z].any())
    want = (rs[:, 0] * rs[:, 1]).view(B, P)
    assert torch.equal(R.bits(lg0[..., z]), R.bits(want))
    # an all-zero e row: cos = 0 exactly as well
    j = dict(i, e=i["e"].clone())
    j["e"][7] = 0.0
    lz, sz, _ = _run(j, B, P, masked=False)
    assert torch.equal(R.bits(lz[0, 7]), R.bits(want[0, 7].expand(Q).contiguous())) and not bool(torch.isnan(lz).any()) and not bool(torch.isnan(sz).any())
    # integer-valued masks other than 1 are valid entries
    m2 = (i["mask"] * 7).contiguous()
    assert torch.equal(_run(i, B, P, mask=m2)[0], _run(i, B, P)[0])


def test_wrapper_validation_on_device_tensors():
    i = _dev(R.make_inputs(1, 4, 5, 64, 128, seed=0))
    args = (i["e"], i["queries"], i["feats"], i["w_shift"], i["b_shift"], i["w_scale"], i["b_scale"])
    with pytest.raises(ValueError, match=r"queries must be \[1, Q, Dt\] or \[Q, Dt\]"):
        ops.class_logits(i["e"], i["queries"].repeat(2, 1, 1), *args[2:], 1, 4)
    with pytest.raises(ValueError, match=r"mask must be \[1, 5\] or \[5\]"):
        ops.class_logits(*args, 1, 4, mask=torch.ones(4, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError, match="mask must be torch.uint8"):
        ops.class_logits(*args, 1, 4, mask=torch.ones(5, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match=r"logits must be \[1, 4, 5\]"):
        ops.class_logits(*args, 1, 4, logits=torch.zeros(1, 4, 6, device=DEV))
    with pytest.raises(ValueError, match=r"e must be \[>= 8, 64\]"):
        ops.class_logits(i["e"], i["queries"][0], *args[2:], 2, 4)
