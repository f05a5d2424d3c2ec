"""-m gpu: the two tail kernels of OWLv2's objectness head (csrc/objectness.hip) on a real MI355X against the float64 closed forms of
tests/objectness_reference.py: every element of logits, du1, dw2, db2 and the column sums inside the bound derived there, nothing excluded; plus the
bitwise properties.  Shapes: objectness_reference.CASES -- the smallest that reach every launcher form (tests/test_objectness_reference.py checks
that).  Each test prints its worst err / tol; profiles/objectness_reference.md records them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402
from tests import objectness_reference as R  # noqa: E402

DEV = "cuda"
PAD = 3                    # NaN guard rows behind `rows`
SENT = 7.0                 # sentinel behind every output
NAN = float("nan")


def _dev(x, rows, D):
    """The inputs on the device: bf16 activations with PAD guard rows of NaN behind them."""
    bf = lambda t: R.padded(t, PAD, NAN).to(DEV).to(torch.bfloat16)
    return {"h1": bf(x["h1"]), "u1": bf(x["u1"]), "w2": x["w2"].to(DEV), "b2": x["b2"].to(DEV), "g": R.padded(x["g"], PAD, NAN).to(DEV)}


def _fwd(d, rows, D):
    out = torch.full((rows + PAD,), SENT, device=DEV)
    ops.objectness_final(d["h1"], d["w2"], d["b2"], out, rows, D)
    return out


def _bwd(d, rows, D, g=None):
    nblk = ops.objectness_final_bwd_blocks(rows)
    assert nblk == R.bwd_blocks(rows)
    o = {"du1": torch.full((rows + PAD, D), SENT, device=DEV, dtype=torch.bfloat16), "part": torch.full((nblk * (2 * D + 4) + 4,), SENT, device=DEV),
         "dw2_db2": torch.full((D + 4 + 4,), SENT, device=DEV), "colsum": torch.full((D + 4,), SENT, device=DEV)}
    ops.objectness_final_bwd(d["g"] if g is None else g, d["h1"], d["u1"], d["w2"], o["du1"], o["part"], o["dw2_db2"], rows, D, du1_colsum=o["colsum"])
    return o


def _sentinels(name, rows, D, logits=None, o=None):
    if logits is not None:
        assert bool((logits[rows:] == SENT).all()), f"{name}: logits behind `rows` were written"
    if o is not None:
        assert bool((o["du1"][rows:].float() == SENT).all()), f"{name}: du1 behind `rows` was written"
        assert bool((o["dw2_db2"][D + 4:] == SENT).all()) and bool((o["colsum"][D:] == SENT).all()) and bool((o["part"][-4:] == SENT).all()), f"{name}: sentinel lost"
        assert bool((o["dw2_db2"][D + 1:D + 4] == 0).all()), f"{name}: the three pad floats behind db2 are zeros"


@pytest.mark.parametrize("profile", ["randn", "saturated"])
@pytest.mark.parametrize("rows,D", R.CASES)
def test_every_element_inside_its_bound(rows, D, profile):
    x = R.make_inputs(rows, D, profile=profile)
    d = _dev(x, rows, D)
    logits, o = _fwd(d, rows, D), _bwd(d, rows, D)
    torch.cuda.synchronize()
    name = f"objectness tail {rows} x {D} {profile}"
    _sentinels(name, rows, D, logits, o)
    rf, rb = R.exact_final(x["h1"], x["w2"], x["b2"]), R.exact_final_bwd(x["g"], x["h1"], x["u1"], x["w2"])
    tf, tb = R.bounds_final(rf), R.bounds_final_bwd(rb)
    got = {"logits": logits[:rows].cpu(), "du1": o["du1"][:rows].float().cpu(), "dw2": o["dw2_db2"][:D].cpu(), "db2": o["dw2_db2"][D].cpu(), "colsum": o["colsum"][:D].cpu()}
    ref = {"logits": rf["logits"], **{k: rb[k] for k in ("du1", "dw2", "db2", "colsum")}}
    tol = {"logits": tf["logits"], **tb}
    fails, worst = [], {}
    for k in got:
        worst[k] = R.check(f"{name} {k}", got[k], ref[k], tol[k], fails)
    print(f"{name}: worst err / tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" (rpw {R.fwd_rpw(rows)}, {R.bwd_blocks(rows)} workgroups of {R.bwd_rpb(rows)} rows)")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows,D", [(37, 128), (5, 520), (4100, 128)])
def test_bitwise_properties(rows, D):
    x = R.make_inputs(rows, D)
    d = _dev(x, rows, D)
    l1, o1 = _fwd(d, rows, D), _bwd(d, rows, D)
    l2, o2 = _fwd(d, rows, D), _bwd(d, rows, D)
    torch.cuda.synchronize()
    # two runs give the same bits
    assert torch.equal(R.bits(l1), R.bits(l2))
    for k in ("du1", "dw2_db2", "colsum"):
        assert torch.equal(R.bits(o1[k]), R.bits(o2[k])), k
    # a row alone equals the row inside the batch, forward and du1
    for r in sorted({0, rows // 2, rows - 1}):
        one = {"h1": d["h1"][r:r + 1].contiguous(), "u1": d["u1"][r:r + 1].contiguous(), "w2": d["w2"], "b2": d["b2"], "g": d["g"][r:r + 1].contiguous()}
        la = torch.full((1,), SENT, device=DEV)
        ops.objectness_final(one["h1"], one["w2"], one["b2"], la, 1, D)
        oa = {"du1": torch.zeros(1, D, device=DEV, dtype=torch.bfloat16), "part": torch.zeros(2 * D + 4, device=DEV), "dw2_db2": torch.zeros(D + 4, device=DEV)}
        ops.objectness_final_bwd(one["g"], one["h1"], one["u1"], one["w2"], oa["du1"], oa["part"], oa["dw2_db2"], 1, D)
        assert torch.equal(R.bits(la), R.bits(l1[r:r + 1])) and torch.equal(R.bits(oa["du1"][0]), R.bits(o1["du1"][r])), r
    # a zero upstream row gives an exactly zero du1 row; the others keep their bits
    g = d["g"].clone()
    z = rows // 2
    g[z] = 0.0
    oz = _bwd(d, rows, D, g=g)
    assert bool((oz["du1"][z].float() == 0).all())
    keep = torch.arange(rows, device=DEV) != z
    assert torch.equal(R.bits(oz["du1"][:rows][keep]), R.bits(o1["du1"][:rows][keep]))
    # an all-zero upstream gives exactly zero sums
    g0 = torch.zeros_like(d["g"])
    g0[rows:] = NAN
    o0 = _bwd(d, rows, D, g=g0)
    torch.cuda.synchronize()
    assert bool((o0["dw2_db2"][:D + 4] == 0).all()) and bool((o0["colsum"][:D] == 0).all()) and bool((o0["du1"][:rows].float() == 0).all())
    _sentinels(f"{rows} x {D}", rows, D, l1, o0)
