"""-m gpu: the kernels of csrc/open_vocab_loss.hip alone, through the C ABI, against tests/open_vocab_loss_reference.py.

Per case of `GPU_CASES`: costT elementwise inside its bound; owl_hungarian on the device's cost equal to the oracle's LSAP on that same cost; the three
losses, dlogits and dboxes elementwise inside their bounds at the device's decisions, nothing excluded.  Bitwise: two runs, +0.0 under the mask, NaN
against -FLT_MAX under the mask, an image alone against the same image in its batch, a shared mask against the repeated one, sentinel rows past B P.
The fixture case (recorded from transformers): the device's indices are HF's.  The measured err / tol per shape is printed (profiles/open_vocab_loss_reference.md)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops  # noqa: E402
from owl_vit_object_detection_amd.matcher import PackedTargets  # noqa: E402
from tests import open_vocab_loss_reference as R  # noqa: E402
from tests.gemm_reference import bits  # noqa: E402

DEV = "cuda"
G3 = torch.tensor([1.0, 5.0, 2.0])
ALPHA, WC, WB, WG = 0.25, 1.0, 5.0, 2.0
SENTINEL = 12345.0
TAIL = 3          # sentinel rows behind every [B P, .] output
_runs = {}


def _pad(B, P, width):
    """[B P + TAIL, width] filled with the sentinel; the kernels get the base pointer of a [B, P, width] tensor."""
    return torch.full((B * P + TAIL, width), SENTINEL, device=DEV)


def run(case, num_boxes=None, labels=None, g3=G3, alpha=ALPHA):
    """Every launch of the criterion on `case`; returns host tensors (and the padded device outputs' tails)."""
    B, P, Q = case["logits"].shape
    lg = case["logits"].to(DEV).contiguous()
    bx = case["boxes"].to(DEV).contiguous()
    mask = None if case["mask"] is None else case["mask"].to(DEV).to(torch.uint8).contiguous()
    nmasks = 1 if mask is None else int(mask.shape[0])
    tg = PackedTargets(case["labels"] if labels is None else labels, case["tgt"], DEV, None, allow_empty=True)
    nb = float(max(1, sum(case["counts"]))) if num_boxes is None else float(num_boxes)
    N = tg.Nmax
    s = ops.stream()
    costT = torch.full((B, N, P), SENTINEL, device=DEV)
    _lib.call("owl_focal_match_cost", s, lg, mask, bx, tg.labels, tg.boxes, tg.counts, costT, B, P, Q, nmasks, N, alpha, WC, WB, WG)
    pred_idx = torch.empty(B, N, dtype=torch.int64, device=DEV)
    tgt_idx = torch.empty(B, N, dtype=torch.int64, device=DEV)
    tc = torch.empty(B, P, dtype=torch.int64, device=DEV)
    _lib.call("owl_hungarian", s, costT, tg.labels, tg.counts, pred_idx, tgt_idx, tc, B, P, N, Q)
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_focal_loss_workspace_bytes", B, P, Q, nbytes)
    assert int(nbytes) == 8 * (3 * B + R.n_parts(B, P, Q))
    ws = torch.full((int(nbytes) // 8 + TAIL,), SENTINEL, dtype=torch.float64, device=DEV)
    dl1, dgiou, dlogits, dboxes = _pad(B, P, 4), _pad(B, P, 4), _pad(B, P, Q), _pad(B, P, 4)
    losses = torch.full((3 + TAIL,), SENTINEL, device=DEV)
    _lib.call("owl_focal_loss_fwd", s, lg, mask, tc, ws, int(nbytes), B, P, Q, nmasks, alpha)
    _lib.call("owl_box_pair_loss", s, bx, mask, tg.labels, tg.boxes, pred_idx, tgt_idx, tg.counts, ws, int(nbytes), dl1, dgiou, B, P, Q, nmasks, N)
    _lib.call("owl_open_vocab_loss_reduce", s, ws, int(nbytes), losses, B, P, Q, nb)
    g = g3.to(DEV)
    _lib.call("owl_focal_loss_bwd", s, g, lg, mask, tc, dlogits, B, P, Q, nmasks, alpha, nb)
    _lib.call("owl_box_pair_loss_bwd", s, g, dl1, dgiou, dboxes, B, P, nb)
    torch.cuda.synchronize()
    tails = [dl1[B * P:], dgiou[B * P:], dlogits[B * P:], dboxes[B * P:], losses[3:], ws[int(nbytes) // 8:].float()]
    assert all(bool((t == SENTINEL).all()) for t in tails), "a kernel wrote past its output"
    return dict(costT=costT.cpu(), pred_idx=pred_idx.cpu(), tgt_idx=tgt_idx.cpu(), tc=tc.cpu(), losses=losses[:3].cpu(), nb=nb,
                dlogits=dlogits[:B * P].view(B, P, Q).cpu(), dboxes=dboxes[:B * P].view(B, P, 4).cpu(),
                dl1=dl1[:B * P].view(B, P, 4).cpu(), dgiou=dgiou[:B * P].view(B, P, 4).cpu())


def _case_run(name):
    if name not in _runs:
        case = R.gpu_case(name)
        _runs[name] = (case, run(case))
    return _runs[name]


def _same_bits(a, b, keys=("costT", "pred_idx", "tgt_idx", "tc", "losses", "dlogits", "dboxes", "dl1", "dgiou")):
    for k in keys:
        x, y = a[k], b[k]
        assert torch.equal(bits(x), bits(y)) if x.dtype == torch.float32 else torch.equal(x, y), k


def _row(case, b):
    m = case["mask"]
    return None if m is None else m[b if m.shape[0] == case["logits"].shape[0] else 0]


@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_every_output_is_inside_its_bound(name):
    case, out = _case_run(name)
    B, P, Q = case["logits"].shape
    worst = {}
    pi, ti, tcs = [], [], []
    for b in range(B):
        n = case["counts"][b]
        st = R.cost_stage(case["logits"][b], case["boxes"][b], case["labels"][b], case["tgt"][b], _row(case, b), ALPHA, WC, WB, WG)
        dev_cost = out["costT"][b, :n].T.contiguous()                                   # [P, n]
        if n:
            worst["cost"] = max(worst.get("cost", 0.0), R.check(f"{name} costT[{b}]", dev_cost, st["ref"], st["tol"]))
        assert bool((out["costT"][b, n:] == SENTINEL).all())                            # rows of padded targets are not written
        # the assignment: the oracle's LSAP on the DEVICE's cost, bit for bit
        i, j, tc = R.decide(dev_cost.numpy(), case["labels"][b], Q)
        assert out["pred_idx"][b, :n].tolist() == i.tolist() and out["tgt_idx"][b, :n].tolist() == j.tolist(), (name, b)
        assert torch.equal(out["tc"][b], tc)
        assert bool((out["pred_idx"][b, n:] == 0).all()) and bool((out["tgt_idx"][b, n:] == 0).all())
        pi.append(i); ti.append(j); tcs.append(tc)
    crit = R.criterion(case["logits"], case["boxes"], case["mask"], torch.stack(tcs), pi, ti, case["tgt"], ALPHA, out["nb"], G3)
    for k in ("losses", "dlogits", "dboxes"):
        worst[k] = R.check(f"{name} {k}", out[k], *crit[k])
    live = R._live(case["mask"], B, P, Q)
    assert bool((bits(out["dlogits"])[~live] == 0).all())                               # exactly +0.0 under the mask
    assert bool(torch.isfinite(out["losses"]).all())
    matched = torch.zeros(B, P, dtype=torch.bool)
    for b in range(B):
        matched[b, pi[b]] = True
    assert bool((bits(out["dboxes"])[~matched] == 0).all()) and bool((bits(out["dl1"])[~matched] == 0).all())
    print(f"open_vocab_loss {name} B={B} P={P} Q={Q} counts={case['counts']}: worst err / tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f" | losses {[round(float(x), 6) for x in out['losses']]}")


@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_two_runs_give_the_same_bits(name):
    case, out = _case_run(name)
    _same_bits(out, run(case))


@pytest.mark.parametrize("name", ["q32_sat_nan", "q33_nan", "q260_sat"])
def test_the_bits_under_the_mask_change_nothing(name):
    case, out = _case_run(name)
    B, P, Q = case["logits"].shape
    live = R._live(case["mask"], B, P, Q)
    was_nan = bool(torch.isnan(case["logits"][~live]).all())
    other = dict(case, logits=torch.where(live, case["logits"], torch.full_like(case["logits"], R.FMIN if was_nan else float("nan"))))
    _same_bits(out, run(other))
    junk = dict(case, logits=torch.where(live, case["logits"], torch.full_like(case["logits"], float("inf"))))
    _same_bits(out, run(junk))


@pytest.mark.parametrize("name", ["q31_empty", "q33_nan", "q260_sat"])
def test_an_image_alone_has_the_bits_it_has_in_the_batch(name):
    case, out = _case_run(name)
    B = case["logits"].shape[0]
    for b in (0, B - 1):
        m = case["mask"]
        alone = dict(logits=case["logits"][b:b + 1], boxes=case["boxes"][b:b + 1], mask=None if m is None else m[b:b + 1] if m.shape[0] == B else m,
                     labels=case["labels"][b:b + 1], tgt=case["tgt"][b:b + 1], counts=case["counts"][b:b + 1])
        one = run(alone, num_boxes=out["nb"])
        n = case["counts"][b]
        for k in ("dlogits", "dboxes", "tc", "dl1", "dgiou"):
            assert torch.equal(bits(one[k][0]) if one[k].dtype == torch.float32 else one[k][0], bits(out[k][b]) if out[k].dtype == torch.float32 else out[k][b]), k
        assert torch.equal(bits(one["costT"][0, :n]), bits(out["costT"][b, :n]))


@pytest.mark.parametrize("name", ["q32_sat_nan", "stride"])
def test_a_shared_mask_is_the_repeated_mask(name):
    case, out = _case_run(name)
    B, _, Q = case["logits"].shape
    assert case["mask"].shape[0] == 1
    _same_bits(out, run(dict(case, mask=case["mask"].expand(B, Q).contiguous())))


def test_the_fixture_case_gives_hfs_indices_and_losses():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f17_open_vocab_loss.npz"))
    counts = z["counts"].tolist()
    case = dict(logits=torch.from_numpy(z["logits"]), boxes=torch.from_numpy(z["boxes"]), mask=torch.from_numpy(z["mask"]), counts=counts,
                labels=[torch.from_numpy(z["labels"][b, :n]) for b, n in enumerate(counts)], tgt=[torch.from_numpy(z["tgt"][b, :n]) for b, n in enumerate(counts)])
    out = run(case, g3=torch.from_numpy(z["weights"]).float())
    pi, ti, tcs = [], [], []
    for b, n in enumerate(counts):
        assert out["pred_idx"][b, :n].tolist() == z["pred_idx"][b, :n].tolist() and out["tgt_idx"][b, :n].tolist() == z["tgt_idx"][b, :n].tolist()
        pi.append(out["pred_idx"][b, :n]); ti.append(out["tgt_idx"][b, :n]); tcs.append(out["tc"][b])
    crit = R.criterion(case["logits"], case["boxes"], case["mask"], torch.stack(tcs), pi, ti, case["tgt"], ALPHA, out["nb"], torch.from_numpy(z["weights"]).float())
    # the bounds' reference values ARE the recorded HF results (to double noise), so the device is held to HF itself
    for k in ("losses", "dlogits", "dboxes"):
        ref, tol = crit[k]
        assert float((ref - torch.from_numpy(z[k])).abs().max()) <= 1e-12 * float(ref.abs().max())
        R.check(f"fixture {k}", out[k], torch.from_numpy(z[k]), tol)


def test_alpha_off_and_other_weights():
    """alpha < 0: no alpha weighting (HF); loss_ce is then the plain sum of softplus(z) sigmoid(z)^2."""
    case = R.gpu_case("q31_empty")
    out = run(case, alpha=-1.0)
    B, P, Q = case["logits"].shape
    pi = [out["pred_idx"][b, :n] for b, n in enumerate(case["counts"])]
    ti = [out["tgt_idx"][b, :n] for b, n in enumerate(case["counts"])]
    crit = R.criterion(case["logits"], case["boxes"], case["mask"], out["tc"], pi, ti, case["tgt"], -1.0, out["nb"], G3)
    for k in ("losses", "dlogits"):
        R.check(f"alpha off {k}", out[k], *crit[k])
    base = _case_run("q31_empty")[1]
    assert float(out["losses"][0]) > float(base["losses"][0])


def test_a_bad_device_resident_label_poisons_loss_ce_alone():
    case = R.gpu_case("q31_empty")
    B, P, Q = case["logits"].shape
    for bad in (Q, -1, Q + 1000, "masked"):
        labels = [l.clone() for l in case["labels"]]
        if bad == "masked":
            dead = (~case["mask"][2]).nonzero()
            labels[2][1] = int(dead[0])
        else:
            labels[2][1] = bad
        out = run(case, labels=[l.to(DEV) for l in labels])
        assert bool(torch.isnan(out["losses"][0])) and bool(torch.isfinite(out["losses"][1:]).all()), bad
        assert bool(torch.isfinite(out["costT"][2, :5]).all()) and bool(torch.isfinite(out["dlogits"]).all())


def test_argument_checks():
    nbytes = torch.zeros(1, dtype=torch.int64)
    for B, P, Q in ((1, 8193, 4), (1, 4, 4097), (0, 4, 4), (1, 4, 0)):
        with pytest.raises(_lib.OwlLibError):
            _lib.call("owl_focal_loss_workspace_bytes", B, P, Q, nbytes)
    x = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int64, device=DEV)
    c = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.OwlLibError, match="Nmax <= P"):
        _lib.call("owl_focal_match_cost", ops.stream(), x, None, x, i, x, c, x, 1, 2, 4, 1, 3, 0.25, 1.0, 5.0, 2.0)
    with pytest.raises(_lib.OwlLibError, match="nmasks = B or 1"):
        _lib.call("owl_focal_loss_bwd", ops.stream(), x, x, x.to(torch.uint8), i, x, 3, 2, 4, 2, 0.25, 1.0)
    with pytest.raises(_lib.OwlLibError, match="workspace of 8 bytes"):
        _lib.call("owl_focal_loss_fwd", ops.stream(), x, None, i, x.double(), 8, 1, 2, 4, 1, 0.25)
    with pytest.raises(_lib.OwlLibError, match="num_boxes must be positive"):
        _lib.call("owl_box_pair_loss_bwd", ops.stream(), x, x, x, x, 1, 2, 0.0)
