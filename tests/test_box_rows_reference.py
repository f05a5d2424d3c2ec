"""CPU checks of tests/box_rows_reference.py: the compaction rule on its edge cases, the six gradients against torch autograd through a float64 box head,
and the bounds against an f32 simulation of the tail in list order (planted errors must fall outside)."""
import numpy as np
import pytest
import torch

from tests import box_rows_reference as R
from tests.gemm_reference import check, dgelu_erf_f32, gelu

CAP = 8


def _db(rows, listed, special=None):
    return R.make_case(rows, 8, listed, special=special)["dboxes"].numpy()


@pytest.mark.parametrize("rows", [7, 64, 577])
def test_compact_edge_cases(rows):
    nan = float("nan")
    cases = {
        "none": ([], None, [], False),
        "first": ([0], None, [0], False),
        "last": ([rows - 1], None, [rows - 1], False),
        "nan_row": ([], {3: [0.0, nan, 0.0, 0.0]}, [3], False),
        "inf_row": ([], {2: [0.0, 0.0, float("inf"), 0.0]}, [2], False),
        "neg_zero_only": ([1], {4: [-0.0, -0.0, -0.0, -0.0]}, [1], False),
        "fourth_component": ([], {5: [0.0, 0.0, 0.0, 1e-30]}, [5], False),
    }
    for name, (listed, special, want, over) in cases.items():
        rl, n, ov = R.compact(_db(rows, listed, special), CAP)
        assert list(rl) == want and n == len(want) and ov == over, name
    if rows >= CAP + 1:
        step = rows // (CAP + 1)
        exact = [i * step for i in range(CAP)]
        rl, n, ov = R.compact(_db(rows, exact), CAP)
        assert list(rl) == exact and n == CAP and not ov
        more = exact + [rows - 1]
        rl, n, ov = R.compact(_db(rows, more), CAP)
        assert list(rl) == exact and n == CAP and ov          # the first cap rows, flagged
    else:          # 7 rows: all of them
        rl, n, ov = R.compact(_db(rows, list(range(rows))), CAP)
        assert list(rl) == list(range(rows)) and n == rows and not ov
    assert R.cap_pad(1) == 8 and R.cap_pad(8) == 8 and R.cap_pad(9) == 16 and R.cap_pad(512) == 512


def _forward64(feats, W0, b0, W1, b1, W2, b2):
    u0 = feats @ W0.t() + b0
    h0 = gelu(u0)
    u1 = h0 @ W1.t() + b1
    h1 = gelu(u1)
    s = torch.sigmoid(h1 @ W2.t() + b2)
    boxes = torch.stack([s[:, 0] - 0.5 * s[:, 2], s[:, 1] - 0.5 * s[:, 3], s[:, 0] + 0.5 * s[:, 2], s[:, 1] + 0.5 * s[:, 3]], -1)
    return u0, h0, u1, h1, s, boxes


def test_exact_six_is_autograd_of_the_box_head():
    rows, D, listed = 40, 16, [3, 17, 18, 39]
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    feats = rn(rows, D)
    P = [rn(D, D) / 4, rn(D), rn(D, D) / 4, rn(D), rn(4, D) / 4, rn(4)]
    P = [p.requires_grad_() for p in P]
    u0, h0, u1, h1, s, boxes = _forward64(feats, *P)
    db = torch.zeros(rows, 4, dtype=torch.float64)
    db[listed] = rn(len(listed), 4)
    (boxes * db).sum().backward()
    x0 = R.exact_six(db, s.detach(), h1.detach(), u1.detach(), h0.detach(), u0.detach(), feats, P[4].detach(), P[2].detach(), listed)
    # without the two bf16 roundings: hand the reference its own unrounded du1 / du0
    du1 = x0["tail"]["du1"]
    du0 = (du1 @ P[2].detach()) * R.gelu_d1(u0.detach()[listed])
    x = R.exact_six(db, s.detach(), h1.detach(), u1.detach(), h0.detach(), u0.detach(), feats, P[4].detach(), P[2].detach(), listed, given_du1=du1, given_du0=du0)
    want = {"dense0.weight": P[0].grad, "dense0.bias": P[1].grad, "dense1.weight": P[2].grad, "dense1.bias": P[3].grad, "dense2.weight": P[4].grad,
            "dense2.bias": P[5].grad}
    for k in R.SIX:
        assert torch.allclose(x["grads"][k], want[k], rtol=1e-12, atol=1e-14), k
    # and the list is all that matters: every row gives the same sums
    xa = R.exact_six(db, s.detach(), h1.detach(), u1.detach(), h0.detach(), u0.detach(), feats, P[4].detach(), P[2].detach(), list(range(rows)),
                     given_du1=None, given_du0=None)
    for k in ("dense2.weight", "dense2.bias", "dense1.bias"):
        assert torch.allclose(xa["grads"][k], x0["grads"][k], rtol=1e-12, atol=1e-14), k


def _emulate_tail(c, rows, cap_pad, drop_last=False):
    """f32 simulation of box_rows_tail_kernel + the slab reduce in workgroup order: -> du1 (bf16 values), dW2, db2, colsum."""
    f = torch.float32
    D = c["hb1"].shape[1]
    nblk = cap_pad // R.RPB
    pw, pb, pu = torch.zeros(nblk, 4, D), torch.zeros(nblk, 4), torch.zeros(nblk, D)
    du1 = torch.zeros(cap_pad, D)
    use = rows[:-1] if drop_last else rows
    for i, r in enumerate(use):
        gq, s = c["dboxes"][r], c["sig"][r]
        dl = torch.stack([gq[0] + gq[2], gq[1] + gq[3], 0.5 * (gq[2] - gq[0]), 0.5 * (gq[3] - gq[1])])
        dp = (dl * s) * (1.0 - s)
        dh1 = torch.zeros(D, dtype=f)
        for k in range(4):
            dh1 = (dp[k].double() * c["w2"][k].double() + dh1.double()).float()          # the FMA chain
        o = dh1 * dgelu_erf_f32(c["ub1"][r])
        du1[i] = o.to(torch.bfloat16).float()
        b = i // R.RPB
        pu[b] += o
        pb[b] += dp
        for k in range(4):
            pw[b, k] = (dp[k].double() * c["hb1"][r].double() + pw[b, k].double()).float()
    return {"du1": du1, "dense2.weight": _seq_sum(pw), "dense2.bias": _seq_sum(pb), "dense1.bias": _seq_sum(pu)}


def _seq_sum(p):
    a = torch.zeros_like(p[0])
    for s in p:
        a = a + s
    return a


@pytest.mark.parametrize("D,count", [(64, 1), (64, 8), (768, 5)])
def test_tail_simulation_is_inside_the_bounds_and_planted_errors_are_not(D, count):
    rows_n = 97
    listed = sorted({(i * 37 + 5) % rows_n for i in range(count)})
    c = R.make_case(rows_n, D, listed)
    rl, n, ov = R.compact(c["dboxes"].numpy(), CAP)
    assert list(rl) == listed and not ov
    x = R.exact_six(c["dboxes"], c["sig"], c["hb1"], c["ub1"], c["hb0"], c["ub0"], c["feats"], c["w2"], c["w1"], rl)
    tol = R.bounds_six(x, rows_n)
    em = _emulate_tail(c, list(rl), R.cap_pad(CAP))
    for k in ("dense2.weight", "dense2.bias", "dense1.bias"):
        assert check(k, em[k], x["grads"][k], tol[k]) <= 1.0
    assert check("du1", em["du1"][:n], x["tail"]["du1"], tol["du1"]) <= 1.0
    bad = _emulate_tail(c, list(rl), R.cap_pad(CAP), drop_last=True)
    fails = []
    for k in ("dense2.weight", "dense2.bias", "dense1.bias"):
        check(k, bad[k], x["grads"][k], tol[k], fails)
    assert len(fails) == 3, fails


def test_empty_list_gives_exact_zeros():
    c = R.make_case(20, 64, [])
    rl, n, ov = R.compact(c["dboxes"].numpy(), CAP)
    assert n == 0 and not ov
    x = R.exact_six(c["dboxes"], c["sig"], c["hb1"], c["ub1"], c["hb0"], c["ub0"], c["feats"], c["w2"], c["w1"], rl)
    for k in R.SIX:
        assert float(x["grads"][k].abs().max()) == 0.0
    tol = R.bounds_six(x, 20)
    assert all(float(tol[k].max()) < 1e-30 for k in R.SIX)
