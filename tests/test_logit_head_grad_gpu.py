"""GPU: the gradients of HF's logit shift and scale -- owl_class_logits_bwd_head (csrc/open_vocab_bwd.hip: the row pass's rowgrad store,
ovb_head_part_kernel, ovb_head_finish_kernel) -- against the float64 closed form inside the derived bounds of tests/logit_head_grad_reference.py, every
element, nothing excluded; and the bitwise properties the header promises: two runs, the existing entry's outputs, rows past B P, poisoned masked
upstream, an all-masked batch, a shared bank, NULL outputs.  err / tol per shape: profiles/logit_head_grad_reference.md.

Shapes: tests/open_vocab_bwd_reference.py's GPU_CASES (P = 4 below one 32-row tile, 36 ragged, 70; D = 128 / 768 / 1024), (2, 576, 31, 64, 128), and
CHUNK_CASE = (2, 600, 5, 64, 128): P = 600 spans three 256-row chunks of the reduction, the last one ragged (88 rows)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402
from tests import logit_head_grad_reference as H  # noqa: E402
from tests import open_vocab_bwd_reference as R  # noqa: E402
from tests.gemm_reference import bits, check  # noqa: E402

DEV = "cuda"
SENT = -12345.0
NAN = float("nan")
VARIANTS = {"plain": {}, "shared": dict(shared=True, shared_mask=True), "underflow": dict(underflow=True), "poison": dict(poison=True)}
CASES = [(c, "plain") for c in H.GPU_CASES] + [(c, v) for c in (R.GPU_CASES[1], R.GPU_CASES[4], H.CHUNK_CASE) for v in VARIANTS if v != "plain"]
BITWISE = [R.GPU_CASES[1], R.GPU_CASES[4], H.CHUNK_CASE]


@functools.lru_cache(maxsize=None)
def _inputs(case, variant):
    """Seeded CPU inputs and their float64 records, made once per (case, variant) and left unchanged."""
    i = R.make_inputs(*case, seed=3, **VARIANTS[variant])
    r, h = H.exact_head_of(i, case[0], case[1])
    return i, r, h


def _call(i, B, P, dfeats=True, dq=True, head=True, pad=2, **over):
    """-> (de, dfeats, dq, dhead, rowgrad).  feats and rowgrad carry `pad` rows of NaN past B P; the outputs sentinel rows."""
    d = {k: (None if v is None else v.to(DEV)) for k, v in {**i, **over}.items() if k != "x"}
    Dt, D = d["e"].shape[1], d["w_shift"].numel()
    de = torch.full((B * P + pad, Dt), SENT, dtype=torch.bfloat16, device=DEV)
    df = torch.full((B * P + pad, D), SENT, device=DEV) if dfeats else False
    dqs = torch.full_like(d["queries"], SENT) if dq else False
    more, dhead, rowgrad = {}, None, None
    if head:
        feats = torch.cat([d["feats"][:B * P], torch.full((pad, D), NAN, dtype=torch.bfloat16, device=DEV)])
        rowgrad = torch.full((B * P + pad, 2), NAN, device=DEV)
        dhead = torch.full((2 * D + 2,), SENT, device=DEV)
        more = dict(feats=feats, dhead=dhead, rowgrad=rowgrad)
    ops.class_logits_bwd(d["g"], d["e"], d["queries"], d["w_shift"], d["w_scale"], d["rowstats"], B, P, mask=d["mask"], de=de, dfeats=df, dqueries=dqs, **more)
    return de, (df if dfeats else None), (dqs if dq else None), dhead, rowgrad


def _same(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("case,variant", CASES)
def test_against_float64_inside_the_derived_bounds(case, variant):
    B, P, Q, Dt, D = case
    i, r, h = _inputs(case, variant)
    de, df, dq, dhead, rowgrad = _call(i, B, P)
    assert bool(torch.isfinite(dhead).all()), "a non-finite gradient"
    worst = H.check_head(f"{case} {variant}", dhead, r, h)
    print(f"logit_head_grad {case} {variant}: err / tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    # rowgrad holds the row pass's two scalars, inside their own bounds; rows past B P (NaN here, as in feats) are neither written nor read
    E_dsh, E_ds = H.row_scalar_bounds(r)
    rg = rowgrad.double().cpu()
    check(f"{case} {variant} rowgrad dshift", rg[:B * P, 0], h["dsh"], E_dsh)
    check(f"{case} {variant} rowgrad ds", rg[:B * P, 1], h["ds"], E_ds)
    assert bool(torch.isnan(rowgrad[B * P:]).all())
    # two runs give equal bits
    assert _same(dhead, _call(i, B, P)[3])
    # de / dfeats / dq carry the existing entry's bits
    de0, df0, dq0, _, _ = _call(i, B, P, head=False)
    assert _same(de, de0) and _same(df, df0) and _same(dq, dq0)


@pytest.mark.parametrize("case", BITWISE)
def test_poisoned_masked_upstream_changes_no_bit(case):
    B, P = case[0], case[1]
    i, ip = _inputs(case, "plain")[0], _inputs(case, "poison")[0]
    assert torch.equal(i["mask"], ip["mask"]) and int((i["mask"] == 0).sum()) > 0 and not bool(torch.isfinite(ip["g"]).all())
    a, b = _call(i, B, P), _call(ip, B, P)
    assert _same(a[3], b[3]) and _same(a[4][:B * P], b[4][:B * P])


@pytest.mark.parametrize("case", BITWISE)
def test_an_all_masked_batch_gives_exact_zeros(case):
    B, P, Q = case[0], case[1], case[2]
    i = _inputs(case, "poison")[0]          # (Inf / NaN stand in the upstream as well: everything is selected out)
    out = _call(i, B, P, mask=torch.zeros(B, Q, dtype=torch.uint8))
    assert bool((out[3] == 0).all()) and bool((out[4][:B * P] == 0).all())


@pytest.mark.parametrize("case", BITWISE)
def test_a_shared_bank_is_the_bank_repeated(case):
    B, P = case[0], case[1]
    i = _inputs(case, "shared")[0]
    a = _call(i, B, P)
    b = _call(i, B, P, queries=i["queries"][None].repeat(B, 1, 1), mask=i["mask"][None].repeat(B, 1))
    assert _same(a[3], b[3]) and _same(a[4][:B * P], b[4][:B * P])


@pytest.mark.parametrize("case,variant", [(R.GPU_CASES[1], "plain"), (R.GPU_CASES[4], "shared"), (H.CHUNK_CASE, "plain")])
def test_null_outputs_leave_the_head_gradients_bits(case, variant):
    B, P = case[0], case[1]
    i = _inputs(case, variant)[0]
    full = _call(i, B, P)
    for kw in (dict(dq=False), dict(dfeats=False), dict(dfeats=False, dq=False)):
        out = _call(i, B, P, **kw)
        assert _same(full[3], out[3]) and _same(full[0], out[0]), kw
        assert (out[1] is None) == ("dfeats" in kw) and (out[2] is None) == ("dq" in kw)


@pytest.mark.parametrize("case", BITWISE)
def test_a_batch_is_the_float64_sum_of_its_images_alone(case):
    B, P, Q, Dt, D = case
    i, r, h = _inputs(case, "plain")
    dhead = _call(i, B, P)[3]
    tot = torch.zeros(2 * D + 2, dtype=torch.float64)
    tol = torch.cat([H.bounds(r, h)[k].reshape(-1) for k in ("dw_shift", "dw_scale", "db_shift", "db_scale")])
    for b in range(B):
        rows = slice(b * P, (b + 1) * P)
        one = dict(e=i["e"][rows].contiguous(), g=i["g"][b:b + 1].contiguous(), queries=i["queries"][b:b + 1].contiguous(),
                   rowstats=i["rowstats"][rows].contiguous(), mask=i["mask"][b:b + 1].contiguous(), feats=i["feats"][rows].contiguous())
        out = _call(i, 1, P, **one)
        tot += out[3].double().cpu()
        # each image alone is known to its own bound
        i1 = {**i, **one}
        r1, h1 = H.exact_head_of(i1, 1, P)
        H.check_head(f"{case} image {b} alone", out[3], r1, h1)
        tol = tol + torch.cat([H.bounds(r1, h1)[k].reshape(-1) for k in ("dw_shift", "dw_scale", "db_shift", "db_scale")])
    check(f"{case} batch against the float64 sum of its images", dhead.double().cpu(), tot, tol)


def test_wrapper_validation_on_device_tensors():
    i = _inputs((1, 4, 1, 64, 128), "plain")[0]
    d = {k: (None if v is None else v.to(DEV)) for k, v in i.items()}
    args = [d[k] for k in ("g", "e", "queries", "w_shift", "w_scale", "rowstats")]
    with pytest.raises(ValueError, match="dhead needs feats"):
        ops.class_logits_bwd(*args, 1, 4, dhead=True)
    with pytest.raises(ValueError, match=r"feats must be bf16 \[>= 4, 128\]"):
        ops.class_logits_bwd(*args, 1, 4, dhead=True, feats=d["feats"][:3])
    with pytest.raises(TypeError, match="feats must be torch.bfloat16"):
        ops.class_logits_bwd(*args, 1, 4, dhead=True, feats=d["feats"].float())
    with pytest.raises(ValueError, match=r"dhead must be f32 \[258\]"):
        ops.class_logits_bwd(*args, 1, 4, dhead=torch.zeros(256, device=DEV), feats=d["feats"])
    with pytest.raises(ValueError, match=r"rowgrad must hold \[4, 2\] floats"):
        ops.class_logits_bwd(*args, 1, 4, dhead=True, feats=d["feats"], rowgrad=torch.zeros(3, 2, device=DEV))
    with pytest.raises(ValueError, match="rowgrad is the scratch of dhead"):
        ops.class_logits_bwd(*args, 1, 4, rowgrad=torch.zeros(4, 2, device=DEV))
    small = ops.class_logits_bwd_workspace_bytes(1, 4, 1, 1, 64, True)
    assert ops.class_logits_bwd_head_workspace_bytes(1, 4, 1, 1, 64, 128, True) == small + 8 * 258
    with pytest.raises(ValueError, match=r"workspace must hold \d+ bytes \(class_logits_bwd_head_workspace_bytes\)"):
        ops.class_logits_bwd(*args, 1, 4, dhead=True, feats=d["feats"], workspace=torch.zeros(small, dtype=torch.uint8, device=DEV))
    out = ops.class_logits_bwd(*args, 1, 4, dhead=True, feats=d["feats"])
    assert len(out) == 4 and out[3].shape == (258,) and len(ops.class_logits_bwd(*args, 1, 4)) == 3
