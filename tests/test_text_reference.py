"""CPU: the references, bounds, profiles and simulations of tests/text_reference.py held against each other.  The simulation without rounding (float64)
equals the exact reference; the f32 simulation sits inside every bound at every shape and profile the GPU test runs (the worst |err| / tol is printed);
every planted error lands outside a bound on a listed case -- a condition on the bounds, not a measurement; the profiles reach what they claim."""
import pytest
import torch

from tests import text_reference as R

SEED = 5
F64 = torch.float64


def _attn(profile, shape, hooks=(), **kw):
    N, S, H = shape
    qkv = R.make_attn_inputs(profile, N, S, H, SEED)
    return qkv, R.emulate_attention(qkv, N, S, H, hooks=hooks, **kw)


def _pool_case(profile, shape, kind):
    N, S, W, P = shape
    return R.make_pool_inputs(profile, N, S, W, P, SEED), R.make_ids(kind, N, S, SEED)


def _pool(inp, ids, hooks=(), **kw):
    return R.emulate_pool(inp["x"], ids, inp["gamma"], inp["beta"], inp["wproj"], R.EPS, hooks=hooks, **kw)


def _pool_exact(inp, ids):
    return R.exact_pool(inp["x"], ids, inp["gamma"], inp["beta"], inp["wproj"], R.EPS)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the simulation with every rounding off is the exact reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", R.ATTN_PROFILES)
@pytest.mark.parametrize("shape", [(2, 2, 1), (3, 16, 8), (2, 63, 2)], ids=str)
def test_attention_simulation_without_rounding_is_exact(profile, shape):
    qkv, got = _attn(profile, shape, dtype=F64)
    ref = R.exact_attention(qkv, *shape)["out"]
    assert float((got - ref).abs().max()) <= 1e-12 * (1.0 + float(ref.abs().max()))


@pytest.mark.parametrize("profile", R.POOL_PROFILES)
@pytest.mark.parametrize("shape", R.POOL_SHAPES[:4], ids=str)
def test_pool_simulation_without_rounding_is_exact(profile, shape):
    inp, ids = _pool_case(profile, shape, "tie")
    got = _pool(inp, ids, dtype=F64)
    ref = _pool_exact(inp, ids)["out"]
    # flat rows: d is a rounding residue of the float64 mean in both, amplified by rstd = 316
    assert float((got - ref).abs().max()) <= (1e-9 if profile == "flat" else 1e-12)


def test_embed_simulation_is_the_f32_sum_and_within_a_rounding_of_exact():
    for N, S, W, vocab in R.EMBED_SHAPES:
        inp = R.make_embed_inputs(N, S, W, vocab, SEED)
        inp["ids"].view(-1)[0] = -1
        inp["ids"].view(-1)[-1] = 2 ** 40
        ref = R.exact_embed(**inp)
        got = R.emulate_embed(**inp)
        assert torch.equal(got, R.embed_f32(**inp))
        if N * S > 1:                                                                                   # the clamp, as text.hip:16 documents it
            assert torch.equal(ref[0], inp["tok"][0].double() + inp["pos"][0].double())
        assert torch.equal(ref[-1], inp["tok"][vocab - 1].double() + inp["pos"][(N * S - 1) % S].double())
        R.check("embed", got, ref, R.bounds_embed(ref))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the f32 simulation sits inside the bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", R.ATTN_PROFILES)
@pytest.mark.parametrize("shape", R.ATTN_SHAPES, ids=str)
def test_attention_simulation_within_bounds(profile, shape):
    qkv, got = _attn(profile, shape)
    r = R.exact_attention(qkv, *shape)
    worst = R.check(f"attention {profile} {shape}", got, r["out"], R.bounds_attention(r))
    print(f"TEXTREF-CPU attention {profile:10s} {shape} worst err/tol {worst:.3f}")


@pytest.mark.parametrize("profile", R.POOL_PROFILES)
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=str)
def test_pool_simulation_within_bounds(profile, shape):
    for kind in R.EOS_KINDS:
        inp, ids = _pool_case(profile, shape, kind)
        r = _pool_exact(inp, ids)
        tol = R.bounds_pool(r)
        got = _pool(inp, ids)
        worst = R.check(f"pool {profile} {shape} {kind}", got, r["out"], tol["out"])
        nerr = float((got.double().norm(dim=1) - 1.0).abs().max())
        assert nerr <= tol["norm"]
        print(f"TEXTREF-CPU pool {profile:8s} {shape} {kind:9s} worst err/tol {worst:.3f}  norm err/tol {nerr / tol['norm']:.3f}")


@pytest.mark.parametrize("W,P", [(64, 64), (64, 40), (320, 7), (512, 512), (768, 768), (200, 300)])
def test_chain_lengths_are_the_ones_the_simulation_performs(W, P):
    c = {}
    inp, ids = _pool_case("randn", (2, 3, W, P), "last")
    _pool(inp, ids, counts=c)
    assert c["n_stat"] == R.n_stat(W) == (W + 255) // 256 + 6 + 3
    assert c["n_proj"] == R.n_proj(W) == (W + 63) // 64 + 6
    assert c["n_norm"] == R.n_norm(P) == (P + 255) // 256 + 6 + 3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# every planted error lands outside a bound
# ---------------------------------------------------------------------------------------------------------------------------------------------
ATTN_PLANTS = [        # (hook, profile, shape): the case on which the bound must reject it
    ("mask_lt", "randn", (2, 2, 1)), ("mask_lt", "randn", (3, 16, 8)),
    ("mask_le_ip1", "randn", (2, 2, 1)), ("mask_le_ip1", "randn", (3, 16, 8)), ("mask_le_ip1", "late_spike", (2, 63, 2)),
    ("no_scale", "randn", (3, 16, 8)), ("scale_twice", "randn", (3, 16, 8)),
    ("no_corr_acc", "ascending", (3, 16, 8)), ("no_corr_acc", "late_spike", (2, 64, 3)),
    ("no_corr_l", "ascending", (3, 16, 8)), ("no_corr_l", "late_spike", (2, 64, 3)),
    ("v_from_k", "randn", (3, 16, 8)), ("no_head_offset", "randn", (3, 16, 8)), ("no_head_offset", "randn", (1, 17, 12)),
]


def _rejected(got, ref, tol):
    return float(R.ratios(got, ref, tol).max()) > 1.0


@pytest.mark.parametrize("hook,profile,shape", ATTN_PLANTS, ids=str)
def test_attention_bounds_reject_planted_error(hook, profile, shape):
    qkv, got = _attn(profile, shape, hooks=(hook,))
    r = R.exact_attention(qkv, *shape)
    assert _rejected(got, r["out"], R.bounds_attention(r)), f"{hook} passes the bound on {profile} {shape}"


@pytest.mark.parametrize("profile,shape", [("randn", (3, 16, 8)), ("ascending", (2, 63, 2))], ids=str)
def test_attention_bounds_reject_one_bf16_ulp(profile, shape):
    """One output moved by one bf16 ulp away from zero, at the element where that shows most: the correct rounding already went away from zero there and the
    value sits low in its binade (u |out| is half an ulp at the bottom of a binade and a whole one at its top)."""
    qkv, got = _attn(profile, shape)
    r = R.exact_attention(qkv, *shape)
    tol = R.bounds_attention(r)
    ulp = torch.exp2(torch.floor(torch.log2(got.double().abs().clamp(min=2.0 ** -120))) - 7.0)
    away = (got.double().abs() - r["out"].abs() + ulp) / tol
    at = tuple(int(v) for v in (away == away.max()).nonzero()[0])
    _, planted = _attn(profile, shape, plant_ulp=at)
    assert int((R.bits(planted.to(torch.bfloat16)) != R.bits(got.to(torch.bfloat16))).sum()) == 1
    assert _rejected(planted, r["out"], tol)


POOL_PLANTS = [        # (hook, profile, shape, eos kind)
    ("last_eos", "randn", (5, 16, 64, 40), "tie"), ("last_eos", "offset", (2, 7, 320, 7), "tie"),
    ("var_wm1", "randn", (5, 16, 64, 40), "first"), ("var_wm1", "randn", (2, 16, 768, 768), "last"),
    ("no_eps", "flat", (5, 16, 64, 40), "first"), ("no_eps", "flat", (3, 16, 512, 512), "tie"),
    ("wproj_T", "randn", (3, 16, 512, 512), "last"), ("wproj_T", "randn", (1, 1, 64, 64), "first"), ("wproj_T", "randn", (5, 16, 64, 40), "last"),
    ("wproj_T", "randn", (2, 7, 320, 7), "first"),
    ("no_norm", "randn", (5, 16, 64, 40), "first"), ("no_norm", "randn", (3, 16, 512, 512), "tie"),
    ("drop_wave3", "offset", (2, 7, 320, 7), "first"), ("drop_wave3", "randn", (3, 16, 512, 512), "last"),
    ("one_pass", "offset", (2, 16, 768, 768), "first"),
]


@pytest.mark.parametrize("hook,profile,shape,kind", POOL_PLANTS, ids=str)
def test_pool_bounds_reject_planted_error(hook, profile, shape, kind):
    inp, ids = _pool_case(profile, shape, kind)
    r = _pool_exact(inp, ids)
    tol = R.bounds_pool(r)
    got = _pool(inp, ids, hooks=(hook,))
    out_bad = _rejected(got, r["out"], tol["out"])
    norm_bad = not bool(((got.double().norm(dim=1) - 1.0).abs() <= tol["norm"]).all())
    assert out_bad, f"{hook} passes the elementwise bound on {profile} {shape} {kind}"
    if hook == "no_norm":
        assert norm_bad


def test_embed_bounds_reject_planted_errors():
    N, S, W, vocab = 3, 5, 128, 97                       # N != S: m / S and m % S differ from row 1 on
    inp = R.make_embed_inputs(N, S, W, vocab, SEED)
    ref = R.exact_embed(**inp)
    assert _rejected(R.emulate_embed(**inp, hooks=("pos_div",)), ref, R.bounds_embed(ref))
    inp["ids"][1, 2], inp["ids"][2, 0] = -1, vocab
    ref = R.exact_embed(**inp)
    R.check("embed clamp", R.emulate_embed(**inp), ref, R.bounds_embed(ref))
    assert _rejected(R.emulate_embed(**inp, hooks=("no_clamp",)), ref, R.bounds_embed(ref))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the profiles are what they claim
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 16, 8), (2, 64, 3)], ids=str)
def test_attention_profiles_reach_what_they_claim(shape):
    N, S, H = shape
    s = {p: R.exact_attention(R.make_attn_inputs(p, N, S, H, SEED), N, S, H)["s"] for p in R.ATTN_PROFILES}
    last = s["ascending"][..., S - 1, :]                                  # the last query sees every key
    gaps = last[..., 1:] - last[..., :-1]
    assert float(gaps.min()) > 6.0 and float(gaps.max()) < 12.0           # every later key beats the running maximum by about 8
    for i in (1, S // 2, S - 1):                                          # ... for every query, over the keys it sees
        g = s["ascending"][..., i, 1:i + 1] - s["ascending"][..., i, :i]
        assert float(g.min()) > 6.0
    d = s["descending"]
    keep = R._causal(S, d.device)
    assert bool((d[..., :, :1] >= d.masked_fill(~keep, float("-inf"))).all())        # key 0 holds the maximum of every row: corr == 1 after it
    sf = s["sink_first"][..., 1:, :]
    over = sf[..., :1] - sf[..., 1:].masked_fill(~keep[1:, 1:], float("-inf")).max(-1, keepdim=True).values
    assert 40.0 < float(over.min()) and 50.0 < float(over.median()) < 65.0 and float(over.max()) < 80.0
    ls = s["late_spike"][..., S - 2:, :]                                   # rows >= S - 2 see the spike
    rest = ls[..., :S - 2].max(-1).values
    assert float((ls[..., S - 2] - rest).min()) > 60.0 and float((ls[..., S - 2] - rest).median()) > 70.0
    eq = s["equal"]
    assert bool((eq == eq[..., :1]).all())


def test_pool_profiles_reach_what_they_claim():
    inp, ids = _pool_case("offset", (2, 16, 768, 768), "first")
    x = inp["x"].double()
    assert float(x.mean(1).abs().min()) > 99.0 and 0.8 < float(x.std(1).mean()) < 1.2
    r = _pool_exact(inp, ids)
    one_pass = _pool(inp, ids, hooks=("one_pass",))
    assert _rejected(one_pass, r["out"], R.bounds_pool(r)["out"])          # a one-pass variance fails here
    inp, ids = _pool_case("flat", (5, 16, 64, 40), "tie")
    assert bool((inp["x"] == inp["x"][:, :1]).all())
    r = _pool_exact(inp, ids)
    assert float((r["y"] - inp["beta"].double()).abs().max()) < 1e-6       # y = beta up to eps
    inp, ids = _pool_case("outlier", (3, 16, 512, 512), "last")
    big = inp["x"].abs() >= 64.0
    assert bool(big[:, 0].all()) and bool(big[:, -1].all()) and int(big.sum(1).max()) <= 4
    for kind, want in (("first", 0), ("last", 15), ("tie", 8), ("all_equal", 0)):
        assert R.first_max(R.make_ids(kind, 4, 16, SEED)).tolist() == [want] * 4
    tie = R.make_ids("tie", 4, 16, SEED)
    assert R.last_max(tie).tolist() == [15] * 4 and int((tie == tie.max()).sum()) == 8
    for _, _, shape in [(0, 0, s) for s in R.POOL_SHAPES]:                 # no case projects to an exact-zero row (the one input HF makes NaN)
        for p in R.POOL_PROFILES:
            inp, ids = _pool_case(p, shape, "tie")
            assert float(_pool_exact(inp, ids)["nrm"].min()) > 0.0
