"""The attention reference helper (tests/attention_reference.py) checked on the CPU: its closed forms against float64 autograd, its emulation against
its exact form, and its bounds against an f32 simulation of the kernels' arithmetic -- wide enough for a correct kernel, and violated by three
deliberately broken ones.  The GPU tests (test_attention_reference_gpu.py) hold the HIP kernels to the same bounds; only here can a kernel be broken
on purpose."""
import math

import pytest
import torch

from tests import attention_reference as R

SCALE = 0.125


def _chunk(profile, T, seed=0, b=0, h=0):
    x, dO = R.make_inputs(profile, 1, 2, T, seed)
    return x[b, :, 0, h].double(), x[b, :, 1, h].double(), x[b, :, 2, h].double(), dO[b, :, h].double()


@pytest.mark.parametrize("profile", ["randn", "sink_last", "big_lse"])
def test_exact_backward_is_float64_autograd(profile):
    """exact_chunk's closed-form dQ / dK / dV against float64 autograd of softmax(Q K^T scale) V: 1e-12 of each gradient's largest element (float64
    round-off over T = 129 terms is ~1e-14 relative)."""
    q, k, v, dO = _chunk(profile, 129)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = torch.softmax(qa @ ka.t() * SCALE, -1) @ va
    out.backward(dO)
    r = R.exact_chunk(q, k, v, dO, SCALE)
    assert float((r["out"] - out.detach()).abs().max()) <= 1e-12 * float(out.detach().abs().max())
    lse = torch.logsumexp(q @ k.t() * SCALE, -1) / math.log(2.0)
    assert float((r["lse"] - lse).abs().max()) <= 1e-12 * max(1.0, float(lse.abs().max()))
    for name, g in (("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
        assert float((r[name] - g).abs().max()) <= 1e-12 * float(g.abs().max()), name


@pytest.mark.parametrize("profile", ["randn", "sink_first", "big_lse"])
def test_emulation_without_rounding_is_exact(profile):
    """With every rounding point off (and the exact O and LSE handed to the backward) the emulation is the exact reference, to float64 round-off: the two
    differ in the order of the float64 operations only, i.e. by ~2^-53 |score| relative on each P (|score| <= 600 here) times the largest operand
    (big_lse: K feature 0 = 208, under the cancelling sum of dS) -- 1e-11 of max(1, |ref|) max(1, |q|, |k|) is two orders above that."""
    q, k, v, dO = _chunk(profile, 129)
    ex = R.exact_chunk(q, k, v, dO, SCALE)
    fw = R.emul_fwd_exact_scores(q, k, v, SCALE)
    bw = R.emul_bwd_chunk(q, k, v, dO, ex["out"], ex["lse"], SCALE, rounding=frozenset(), with_tol=False)
    for name, got in (("out", fw["out"]), ("lse", fw["lse"]), ("dq", bw["dq"]), ("dk", bw["dk"]), ("dv", bw["dv"]), ("dvec", bw["dvec"])):
        amp = max(1.0, float(q.abs().max()), float(k.abs().max()))
        assert float((got - ex[name]).abs().max()) <= 1e-11 * max(1.0, float(ex[name].abs().max())) * amp, name
    # and each rounding point, switched on alone, moves the result (the switches are wired to something)
    on = R.emul_bwd_chunk(q, k, v, dO, ex["out"], ex["lse"], SCALE, rounding=frozenset({"ks_bwd"}), with_tol=False)
    assert not torch.equal(on["dk"], bw["dk"]) and torch.equal(on["dq"], bw["dq"])
    on = R.emul_bwd_chunk(q, k, v, dO, ex["out"], ex["lse"], SCALE, rounding=frozenset({"qs_bwd"}), with_tol=False)
    assert torch.equal(on["dk"], bw["dk"]) and not torch.equal(on["dq"], bw["dq"])


def _sim_ratios(profile, T):
    q, k, v, dO = _chunk(profile, T, seed=T)
    out, lse = R.simulate_fwd_f32(q, k, v, SCALE)
    fw = R.emul_fwd_chunk(q, k, v, SCALE)
    dq, dk, dv, dvec = R.simulate_bwd_f32(q, k, v, dO, out, lse, SCALE)
    bw = R.emul_bwd_chunk(q, k, v, dO, out, lse, SCALE)
    return {"out": R.worst_ratio(out, fw["out"], fw["tol_out"]), "lse": R.worst_ratio(lse, fw["lse"], fw["tol_lse"]),
            "dq": R.worst_ratio(dq, bw["dq"], bw["tol_dq"]), "dk": R.worst_ratio(dk, bw["dk"], bw["tol_dk"]),
            "dv": R.worst_ratio(dv, bw["dv"], bw["tol_dv"]), "dvec": R.worst_ratio(dvec, bw["dvec"], bw["tol_dvec"])}


@pytest.mark.parametrize("T", [129, 577])
@pytest.mark.parametrize("profile", R.PROFILES)
def test_f32_simulation_stays_inside_the_bounds(profile, T):
    """An f32 simulation of the kernels' arithmetic (bf16 P, bf16 dS, bf16 outputs, f32 sums, (hi, lo) pairs for -lse and -D) against `emul`, every
    profile, T = 129 and 577: the worst |sim - emul| / bound per output must be <= 1.
    Measured worst ratios over the 14 cases: out 0.83 (peaked, T = 577), lse 0.08 (sink_mid80), dq 0.72 (peaked), dk 0.77 (peaked), dv 0.75 (peaked),
    dvec 0.02.  The sink profiles sit at 0.5 - 0.7 (one term owns the sum, so its single rounding is most of the bound), big_lse at 0.13 - 0.30."""
    ratios = _sim_ratios(profile, T)
    print(f"ATTNSIM profile={profile} T={T} " + " ".join(f"{n}={r:.3f}" for n, r in ratios.items()))
    for name, r in ratios.items():
        assert r <= 1.0, (profile, T, name, r)


@pytest.mark.parametrize("T", [129, 577])
def test_leaked_pad_keys_violate_the_lse_bound(T):
    """7 zero pad keys let into the softmax (T = 577 -> Tp = 584 has exactly 7): the LSE moves by log2(1 + 7 / sum_j 2^s_j), far outside the LSE
    bound -- while the output moves by under one bf16 ulp and stays inside ITS bound on most elements: the LSE check is the one that catches it."""
    q, k, v, _ = _chunk("randn", T, seed=T)
    fw = R.emul_fwd_chunk(q, k, v, SCALE)
    out, lse = R.simulate_fwd_f32(q, k, v, SCALE)
    assert R.worst_ratio(lse, fw["lse"], fw["tol_lse"]) <= 1.0
    out, lse = R.simulate_fwd_f32(q, k, v, SCALE, defect="leak7")
    ratio = R.worst_ratio(lse, fw["lse"], fw["tol_lse"])
    print(f"leak7 T={T}: lse ratio {ratio:.1f}, out ratio {R.worst_ratio(out, fw['out'], fw['tol_out']):.2f}")
    assert ratio > 1.0
    assert bool(((lse.double() - fw["lse"]).abs() > fw["tol_lse"]).all())        # every row, not a lucky one


@pytest.mark.parametrize("T", [129, 577])
def test_duplicated_last_key_violates_the_output_bound_under_sink_last(T):
    """The clamped duplicate of row T - 1 let into the softmax doubles the weight of key T - 1.  Under sink_last the contested queries (sink weight
    about one half) move by a large fraction of |v_sink|: outside the output bound."""
    q, k, v, _ = _chunk("sink_last", T, seed=T)
    fw = R.emul_fwd_chunk(q, k, v, SCALE)
    out, lse = R.simulate_fwd_f32(q, k, v, SCALE)
    assert R.worst_ratio(out, fw["out"], fw["tol_out"]) <= 1.0
    out, lse = R.simulate_fwd_f32(q, k, v, SCALE, defect="dup_last")
    bad_rows = ((out.double() - fw["out"]).abs() > fw["tol_out"]).any(-1)
    print(f"dup_last T={T}: out ratio {R.worst_ratio(out, fw['out'], fw['tol_out']):.1f}, rows off {int(bad_rows.sum())}/{T}")
    assert int(bad_rows.sum()) >= T // 16                                      # at least half of the contested queries (every 8th)
    assert R.worst_ratio(lse, fw["lse"], fw["tol_lse"]) > 1.0


@pytest.mark.parametrize("profile", ["randn", "peaked"])
def test_dropped_tile_without_renormalisation_violates_the_output_bound(profile):
    """A 64-key tile missing from the PV product while the row sum keeps it."""
    q, k, v, _ = _chunk(profile, 577, seed=5)
    fw = R.emul_fwd_chunk(q, k, v, SCALE)
    out, _ = R.simulate_fwd_f32(q, k, v, SCALE, defect="drop_tile")
    bad_rows = ((out.double() - fw["out"]).abs() > fw["tol_out"]).any(-1)
    print(f"drop_tile {profile}: out ratio {R.worst_ratio(out, fw['out'], fw['tol_out']):.1f}, rows off {int(bad_rows.sum())}/577")
    assert int(bad_rows.sum()) > 577 // 2


def test_profiles_are_what_they_claim():
    """The crafted profiles reach the score ranges they are named for (float64, exact scores)."""
    for T in (129, 577):
        for prof, j in (("sink_first", 0), ("sink_last", T - 1)):
            q, k, v, _ = _chunk(prof, T, seed=T)
            s = q @ k.t() * R.C
            p = torch.softmax(s * math.log(2.0), -1)
            cont = torch.arange(T) % 8 == 3
            assert float((p[~cont, j] > 0.99).double().mean()) > 0.9          # the sink owns most queries
            assert float(s[~cont, j].median()) > 100.0                        # with scores in the hundreds
            assert float(((p[cont, j] > 0.1) & (p[cont, j] < 0.9)).double().mean()) > 0.9   # the contested queries share
        q, k, v, _ = _chunk("big_lse", T, seed=T)
        lse = R.exact_chunk(q, k, v, None, SCALE)["lse"]
        assert float(lse[0::2].min()) > 280.0 and float(lse[1::2].max()) < -280.0
        for above in (80, 120):
            q, k, v, _ = _chunk(f"sink_mid{above}", T, seed=T)
            s = q @ k.t() * R.C
            key = R.sink_mid_key(T)
            assert key >= 64 and abs(float(s[:, key].min()) - above) < 0.5 and abs(float(s[:, key].max()) - above) < 0.5
            s[:, key] = 0.0
            assert float(s.abs().max()) < 1.0
