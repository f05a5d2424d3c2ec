"""The fused attention forward and backward against the float64 references and derived bounds of tests/attention_reference.py, at the tile edges
(T = 37 ... 3601, B H not a multiple of 8), at sink-like score scales, and with every pad row poisoned.

What is pinned: out / lse / dQ / dK / dV / dvec elementwise inside the derived bounds of `emul` (the float64 reference with the kernels' deterministic
rounding points); pad rows untouched (sentinels), whatever the pads of the inputs hold (finite garbage built to hurt if read, or NaN); the `phases`
mask, repeated runs, the batch invariant and lse = None bit for bit.  Against `exact` only a sanity level is asserted.  tests/test_attention_reference.py
shows on the CPU that these bounds hold for a correct f32 kernel and catch a leaked pad key, a duplicated last key and a dropped tile."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402
from tests import attention_reference as R  # noqa: E402

DEV = "cuda"
SCALE = 0.125
OUT_SENTINEL = 7.0
LSE_SENTINEL = -3.0

SHAPES_ALL_PROFILES = [(2, 1, 129), (2, 3, 193), (3, 12, 577), (1, 5, 2305), (2, 12, 2305)]
SHAPES_TWO_PROFILES = [(1, 1, 37), (2, 3, 64), (1, 2, 65), (3, 1, 127), (1, 3, 128), (1, 2, 191), (1, 16, 3601)]
CASES = [(B, H, T, p) for (B, H, T) in SHAPES_ALL_PROFILES for p in R.PROFILES] + \
        [(B, H, T, p) for (B, H, T) in SHAPES_TWO_PROFILES for p in ("randn", "sink_last")]


def _can_peel(T):
    return T >= 65 and (T - 1) % 64 == 0


def _variants(T):
    return (1, 2, 0) if _can_peel(T) else (1,)


class Buffers:
    """qkv / dO rows as the model lays them out, with every row t in [T, Tp) of every image and every row past B Tp poisoned."""

    def __init__(self, x, dO, B, H, T, poison):
        self.B, self.H, self.T = B, H, T
        self.Tp = Tp = (T + 7) // 8 * 8
        self.D = D = H * 64
        self.M = M = B * Tp
        self.rows = rows = ops.pad_rows(M)
        self.x = x.to(DEV)
        self.dO = dO.to(DEV)
        nan = float("nan")
        self.poison = poison
        self.p_big = nan if poison == "nan" else 1e4          # V, dO, O pads
        self.p_lse = nan if poison == "nan" else -1e4          # an lse pad that is read turns P into inf
        qkv = torch.empty(rows, 3 * D, device=DEV, dtype=torch.bfloat16)
        if poison == "nan":
            qkv[:] = nan
        else:
            # Q and K pads = 50 sign(q of the image's token 0): read as a key, it scores ~ 50 |q_0|_1 with query 0
            sgn = torch.sign(self.x[:, 0, 0].reshape(B, D) + 1e-3) * 50.0
            img = sgn[(torch.arange(rows, device=DEV) // Tp).clamp(max=B - 1)]
            qkv[:, :D] = img; qkv[:, D:2 * D] = img; qkv[:, 2 * D:] = self.p_big
        qkv[:M].view(B, Tp, 3 * D)[:, :T] = self.x.reshape(B, T, 3 * D).bfloat16()
        self.qkv = qkv
        do = torch.full((rows, D), self.p_big, device=DEV, dtype=torch.bfloat16)
        do[:M].view(B, Tp, D)[:, :T] = self.dO.reshape(B, T, D).bfloat16()
        self.do = do

    def valid(self, buf):
        return buf[:self.M].view(self.B, self.Tp, -1)[:, :self.T]

    def pads_hold(self, buf, value):
        pad = torch.cat([buf[:self.M].view(self.B, self.Tp, -1)[:, self.T:].reshape(-1), buf[self.M:].reshape(-1)])
        return bool((pad.float() == value).all())

    def forward(self, variant, with_lse=True, counter=None):
        out = torch.full((self.rows, self.D), OUT_SENTINEL, device=DEV, dtype=torch.bfloat16)
        lse = torch.full((self.B, self.H, self.Tp), LSE_SENTINEL, device=DEV) if with_lse else None
        D = self.D
        ops.attention_fwd_vrow(self.qkv, self.qkv[:, D:], self.qkv[:, 2 * D:], 3 * D, out, D, lse, self.B, self.H, self.T, self.Tp, SCALE,
                               variant=variant, slow_tiles=counter)
        return out, lse

    def backward_inputs(self, out, lse):
        """The forward's O and LSE as the backward gets them, their pads poisoned."""
        o = torch.full_like(out, self.p_big)
        self.valid(o)[:] = self.valid(out)
        l = torch.full_like(lse, self.p_lse)
        l[:, :, :self.T] = lse[:, :, :self.T]
        return o, l

    def backward(self, o, l, phases=(0,)):
        dvec = torch.full((self.B, self.H, self.Tp), LSE_SENTINEL, device=DEV)
        dqkv = torch.full_like(self.qkv, OUT_SENTINEL)
        for ph in phases:
            ops.attention_bwd(self.qkv, self.do, o, l, dvec, dqkv, self.B, self.H, self.T, self.Tp, SCALE, phases=ph)
        return dqkv, dvec

    def chunk(self, b, h):
        return self.x[b, :, 0, h].double(), self.x[b, :, 1, h].double(), self.x[b, :, 2, h].double(), self.dO[b, :, h].double()


class Tally:
    """Per tensor: worst |got - emul| / bound, the first offenders, and the squared distances got - exact, emul - exact, |exact|^2."""

    def __init__(self):
        self.t = {}

    def add(self, name, where, got, emul, tol, exact):
        e = self.t.setdefault(name, {"ratio": 0.0, "bad": 0, "n": 0, "first": [], "ge": 0.0, "ee": 0.0, "xx": 0.0})
        got = got.double()
        err = (got - emul).abs()
        bad = ~(err <= tol)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        e["ratio"] = max(e["ratio"], float(ratio.max()))
        e["n"] += err.numel()
        nb = int(bad.sum())
        if nb:
            e["bad"] += nb
            for idx in bad.nonzero()[:max(0, 4 - len(e["first"]))].tolist():
                i = tuple(idx)
                e["first"].append(f"{where}{list(i)}: got {float(got[i]):.6g} emul {float(emul[i]):.6g} bound {float(tol[i]):.3g} exact {float(exact[i]):.6g}")
        e["ge"] += float(((got - exact) ** 2).sum()); e["ee"] += float(((emul - exact) ** 2).sum()); e["xx"] += float((exact ** 2).sum())

    def finish(self, tag):
        fails = []
        for name, e in self.t.items():
            xx = math.sqrt(e["xx"]) if e["xx"] > 0 else 1.0
            d_got, d_emul = math.sqrt(e["ge"]) / xx, math.sqrt(e["ee"]) / xx
            print(f"ATTNREF {tag} tensor={name} ratio={e['ratio']:.3f} got_vs_exact={d_got:.3e} emul_vs_exact={d_emul:.3e}")
            if e["bad"]:
                fails.append(f"{name}: {e['bad']}/{e['n']} outside the bound, worst ratio {e['ratio']:.3f}; " + "; ".join(e["first"]))
            # sanity level against `exact` (not the pin): the P and dS rounding realisations add to the emulation's deterministic prescale shift,
            # hence twice the emulation's own distance, plus one bf16 round-off for the stored output
            if not d_got <= 2.0 * d_emul + R.U:
                fails.append(f"{name}: relative Frobenius distance to exact {d_got:.3e} > 2 x {d_emul:.3e} (emul to exact) + u")
        assert not fails, tag + "\n" + "\n".join(fails)


@pytest.mark.parametrize("poison", ["finite", "nan"])
@pytest.mark.parametrize("B,H,T,profile", CASES)
def test_attention_inside_derived_bounds(B, H, T, profile, poison):
    """Forward (variant 1 everywhere; 2 and 0 where T - 1 is a multiple of 64) and backward of one (shape, profile) with poisoned pads: every valid
    element inside the derived bound of `emul`, pads untouched, lse = None same bits, slow_tiles as the profile predicts.  The measured worst ratios
    are kept in profiles/attention_reference.md."""
    x, dO = R.make_inputs(profile, B, H, T, seed=1)
    bufs = Buffers(x, dO, B, H, T, poison)
    fw = {}
    for variant in _variants(T):
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
        out, lse = bufs.forward(variant, counter=counter)
        assert bufs.pads_hold(out, OUT_SENTINEL), f"variant {variant}: out written in a pad row"
        assert bool((lse[:, :, T:] == LSE_SENTINEL).all()), f"variant {variant}: lse written at t >= T"
        out_nolse, _ = bufs.forward(variant, with_lse=False)
        assert torch.equal(out_nolse, out), f"variant {variant}: lse = None changes the output bits"
        slow = int(counter.item())
        if profile in ("randn", "peaked"):
            assert slow == 0, (variant, slow)
        if profile == "sink_mid120":
            assert slow > 0, (variant, slow)
        fw[variant] = (out, lse)
    if 0 in fw:
        assert torch.equal(fw[0][0], fw[2][0]) and torch.equal(fw[0][1], fw[2][1]), "variant 0 is not the peeled tiling where it can be"
    o_in, lse_in = bufs.backward_inputs(*fw[_variants(T)[-1]])         # the library's choice feeds the backward, as in the model
    dqkv, dvec = bufs.backward(o_in, lse_in)
    assert bufs.pads_hold(dqkv, OUT_SENTINEL), "dqkv written in a pad row"
    assert bool(torch.isfinite(dvec).all()), "dvec_ws not finite"
    g = bufs.valid(dqkv).view(B, T, 3, H, 64)
    tally = Tally()
    for b in range(B):
        for h in range(H):
            q, k, v, d_o = bufs.chunk(b, h)
            ex = R.exact_chunk(q, k, v, d_o, SCALE)
            em = R.emul_fwd_chunk(q, k, v, SCALE)
            em0 = R.emul_fwd_chunk(q[:1], k, v, SCALE, round_qs=False) if _can_peel(T) else None
            where = f"[b={b},h={h}]"
            for variant, (out, lse) in fw.items():
                if variant == 0:
                    continue                                            # same bits as variant 2 (asserted above)
                ref = em
                if variant == 2:                                        # the class-token row scales Q in f32 and does not round it
                    ref = {n: torch.cat([em0[n], em[n][1:]]) for n in ("out", "lse", "tol_out", "tol_lse")}
                tally.add(f"out.v{variant}", where, bufs.valid(out).view(B, T, H, 64)[b, :, h], ref["out"], ref["tol_out"], ex["out"])
                tally.add(f"lse.v{variant}", where, lse[b, h, :T], ref["lse"], ref["tol_lse"], ex["lse"])
            del em, em0
            o_c = bufs.valid(o_in).view(B, T, H, 64)[b, :, h]
            bw = R.emul_bwd_chunk(q, k, v, d_o, o_c, lse_in[b, h, :T], SCALE)
            for i, n in enumerate(("dq", "dk", "dv")):
                tally.add(n, where, g[b, :, i, h], bw[n], bw["tol_" + n], ex[n])
            tally.add("dvec", where, dvec[b, h, :T], bw["dvec"], bw["tol_dvec"], ex["dvec"])
            del bw, ex
    tally.finish(f"profile={profile} B={B} H={H} T={T} poison={poison}")


BITS_CASES = [(2, 3, 193, "randn"), (3, 12, 577, "sink_last"), (1, 5, 2305, "big_lse"), (3, 1, 127, "sink_last"), (1, 2, 65, "randn")]


@pytest.mark.parametrize("B,H,T,profile", BITS_CASES)
def test_backward_phases_and_reruns_give_the_same_bits(B, H, T, profile):
    """The `phases` mask (the two-stream schedule's calls): dvec (1), then dK / dV (2), then dQ (4) as three calls -- and in the order 1, 4, 2 -- give
    the bits of phases = 0; so does a second run of everything."""
    x, dO = R.make_inputs(profile, B, H, T, seed=2)
    bufs = Buffers(x, dO, B, H, T, "nan")
    out, lse = bufs.forward(0)
    out2, lse2 = bufs.forward(0)
    assert torch.equal(out2, out) and torch.equal(lse2, lse), "forward: two runs differ"
    o_in, lse_in = bufs.backward_inputs(out, lse)
    dqkv, dvec = bufs.backward(o_in, lse_in)
    for phases in ((0,), (1, 2, 4), (1, 4, 2)):
        dqkv2, dvec2 = bufs.backward(o_in, lse_in, phases)
        assert torch.equal(dqkv2, dqkv), f"phases {phases}: dqkv differs from phases = 0"
        assert torch.equal(dvec2, dvec), f"phases {phases}: dvec_ws differs from phases = 0"
    # a phase writes its own third of dqkv only
    part, _ = bufs.backward(o_in, lse_in, (1, 2))
    assert bool((part[:, :bufs.D].float() == OUT_SENTINEL).all()) and torch.equal(part[:, bufs.D:], dqkv[:, bufs.D:])
    part, _ = bufs.backward(o_in, lse_in, (1, 4))
    assert bool((part[:, bufs.D:].float() == OUT_SENTINEL).all()) and torch.equal(part[:, :bufs.D], dqkv[:, :bufs.D])


@pytest.mark.parametrize("B,H,T,profile", [(3, 1, 127, "randn"), (3, 12, 577, "randn"), (3, 12, 577, "sink_first"), (3, 2, 2305, "peaked")])
def test_image_of_a_batch_holds_its_batch1_bits(B, H, T, profile):
    """The batch invariant at kernel level: image b of a B = 3 call holds the bits of a B = 1 call on that image alone, forward (each variant) and
    backward."""
    x, dO = R.make_inputs(profile, B, H, T, seed=3)
    bufs = Buffers(x, dO, B, H, T, "finite")
    fw = {v: bufs.forward(v) for v in _variants(T)}
    o_in, lse_in = bufs.backward_inputs(*fw[_variants(T)[-1]])
    dqkv, dvec = bufs.backward(o_in, lse_in)
    for b in range(B):
        one = Buffers(x[b:b + 1], dO[b:b + 1], 1, H, T, "finite")
        for v in _variants(T):
            out1, lse1 = one.forward(v)
            assert torch.equal(one.valid(out1)[0], bufs.valid(fw[v][0])[b]), f"image {b}, variant {v}: out differs from its batch-1 call"
            assert torch.equal(lse1[0, :, :T], fw[v][1][b, :, :T]), f"image {b}, variant {v}: lse differs from its batch-1 call"
        o1, l1 = one.backward_inputs(out1, lse1)
        dqkv1, dvec1 = one.backward(o1, l1)
        assert torch.equal(one.valid(dqkv1)[0], bufs.valid(dqkv)[b]), f"image {b}: dqkv differs from its batch-1 call"
        assert torch.equal(dvec1[0, :, :T], dvec[b, :, :T]), f"image {b}: dvec_ws differs from its batch-1 call"
