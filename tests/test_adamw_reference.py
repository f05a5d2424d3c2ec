"""The AdamW step without a GPU: the float64 reference and its derived bounds (tests/adamw_reference.py) hold both f32 emulations of the kernels'
expression sequence (unfused and contracted) on every input profile, and every named wrong variant leaves them.

Where each mutant leaves the bound (WHERE below: profile, hyper-parameter set, step, (grad_scale, coef), output), with the factor
max |got - ref| / bound printed by test_every_mutant_leaves_the_bound:
    eps inside the root                        p' 1.6e4      eps added before the division by bc2_sqrt     p' 1.7e5
    bias correction on v missing               p' 1.0e6      bias correction on v not rooted               p' 8.7e4
    bc1 missing                                p' 2.5e4      decay applied after the update                p' 1.5e2
    L2 decay instead of decoupled decay        m' 6.5e7      beta2 used for m                              m' 3.7e6
    v fed the unscaled gradient                v' 5.9e7
against at most 0.99 for the two correct emulations over every profile, set, step and scale (test_both_emulations_stay_inside_the_bounds prints the
largest per profile and set).
"""
import numpy as np
import pytest

from tests import adamw_reference as R

N = 4096
# lr, wd, beta1, beta2, eps: the reference run's; the existing tests'; other betas and eps without decay
HYPERS = {"run": (3e-6, 0.1, 0.9, 0.999, 1e-8), "lr3e-3": (3e-3, 0.1, 0.9, 0.999, 1e-8), "b8_9": (1e-3, 0.0, 0.8, 0.9, 1e-6)}
STEPS = (1, 2, 7, 1000, 100000)
SCALES = ((1.0, 1.0), (-0.5, 0.37))


def _case(profile, hyper, step, scale, n=N):
    lr, wd, b1, b2, eps = HYPERS[hyper]
    gs, coef = scale
    p, g, m, v = R.profile(profile, n, seed=step, beta1=b1, scale=gs * R.f32(coef))
    kw = dict(lr=np.float32(lr), wd=np.float32(wd), beta1=b1, beta2=b2, eps=eps, grad_scale=gs)
    ref = R.step_reference(p, g, m, v, step=step, coef=R.f32(coef), **kw)          # (an f32 coefficient handed over exactly: no allowance)
    bc1, bc2 = R.host_bias_corrections(b1, b2, step)
    return (p, g, m, v), dict(kw, bc1=bc1, bc2_sqrt=bc2, coef=coef), ref


@pytest.mark.parametrize("hyper", list(HYPERS))
@pytest.mark.parametrize("profile", R.PROFILES)
def test_both_emulations_stay_inside_the_bounds(profile, hyper):
    worst = {}
    for step in STEPS:
        for scale in SCALES:
            x, kw, ref = _case(profile, hyper, step, scale)
            for contracted in (False, True):
                f = R.miss_factors(*R.emulate(*x, contracted=contracted, **kw), ref)
                for k, val in f.items():
                    assert val <= 1.0, (profile, hyper, step, scale, contracted, k, val)
                    worst[k] = max(worst.get(k, 0.0), val)
    print(f"{profile} {hyper}: largest miss factors " + " ".join(f"{k} {val:.3f}" for k, val in worst.items()))


def test_single_group_form_without_a_coefficient():
    """adamw_kernel has no coefficient: one rounding on gg."""
    for profile in R.PROFILES:
        p, g, m, v = R.profile(profile, N, seed=3)
        kw = dict(lr=np.float32(3e-3), wd=np.float32(0.1), beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=-0.5)
        ref = R.step_reference(p, g, m, v, step=3, **kw)
        bc1, bc2 = R.host_bias_corrections(0.9, 0.999, 3)
        for contracted in (False, True):
            f = R.miss_factors(*R.emulate(p, g, m, v, bc1=bc1, bc2_sqrt=bc2, contracted=contracted, **kw), ref)
            assert max(f.values()) <= 1.0, (profile, contracted, f)


def test_bounds_are_rounding_bounds():
    """Not a loose envelope: on unit-scale inputs the bounds are a few u of the values themselves (p: of |p| plus the update).  Step 1000: at small steps
    the allowance on bc2_sqrt, where 1 - beta2^t cancels, rightly dominates the bound of p."""
    x, kw, ref = _case("unit", "lr3e-3", 1000, (1.0, 1.0))
    p, g, m, v = (a.astype(np.float64) for a in x)
    assert float(np.max(ref["bound_v"] / ref["v"])) < 12 * R.U
    assert float(np.max(ref["bound_m"] / (0.9 * np.abs(m) + 0.1 * np.abs(g)))) < 6 * R.U
    terms = 3e-3 / (1.0 - 0.9 ** 1000) *(0.9 * np.abs(m) + 0.1 * np.abs(g)) / ref["denom"]          # the update with the two terms of m' not cancelling
    assert float(np.max(ref["bound_p"] / (np.abs(p) + terms))) < 40 * R.U


# mutant -> (profile, hyper, step, (grad_scale, coef), output) where it is shown to leave the bound
WHERE = {
    "eps_inside_root": ("eps_band", "run", 1000, (1.0, 1.0), "p"),
    "eps_before_bc2": ("eps_band", "lr3e-3", 7, (1.0, 1.0), "p"),
    "no_bc2": ("unit", "lr3e-3", 7, (1.0, 1.0), "p"),
    "bc2_not_rooted": ("unit", "lr3e-3", 7, (1.0, 1.0), "p"),
    "no_bc1": ("unit", "lr3e-3", 2, (1.0, 1.0), "p"),
    "decay_after_update": ("fresh", "lr3e-3", 1, (1.0, 1.0), "p"),
    "l2_decay": ("unit", "lr3e-3", 7, (1.0, 1.0), "m"),
    "beta2_for_m": ("unit", "run", 7, (1.0, 1.0), "m"),
    "v_unscaled_grad": ("unit", "run", 7, (-0.5, 0.37), "v"),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    profile, hyper, step, scale, out = WHERE[mutant]
    x, kw, ref = _case(profile, hyper, step, scale)
    f = R.miss_factors(*R.emulate(*x, mutant=mutant, **kw), ref)
    print(f"{mutant}: {profile} {hyper} step {step} scale {scale}: " + " ".join(f"{k} {val:.3e}" for k, val in f.items()))
    assert f[out] > 100.0, (mutant, f)


def test_every_mutant_over_all_profiles():
    """The largest factor of each mutant over every profile / set / step / scale, for the record; each must leave some bound somewhere."""
    for mutant in R.MUTANTS:
        best = (0.0, None)
        for profile in R.PROFILES:
            for hyper in HYPERS:
                for step in (1, 2, 1000):
                    for scale in SCALES:
                        x, kw, ref = _case(profile, hyper, step, scale, n=256)
                        with np.errstate(all="ignore"):
                            f = R.miss_factors(*R.emulate(*x, mutant=mutant, **kw), ref)
                        k = max(f, key=lambda key: f[key])
                        if f[k] > best[0]:
                            best = (f[k], (profile, hyper, step, scale, k))
        print(f"{mutant}: largest factor {best[0]:.3e} at {best[1]}")
        assert best[0] > 100.0, mutant


@pytest.mark.parametrize("beta", [0.9, 0.999, 0.8])
def test_bias_correction_allowance_covers_the_f32_host_arithmetic(beta):
    worst = 0.0
    for step in list(range(1, 2001)) + [10 ** 4, 10 ** 5, 2 ** 24 + 1]:
        B1, R1, B2, R2 = R.bias_corrections(beta, beta, step)
        bc1, bc2 = R.host_bias_corrections(beta, beta, step)
        e1, e2 = abs(float(bc1) - B1) / B1, abs(float(bc2) - B2) / B2
        if step == 1:
            assert e1 == 0.0 == R1 and R2 == pytest.approx(R.U, rel=1e-6)          # powf(x, 1) and Sterbenz: only the root rounds
        assert e1 <= R1 and e2 <= R2, (beta, step, e1, R1, e2, R2)
        if R1 > 0:
            worst = max(worst, e1 / R1, e2 / R2)
    B1, R1, B2, R2 = R.bias_corrections(0.9, 0.999, 2)
    assert 5e2 * R.U < R2 < R1 * 1e3 and 5e2 * R.U < 2 * R2 < 2e3 * R.U            # the cancellation at step 2: about 1e3 u on 1 - beta2^2, half after the root
    print(f"beta {beta}: largest |bc - B| / (B R) = {worst:.3f}")


@pytest.mark.parametrize("contracted", [False, True])
def test_zero_lr_leaves_p_bit_for_bit(contracted):
    """lr = 0 (with decay) and wd = 0 with lr = 0: p keeps its bits, m and v still move."""
    for profile in R.PROFILES:
        for wd in (0.1, 0.0):
            p, g, m, v = R.profile(profile, N, seed=5)
            bc1, bc2 = R.host_bias_corrections(0.9, 0.999, 2)
            p1, m1, v1 = R.emulate(p, g, m, v, lr=np.float32(0.0), wd=np.float32(wd), beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, bc1=bc1,
                                   bc2_sqrt=bc2, contracted=contracted)
            assert p1.tobytes() == p.tobytes(), (profile, wd)
            if profile not in ("zero_grad",):
                assert not np.array_equal(m1, m) and not np.array_equal(v1, v), profile
            ref = R.step_reference(p, g, m, v, lr=np.float32(0.0), wd=np.float32(wd), beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, step=2)
            assert np.array_equal(ref["p"], p.astype(np.float64)) and max(R.miss_factors(p1, m1, v1, ref).values()) <= 1.0


@pytest.mark.parametrize("hyper", list(HYPERS))
def test_a_wrong_segment_row_leaves_the_bound(hyper):
    """Rows 15 % apart in lr with wd alternating (the GPU test's tables): the neighbouring row's values are outside the bound of p', the reference run's
    learning rate included."""
    n, ends = 1028, [4, 12, 16, 24, 512, 516, 1028]
    lr, wd, b1, b2, eps = HYPERS[hyper]
    seg_lr = np.array([lr * 1.15 ** s for s in range(len(ends))], dtype=np.float32)
    seg_wd = np.array([(wd or 0.05) * (s % 2) for s in range(len(ends))], dtype=np.float32)
    p, g, m, v = R.profile("unit", n, seed=2)
    kw = dict(beta1=b1, beta2=b2, eps=eps, grad_scale=1.0)
    ref = R.step_reference(p, g, m, v, lr=R.rows(ends, seg_lr, n), wd=R.rows(ends, seg_wd, n), step=2, **kw)
    bc1, bc2 = R.host_bias_corrections(b1, b2, 2)
    right = R.emulate(p, g, m, v, lr=R.rows(ends, seg_lr, n), wd=R.rows(ends, seg_wd, n), bc1=bc1, bc2_sqrt=bc2, **kw)
    wrong = R.emulate(p, g, m, v, lr=R.rows(ends, np.roll(seg_lr, 1), n), wd=R.rows(ends, np.roll(seg_wd, 1), n), bc1=bc1, bc2_sqrt=bc2, **kw)
    f_right, f_wrong = R.miss_factors(*right, ref)["p"], R.miss_factors(*wrong, ref)["p"]
    print(f"{hyper}: the right rows {f_right:.3f}, the neighbouring rows {f_wrong:.3e}")
    assert f_right <= 1.0 < 10.0 < f_wrong


def test_rows_and_clip_coefficient():
    ends, lr = [4, 12, 16, 24], [1.0, 2.0, 3.0, 4.0]
    got = R.rows(ends, lr, 24)
    assert got.dtype == np.float32 and got.tolist() == [1.0] * 4 + [2.0] * 8 + [3.0] * 4 + [4.0] * 8
    g = np.full(16, 0.5, dtype=np.float32)                       # norm 2
    assert R.clip_coef(g, 1.0, 0.0) == (None, 0.0)
    c, rel = R.clip_coef(g, -0.5, 0.25)                          # scaled norm 1
    assert c == pytest.approx(0.25 / (1.0 + 1e-6), rel=1e-15) and R.U < rel < 1.001 * R.U
    assert R.clip_coef(g, 1.0, 5.0)[0] == 1.0
