"""Float64 reference and derived error bound for the exponential moving average of the trainable bucket (csrc/optim_ema.hip).

What the kernels compute, per element and per update t = 1, 2, ... (owl_ema_update, and the tail of owl_adamw_step_ema):

    s_t  = fl(w_t p_t)                        __fmul_rn: one rounding
    E^_t = fl(d_t E^_{t-1} + s_t)             __fmaf_rn: one rounding of the exact d_t E^_{t-1} + s_t

with f32 d_t, w_t handed over by the host and the f32 parameters p_t the step has just produced.  The reference takes exactly those f32 values as
GIVEN inputs (it does not ask whether w_t is a good 1 - d_t, nor where p_t comes from) and runs the recursion in float64:

    E_t = d_t E_{t-1} + w_t p_t,      E_0 = E^_0 = the seed.

The bound.  Write E^_t = E_t + e_t with |e_t| <= B_t, B_0 = 0, and u = 2^-24 (round to nearest, f32).  With |a1|, |a2| <= u:

    s_t  = w_t p_t (1 + a1)
    E^_t = (d_t (E_{t-1} + e_{t-1}) + w_t p_t (1 + a1)) (1 + a2)
         = E_t + d_t e_{t-1} + a1 w_t p_t + a2 (E_t + d_t e_{t-1} + a1 w_t p_t)

so, d_t >= 0,

    |e_t| <= (1 + u) (d_t B_{t-1} + u |w_t p_t|) + u |E_t|  =:  B_t.

This is the issue's B_t = d_t B_{t-1} + u (|w_t p_t| + |E_t|) with the second-order terms (the factor 1 + u) carried.  Two small additions, both from
first principles and neither from any measurement:
  * underflow: a rounding whose result is subnormal errs by at most ETA = 2^-150 (half the smallest subnormal) instead of u |x|; ETA is added once per
    rounding, 2 ETA per step;
  * the reference's own arithmetic: the float64 recursion and this bound are evaluated with unit roundoff 2^-53 = u 2^-29, so by the same derivation
    the float64 E_t is off the exact one by at most B_t 2^-29; the bound is returned as B_t (1 + 2^-28), which covers that, the rounding of B_t's own
    evaluation, and the double rounding of an emulation that forms the fused multiply-add in float64 first.
Nothing here is tuned: a result outside B_t has made a rounding the two above do not account for (or used other inputs).

`decays` is the closed form of the per-update decay, written out here independently of optim.ema_decay_at.
"""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -150
SLACK = 1.0 + 2.0 ** -28


def decays(steps: int, decay: float, warmup: bool):
    """-> (d [steps] f32, w [steps] f32): d_t = min(decay, (1 + t) / (10 + t)) with warm-up, else decay, rounded to f32; w_t = 1 - d_t taken in double
    from the f32 d_t, rounded to f32."""
    t = np.arange(1, steps + 1, dtype=np.float64)
    d = np.minimum(float(decay), (1.0 + t) / (10.0 + t)) if warmup else np.full(steps, float(decay))
    d = d.astype(np.float32)
    return d, (1.0 - d.astype(np.float64)).astype(np.float32)


def recursion(seed, params, d, w):
    """seed: f32 array E_0; params: the f32 arrays p_1 .. p_T; d, w: f32 sequences of length T.  -> (E_T, B_T), float64 arrays of seed's shape."""
    assert len(params) == len(d) == len(w)
    seed = np.asarray(seed)
    assert seed.dtype == np.float32
    E = seed.astype(np.float64)
    B = np.zeros_like(E)
    for p, dt, wt in zip(params, d, w):
        p = np.asarray(p)
        assert p.dtype == np.float32 and np.asarray(dt).dtype == np.float32 and np.asarray(wt).dtype == np.float32
        dt, wt = float(dt), float(wt)
        wp = wt * p.astype(np.float64)
        E = dt * E + wp
        B = (1.0 + U) * (dt * B + U * np.abs(wp)) + U * np.abs(E) + 2.0 * ETA
    return E, B * SLACK


def emulate(seed, params, d, w):
    """The kernel's order in numpy: an f32 product, then the fused multiply-add formed in float64 (d E^ is exact there: 24 x 24 bits) and rounded to f32."""
    E = np.asarray(seed, dtype=np.float32).copy()
    for p, dt, wt in zip(params, d, w):
        s = np.float32(wt) * np.asarray(p, dtype=np.float32)
        assert s.dtype == np.float32
        E = (np.float64(dt) * E.astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return E


def miss_factor(got, E, B):
    """max |got - E| / B over the elements: at most 1 inside the bound (B >= 2 ETA > 0 after the first update)."""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - E) / B))
