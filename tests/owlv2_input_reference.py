"""Float64 restatement, derived error bound and an f32 emulation for csrc/pad_resize.hip (owl_pad_resize_coeffs, owl_preprocess_u8_pad_resize): OWLv2's
input stage.  Checker side: pure numpy, no scipy, no transformers, nothing of the package's Python.

Restatement (float64)
---------
HF's Owlv2ImageProcessorPil: x(1/255), pad bottom / right to a square of side S = max(H, W), scipy.ndimage.gaussian_filter (sigma = max(0, (S/N - 1)/2) per
spatial axis, truncate 4, "mirror"), scipy.ndimage.zoom (order 1, "mirror", grid_mode=True) to N x N, (x - mean) / std.  Per axis both operators are
matrices on the padded length S:
    G [S, S]: G[r, mirror(r + k)] += g_k, k = -lw .. lw, lw = int(4 sigma + 0.5), g_k = exp(-k^2 / (2 sigma^2)) / sum (the identity for sigma <= 1e-15);
    Z [N, S]: centre c_i = (i + 0.5) S/N - 0.5, f = floor(c_i), t = c_i - f: Z[i, mirror(f)] += 1 - t, Z[i, mirror(f + 1)] += t;
    mirror(i) reflects about 0 and S - 1 WITHOUT repeating the edge (period 2 (S - 1); S = 1: always 0).
`axis_matrix(S, N)` = Z G, and the stage is  out = ((A P A^T) rescale - mean) / std  per channel, P the padded image in u8 units (`forward64`).
tests/test_owlv2_input_reference.py holds this to scipy's two calls and to HF's processor.  `variant=` builds the WRONG stages the bound must reject
(PLANTS).  `axis_rows(extent, S, N)` restricts A to the real pixels -- the columns below `extent`; the others multiply the pad -- and trims each row to its
non-zero span: the tables owl_pad_resize_coeffs must emit.

Bound (elementwise, from the kernels' evaluation order; U = 2^-24, gamma(n) = n U / (1 - n U); every operation charges the propagated error of its
operands plus ONE rounding of its result, carried as (value, error) pairs).  All weights and pixels are >= 0, so sum |terms| = the value itself.
 weights          w~ = w (1 + d), |d| <= U (the f64 table rounded once)                                         E_w = U w
 horizontal pass  h~ = fmaf chain over nx taps from 0, u8 -> f32 exact:   h~ <= (1 + U)(1 + gamma(nx)) h         (nx roundings)
 vertical pass    v~ = fmaf chain over ny rows on h~ and w~y:             v~ <= (1 + U)^2 (1 + gamma(nx))(1 + gamma(ny)) v
                  E_v = ((1 + U)^2 (1 + gamma(nx_j)) (1 + gamma(ny_i)) - 1) v
 pad term         (pad_value != 0)  P = 255 pad, P~ = fl(P): E_P = U P;  s~x, s~y = the f64 row sums rounded once: E_s = U s;
                  q = fl(s~x s~y): E_q = (sx + E_sx)(sy + E_sy)(1 + U) - sx sy;   r = fl(1 - q): E_r = E_q + U (r + E_q);
                  v' = fmaf(P~, r~, v~): E_in = E_v + (P + E_P)(r + E_r) - P r,  E_v' = E_in + U (v' + E_in)
 affine           a = fl(rescale / std), b = fl(-mean / std), each formed in f64 and rounded once: E_a = U a, E_b = U |b|;
                  o = fmaf(v', a, b): E_in = (v' + E_v')(a + E_a) - v' a + E_b,  E_o = E_in + U (|o| + E_in)
 bf16             + 2^-8 (|o| + E_o)
 slack            1e-12 (1 + |o|) for the f64 arithmetic of the tables and of this file, and TINY for underflow.
The reference value is forward64's; the pairs' value (v + P r) a + b differs from it only by the rows of A summing to 1 up to f64 rounding.

`emulate` runs the kernels' sequence in numpy float32 (fmaf as an exact f64 product and sum rounded to f32); it serves the CPU test only and is NEVER a
reference on the GPU.
"""
import functools

import numpy as np

U = 2.0 ** -24
U_BF16 = 2.0 ** -8           # bf16 keeps 8 significant bits
TINY = 2.0 ** -126
MAX_RATIO = 16            # owl_pad_resize_coeffs: S <= 16 N
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
RESCALE = 1 / 255

# (H, W) -> N: the GPU test's cases (the issue's list), also the inputs of the planted errors
CASES = ((37, 53, 16), (53, 37, 16), (16, 16, 16), (24, 17, 24), (9, 23, 16), (11, 7, 16), (65, 64, 16), (1, 40, 16), (100, 31, 24), (200, 123, 48),
         (384, 5, 24))
# extra shapes of the CPU comparisons with scipy / HF (the issue's nine: these four beside five of CASES)
EXTRA_SHAPES = ((40, 40, 16), (7, 11, 16), (64, 65, 16), (30, 90, 24))
PLANTS = ("reflect", "trunc3", "sigma_f2", "align", "nohalf", "pad_centred", "warp", "blur_edge", "no_renorm", "u8_mid")


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def case_key(H, W, N):
    return f"{H}x{W}_{N}"


def make_image(H, W, seed=19):
    """Seeded u8 [H, W, 3]: noise (every tap matters) with a saturated and a black block (the ends of the u8 range)."""
    g = np.random.default_rng(1000003 * seed + 1009 * H + W)
    img = g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    img[: max(H // 4, 1), : max(W // 3, 1)] = 255
    img[H - max(H // 5, 1):, W - max(W // 4, 1):] = 0
    return img


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def mirror(i, n, variant=None):
    i = np.asarray(i, np.int64)
    if n <= 1:
        return np.zeros_like(i)
    if variant == "reflect":                     # edge-repeating: d c b a | a b c d | d c b a
        m = i % (2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    period = 2 * (n - 1)
    m = i % period
    return np.where(m < n, m, period - m)


def gauss_matrix(S, sigma, variant=None):
    if not sigma > 1e-15:
        return np.eye(S)
    lw = int((3.0 if variant == "trunc3" else 4.0) * sigma + 0.5)
    k = np.arange(-lw, lw + 1)
    g = np.exp(-0.5 / (sigma * sigma) * k.astype(np.float64) ** 2)
    g = g / (np.exp(-0.5 / (sigma * sigma) * np.arange(-lw - 40, lw + 41, dtype=np.float64) ** 2).sum() if variant == "no_renorm" else g.sum())
    G = np.zeros((S, S))
    r = np.arange(S)
    for kk, gk in zip(k.tolist(), g.tolist()):
        np.add.at(G, (r, mirror(r + kk, S, variant)), gk)
    return G


def zoom_matrix(S, N, variant=None):
    i = np.arange(N, dtype=np.float64)
    if variant == "align":
        c = i * ((S - 1) / (N - 1)) if N > 1 else np.zeros(N)
    elif variant == "nohalf":
        c = i * (S / N)
    else:
        c = (i + 0.5) * (S / N) - 0.5
    f = np.floor(c)
    t = c - f
    Z = np.zeros((N, S))
    o = np.arange(N)
    np.add.at(Z, (o, mirror(f.astype(np.int64), S, variant)), 1.0 - t)
    np.add.at(Z, (o, mirror(f.astype(np.int64) + 1, S, variant)), t)
    return Z


def sigma_of(S, N, variant=None):
    f = S / N
    return f / 2.0 if variant == "sigma_f2" else max(0.0, (f - 1.0) / 2.0)


@functools.lru_cache(maxsize=None)
def axis_matrix(S, N, variant=None):
    """A = Z G [N, S] float64 for one axis of padded length S (cached; read-only)."""
    A = zoom_matrix(S, N, variant) @ gauss_matrix(S, sigma_of(S, N, variant), variant)
    A.setflags(write=False)
    return A


def axis_rows(extent, S, N):
    """A restricted to the columns below `extent` and trimmed per row to its non-zero span -> (first [N] int, count [N] int, rows: list of float64 arrays,
    wsum [N] float64).  A row without a tap on a real pixel: first 0, count 0."""
    A = axis_matrix(S, N)[:, :extent]
    first, count, rows = np.zeros(N, np.int64), np.zeros(N, np.int64), []
    for i in range(N):
        nz = np.flatnonzero(A[i])
        if nz.size:
            first[i], count[i] = nz[0], nz[-1] - nz[0] + 1
        rows.append(A[i, first[i]:first[i] + count[i]].copy())
    return first, count, rows, np.asarray([r.sum() for r in rows])


def padded_u8_units(img, pad_value=0.0, variant=None):
    """[H, W, 3] u8 -> the padded square [S, S, 3] float64 in u8 units; the pad holds 255 * float32(pad_value)."""
    H, W = img.shape[:2]
    S = max(H, W)
    P = np.full((S, S, 3), 255.0 * float(np.float32(pad_value)))
    y0, x0 = ((S - H) // 2, (S - W) // 2) if variant == "pad_centred" else (0, 0)
    P[y0:y0 + H, x0:x0 + W] = img.astype(np.float64)
    return P


def forward64(img, N, pad_value=0.0, mean=CLIP_MEAN, std=CLIP_STD, rescale=RESCALE, variant=None):
    """u8 [H, W, 3] -> [3, N, N] float64: the stage of the module docstring (or, with `variant`, one of the planted errors)."""
    H, W = img.shape[:2]
    S = max(H, W)
    if variant == "warp":                        # per-axis factors H/N, W/N and no pad: the plain resize
        Ay, Ax, P = axis_matrix(H, N), axis_matrix(W, N), img.astype(np.float64)
    elif variant == "blur_edge":                 # the blur mirrored at the image's edge, then the pad, then the zoom
        s = sigma_of(S, N)
        B = np.einsum("ys,swc,xw->yxc", gauss_matrix(H, s), img.astype(np.float64), gauss_matrix(W, s), optimize=True)
        P = np.full((S, S, 3), 255.0 * float(np.float32(pad_value)))
        P[:H, :W] = B
        Ay = Ax = zoom_matrix(S, N)
    else:
        P = padded_u8_units(img, pad_value, variant)
        Ay = Ax = axis_matrix(S, N, variant)
    if variant == "u8_mid":                      # the intermediate rounded to u8, as the Pillow path's is
        h = np.clip(np.rint(np.einsum("swc,xw->sxc", P, Ax)), 0.0, 255.0)
        v = np.einsum("ys,sxc->cyx", Ay, h)
    else:
        v = np.einsum("ys,swc,xw->cyx", Ay, P, Ax, optimize=True)
    m, s = np.asarray(mean, np.float64)[:, None, None], np.asarray(std, np.float64)[:, None, None]
    return (v * rescale - m) / s


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bound
# ---------------------------------------------------------------------------------------------------------------------------------------------
def bound(img, N, pad_value=0.0, bf16=False, mean=CLIP_MEAN, std=CLIP_STD, rescale=RESCALE):
    """-> (ref [3, N, N] = forward64, tol [3, N, N]): the elementwise tolerance of owl_preprocess_u8_pad_resize against forward64 (module docstring)."""
    H, W = img.shape[:2]
    S = max(H, W)
    A = axis_matrix(S, N)
    Ax, Ay = A[:, :W], A[:, :H]
    _, nx, _, sx = axis_rows(W, S, N)
    _, ny, _, sy = axis_rows(H, S, N)
    v = np.einsum("ys,swc,xw->cyx", Ay, img.astype(np.float64), Ax, optimize=True)
    E = ((1.0 + U) ** 2 * (1.0 + gamma(nx))[None, None, :] * (1.0 + gamma(ny))[None, :, None] - 1.0) * v
    pad = float(np.float32(pad_value))
    if pad != 0.0:
        P, E_P = 255.0 * pad, U * 255.0 * pad
        Esx, Esy = U * sx[None, :], U * sy[:, None]
        q = sx[None, :] * sy[:, None]
        E_q = (sx[None, :] + Esx) * (sy[:, None] + Esy) * (1.0 + U) - q
        r = 1.0 - q
        E_r = E_q + U * (np.abs(r) + E_q)
        E_in = E + ((P + E_P) * (np.abs(r) + E_r) - P * np.abs(r))[None]
        v = v + (P * r)[None]
        E = E_in + U * (np.abs(v) + E_in)
    a = (rescale / np.asarray(std, np.float64))[:, None, None]
    b = (-np.asarray(mean, np.float64) / np.asarray(std, np.float64))[:, None, None]
    o = v * a + b
    E_in = (np.abs(v) + E) * (a + U * a) - np.abs(v) * a + U * np.abs(b)
    E = E_in + U * (np.abs(o) + E_in)
    if bf16:
        E = E + U_BF16 * (np.abs(o) + E)
    ref = forward64(img, N, pad_value, mean, std, rescale)
    assert float(np.abs(ref - o).max()) < 1e-11          # the pairs carry forward64's value
    return ref, E + 1e-12 * (1.0 + np.abs(ref)) + TINY


def check(name, got, img, N, pad_value=0.0, bf16=False):
    """Every element of `got` [3, N, N] against forward64 inside the bound -> (worst err / tol, max err, max tol); raises AssertionError naming the element."""
    ref, tol = bound(img, N, pad_value, bf16)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = err / tol
    k = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert ratio[k] <= 1.0, f"{name}: element {k}: got {got[k]!r}, reference {ref[k]!r}, err {err[k]:.3e} > tol {tol[k]:.3e} (err / tol {ratio[k]:.2f})"
    return float(ratio[k]), float(err.max()), float(tol.max())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 emulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def norm_constants(mean=CLIP_MEAN, std=CLIP_STD, rescale=RESCALE):
    """[6] float32: a_c = rescale / std_c, b_c = -mean_c / std_c, each formed in f64 and rounded once (what preprocess.py hands the kernel)."""
    m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return np.concatenate([rescale / s, -m / s]).astype(np.float32)


def emulate(img, N, pad_value=0.0, bf16=False):
    """pr_h_kernel + pr_v_kernel in float32 -> [3, N, N] float32 (bf16: the values a bf16 store holds, as float32)."""
    H, W = img.shape[:2]
    S = max(H, W)
    fx, cx, rx, sx = axis_rows(W, S, N)
    fy, cy, ry, sy = axis_rows(H, S, N)
    p = img.astype(np.float32)
    h = np.zeros((H, N, 3), np.float32)
    for j in range(N):
        w = rx[j].astype(np.float32)
        for t in range(int(cx[j])):
            h[:, j] = _fma32(p[:, fx[j] + t], w[t], h[:, j])
    v = np.zeros((N, N, 3), np.float32)
    for i in range(N):
        w = ry[i].astype(np.float32)
        for t in range(int(cy[i])):
            v[i] = _fma32(h[fy[i] + t], w[t], v[i])
    pad32 = np.float32(pad_value)
    if pad32 != 0:
        pad255 = np.float32(255.0 * float(pad32))
        q = (sy.astype(np.float32)[:, None] * sx.astype(np.float32)[None, :]).astype(np.float32)
        r = (np.float32(1.0) - q).astype(np.float32)
        v = _fma32(pad255, r[..., None], v)
    c = norm_constants()
    out = _fma32(v, c[None, None, :3], c[None, None, 3:]).transpose(2, 0, 1)
    if bf16:
        out = round_bf16(out)
    return np.ascontiguousarray(out)


def round_bf16(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)
