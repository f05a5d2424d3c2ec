"""The colour restatement (tests/color_reference.py) pinned to live Pillow and to tests/golden/f16_color.npz, no GPU: luma on all 2^24 colours, the
uint8 blend on all 256 x 256 pairs under 51 factors, contrast's rounded mean, every shared case against `ImageEnhance`.  Then seven errors a kernel could
carry, each planted in a copy of the restatement: the pins catch every one, and every one changes the output of at least one case the GPU test runs --
a kernel carrying it cannot pass tests/test_color_jitter_gpu.py."""
import os

import numpy as np
import pytest

from tests import color_reference as C

SRC = C.sources()
CASES = C.cases()

BLEND_FACTORS = [0.0, 0.1, 0.25, float(np.float32(1.0 / 3.0)), 0.6, 0.9999999, 1.0, 1.4, 1.875, 2.5, 3.0] \
    + np.random.default_rng(40).uniform(0.0, 2.0, 40).tolist()


# ---- the pins: each returns the number of mismatches of an implementation against live Pillow ----------------------------------------------------
def pin_luma(impl):
    from PIL import Image
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    rgb = np.stack([i >> 16, (i >> 8) & 255, i & 255], axis=2).astype(np.uint8)
    want = np.asarray(Image.fromarray(rgb).convert("L"))
    return int((impl.luma(rgb) != want).sum())


def pin_blend(impl, factors=BLEND_FACTORS):
    from PIL import Image
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    ia, ib = Image.fromarray(a), Image.fromarray(b)
    bad = 0
    for f in factors:
        want = np.asarray(Image.blend(ia, ib, f))
        bad += int((impl.blend_u8(a, b, np.float32(f)) != want).sum())
    return bad


def _two_levels(k, shape=(6, 10)):
    img = np.full(shape + (3,), k, dtype=np.uint8)
    img.reshape(-1, 3)[::2] = k + 1                              # every other pixel: equal numbers, mean luma k + 0.5 exactly
    return img


def pin_mean(impl):
    from PIL import Image, ImageEnhance
    bad = 0
    for k in (0, 1, 100, 127, 128, 254):
        img = _two_levels(k)
        for f in (0.0, 0.25, 1.5):
            want = np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f))
            bad += int((impl.enhance(img, "c", np.float32(f)) != want).sum())
    return bad


def pin_cases(impl):
    bad = 0
    for name, (tiles, color, n_out, size) in CASES.items():
        bad += int((impl.render_color(SRC, tiles, color, n_out, size) != C.render_color_pil(SRC, tiles, color, n_out, size)).sum())
    return bad


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def test_luma_equals_pillow_on_all_colours():
    pytest.importorskip("PIL")
    assert pin_luma(C.REF) == 0


def test_blend_equals_pillow_on_all_pairs():
    pytest.importorskip("PIL")
    assert len(BLEND_FACTORS) == 51 and sum(1 for f in BLEND_FACTORS if f > 1.0) > 10 and sum(1 for f in BLEND_FACTORS if f < 1.0) > 10
    assert pin_blend(C.REF) == 0
    assert pin_blend(C.REF, [float(f) for f in np.float32(BLEND_FACTORS)]) == 0         # the factor as a double or as its float32 rounding: the same image


def test_contrast_mean_rounds_half_up_like_pillow():
    pytest.importorskip("PIL")
    assert pin_mean(C.REF) == 0
    assert C.REF.mean_level(C.luma(_two_levels(100))) == 101
    assert (C.enhance(_two_levels(100), "c", 0.0) == 101).all()


def test_enhance_equals_pillow():
    """The three ops x five factors on a 17 x 23 random image: both of Blend.c's branches."""
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    img = np.random.default_rng(2).integers(0, 256, size=(17, 23, 3), dtype=np.uint8)
    for kind, op in (("b", ImageEnhance.Brightness), ("c", ImageEnhance.Contrast), ("s", ImageEnhance.Color)):
        for f in (0.0, 0.3, 1.0, 1.6, 2.5):
            assert np.array_equal(C.enhance(img, kind, np.float32(f)), np.asarray(op(Image.fromarray(img)).enhance(f))), (kind, f)
    assert np.array_equal(C.enhance(img, "s", 0.0), np.repeat(C.luma(img)[..., None], 3, axis=2))         # grayscale = saturation 0


def test_cases_equal_live_pillow():
    pytest.importorskip("PIL")
    assert pin_cases(C.REF) == 0


def test_restatement_matches_the_pillow_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "f16_color.npz"))
    for k, im in enumerate(SRC):
        assert np.array_equal(im, z[f"src_{k}"])
    assert int(z["size"]) == C.SIZE
    seen = 0
    for name, (tiles, color, n_out, size) in CASES.items():
        if size != C.SIZE:
            continue
        ta = z[f"tiles_{name}"]
        assert ta.shape[0] == len(tiles)
        for row, t in zip(ta, tiles):                          # the fixture was written for these very tiles and colour rows
            assert tuple(row) == (t.src, *t.box, float(t.flip), t.b, t.x0, t.y0, t.cw, t.ch)
        assert np.array_equal(z[f"color_{name}"], color) and z[f"color_{name}"].dtype == np.float32
        assert np.array_equal(C.render_color(SRC, tiles, color, n_out, size), z[f"canvas_{name}"]), name
        seen += 1
    assert seen == 4


def test_cases_reach_what_they_claim():
    from tests import augment_reference as A
    col = {name: c[1] for name, c in CASES.items()}
    assert {int(o) for o in col["orders"][:, 3]} == set(range(6)) and (col["orders"][:, :3] != 1).all()
    assert (col["orders"][:, 1] < 1).any() and (col["orders"][:, 1] > 1).any()
    for k in range(3):                                           # each op alone
        alone = (col["single"][:, k] != 1) & (np.delete(col["single"][:, :3], k, axis=1) == 1).all(axis=1)
        assert alone.any(), k
    assert (col["single"][:, 2] == 0).any() and (col["single"] == (1, 1, 1, 0)).all(axis=1).any()
    tiles, color, n_out, size = CASES["single"]
    bright = C.resized_cell(SRC, tiles[4]).astype(np.float32) * np.float32(2.5)
    assert (bright >= 255).any() and (bright < 255).any()                                # the upper clip, and pixels below it
    m = C.REF.mean_level(C.luma(C.resized_cell(SRC, tiles[5])))
    v = C.REF.blend_value(m, C.resized_cell(SRC, tiles[5]), np.float32(3.0))
    assert (v <= 0).any() and (v >= 255).any()                                           # contrast 3: both clips
    for name in ("mixed", "big"):                                # contrast on and off in one launch, also inside one canvas
        tiles, color, _, _ = CASES[name]
        per_b = {}
        for t, row in zip(tiles, color):
            per_b.setdefault(t.b, set()).add(bool(row[1] != 1))
        assert any(v == {True, False} for v in per_b.values()), name
    tiles, color, _, size = CASES["twogrey"]
    assert all(int(C.luma(C.resized_cell(SRC, t)).astype(np.int64).sum()) * 2 == (2 * C.GREY + 1) * size * size for t in tiles)   # mean = GREY + 0.5
    tiles, _, _, size = CASES["big"]
    assert size == 330 and {t.cw for t in tiles} == {330, 165, 110} and size > 256 and size % 4 != 0
    assert A.SIZE == C.SIZE


# ---- planted errors ----------------------------------------------------------------------------------------------------------------------------
class Fused(C.Restatement):
    """One rounding: the product is not rounded to float32 before the sum (what a contracted multiply-add computes)."""
    def blend_value(self, a, b, f):
        a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
        return (a + np.float64(np.float32(f)) * (b - a)).astype(np.float32)             # the float64 sum is exact: 24 x 9 bits + 8 bits


class Nearest(C.Restatement):
    def to_u8(self, v, f):
        return super().to_u8(np.floor(v.astype(np.float64) + 0.5), f)


class TruncatedMean(C.Restatement):
    def mean_level(self, L):
        return int(np.asarray(L).astype(np.int64).sum()) // int(L.size)


class FloatLuma(C.Restatement):
    def luma(self, rgb):
        c = np.asarray(rgb).astype(np.float64)
        return np.floor(0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2] + 0.5).astype(np.uint8)


class NoClip(C.Restatement):
    def to_u8(self, v, f):
        return (np.trunc(v).astype(np.int64) & 255).astype(np.uint8)


class CanvasMean(C.Restatement):
    """Contrast's sum taken over all the cells of the output image (a kernel that keeps one total per canvas, not per tile)."""
    def tile_means(self, cells, tiles, color):
        tot, cnt = {}, {}
        for t, cell, row in zip(tiles, cells, np.asarray(color, dtype=np.float32)):
            cur = cell
            for kind in C.ORDERS[int(row[3])]:
                if kind == "c":
                    break
                cur = self.enhance(cur, kind, row["bcs".index(kind)])
            tot[t.b] = tot.get(t.b, 0) + int(self.luma(cur).astype(np.int64).sum())
            cnt[t.b] = cnt.get(t.b, 0) + t.cw * t.ch
        return [(2 * tot[t.b] + cnt[t.b]) // (2 * cnt[t.b]) for t in tiles]


class MeanBeforeTheOps(C.Restatement):
    def contrast_input(self, original, current):
        return original


PLANTED = [(Fused, pin_blend), (Nearest, pin_blend), (TruncatedMean, pin_mean), (FloatLuma, pin_luma), (NoClip, pin_blend), (CanvasMean, pin_cases),
           (MeanBeforeTheOps, pin_cases)]


@pytest.mark.parametrize("mutant,pin", PLANTED, ids=[m.__name__ for m, _ in PLANTED])
def test_planted_error_is_caught_by_its_pin(mutant, pin):
    pytest.importorskip("PIL")
    assert pin(mutant()) > 0


@pytest.mark.parametrize("mutant", [m for m, _ in PLANTED], ids=[m.__name__ for m, _ in PLANTED])
def test_planted_error_changes_a_gpu_case(mutant):
    """tests/test_color_jitter_gpu.py compares the kernel with `render_color` on exactly these cases."""
    impl = mutant()
    changed = [name for name, (tiles, color, n_out, size) in CASES.items()
               if not np.array_equal(impl.render_color(SRC, tiles, color, n_out, size), C.render_color(SRC, tiles, color, n_out, size))]
    assert changed, mutant.__name__
