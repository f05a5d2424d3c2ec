"""Colour jitter, host side (no GPU): the `ColorJitter` sampler's determinism, ranges and fixed draw sequence; colour on or off leaves the geometric
sampler's output alone; `check_color`; the two new C entries are exported, the workspace query answers and the launcher refuses bad arguments
before any launch."""
import ctypes

import numpy as np
import pytest

from tests import augment_reference as R
from owl_vit_object_detection_amd import _lib
from owl_vit_object_detection_amd import preprocess as P

KEY = (7, 0, 2, 5)                                               # (seed, rank, epoch, index)


# ---- sampler -----------------------------------------------------------------------------------------------------------------------------------
def test_sampler_is_keyed_by_seed_rank_epoch_index():
    cj = P.ColorJitter(0.4, 0.4, 0.4, gray=0.2)
    ref = cj.sample(64, KEY)
    assert ref.dtype == np.float32 and ref.shape == (64, 4)
    cj.sample(64, (7, 0, 0, 0))                                  # earlier calls leave no trace
    assert np.array_equal(cj.sample(64, KEY), ref)
    assert np.array_equal(P.ColorJitter(0.4, 0.4, 0.4, gray=0.2).sample(64, KEY), ref)
    for other in ((8, 0, 2, 5), (7, 1, 2, 5), (7, 0, 3, 5), (7, 0, 2, 6)):
        assert not np.array_equal(cj.sample(64, other), ref), other


def test_sampler_is_a_stream_of_its_own():
    """numpy.random.default_rng((seed, rank, epoch, index, 1)): the geometric sampler's key with one more word."""
    cj = P.ColorJitter(0.4, 0.0, 0.0)
    u = np.random.default_rng(KEY + (1,)).random(9)
    assert np.array_equal(cj.sample(9, KEY)[:, 0], (0.6 + u * (1.4 - 0.6)).astype(np.float32))
    assert not np.array_equal(np.random.default_rng(KEY).random(9), u)


def test_ranges_are_respected_and_values_are_float32():
    n = 4000
    c = P.ColorJitter(0.4, 1.5, (0.25, 0.75)).sample(n, KEY)
    assert c.dtype == np.float32
    assert (c[:, 0] >= np.float32(0.6)).all() and (c[:, 0] <= np.float32(1.4)).all() and c[:, 0].min() < 0.62 and c[:, 0].max() > 1.38
    assert (c[:, 1] >= 0.0).all() and (c[:, 1] <= 2.5).all() and c[:, 1].min() < 0.05 and c[:, 1].max() > 2.45         # max(0, 1 - 1.5) = 0
    assert (c[:, 2] >= 0.25).all() and (c[:, 2] <= 0.75).all()
    assert set(np.unique(c[:, 3]).tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    assert np.array_equal(P.check_color(c, n), c)
    z = P.ColorJitter().sample(50, KEY)                          # no strength: unit factors, orders still drawn
    assert (z[:, :3] == 1).all()
    with pytest.raises(ValueError):
        P.ColorJitter(brightness=-0.1)
    with pytest.raises(ValueError):
        P.ColorJitter(contrast=(0.8, 0.2))
    with pytest.raises(ValueError):
        P.ColorJitter(gray=1.5)


def test_gray_and_p():
    c = P.ColorJitter(0.4, 0.4, 0.4, gray=1.0).sample(100, KEY)
    assert (c[:, 2] == 0).all() and (c[:, 0] != 1).any()
    assert np.array_equal(P.ColorJitter(0.4, 0.4, 0.4, gray=1.0, p=0.0).sample(100, KEY), np.ones((100, 4), dtype=np.float32))
    half = P.ColorJitter(0.4, 0.4, 0.4, gray=0.3, p=0.5).sample(2000, KEY)
    ident = (half == 1).all(axis=1)
    assert 800 < int(ident.sum()) < 1200
    grey = half[~ident, 2] == 0
    assert 0.2 < grey.mean() < 0.4
    full = P.ColorJitter(0.4, 0.4, 0.4, gray=0.3, p=1.0).sample(2000, KEY)
    assert np.array_equal(half[~ident], full[~ident])           # p only masks: the other draws stay where they were


def test_changing_one_strength_never_shifts_another_draw():
    a = P.ColorJitter(0.4, 0.4, 0.4, gray=0.2, p=0.9).sample(300, KEY)
    b = P.ColorJitter(0.4, 0.9, 0.4, gray=0.2, p=0.9).sample(300, KEY)
    assert np.array_equal(a[:, [0, 2, 3]], b[:, [0, 2, 3]]) and not np.array_equal(a[:, 1], b[:, 1])
    c = P.ColorJitter(0.0, 0.4, 0.4, gray=0.2, p=0.9).sample(300, KEY)
    assert np.array_equal(a[:, 1:], c[:, 1:])
    d = P.ColorJitter(0.4, 0.4, 0.4, gray=0.7, p=0.9).sample(300, KEY)
    assert np.array_equal(a[:, [0, 1, 3]], d[:, [0, 1, 3]])


def _batch(n=6):
    shapes = [R.SHAPES[i % 3] for i in range(n)]
    boxes = [np.array([[w / 4, h / 4, w / 2, h / 2]]) for h, w in shapes]
    labels = [np.array([i % 4]) for i in range(n)]
    return shapes, boxes, labels


def test_colour_never_changes_the_geometric_sample():
    shapes, boxes, labels = _batch()
    kw = dict(mosaic=(1, 2, 3), seed=7)
    off = P.TrainAugment(R.SIZE, **kw)
    on = P.TrainAugment(R.SIZE, color=P.ColorJitter(0.4, 0.4, 0.4, gray=0.2), **kw)
    assert off.color is None and off.sample_color(5, 0, 0) is None
    for epoch, index in ((0, 0), (2, 5), (3, 1)):
        a, b = off.sample(shapes, boxes, labels, epoch, index), on.sample(shapes, boxes, labels, epoch, index)
        assert len(b) == 3 and a[0] == b[0]
        assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        col = on.sample_color(len(b[0]), epoch, index)
        assert np.array_equal(col, on.color.sample(len(b[0]), (7, 0, epoch, index))) and col.shape == (len(b[0]), 4)
    assert not np.array_equal(on.sample_color(9, 0, 0), P.TrainAugment(R.SIZE, rank=1, color=on.color, **kw).sample_color(9, 0, 0))
    with pytest.raises(TypeError):
        P.TrainAugment(R.SIZE, P.ColorJitter())                  # keyword-only
    with pytest.raises(TypeError):
        P.TrainAugment(R.SIZE, color=0.4)


def test_check_color():
    good = np.array([[1, 1, 1, 0], [0, 2.5, 0.3, 5]], dtype=np.float64)
    out = P.check_color(good, 2)
    assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, good.astype(np.float32))
    for bad in ([[np.nan, 1, 1, 0]], [[1, np.inf, 1, 0]], [[1, 1, -0.5, 0]], [[1, 1, 1, 6]], [[1, 1, 1, -1]], [[1, 1, 1, 2.5]]):
        with pytest.raises(ValueError, match="color"):
            P.check_color(np.asarray(bad), 1)
    with pytest.raises(ValueError, match="shape"):
        P.check_color(good, 3)
    with pytest.raises(ValueError, match="shape"):
        P.check_color(good[:, :3], 2)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_exported_and_abi_stays_8():
    lib = _lib.load()
    assert hasattr(lib, "owl_preprocess_u8_tiles_color") and hasattr(lib, "owl_preprocess_color_workspace_bytes")
    protos = _lib.protos()
    assert [n for _, n in protos["owl_preprocess_u8_tiles_color"][1]] == ["stream", "desc", "color", "n_tiles", "max_rows", "tmp", "workspace", "workspace_bytes",
                                                                         "lut", "out", "out_bf16", "n_out", "out_h", "out_w"]
    assert [n for _, n in protos["owl_preprocess_color_workspace_bytes"][1]] == ["n_tiles", "out_h", "out_w", "bytes"]
    assert _lib.header_abi_version() == 8 and int(lib.owl_abi_version()) == 8


def test_workspace_query():
    sizes = {}
    for n, s in ((1, 24), (14, 24), (32, 768), (288, 768), (22, 330)):
        sizes[(n, s)] = P.color_workspace_bytes(n, s)
        assert sizes[(n, s)] > 0 and sizes[(n, s)] % 256 == 0
    assert sizes[(288, 768)] > sizes[(32, 768)] > sizes[(14, 24)]
    assert sizes[(288, 768)] < 288 * 768 * 768                   # partial sums, not pixels
    got = np.zeros(1, dtype=np.int64)
    for args in ((0, 24, 24), (65536, 24, 24), (4, 0, 24), (4, 24, 65536)):
        with pytest.raises(_lib.OwlLibError, match="owl_preprocess_color_workspace_bytes"):
            _lib.call("owl_preprocess_color_workspace_bytes", *args, got.ctypes.data)
    with pytest.raises(_lib.OwlLibError, match="null"):
        _lib.call("owl_preprocess_color_workspace_bytes", 4, 24, 24, None)


def test_the_launcher_refuses_bad_arguments_before_any_launch():
    """Host memory stands in for the device pointers: every call below must return its error before it launches anything."""
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    need = P.color_workspace_bytes(4, 24)

    def call(desc=p, color=p, n_tiles=4, max_rows=10, tmp=p, ws=p, ws_bytes=need, lut=p, out=p, bf16=0, n_out=2, out_h=24, out_w=24):
        _lib.call("owl_preprocess_u8_tiles_color", None, desc, color, n_tiles, max_rows, tmp, ws, ws_bytes, lut, out, bf16, n_out, out_h, out_w)

    for kw in (dict(desc=None), dict(color=None), dict(tmp=None), dict(ws=None), dict(lut=None), dict(out=None)):
        with pytest.raises(_lib.OwlLibError, match="null pointer"):
            call(**kw)
    for kw in (dict(n_tiles=0), dict(n_tiles=65536), dict(max_rows=0), dict(n_out=0), dict(n_out=5), dict(out_h=0), dict(out_w=65536)):
        with pytest.raises(_lib.OwlLibError, match="bad sizes"):
            call(**kw)
    with pytest.raises(_lib.OwlLibError, match="workspace of"):
        call(ws_bytes=need - 1)
    with pytest.raises(_lib.OwlLibError, match="workspace of"):
        call(ws_bytes=0)
    with pytest.raises(_lib.OwlLibError, match="aligned"):
        call(color=p + 4)
    with pytest.raises(_lib.OwlLibError, match="aligned"):
        call(ws=p + 2)


def test_plain_surface_is_unchanged():
    import inspect
    sig = inspect.signature(P.TrainAugment.sample)
    assert list(sig.parameters) == ["self", "shapes", "boxes", "labels", "epoch", "index"]
    assert inspect.signature(P.DeviceImageProcessor.tiles).parameters["color"].default is None
    assert inspect.signature(P.DeviceImageProcessor.run_tiles).parameters["color"].default is None
    assert inspect.signature(P.TrainAugment.__init__).parameters["color"].kind is inspect.Parameter.KEYWORD_ONLY
