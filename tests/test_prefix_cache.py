"""CPU side of the frozen-prefix activation cache (owl_vit_object_detection_amd/prefix_cache.py): `PrefixCache.plan()` is a pure host function -- which
batch position reads which slot, which images are computed, which of those get a slot -- and the header, the version script and ops.py agree on the two
entry points of csrc/prefix_cache.hip.  No test here touches a device: the slabs of a cache built with device="cpu" are host tensors."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from owl_vit_object_detection_amd import _lib, ops
from owl_vit_object_detection_amd.prefix_cache import DEFAULT_MAX_BYTES, Plan, PrefixCache, _id_list

E = 40 * 128          # one image of the `tiny` configs: Tp = 40 rows of D = 128
ENTRIES = ("owl_prefix_emit", "owl_prefix_gather")


def _cache(slots=None, **kw):
    return PrefixCache(E, max_bytes=DEFAULT_MAX_BYTES if slots is None else slots * 4 * E + 17, device="cpu", **kw)


def _run(cache, ids):
    """plan + commit, touching every admitted slot as the model's fill() does (so the slabs exist), without any launch."""
    plan = cache.plan(ids)
    for s in plan.miss_slots:
        if s >= 0:
            cache.slot_addr(s)
    cache.commit(plan)
    return plan


def test_cold_warm_and_mixed_batches():
    c = _cache()
    ids = [7, 3, 9, 1, 5]
    cold = c.plan(ids)
    assert cold == Plan([], [], [0, 1, 2, 3, 4], ids, [0, 1, 2, 3, 4], [], [])
    assert c.plan(ids) == cold and len(c) == 0 and c.nbytes == 0          # plan() alone changes nothing and allocates nothing
    _run(c, ids)
    assert c.contains(ids) == [True] * 5 and c.contains([2, 7]) == [False, True]
    warm = c.plan([5, 1, 9, 3, 7])                                          # another order than when filled
    assert warm == Plan([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [], [], [], [], [])
    mixed = c.plan([11, 3, 12, 5, 13])                                      # 2 hits between 3 misses
    assert mixed == Plan([1, 3], [1, 4], [0, 2, 4], [11, 12, 13], [5, 6, 7], [], [])
    _run(c, [5, 1, 9, 3, 7]); _run(c, [11, 3, 12, 5, 13])
    s = c.stats
    assert (s["hits"], s["misses"], s["admitted"], s["refused"], s["slots"]) == (7, 8, 8, 0, 8)
    assert s["bytes"] == c.nbytes > 0


def test_an_id_twice_in_a_batch_is_computed_once_and_stored_once():
    c = _cache()
    p = _run(c, [4, 8, 4, 4, 8])
    assert p == Plan([], [], [0, 1], [4, 8], [0, 1], [2, 3, 4], [0, 0, 1])
    assert len(c) == 2 and c.stats["duplicates"] == 3 and c.stats["misses"] == 2
    # ... also where the budget refuses it: the later positions copy the first one's block, nothing is stored
    c = _cache(slots=1)
    p = _run(c, [4, 8, 8])
    assert p.miss_slots == [0, -1] and p.dup_pos == [2] and p.dup_src == [1] and c.contains([4, 8]) == [True, False]


def test_budget_first_come_first_kept_no_eviction():
    c = _cache(slots=3)
    assert c.capacity == 3
    p = _run(c, [10, 11, 12, 13, 14])
    assert p.miss_slots == [0, 1, 2, -1, -1]
    s = c.stats
    assert s["admitted"] == 3 and s["refused"] == 2 and s["slots"] == 3
    assert 0 < c.nbytes == 3 * 4 * E <= c.max_bytes
    p = _run(c, [14, 13, 12, 11, 10])          # the refused two are computed again, and refused again: nothing is evicted for them
    assert p.hit_pos == [2, 3, 4] and p.hit_slots == [2, 1, 0] and p.miss_ids == [14, 13] and p.miss_slots == [-1, -1]
    assert c.stats["refused"] == 4 and c.contains([10, 11, 12, 13, 14]) == [True, True, True, False, False] and c.nbytes <= c.max_bytes
    assert _cache(slots=0).plan([1]).miss_slots == [-1]


def test_max_images_and_lazy_slabs():
    c = _cache(max_images=2)
    assert c.capacity == 2 and c.nbytes == 0          # an unused budget costs nothing
    assert _run(c, [1, 2, 3]).miss_slots == [0, 1, -1]
    assert c.nbytes == 2 * 4 * E
    # slots in several slabs: the last slab is cut to the capacity, so the bytes never pass the budget
    c = _cache(slots=5)
    c.slab_slots = 2
    _run(c, list(range(7)))
    assert [s.numel() // E for s in c._slabs] == [2, 2, 1] and c.nbytes == 5 * 4 * E <= c.max_bytes
    assert c.slot_addr(3) == c._slabs[1].data_ptr() + 4 * E and c.slot_view(4).data_ptr() == c._slabs[2].data_ptr()
    with pytest.raises(IndexError):
        c.slot_addr(5)


def test_clear_forgets_ids_and_releases_the_slabs():
    c = _cache()
    _run(c, [1, 2, 3])
    c.clear()
    assert len(c) == 0 and c.nbytes == 0 and c.contains([1, 2, 3]) == [False] * 3
    assert c.plan([3, 2]).miss_slots == [0, 1]
    assert c.stats["misses"] == 3          # the counters describe the run


def test_ids_are_python_integers_of_any_size_or_sign():
    c = _cache()
    ids = [-1, 2 ** 31, 2 ** 40 + 3, -(2 ** 33), 0]
    _run(c, ids)
    assert c.contains(ids) == [True] * 5 and c.contains([1, 2 ** 31 - 1, -2]) == [False] * 3
    t = torch.tensor(ids, dtype=torch.int64)          # a CPU tensor gives the same keys
    assert c.plan(t).hit_slots == [0, 1, 2, 3, 4]
    import numpy as np
    assert c.plan(list(np.asarray(ids, dtype=np.int64))).hit_slots == [0, 1, 2, 3, 4]
    assert _id_list(torch.tensor([3, 4], dtype=torch.int32)) == [3, 4]
    for bad in ([1.5], ["a"], [True], torch.tensor([1.0, 2.0]), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(TypeError):
            c.plan(bad)


def test_a_device_tensor_is_refused_before_anything_reads_it():
    c = _cache()

    class Dev:          # stands for a CUDA tensor: `is_cuda` is all the check may look at (reading a value would synchronise)
        is_cuda = True

        def tolist(self):
            raise AssertionError("the device tensor was read")

        def __iter__(self):
            raise AssertionError("the device tensor was read")

    for f in (c.plan, c.contains, _id_list):
        with pytest.raises(TypeError, match="device tensor"):
            f(Dev())
    t = torch.tensor([1, 2])
    fake = SimpleNamespace(is_cuda=True, tolist=t.tolist)
    with pytest.raises(TypeError, match="device tensor"):
        c.plan(fake)


def test_constructor_refuses_blocks_the_kernels_cannot_move():
    for bad in (0, -8, 12):
        with pytest.raises(ValueError):
            PrefixCache(bad, device="cpu")
    with pytest.raises(ValueError):
        PrefixCache(E, max_bytes=-1, device="cpu")


def test_header_map_and_ops_agree_on_the_two_exports():
    protos = _lib.parse_header()
    for name in ENTRIES:
        assert name in protos and protos[name][0] == "int" and protos[name][1][0] == ("void*", "stream")
    assert [n for _, n in protos["owl_prefix_emit"][1]] == ["stream", "xs", "delta1_bf16", "delta2_bf16", "n", "block_elems", "dst_addr", "slot_addr"]
    assert [n for _, n in protos["owl_prefix_gather"][1]] == ["stream", "n", "block_elems", "src_addr", "dst_addr"]
    assert [t for t, _ in protos["owl_prefix_emit"][1]][-2:] == ["const int64_t*", "const int64_t*"]          # host address tables: passed by value to the kernel
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    # the version script exports by the `owl_` prefix, the build compiles every .hip of csrc/: the new file needs no line in either, only its names right
    assert re.search(r"global:\s*owl_\*;", open(os.path.join(csrc, "libowlhip.map")).read())
    assert "ls *.hip" in open(os.path.join(csrc, "build.sh")).read()
    src = open(os.path.join(csrc, "prefix_cache.hip")).read()
    for name in ENTRIES:
        assert re.search(rf"OWL_API int {name}\(", src), name
    wrappers = open(ops.__file__).read()
    assert '"owl_prefix_emit"' in wrappers and '"owl_prefix_gather"' in wrappers and callable(ops.prefix_emit) and callable(ops.prefix_gather)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_the_library_exports_them_and_checks_arguments_before_any_launch(built):
    for name in ENTRIES:
        assert hasattr(built, name)
    h = torch.zeros(64)          # host memory nothing reads: every case below is refused before any HIP call
    a = torch.tensor([4096], dtype=torch.int64)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_prefix_emit", None, None, None, None, 1, E, a, a)
    with pytest.raises(_lib.OwlLibError, match="multiple of 8"):
        _lib.call("owl_prefix_emit", None, h, None, None, 1, 12, a, a)
    with pytest.raises(_lib.OwlLibError, match="delta2 without delta1"):
        _lib.call("owl_prefix_emit", None, h, None, h, 1, E, a, a)
    with pytest.raises(_lib.OwlLibError, match="16-byte aligned"):
        _lib.call("owl_prefix_emit", None, h, None, None, 1, E, torch.tensor([4100], dtype=torch.int64), a)
    # the destination may not overlap the compacted source (another workgroup may not have read it yet)
    inside = torch.tensor([h.data_ptr() // 16 * 16 + 16], dtype=torch.int64)
    with pytest.raises(_lib.OwlLibError, match="overlaps"):
        _lib.call("owl_prefix_emit", None, h, None, None, 1, E, inside, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(_lib.OwlLibError, match="n >= 1"):
        _lib.call("owl_prefix_gather", None, 0, E, a, a)
    with pytest.raises(_lib.OwlLibError, match="non-null"):
        _lib.call("owl_prefix_gather", None, 1, E, torch.zeros(1, dtype=torch.int64), a)
    with pytest.raises(ValueError):
        ops.prefix_gather(2, E, [4096], [4096, 8192])
