"""CPU: the host side of the query bank from image exemplars -- the slot rule, the CSR builder, every error path that needs no device, the C ABI's
argument validation and the workspace query (csrc/image_query.hip checks its arguments before any HIP call)."""
import types

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd import _lib, models, ops


@pytest.fixture(scope="module")
def built():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_slot_rule_per_class_count():
    # class c has n_c = (0, 1, 2, 3, 4, 7)[c] exemplars, given class by class
    counts = (0, 1, 2, 3, 4, 7)
    ids = [c for c, n in enumerate(counts) for _ in range(n)]
    first = np.cumsum((0,) + counts)          # global index of each class's exemplar 0
    t = models.exemplar_slots(ids, len(counts))
    assert len(t) == 18 and t[0:3] == [[], [], []]
    g = lambda c, ks: [int(first[c]) + k for k in ks]          # noqa: E731
    assert t[3:6] == [g(1, [0])] * 3                                          # one exemplar: every slot
    assert t[6:9] == [g(2, [0]), g(2, [1]), g(2, [0])]                        # two: slot 2 is empty -> exemplar 2 % 2
    assert t[9:12] == [g(3, [0]), g(3, [1]), g(3, [2])]
    assert t[12:15] == [g(4, [0, 3]), g(4, [1]), g(4, [2])]
    assert t[15:18] == [g(5, [0, 3, 6]), g(5, [1, 4]), g(5, [2, 5])]


def test_slot_rule_interleaved_order():
    # the numbering inside a class follows the order GIVEN, whatever lies between
    ids = [2, 0, 2, 1, 2, 0, 2]
    t = models.exemplar_slots(ids, 4)
    assert t[0:3] == [[1], [5], [1]]
    assert t[3:6] == [[3], [3], [3]]
    assert t[6:9] == [[0, 6], [2], [4]]
    assert t[9:12] == [[], [], []]
    assert all(m == sorted(m) for m in t)
    assert models.exemplar_slots(torch.tensor(ids), 4) == t


def test_csr_builder():
    row_ptr, members = models.slots_csr([[1], [], [0, 6], [2], []])
    assert row_ptr.dtype == np.int32 and members.dtype == np.int32
    assert row_ptr.tolist() == [0, 1, 1, 3, 4, 4] and members.tolist() == [1, 0, 6, 2]
    row_ptr, members = models.slots_csr([[], []])          # nothing assigned: still one (unread) entry, the kernel takes no null pointer
    assert row_ptr.tolist() == [0, 0, 0] and members.tolist() == [0]


def test_exemplar_validation_errors():
    with pytest.raises(ValueError, match=r"exemplar 1 has class 4, outside \[0, 4\)"):
        models.check_exemplars([0, 4], None, 2, 4)
    with pytest.raises(ValueError, match="exemplar 0 has class -1"):
        models.check_exemplars(torch.tensor([-1]), None, 1, 4)
    with pytest.raises(ValueError, match="one class id per example image"):
        models.check_exemplars([0, 1, 2], None, 2, 4)
    with pytest.raises(ValueError, match="one class id per example image"):
        models.check_exemplars([], None, 0, 4)
    with pytest.raises(ValueError, match=r"exemplar 1 \(class 3\) has query box .* x0 < x1"):
        models.check_exemplars([0, 3], [[0.1, 0.1, 0.5, 0.5], [0.5, 0.1, 0.5, 0.9]], 2, 4)
    with pytest.raises(ValueError, match=r"exemplar 0 \(class 2\)"):
        models.check_exemplars([2], torch.tensor([[0.1, 0.6, 0.5, 0.2]]), 1, 4)
    with pytest.raises(ValueError, match=r"exemplar 0 \(class 2\)"):
        models.check_exemplars([2], torch.tensor([[0.1, float("nan"), 0.5, 0.2]]), 1, 4)
    with pytest.raises(ValueError, match=r"must be \[2, 4\]"):
        models.check_exemplars([0, 1], torch.zeros(2, 5), 2, 4)
    assert models.check_exemplars(torch.tensor([1, 0]), [[0, 0, 1, 1], [0.2, 0.2, 0.3, 0.3]], 2, 4) == [1, 0]


def test_set_queries_is_refused_inside_the_ema_scope():
    """The check comes first and needs no device: the method on a stand-in that only says `inside ema_weights()`."""
    stub = types.SimpleNamespace(_ema_scope=True)
    with pytest.raises(RuntimeError, match="ema_weights"):
        models.OwlViT.set_queries_from_exemplars(stub, torch.zeros(1, 3, 96, 96), [0])


def test_set_queries_validates_before_any_forward():
    stub = types.SimpleNamespace(_ema_scope=False, cfg=types.SimpleNamespace(n_classes=4))          # no forward is reached: nothing else is needed
    with pytest.raises(ValueError, match="exemplar 0 has class 9"):
        models.OwlViT.set_queries_from_exemplars(stub, torch.zeros(1, 3, 96, 96), [9])
    with pytest.raises(ValueError, match=r"exemplar 0 \(class 1\) has query box"):
        models.OwlViT.set_queries_from_exemplars(stub, torch.zeros(1, 3, 96, 96), [1], [[0.5, 0.5, 0.4, 0.9]])


def test_workspace_query(built):
    assert ops.image_query_workspace_bytes(1, 1, 64) == 1 * 1 * 64 * 8
    assert ops.image_query_workspace_bytes(3, 64, 64) == 3 * 1 * 64 * 8
    assert ops.image_query_workspace_bytes(3, 65, 64) == 3 * 2 * 64 * 8
    assert ops.image_query_workspace_bytes(16, 3600, 768) == 16 * 57 * 768 * 8
    with pytest.raises(_lib.OwlLibError, match="P in 1 .. 8192"):
        ops.image_query_workspace_bytes(1, 8193, 64)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_image_query_workspace_bytes", 1, 36, 64, None)


def test_abi_argument_validation_without_gpu(built):
    """Argument checks run before any HIP call: safe without a device (the pointers are host memory nothing reads)."""
    h = torch.zeros(8)
    sel = lambda *a: _lib.call("owl_image_query_select", None, *a)          # noqa: E731
    with pytest.raises(_lib.OwlLibError, match="owl_image_query_select: null pointer"):
        sel(None, h, None, 1, 36, 64, h, 1 << 20, h, h, h, None, None, None)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        sel(h, h, None, 1, 36, 64, None, 1 << 20, h, h, h, None, None, None)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        sel(h, h, None, 1, 36, 64, h, 1 << 20, h, h, None, None, None, None)
    assert "null pointer" in _lib.last_error()
    for N, P, Dt in ((0, 36, 64), (1, 0, 64), (1, 8193, 64), (1, 36, 66), (1, 36, 0), (1, 36, 1028)):
        with pytest.raises(_lib.OwlLibError, match="N in 1 .. .* P in 1 .. 8192, Dt a positive multiple of 4"):
            sel(h, h, None, N, P, Dt, h, 1 << 30, h, h, h, None, None, None)
    with pytest.raises(_lib.OwlLibError, match="workspace of 8 bytes"):
        sel(h, h, None, 1, 36, 64, h, 8, h, h, h, None, None, None)
    with pytest.raises(_lib.OwlLibError, match="owl_query_bank_fill: null pointer"):
        _lib.call("owl_query_bank_fill", None, h, h, None, h, 1, 12, 64)
    for N, nq, Dt in ((0, 12, 64), (1, 0, 64), (1, 1153, 64), (1, 12, 62), (1, 12, 2048)):
        with pytest.raises(_lib.OwlLibError, match="owl_query_bank_fill: N in 1"):
            _lib.call("owl_query_bank_fill", None, h, h, h, h, N, nq, Dt)


def test_wrappers_refuse_host_tensors_and_bad_shapes(built):
    with pytest.raises(ValueError, match="must be a device tensor"):
        ops.image_query_select(torch.zeros(36, 64), torch.zeros(36, 4), None, 1, 36, 64)
    with pytest.raises(ValueError, match="must be a device tensor"):
        ops.query_bank_fill(torch.zeros(1, 64), torch.zeros(13, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(12, 64), 1, 12, 64)


def test_load_model_signature_keeps_its_defaults():
    import inspect
    sig = inspect.signature(models.load_model)
    assert sig.parameters["exemplars"].default is None and sig.parameters["exemplars"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig.parameters)[:5] == ["labelmap", "device", "arch", "seed", "state"]
    assert ops.image_query_select.__doc__ and models.EXEMPLAR_CHUNK == 32
