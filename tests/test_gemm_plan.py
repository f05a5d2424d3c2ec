"""What owl_gemm_nt_bf16 launches, asked of the library (owl_gemm_nt_plan: the argument checks and the planner of the launch itself, csrc/gemm_plan.h)
and held to the independent restatement tests/gemm_reference.py::dispatch_path -- kernels and row counts, over a grid that crosses every threshold
of the rules.  Host functions only: no device."""
import os
from collections import Counter

import pytest

from owl_vit_object_detection_amd import _lib
from tests import gemm_reference as R

MS = (1, 255, 256, 257, 511, 512, 513, 2644, 2900, 3072, 12032, 16385, 32768, 65536, 65537, 73984, 76700)
NS = (8, 248, 256, 264, 520, 768, 1000, 1024, 1032, 2304, 3072)
KS = (64, 128, 192)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_library_plan_equals_the_restatement_on_the_grid(built):
    """50 490 points: every M x N x K x tile x epilogue above with a_rows = M and a_rows = M + 3 (rows behind the problem change nothing).  All five
    plan shapes occur -- the single-phase 128 and 256 kernels, the two-phase kernel, the half-height kernel alone (tile 6) and whole rounds + half-height
    remainder -- so agreement cannot come from a kernel that is never reached."""
    shapes = Counter()
    for M in MS:
        for N in NS:
            for K in KS:
                for tile in R.TILES:
                    for epi in R.EPI_NAMES:
                        for a_rows in (M, M + 3):
                            want = R.dispatch_path(epi, M, N, K, tile, a_rows)
                            got = R.library_path(epi, M, N, K, tile, a_rows)
                            assert got == want, (R.EPI_NAMES[epi], M, N, K, tile, a_rows, got, want)
                            assert sum(r for _, r in got) == M
                            shapes["+".join(k for k, _ in got)] += 1
    assert sum(shapes.values()) == 50490
    assert set(shapes) == {"sp128", "sp256", "pp2", "pph", "pp2+pph"} and min(shapes.values()) > 0, shapes


def test_fewer_a_rows_than_M_keeps_the_problem_whole(built):
    """a_rows < M (the loads clamp to the last row of A): no row slicing, hence neither the half-height kernel nor the remainder split -- where
    a_rows = M takes them, the whole problem stays on the two-phase kernel."""
    for (M, N, K), tile, full in ((R.SHAPES[-1], 6, [("pph", 2900)]), (R.TALL, 0, [("pp2", 65536), ("pph", 76700 - 65536)]), ((73984, 768, 192), 6, None)):
        for epi in R.PPH_EPIS:
            if full is not None:
                assert R.library_path(epi, M, N, K, tile, M) == full
            for a_rows in (1, M // 2, M - 1):
                got = R.library_path(epi, M, N, K, tile, a_rows)
                assert got == R.dispatch_path(epi, M, N, K, tile, a_rows) == [("pp2", M)], (epi, M, N, K, tile, a_rows, got)


def test_query_refuses_what_the_launch_refuses(built):
    """The epilogues that read aux (8, 9) without one, at every point of the grid and with the launch's own message; the patch gathers (7, 12), which
    only owl_patch_embed_bf16 may run; split-K on an epilogue without slabs; a tile value of a tuning build."""
    for epi, msg in ((R.EPI_DQGELU, "EPI_DQGELU needs aux"), (R.EPI_DGELU, "EPI_DGELU needs aux")):
        for M in MS:
            for N in NS:
                for K in KS:
                    for tile in R.TILES:
                        with pytest.raises(_lib.OwlLibError, match=msg):
                            R.library_path(epi, M, N, K, tile, has_aux=0)
    for epi in (7, 12, 13, -1):
        for (M, N, K) in R.SHAPES + [R.TALL]:
            for tile in R.TILES:
                with pytest.raises(_lib.OwlLibError, match=f"unknown epilogue {epi}"):
                    R.library_path(epi, M, N, K, tile)
    with pytest.raises(_lib.OwlLibError, match="split-K needs the slab epilogue"):
        R.library_path(R.EPI_BIAS, 513, 520, 256, 0, splits=2)
    assert R.library_path(R.EPI_SLAB, 513, 520, 256, 0, splits=2) == [("sp128", 513)]          # split-K: the single-phase kernels
    assert R.library_path(R.EPI_SLAB, 76700, 256, 256, 0, splits=4) == [("sp256", 76700)]
    with pytest.raises(_lib.OwlLibError, match="multiple of 64"):
        R.library_path(R.EPI_BIAS, 513, 520, 100, 0)
    if not _lib.is_tuning_build():
        with pytest.raises(_lib.OwlLibError, match="tile must be"):
            R.library_path(R.EPI_BIAS, 513, 520, 256, 9)
