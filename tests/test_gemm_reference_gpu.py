"""The bf16 MFMA GEMM family (gemm.hip, gemm_pp2.hip, gemm_pph.hip, the epilogues of gemm_common.h, the dispatcher) against the float64 references
and derived bounds of tests/gemm_reference.py: every epilogue on every kernel at the smallest shapes at which each mechanism exists, with leading
dimensions other than the logical width, clamped a_rows / w_rows, pre-activations in the tails of the activations, and sentinels around every
output.

What is pinned: every output element (out, the saved aux, the reduced slabs) inside its elementwise bound of `exact`; every element outside
[0, M) x [0, N) bit for bit what it was; two runs of a call give the same bits; the kernels documented as bit-identical (tile 256, 7, 0, 6) give
equal out and aux (tile 128 is compared with tile 256 and the difference printed, not asserted: the code documents nothing about it); aux = None
does not change the output's bits.  tests/test_gemm_reference.py shows on the CPU that these bounds hold for a correct f32 kernel and reject each of
a dozen planted errors.  The worst err / tol per epilogue and kernel belong in profiles/gemm_reference.md; the GEMMREF lines this test prints are
their source."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops  # noqa: E402
from tests import gemm_reference as R  # noqa: E402

DEV = "cuda"
SENTINEL = 7.0           # the finite sentinel, and what the rows >= M of A / >= N of W hold (as the TN test does)


def _tuning():
    try:
        return _lib.is_tuning_build()
    except _lib.OwlLibError:
        return False


TUNING_TILES = (8, 5) if _tuning() else ()
TILES = R.TILES + TUNING_TILES
SAME_BITS = R.SAME_BITS_TILES + TUNING_TILES
LAYOUTS = ("lda", "ldw", "ldo_pad", "ldo_qkv", "ld_aux", "a_rows_sentinel", "w_rows_sentinel", "exact_rows", "slab_fallback")


class Call:
    """One GEMM problem on the device in a given layout; run(tile, ...) calls the library into freshly poisoned buffers and returns the valid regions
    after checking that nothing else changed."""

    def __init__(self, M, N, K, form, profile, layout=None, rows=None, seed=1):
        self.M, self.N, self.K, self.form, self.layout = M, N, K, form, layout
        _, self.epi, self.alpha, self.with_bias, self.inplace, self.splits = R.FORM[form]
        epi = self.epi
        inp = R.make_inputs(profile, M, N, K, seed, epi)
        inp = {k: v.to(DEV) for k, v in inp.items()}
        self.bias = inp["bias"].contiguous() if self.with_bias else None
        self.lda = K + 64 if layout in ("lda", "slab_fallback") else K
        self.ldw = K + 8 if layout == "ldw" else (K + 64 if layout == "slab_fallback" else K)
        self.a_rows, self.w_rows = M, N
        a_alloc, w_alloc = M, N                                  # no pad rows behind A / W: the clamped loads must stay inside
        if layout == "a_rows_sentinel":
            self.a_rows = a_alloc = (M + 255) // 256 * 256 + 8
        if layout == "w_rows_sentinel":
            self.w_rows = w_alloc = (N + 255) // 256 * 256 + 8
        self.A = torch.full((a_alloc, self.lda), SENTINEL, dtype=torch.bfloat16, device=DEV)
        self.A[:M, :K] = inp["A"].bfloat16()
        self.W = torch.full((w_alloc, self.ldw), SENTINEL, dtype=torch.bfloat16, device=DEV)
        self.W[:N, :K] = inp["W"].bfloat16()
        self.resid, self.aux_in = inp["resid"], inp["aux_in"]
        self.col0, self.ldo = 0, N
        if layout == "ldo_pad":
            self.ldo = N + 8
        elif layout == "ldo_qkv":
            self.col0, self.ldo = N, 3 * N
        self.ld_aux = N + 8 if layout == "ld_aux" else N
        self.out_dtype = torch.bfloat16 if epi in R.BF16_OUT else torch.float32
        # float64 reference (on the sampled rows of the tall case) and its bounds
        self.rows = None if rows is None else torch.tensor(rows, device=DEV)
        sel = (lambda t: t) if rows is None else (lambda t: t[self.rows])
        kw = dict(bias=self.bias, alpha=self.alpha, resid=sel(self.resid), aux_in=sel(self.aux_in), splits=self.splits)
        self.ex = [R.exact(epi, sel(inp["A"]), inp["W"], accumulate=acc, **kw) for acc in ((0, 1) if epi == R.EPI_SLAB else (0,))]
        self.tol = [R.bounds(e) for e in self.ex]
        self.ns = len(self.ex[0]["ranges"]) if epi == R.EPI_SLAB else 1
        assert self.ns == (_lib.load().owl_gemm_effective_splits(K, self.splits) if epi == R.EPI_SLAB else 1)

    def _buffer(self, rows, ld, col0, dtype, poison, valid=None, M=None):
        """[rows + 3, ld] of the sentinel (3 rows past the end), `valid` placed at [0, M) x [col0, col0 + N)."""
        buf = torch.full((rows + 3, ld), poison, dtype=dtype, device=DEV)
        if valid is not None:
            buf[:M, col0:col0 + self.N] = valid.to(dtype)
        return buf

    def run(self, tile, poison, with_aux=True, fails=None):
        """-> dict of the valid regions: out, aux (forward activations), reduced0 / reduced1 (slab: accumulate 0 / 1)."""
        M, N, epi, tag = self.M, self.N, self.epi, f"{self.form} tile={tile}"
        nanv = float("nan")
        pz = nanv if poison == "nan" else SENTINEL
        prefill = None
        if epi == R.EPI_ACC or (epi == R.EPI_RESID and self.inplace):
            pz, prefill = SENTINEL, self.resid               # the buffer is read: finite outside the written region
        out = self._buffer(self.ns * M, self.ldo, self.col0, self.out_dtype, pz, prefill, M)
        before = out.clone()
        out_arg = out[:, self.col0:]
        aux = aux_before = None
        if epi in (R.EPI_DQGELU, R.EPI_DGELU):
            aux = self._buffer(M, self.ld_aux, 0, torch.bfloat16, SENTINEL, self.aux_in, M)
        elif epi in (R.EPI_QGELU, R.EPI_GELU) and with_aux:
            aux = self._buffer(M, self.ld_aux, 0, torch.bfloat16, nanv if poison == "nan" else SENTINEL)
        if aux is not None:
            aux_before = aux.clone()
        resid = None
        if epi == R.EPI_RESID:
            resid = out_arg if self.inplace else self._buffer(M, self.ldo, self.col0, torch.float32, SENTINEL, self.resid, M)[:, self.col0:]
        ops.gemm(epi, self.A, self.W, out_arg, bias=self.bias, resid=resid, aux=aux, M=M, N=N, K=self.K, lda=self.lda, ldw=self.ldw, ldo=self.ldo,
                 ld_aux=self.ld_aux, a_rows=self.a_rows, w_rows=self.w_rows, alpha=self.alpha, splits=self.splits, tile=tile)
        res = {}
        if epi == R.EPI_SLAB:
            # slab s = rows [s M, (s + 1) M) of the buffer (slab_stride = M ldo): the valid region is ns M rows
            R.untouched(f"{tag} slabs", out, before, self.ns * M, self.col0, N, fails)
            cols = slice(self.col0, self.col0 + N)
            res["out"] = out[:self.ns * M, cols].reshape(self.ns, M, N).clone()
            n = M * self.ldo
            for accumulate in (0, 1):
                tgt = self._buffer(M, self.ldo, self.col0, torch.float32, SENTINEL, self.resid if accumulate else None, M)
                src = out.clone()
                src[:, :self.col0] = 0.0; src[:, self.col0 + N:] = 0.0      # (the reduce walks whole rows: pad columns 0, not NaN)
                tb = tgt.clone()
                _lib.call("owl_slab_reduce", ops.stream(), src, tgt, n, n, self.ns, accumulate)
                if bool((R.bits(tgt[M:]) != R.bits(tb[M:])).any()) and fails is not None:
                    fails.append(f"{tag}: slab reduce wrote past n")
                res[f"reduced{accumulate}"] = tgt[:M, cols].clone()
            return res
        R.untouched(f"{tag} out", out, before, M, self.col0, N, fails)
        res["out"] = out[:M, self.col0:self.col0 + N].clone()
        if aux is not None:
            if epi in (R.EPI_QGELU, R.EPI_GELU):
                R.untouched(f"{tag} aux", aux, aux_before, M, 0, N, fails)
                res["aux"] = aux[:M, :N].clone()
            elif bool((R.bits(aux) != R.bits(aux_before)).any()) and fails is not None:
                fails.append(f"{tag}: the given aux changed")
        return res

    def judge(self, tile, res, fails, tally):
        sel = (lambda t: t) if self.rows is None else (lambda t: t[..., self.rows, :])
        tag = f"{self.form} tile={tile}"
        ex, tol = self.ex[0], self.tol[0]
        worst = {"out": R.check(f"{tag} out", sel(res["out"]), ex["out"], tol["out"], fails)}
        if "aux" in res:
            worst["aux"] = R.check(f"{tag} aux", sel(res["aux"]), ex["aux"], tol["aux"], fails)
        for accumulate in (0, 1):
            if f"reduced{accumulate}" in res:
                worst[f"reduced{accumulate}"] = R.check(f"{tag} reduced (accumulate {accumulate})", sel(res[f"reduced{accumulate}"]),
                                                        self.ex[accumulate]["reduced"], self.tol[accumulate]["reduced"], fails)
        tally.append((tile, worst))


def _equal(a, b):
    return a.keys() == b.keys() and all(bool((R.bits(a[k]) == R.bits(b[k])).all()) for k in a)


def _run_all_tiles(call, tiles, poison, where):
    """Every tile twice (same bits), inside the bounds, untouched surroundings; then the same bits across the kernels documented as bit-identical."""
    fails, tally, results = [], [], {}
    for tile in tiles:
        res = call.run(tile, poison, fails=fails)
        again = call.run(tile, poison, fails=fails)
        if not _equal(res, again):
            fails.append(f"{call.form} tile={tile}: two runs give different bits")
        call.judge(tile, res, fails, tally)
        if call.epi in (R.EPI_QGELU, R.EPI_GELU):
            plain = call.run(tile, poison, with_aux=False, fails=fails)
            if not bool((R.bits(plain["out"]) == R.bits(res["out"])).all()):
                fails.append(f"{call.form} tile={tile}: aux = None changes the output's bits")
        results[tile] = res
    base = results.get(256)
    for tile in tiles:
        if base is not None and tile in SAME_BITS and not _equal(results[tile], base):
            k = next(k for k in base if not bool((R.bits(results[tile][k]) == R.bits(base[k])).all()))
            d = (results[tile][k].double() - base[k].double()).abs()
            fails.append(f"{call.form} tile={tile}: {k} differs from tile 256 at {int((d > 0).sum())} elements, max |diff| {float(d.max()):.3g}")
    if base is not None and 128 in results:
        d = max(float((results[128][k].double() - base[k].double()).abs().max()) for k in base)
        print(f"GEMMREF {where} form={call.form} tile128_vs_256 equal={_equal(results[128], base)} maxdiff={d:.3g}")
    for tile, worst in tally:
        lib_path = R.library_path(call.epi, call.M, call.N, call.K, tile, call.a_rows, splits=call.splits)          # what the library says it launched
        if tile in R.TILES:
            assert lib_path == R.dispatch_path(call.epi, call.M, call.N, call.K, tile, call.a_rows), (call.form, tile, lib_path)
        path = "+".join(k for k, _ in lib_path)
        print(f"GEMMREF {where} epi={R.EPI_NAMES[call.epi]} form={call.form} tile={tile} path={path} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert not fails, where + "\n" + "\n".join(fails)


_LAST = {}


def _call(*key):
    """The problem and its float64 reference, built once and shared by the consecutive tests that differ in the sentinel only (never modified)."""
    if _LAST.get("key") != key:
        _LAST.clear()
        _LAST.update(key=key, call=Call(*key))
    return _LAST["call"]


@pytest.mark.parametrize("poison", ["finite", "nan"])
@pytest.mark.parametrize("M,N,K,form,profile", R.cases())
def test_gemm_inside_derived_bounds(M, N, K, form, profile, poison):
    """One (shape, form, profile) on every kernel: every element inside the derived bound of the float64 reference, the surroundings untouched
    (sentinel finite or NaN), two runs and the bit-identical kernels equal, aux = None the same output bits."""
    _run_all_tiles(_call(M, N, K, form, profile), TILES, poison, f"shape={M}x{N}x{K} profile={profile} poison={poison}")


LAYOUT_FORMS = ["bias", "qgelu", "gelu", "resid_inplace", "resid", "f32_a0.5_b", "acc", "slab2", "dqgelu", "dgelu"]
HAS_AUX = ("qgelu", "gelu", "dqgelu", "dgelu")
LAYOUT_CASES = [(M, N, K, form, layout) for (M, N, K) in R.LAYOUT_SHAPES for form in LAYOUT_FORMS for layout in LAYOUTS
                if (layout != "ld_aux" or form in HAS_AUX) and (layout != "slab_fallback" or form == "slab2")]


@pytest.mark.parametrize("M,N,K,form,layout", LAYOUT_CASES)
def test_gemm_layouts(M, N, K, form, layout):
    """Leading dimensions other than the logical width (lda = K + 64, ldw = K + 8, ldo = N + 8, ldo = 3 N with out at the middle third -- the QKV
    buffer's form --, ld_aux = N + 8), a_rows / w_rows beyond M / N with sentinel rows that must not reach a stored value, a_rows = M and w_rows = N
    exactly with nothing behind A and W, and the weight-gradient fallback's own form (lda = ldw = ld > K, a_rows = M, w_rows = N, split-K slabs):
    same checks as test_gemm_inside_derived_bounds, NaN sentinels."""
    profile = "tails" if form in ("qgelu", "gelu", "dgelu") else "randn"
    _run_all_tiles(Call(M, N, K, form, profile, layout=None if layout == "exact_rows" else layout, seed=2), TILES, "nan",
                   f"shape={M}x{N}x{K} layout={layout} profile={profile}")


TALL_FORMS = [("bias", "randn", (0, 7, 256)), ("qgelu", "tails", (0, 7, 256)), ("dqgelu", "randn", (0, 7, 256)), ("gelu", "tails", (0, 7, 256)),
              ("dgelu", "tails", (0, 7, 256)),
              # the epilogues the half-height kernel does not have: still right at this shape through the fall-through
              ("resid_inplace", "resid_large", (0, 256)), ("f32_a0.5_b", "randn", (0, 256)), ("acc", "randn", (0, 256)), ("slab2", "randn", (0, 256))]


@pytest.mark.parametrize("form,profile,tiles", TALL_FORMS, ids=[f[0] for f in TALL_FORMS])
def test_gemm_tall_whole_round_plus_half_height_remainder(form, profile, tiles):
    """300 x 1 tiles of 256: tile 0 runs one whole round (M_main = 65 536 rows) on the two-phase kernel and the 44 remainder tiles on the half-height
    kernel (gemm_plan.h, gemm_plan; asserted with the arithmetic of gemm_split); tile 7 the two-phase kernel alone (persistent: 300 items), tile 256 the
    single-phase reference.  Rows sampled by the rule of sample_rows: every 128-row band, both sides of the split row, the first and last rows;
    the bits of ALL rows are compared across the kernels."""
    M, N, K = R.TALL
    M_main = R.gemm_split(M, N, 0)
    assert M_main == 65536 and 0 < M_main < M
    rows = R.sample_rows(M, M_main)
    assert M_main - 1 in rows and M_main in rows
    _run_all_tiles(Call(M, N, K, form, profile, rows=rows, seed=3), tiles, "nan", f"shape={M}x{N}x{K} profile={profile} tall")
