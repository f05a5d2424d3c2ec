"""The weight-gradient checker (tests/dw_reference.py) checked without a GPU: over the case set of tests/test_dw_reference_gpu.py the f32 simulation
of the kernels sits inside every derived bound and equals the float64 reference bit for bit on the exact-integer profile; the profiles are what they
claim to be; every planted error is rejected -- on `int_tagged` by inequality and on the float profiles named in PLANTED through the bounds; the
split rule is the library's."""
import pytest
import torch

from tests import dw_reference as R

NAN = float("nan")


def _tn(profile, rows, splits, n_out, n_in, ldy=None, ldx=None, hooks=None, pos=None, poison=NAN, seed=1):
    dy, x = R.make_inputs(profile, rows, n_out, n_in, seed, ldy, ldx, poison, pos)
    ex = R.exact_tn(dy, x, rows, n_out, n_in, splits)
    old_w, old_b = R.make_old(profile, ex["w0"], seed), R.make_old(profile, ex["b0"], seed + 1)
    R.set_old(ex, old_w, old_b)
    em = R.emulate_tn(dy, x, rows, n_out, n_in, splits, old_w, old_b, hooks=hooks(dy, x) if hooks else None)
    return ex, R.bounds_tn(ex), em


KEYS = ("slab", "bias", "w0", "w1", "b0", "b1")


def _judge(profile, ex, tol, em, fails, keys=KEYS):
    worst = {}
    for k in keys:
        if profile == "int_tagged":
            R.check_exact(k, em[k], ex[k], fails)
        worst[k] = R.check(k, em[k], ex[k], tol[k], fails)
    return worst


def test_constants_and_case_arithmetic():
    """What the case set claims to reach, from the launcher's arithmetic (gemm_tn.hip:404-408, :415, :425; backward.hip:779, :813)."""
    from owl_vit_object_detection_amd import ops
    assert R.ROW_PAD == ops.ROW_PAD
    want = {(5, 1): (1, 1, 1, 5), (384, 1): (6, 6, 1, 64), (357, 1): (6, 6, 1, 37), (357, 2): (6, 3, 2, 37), (385, 3): (7, 3, 3, 1), (129, 8): (3, 1, 3, 1)}
    for (rows, splits), (nk, per, ns, tail) in want.items():
        k, p, n, rg = R.split_rule(rows, splits)
        assert (k, p, n) == (nk, per, ns) and rg[-1][1] == rows and rows - 64 * (nk - 1) == tail, (rows, splits)
        assert [a for a, _ in rg] == [64 * per * s for s in range(ns)] and all(b == rg[i + 1][0] for i, (_, b) in enumerate(rg[:-1]))
    assert R.split_rule(385, 3)[3][-1] == (384, 385)           # the last split: ONE K-tile holding ONE valid row
    rows, splits, n_out, n_in = R.PERSISTENT
    assert R.split_rule(rows, splits)[:3] == (88, 2, 44) and R.n_items(rows, splits, n_out, n_in) == 264 > 256
    cases = R.tn_cases()
    assert {(c[2], c[3]) for c in cases} == set(R.WIDTHS) and {(c[0], c[1]) for c in cases if c[2:4] == (256, 256)} >= set(R.ROW_CASES)
    assert any(R.n_items(*c[:4]) % 8 for c in cases) and any(c[4] > c[2] and c[5] > c[3] for c in cases)
    assert max(R.split_rule(c[0], c[1])[1] for c in cases) >= 3          # the ping-pong stream's depth: prologue, c + 2 request, counted wait
    assert [R.cdiv(r, 256) for r in R.COLSUM_R] == [1, 1, 1, 1, 2, 5] and [R.cdiv(r, 512) for r in R.TRANSPOSE_R] == [1, 1, 1, 2]
    assert R.TRANSPOSE_ONLY_C % 8 == 4 and all(c % 4 == 0 for c in R.TRANSPOSE_C)
    # the chains of the bounds
    assert R.colsum_chain("bf16", 1029) == 64 + 2 + 1 + 16 and R.colsum_chain("f32", 3) == 1 + 2 + 1 + 16 and R.colsum_chain("transpose", 523) == 16 + 32 + 1 + 16
    assert R.gamma_x(10) == R.gamma2(10)


def test_split_rule_is_the_librarys():
    """split_rule against owl_gemm_tn_slab_workspace_bytes (host only: the library loads without a device), over every (rows, splits) near the edges."""
    from owl_vit_object_detection_amd import _lib
    b = torch.zeros(1, dtype=torch.int64)
    for rows in (1, 5, 63, 64, 65, 128, 129, 357, 384, 385, 5605, 73984):
        for splits in (1, 2, 3, 4, 5, 7, 8, 44, 45, 87, 88, 89, 256, 10000):
            _lib.call("owl_gemm_tn_slab_workspace_bytes", rows, 8, 16, splits, b)
            assert int(b.item()) == R.split_rule(rows, splits)[2] * 8 * 16 * 4, (rows, splits)


def test_profiles_are_what_they_claim():
    dy, x = R.make_inputs("int_tagged", 357, 40, 256, poison=R.POISON_INT)
    Y, X = dy[:357, :40], x[:357, :256]
    assert float(Y.abs().max()) == 2 and float(X.abs().max()) == 3 and bool((Y == Y.round()).all())
    # rows and columns are not exchangeable: no two tokens and no two features alike, in either operand
    for t in (Y, X, Y.t(), X.t()):
        assert len({tuple(r.tolist()) for r in t}) == t.shape[0]
    assert bool((dy[357:] == R.POISON_INT).all()) and bool((x[357:] == R.POISON_INT).all()) and dy.shape[0] == 384
    dy, x = R.make_inputs("int_tagged", 357, 256, 256, ldy=264, ldx=328)
    assert bool(torch.isnan(dy[:, 256:]).all()) and bool(torch.isnan(x[:, 256:]).all()) and not bool(torch.isnan(x[:357, :256]).any())
    # the largest case of the GPU test stays exact
    rows, splits, n_out, n_in = R.PERSISTENT
    assert rows * 6 + 1000 < R.EXACT_LIMIT
    # 2^24 is noticed
    big = torch.full((64, 8), 2.0 ** 12)
    assert not R.exact_tn(big, big, 64, 8, 8, 1)["exact_ok"]
    with pytest.raises(AssertionError):
        R.assert_exact_ok(R.exact_tn(big, big, 64, 8, 8, 1))
    # cancel: |slab| << slab_abs per split; a relative-to-result bound would be far wider than the derived one
    ex, tol, em = _tn("cancel", 384, 1, 40, 256)
    assert float((ex["slab"].abs() / ex["slab_abs"]).median()) < 2.0 ** -5 and float((ex["bias"].abs() / ex["bias_abs"]).max()) < 2.0 ** -5
    # one_hot_token: the positions asked for
    assert R.one_hot_positions(385, 3) == [191, 192, 256, 319, 383, 384]
    assert R.one_hot_positions(357, 2) == [191, 192, 256, 319, 356]
    assert R.one_hot_positions(5, 1) == [0, 4]
    for pos in R.one_hot_positions(357, 2):
        dy, x = R.make_inputs("one_hot_token", 357, 40, 256, pos=pos)
        assert int((dy[:357, :40] != 0).any(1).sum()) == 1 and bool((dy[pos, :40] != 0).all())


TN_CASES = R.tn_cases() + [R.PERSISTENT + R.PERSISTENT[2:]]


@pytest.mark.parametrize("rows,splits,n_out,n_in,ldy,ldx", TN_CASES)
def test_emulation_inside_bounds_and_bit_equal_on_integers(rows, splits, n_out, n_in, ldy, ldx):
    """Every case and profile of the GPU test: the f32 simulation inside the bounds at every element, equal to the reference on int_tagged (with both
    poisons); the bounds are not slack (median tol / abs within 4 gamma of the any-order chain)."""
    fails = []
    big = (rows, splits, n_out, n_in) == R.PERSISTENT
    for profile, poison in (("int_tagged", R.POISON_INT), ("int_tagged", NAN), ("randn", NAN)) + (() if big else (("cancel", NAN),)):
        ex, tol, em = _tn(profile, rows, splits, n_out, n_in, ldy, ldx, poison=poison)
        if profile == "int_tagged":
            R.assert_exact_ok(ex, f"{rows} x {n_out} x {n_in}")
        _judge(profile, ex, tol, em, fails)
        if profile == "randn":
            assert float((tol["w1"] / (ex["slab_abs"].sum(0) + ex["old_w"].abs())).median()) <= 4.0 * R.gamma(rows + 64 + ex["ns"] + 1)
            assert float((tol["b1"] / (ex["bias_abs"].sum(0) + ex["old_b"].abs())).median()) <= 4.0 * R.gamma(rows + 64 + ex["ns"] + 1)
    for pos in ([] if big else R.one_hot_positions(rows, splits)):
        ex, tol, em = _tn("one_hot_token", rows, splits, n_out, n_in, ldy, ldx, pos=pos)
        _judge("one_hot_token", ex, tol, em, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", ["bf16", "f32", "transpose"])
def test_emulated_column_sums_inside_bounds(kind):
    fails = []
    Rs, Cs = (R.TRANSPOSE_R, R.TRANSPOSE_C) if kind == "transpose" else (R.COLSUM_R, R.COLSUM_C[kind])
    shapes = [(r, c, c) for r in Rs for c in Cs] + ([R.COLSUM_LD] if kind == "bf16" else [])
    for rows, C, ld in shapes:
        for profile in ("int_tagged", "randn", "cancel"):
            src = R.make_colsum_input(profile, kind, rows, C, ld=ld, poison=R.POISON_INT if profile == "int_tagged" else NAN)
            old = R.make_old(profile, src[:rows, :C].sum(0))
            ex = R.exact_colsum(src, rows, C, old)
            em = R.emulate_colsum(kind, src, rows, C, old)
            if profile == "int_tagged":
                R.assert_exact_ok(ex)
                R.check_exact(f"{kind} {rows}x{C} {profile}", em, ex["ref"], fails)
            R.check(f"{kind} {rows}x{C} {profile}", em, ex["ref"], R.bounds_colsum(kind, rows, ex), fails)
            # a dropped row, a row counted twice and a leaked pad row are all outside
            for name, bad in (("dropped", em - src[rows - 1, :C]), ("twice", em + src[rows - 1, :C]), ("leak", em + src[rows, :C])):
                f2 = []
                if profile == "int_tagged":
                    assert R.check_exact(name, bad, ex["ref"], f2) > 0
                else:
                    R.check(name, bad, ex["ref"], R.bounds_colsum(kind, rows, ex), f2)
                    assert f2, (kind, rows, C, profile, name)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted errors: small mutators of the simulation.  Each must be unequal on int_tagged and outside the bounds on the float profiles named.
# ---------------------------------------------------------------------------------------------------------------------------------------------
P_ROWS, P_SPLITS, P_NOUT, P_NIN = 357, 2, 40, 256          # nk = 6, per = 3, nsplit = 2; the tail K-tile (tile 5) holds 37 valid rows
TAIL_KT, TAIL_VALID = 5, 37


def _drop_last_row_of_a_ktile(dy, x):
    def stage(kt, Y, X):
        if kt == 1:
            Y, X = Y.clone(), X.clone()
            Y[63] = 0.0; X[63] = 0.0
        return Y, X
    return {"stage": stage}


def _last_token_twice(dy, x):
    def stage(kt, Y, X):
        if kt == TAIL_KT:                                    # tail clamp in place of the zero row: the first pad row repeats token M - 1
            Y, X = Y.clone(), X.clone()
            Y[TAIL_VALID], X[TAIL_VALID] = Y[TAIL_VALID - 1], X[TAIL_VALID - 1]
        return Y, X
    return {"stage": stage}


def _pad_row_leaked(dy, x):
    def stage(kt, Y, X):
        if kt == TAIL_KT:                                    # row M of the buffers (poison) in place of the zero row
            Y, X = Y.clone(), X.clone()
            Y[TAIL_VALID], X[TAIL_VALID] = dy[P_ROWS, :P_NOUT], x[P_ROWS, :P_NIN]
        return Y, X
    return {"stage": stage}


def _ktile_to_the_neighbour(dy, x):
    return {"walk": lambda s, kts: kts[:-1] if s == 0 else [kts[0] - 1] + kts}


def _stale_stage_buffer(dy, x):
    return {"walk": lambda s, kts: [kts[0], kts[1], kts[0]] if s == 0 else kts}          # K-tile c read again in place of c + 2


def _chunks_swapped(dy, x):
    def stage(kt, Y, X):
        if kt == 4:
            X = X.clone()
            X[9, 8:16], X[9, 16:24] = X[9, 16:24].clone(), X[9, 8:16].clone()
        return Y, X
    return {"stage": stage}


def _clamped_chunk_on_a_real_row(dy, x):
    def slab(s, acc):                                        # n_out = 40: the duplicate of features 32 .. 39 (nn = N - 8) lands on rows 24 .. 31
        acc = acc.clone(); acc[24:32] = acc[32:40]
        return acc
    return {"slab": slab}


def _fold_first_pair_four_times(dy, x):
    return {"fold_pairs": (0, 0, 0, 0)}


def _bias_of_the_next_split(dy, x):
    return {"bias_walk": lambda s, kts: [k + 3 for k in kts] if s == 0 else kts}


# name -> (hooks, outputs that must be rejected, float profiles that reject it through the bounds [one_hot_token: at the position given])
PLANTED = {
    "token dropped at the last row of a K-tile": (_drop_last_row_of_a_ktile, ("slab", "bias", "w1", "b1"), [("randn", None), ("cancel", None), ("one_hot_token", 127)]),
    "token M - 1 counted twice": (_last_token_twice, ("slab", "bias", "w1", "b1"), [("randn", None), ("one_hot_token", 356)]),
    "one pad row >= M leaked": (_pad_row_leaked, ("slab", "bias", "w1", "b1"), [("randn", None), ("cancel", None)]),
    "one K-tile attributed to the neighbouring split": (_ktile_to_the_neighbour, ("slab", "bias"), [("randn", None), ("one_hot_token", 191)]),
    "stale stage buffer: K-tile c in place of c + 2": (_stale_stage_buffer, ("slab", "bias", "w1", "b1"), [("randn", None), ("one_hot_token", 128)]),
    "two 16-byte feature chunks swapped in a row": (_chunks_swapped, ("slab", "w1"), [("randn", None), ("one_hot_token", 265)]),
    "clamped duplicate chunk on a real output row": (_clamped_chunk_on_a_real_row, ("slab", "w1"), [("randn", None), ("cancel", None)]),
    "bias fold reads a fragment's first token pair four times": (_fold_first_pair_four_times, ("bias", "b1"), [("randn", None), ("cancel", None), ("one_hot_token", 130)]),
    "bias partial of split s sums split s + 1's tokens": (_bias_of_the_next_split, ("bias",), [("randn", None), ("one_hot_token", 192)]),
}


def _rejected(profile, ex, tol, em, key):
    fails = []
    if profile == "int_tagged":
        return R.check_exact(key, em[key], ex[key], fails) > 0
    R.check(key, em[key], ex[key], tol[key], fails)
    return bool(fails)


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_error_is_rejected(name):
    hooks, keys, float_profiles = PLANTED[name]
    missed = []
    for profile, pos in [("int_tagged", None)] + float_profiles:
        poison = R.POISON_INT if profile == "int_tagged" else NAN
        ex, tol, em = _tn(profile, P_ROWS, P_SPLITS, P_NOUT, P_NIN, hooks=hooks, pos=pos, poison=poison)
        clean = _tn(profile, P_ROWS, P_SPLITS, P_NOUT, P_NIN, pos=pos, poison=poison)[2]
        for key in keys:
            assert not _rejected(profile, ex, tol, clean, key)          # (the unplanted simulation passes the same check)
            if not _rejected(profile, ex, tol, em, key):
                missed.append((profile, pos, key))
    assert not missed, f"{name}: passed at {missed}"


def test_a_misattributed_ktile_is_invisible_in_the_sum():
    """The K-tile counted in the neighbouring split leaves the sum over splits unchanged -- on int_tagged bit for bit, on randn inside the bound: only
    the per-split check sees it, which is why the GPU test judges every slab and every bias partial on its own."""
    for profile in ("int_tagged", "randn"):
        ex, tol, em = _tn(profile, P_ROWS, P_SPLITS, P_NOUT, P_NIN, hooks=_ktile_to_the_neighbour, poison=R.POISON_INT)
        for key in ("w0", "w1", "b0", "b1"):
            assert not _rejected(profile, ex, tol, em, key)
        assert _rejected(profile, ex, tol, em, "slab") and _rejected(profile, ex, tol, em, "bias")


def test_untouched_rows_reports_a_write_past_nsplit():
    for sentinel in (7.0, NAN):
        before = torch.full((5, 40, 256), sentinel)
        ok = before.clone(); ok[:3] = 1.0
        assert R.untouched_rows("ok", ok, before, 3, fails=[]) == 0
        bad = ok.clone(); bad[3, 39, 252:] = 2.0
        fails = []
        assert R.untouched_rows("bad", bad, before, 3, fails) == 4 and fails
