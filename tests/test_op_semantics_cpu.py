"""oracle/op_ref.py -- the independent NumPy statement of the engine's logic / select / rounding / reduce / arg-reduce / copy / Pad / Resize operators -- checked
without a GPU: known answers written out from the ONNX operator text, agreement with oracle/onnx_ref.py (torch) on the very graphs and inputs that
tests/test_gpu_op_semantics.py runs through the engine (both import oracle/op_cases.py), the condition under which the engine's f32 coordinate arithmetic
may be compared with the exact nearest-Resize index map at all, and the quality of the shared inputs."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import onnx_ref, op_cases, op_ref

F32, I64 = np.float32, np.int64
f = lambda *v: np.array(v, F32)
bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    assert np.array_equal(bits(got), bits(want)) if want.dtype == F32 else np.array_equal(got, want), (got, want)


# ---------------------------------------------------------------------------------------------- known answers
def test_round_is_half_to_even_and_keeps_the_sign_of_zero():
    same(op_ref.round_(f(0.5, 1.5, 2.5, -0.5, -1.5, 8388607.5)), f(0, 2, 2, -0.0, -2, 8388608))
    same(op_ref.round_(f(0.49999997, -0.49999997, -0.0, np.inf)), f(0, -0.0, -0.0, np.inf))
    same(op_ref.floor(f(-0.5, -0.0, 2.5)), f(-1, -0.0, 2))
    same(op_ref.ceil(f(-0.5, 0.5, -1.5)), f(-0.0, 1, -1))


def test_comparisons_logic_and_select():
    a, b = f(-0.0, 1, np.inf, -np.inf, 2), f(0.0, 2, np.inf, 3, 2)
    assert op_ref.equal(a, b).tolist() == [True, False, True, False, True]
    assert op_ref.less(a, b).tolist() == [False, True, False, True, False]
    assert op_ref.greater(b, a).tolist() == [False, True, False, True, False]
    assert op_ref.and_(f(0.5, -0.0, 3), f(-2, 1, 0)).tolist() == [True, False, False]
    assert op_ref.or_(f(0.5, -0.0, 0), f(0, 0, 0)).tolist() == [True, False, False]
    assert op_ref.not_(f(0.5, -0.0, 0)).tolist() == [False, True, True]
    same(op_ref.where(np.array([[True], [False], [True]]), f(1, 2, 3).reshape(1, 3), F32(-0.0)),
         np.array([[1, 2, 3], [-0.0, -0.0, -0.0], [1, 2, 3]], F32))                                  # [3,1] x [1,3] x scalar -> [3,3]
    same(op_ref.clip(f(-np.inf, -3, -0.0, 5, np.inf), F32(-1)), f(-1, -1, -0.0, 5, np.inf))         # only a lower bound: +inf passes
    same(op_ref.clip(f(-np.inf, -3, 5), None, F32(2)), f(-np.inf, -3, 2))


def test_integer_semantics():
    same(op_ref.div(np.array([-7, 7, -7, 7, 6], I64), np.array([2, -2, -2, 2, 3], I64)), np.array([-3, -3, 3, 3, 2], I64))
    same(op_ref.cast(f(-17.5, -0.9, 0.9, 2.5), 7), np.array([-17, 0, 0, 2], I64))
    assert op_ref.cast(f(0.5, -2, 0, -0.0, 3, 1e-38), 9).tolist() == [True, True, False, False, True, True]
    same(op_ref.cast(op_ref.cast(f(0.5, -2, 0, -0.0, 3, 1e-38), 9), 1), f(1, 1, 0, 0, 1, 1))
    same(op_ref.pow_(np.array([3, 7, 2], I64), np.array([2, 0, 3], I64)), np.array([9, 1, 8], I64))
    same(op_ref.div(f(1, -7), f(3, 2)), f(np.float32(1) / np.float32(3), -3.5))


def test_arg_reductions_pick_the_first_or_the_last_of_equal_values():
    x = f(1, 3, 3, 0)
    assert op_ref.argreduce(x, 0, 0, 0).tolist() == 1 and op_ref.argreduce(x, 0, 0, 1).tolist() == 2
    assert op_ref.argreduce(x, 0, 1, 0, is_min=True).tolist() == [3]
    z = f(0.0, -0.0, 0.0).reshape(1, 3)                                                               # equal values
    assert op_ref.argreduce(z, 1, 0, 0).tolist() == [0] and op_ref.argreduce(z, 1, 0, 1, is_min=True).tolist() == [2]
    assert op_ref.argreduce(f(-np.inf, np.inf, 1, np.inf), 0, 0, 1).tolist() == 3
    same(op_ref.reduce("prod", f(2, -1, 0.5, -1, 2).reshape(1, 5), [1], 0), f(2))
    same(op_ref.reduce("sum", f(3, -9, 4).reshape(1, 3), [-1], 1), f(-2).reshape(1, 1))
    with pytest.raises(AssertionError):
        op_ref.reduce("sum", f(0.1, 0.2), [0], 0)                                                     # no single right f32 answer: refused


def test_copies_generators_and_pad():
    same(op_ref.expand(f(1, 2, 3).reshape(3, 1), [2, 1, 2]), np.broadcast_to(f(1, 2, 3).reshape(1, 3, 1), (2, 3, 2)).copy())
    same(op_ref.expand(f(1, 2, 3), [1]), f(1, 2, 3))
    same(op_ref.tile(f(1, 2).reshape(1, 2), [2, 2]), f(1, 2, 1, 2, 1, 2, 1, 2).reshape(2, 4))
    same(op_ref.range_(np.array(5, I64), np.array(-4, I64), np.array(-2, I64)), np.array([5, 3, 1, -1, -3], I64))
    same(op_ref.range_(F32(0), F32(1), F32(0.25)), f(0, 0.25, 0.5, 0.75))
    assert op_ref.range_(np.array(3, I64), np.array(3, I64), np.array(1, I64)).shape == (0,)
    x = f(0, 1, 2, 3, 4)
    same(op_ref.pad(x, [-1, -2]), f(1, 2))                                                            # a crop
    same(op_ref.pad(x, [2, -1], "reflect"), f(2, 1, 0, 1, 2, 3))
    same(op_ref.pad(x, [-3, 1], "reflect"), f(3, 4, 3))                                               # reflected on what the crop left
    same(op_ref.pad(x, [-1, 2], "edge"), f(1, 2, 3, 4, 4, 4))
    same(op_ref.pad(x, [1, -2], "constant", 7.0), f(7, 0, 1, 2))
    same(op_ref.pad(f(9).reshape(1, 1), [0, 2, 0, 1], "reflect"), f(9, 9, 9, 9).reshape(1, 4))       # a length-1 axis reflects onto its only element
    same(op_ref.pad(f(1, 2, 3, 4).reshape(2, 2), [1, 0], "constant", 0.0, axes=[-1]), f(0, 1, 2, 0, 3, 4).reshape(2, 3))
    same(op_ref.constant_of_shape([2, 2], f(1.5)), f(1.5, 1.5, 1.5, 1.5).reshape(2, 2))
    same(op_ref.transpose(np.arange(6, dtype=F32).reshape(1, 2, 3), [2, 0, 1]), f(0, 3, 1, 4, 2, 5).reshape(3, 1, 2))


def test_nearest_index_maps_from_the_resize_text():
    idx = lambda i, o, c, n: op_ref.nearest_index(i, o, Fraction(o, i), c, n).tolist()
    assert idx(2, 4, "asymmetric", "floor") == [0, 0, 1, 1]
    assert idx(2, 4, "half_pixel", "round_prefer_floor") == [0, 0, 1, 1]                             # coordinates -0.25, 0.25, 0.75, 1.25
    assert idx(4, 2, "half_pixel", "round_prefer_floor") == [0, 2] and idx(4, 2, "half_pixel", "round_prefer_ceil") == [1, 3]   # 0.5 and 2.5: the ties
    assert idx(4, 2, "half_pixel", "ceil") == [1, 3] and idx(4, 2, "half_pixel", "floor") == [0, 2]
    assert idx(3, 5, "align_corners", "round_prefer_floor") == [0, 0, 1, 1, 2] and idx(3, 5, "align_corners", "round_prefer_ceil") == [0, 1, 1, 2, 2]
    assert idx(4, 1, "align_corners", "ceil") == [0] and idx(4, 1, "pytorch_half_pixel", "ceil") == [0] and idx(4, 1, "half_pixel", "ceil") == [2]
    assert idx(1, 4, "asymmetric", "ceil") == [0, 0, 0, 0]                                            # clamped
    y = op_ref.resize(np.arange(4, dtype=F32).reshape(1, 1, 1, 4), sizes=[1, 1, 1, 2], mode="linear", ctm="half_pixel")
    assert np.allclose(y.reshape(-1), [0.5, 2.5]) and y.dtype == np.float64


# ---------------------------------------------------------------------------------------------- agreement with the torch oracle, on the GPU test's own graphs
def _against_onnx_ref(case):
    compared = 0
    for feeds, expect in case.runs:
        names = list(expect)
        for n, g in zip(names, onnx_ref.run(case.model, dict(feeds), want=names)):
            ref, rule = expect[n]
            err = op_cases.compare(g.astype(F32) if g.dtype == np.bool_ else g, ref, rule)
            assert err is None, (case.name, n, err)
            compared += 1
    return compared


@pytest.mark.parametrize("group", list(op_cases.GROUPS))
def test_op_ref_agrees_with_the_torch_oracle(group):
    for case in op_cases.GROUPS[group]():
        assert case.onnx_ref
        assert _against_onnx_ref(case) == sum(len(e) for _, e in case.runs), case.name


def test_grid_stride_references_are_plain_comparisons():
    for case in op_cases.grid_stride_cases():
        (feeds, expect), = case.runs
        (ref, rule), = expect.values()
        a, b = feeds[0][1], feeds[1][1]
        assert rule == "exact" and ref.size > 8192 * 256 and np.array_equal(ref, (a < b).astype(F32))


# ---------------------------------------------------------------------------------------------- the nearest-Resize condition
def _f32_index(n_in, n_out, scale, ctm, nm):
    """the engine's arithmetic, restated in np.float32: o / s, (o + .5) / s - .5, o * (in - 1) / (out - 1)"""
    o = np.arange(n_out, dtype=F32)
    s = F32(scale)
    if ctm == "asymmetric":
        x = o / s
    elif ctm == "align_corners":
        x = o * F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else np.zeros_like(o)
    elif ctm == "pytorch_half_pixel" and n_out == 1:
        x = np.zeros_like(o)
    else:
        x = (o + F32(0.5)) / s - F32(0.5)
    assert x.dtype == F32
    r = {"floor": np.floor(x), "ceil": np.ceil(x), "round_prefer_floor": np.ceil(x - F32(0.5)), "round_prefer_ceil": np.floor(x + F32(0.5))}[nm]
    return np.clip(r, 0, n_in - 1).astype(I64)


PAIRS = [(i, o, True) for i, o in op_cases.SCALE_PAIRS] + [(i, o, False) for i, o in op_cases.SIZE_PAIRS]


@pytest.mark.parametrize("n_in,n_out,by_scale", PAIRS)
def test_f32_coordinates_select_the_rational_index(n_in, n_out, by_scale):
    """ZERO disagreements allowed: only then may the engine's gather be compared bit for bit with the exact map"""
    s32 = F32(n_out / n_in) if by_scale else F32(n_out) / F32(n_in)          # the scale as the engine forms it
    exact = Fraction(float(s32)) if by_scale else Fraction(n_out, n_in)
    if by_scale:
        assert int(np.floor(F32(n_in) * s32)) == n_out
    for ctm, nm in op_cases.MODE_PAIRS:
        want = op_ref.nearest_index(n_in, n_out, exact, ctm, nm)
        got = _f32_index(n_in, n_out, s32, ctm, nm)
        assert np.array_equal(got, want), (ctm, nm, got.tolist(), want.tolist())


def test_the_excluded_pair_really_is_a_knife_edge():
    """21 -> 3 by sizes: 3 / 21 rounds up in f32, 1 / scale lands just below 7 -- `floor` then differs from the rational map, which is why it is not in the table"""
    bad = sum(int((_f32_index(21, 3, F32(3) / F32(21), c, "floor") != op_ref.nearest_index(21, 3, Fraction(3, 21), c, "floor")).sum()) for c in ("asymmetric",))
    assert bad == 2


def test_every_pair_and_mode_is_in_the_gpu_table():
    cases = op_cases.resize_nearest_cases()
    assert len(cases) == 16 * 2
    for case in cases:
        (feeds, expect), = case.runs
        assert len([n for n, _ in feeds if n.startswith("x")]) == 13 and 13 <= len(expect) <= 16


# ---------------------------------------------------------------------------------------------- input quality
def _both_outcomes(case_list, only_noted=False, min_size=10):
    seen = 0
    for case in case_list:
        for feeds, expect in case.runs:
            for name, (ref, rule) in expect.items():
                if only_noted and name not in case.notes.get("logic", []):
                    continue
                if name in case.notes.get("one_sided", []) or ref.dtype != F32 or ref.size < min_size or not np.isin(ref, (0.0, 1.0)).all() or rule != "exact":
                    continue                                                 # 0 / 1 outputs are the comparison and logic results (Pow / Sub / Div never are, at these sizes)
                share = float(ref.mean())
                assert 0.10 <= share <= 0.90, (case.name, name, share)
                seen += 1
    return seen


def test_comparison_and_logic_cases_see_both_outcomes():
    """each outcome on at least 10 % of the elements, wherever there are 10 elements to speak of (And / Or against a single-element operand are decided
    by that operand alone and are left out; the comparisons against it are not)"""
    assert _both_outcomes(op_cases.binary_cases()) == 7 * 35 - 2 * 4      # 35 cases of 10 elements or more, 7 such outputs each; 4 of them have a scalar partner
    assert _both_outcomes(op_cases.unary_cases(), only_noted=True) == 2
    assert _both_outcomes(op_cases.where_cases() + op_cases.twin_cases()) >= 0


def test_arg_reduce_ties_inputs_have_ties():
    for C in op_cases.RED_C:
        for rows in op_cases.RED_ROWS:
            x = op_cases.arg_inputs(rows, C)["ties"]
            assert (x[0] == x[0, 0]).all()                                   # an all-equal row
            if rows >= 2 and C >= 6:
                assert ((x == x.max(1, keepdims=True)).sum(1) >= 3).any() and ((x == x.min(1, keepdims=True)).sum(1) >= 3).any()
                assert (x[1] == x[1].max()).sum() >= 3 and (x[1] == x[1].min()).sum() >= 3 and x[1].max() > x[1].min()


def test_reduce_prod_rows_are_exact_normal_and_non_zero():
    tiny = float(np.finfo(F32).tiny)
    for C in op_cases.RED_C:
        for rows in op_cases.RED_ROWS:
            p = np.prod(op_cases.reduce_inputs(rows, C)[1].astype(np.float64), axis=1)
            assert np.isfinite(p).all() and (p != 0).all() and (np.abs(p) >= tiny).all() and np.array_equal(p.astype(F32).astype(np.float64), p)
