"""The engine's second operator family -- comparisons, logic, Where, rounding, Clip, Pow, Reduce{Sum,Prod,Max,Min}, ArgMax / ArgMin, Expand / Tile, ConstantOfShape,
Range, Cast, Pad, Transpose, nearest and linear Resize -- as small graphs through Seam A, against oracle/op_ref.py: the bits of every f32 result for the exact
operators (indices as int64), the suite's 2e-4 rule against float64 for Pow, linear Resize, Sigmoid and Softmax.

The graphs, inputs and expected values come from oracle/op_cases.py, the table tests/test_op_semantics_cpu.py checks against the torch oracle without a GPU.
Every plan-time (`Planner::op_host`) implementation is run next to its kernel twin on the same node list, and plan-time values are sent into operators that
exist only as kernels (they used to arrive there as a null pointer)."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth.onnx_writer import GraphBuilder
from oracle import op_cases

pytestmark = pytest.mark.gpu

F32 = np.float32


def _run(case, worst=None):
    """every run of the case through one engine; returns the outputs of the last run"""
    eng = api.OrtInfer(case.model)
    try:
        for feeds, expect in case.runs:
            got = dict(eng.infer(feeds))
            assert set(expect) <= set(got), (case.name, sorted(set(expect) - set(got)))
            for name, (ref, rule) in expect.items():
                if rule == "tol" and worst is not None and ref.size:
                    worst.append(float(np.abs(got[name].astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max())))
                err = op_cases.compare(got[name], ref, rule)
                assert err is None, (case.name, name, rule, err)
        return got
    finally:
        eng.close()


def _binary(select):
    worst = []
    cases = [c for c in op_cases.binary_cases() if select(c.name)]
    assert cases
    for case in cases:
        got = _run(case, worst)
        for name, mask in case.notes["pow_one"]:                               # x ** 0 is 1, not nearly 1
            assert np.array_equal(got[name][mask].view(np.uint32), np.ones(int(mask.sum()), F32).view(np.uint32)), (case.name, name)
    print(f"Pow: largest |d| / max(1, |ref|.max()) over {len(worst)} outputs = {max(worst):.3g} (allowed {op_cases.TOL})")


def test_binary_same_shape_covers_the_vector_body_and_the_tail():
    _binary(lambda n: n.startswith("flat"))


@pytest.mark.parametrize("C", [8, 6])
def test_binary_against_a_channels_last_producer(C):
    """C = 8 takes binary_chan_kernel where the partner is per channel, C = 6 never does; [1,C,1,1], [C,1,1], [N,C,1,1], [N,1,H,W], [1,1,1,W], a scalar, a computed tensor"""
    _binary(lambda n: n.startswith(f"channels-last C={C}"))


def test_binary_broadcast_ranks_2_5_6():
    _binary(lambda n: n.startswith("rank"))


def test_binary_operand_that_is_a_view_off_its_alignment():
    _binary(lambda n: n.startswith("Slice view"))


def test_binary_grid_stride_loops():
    for case in op_cases.grid_stride_cases():
        _run(case)


def test_unary_rounding_logic_clip_and_bool_cast():
    for case in op_cases.unary_cases():
        _run(case)


def test_where_broadcasts_three_ways():
    for case in op_cases.where_cases():
        _run(case)


@pytest.mark.parametrize("C", op_cases.RED_C)
def test_reductions_over_the_last_axis(C):
    case, = [c for c in op_cases.reduce_cases() if c.name == f"reduce C={C}"]
    _run(case)


def test_reductions_over_non_trailing_axes():
    case, = [c for c in op_cases.reduce_cases() if "non-trailing" in c.name]
    _run(case)


@pytest.mark.parametrize("C", op_cases.RED_C)
def test_arg_reductions(C):
    case, = [c for c in op_cases.argreduce_cases() if c.name == f"arg-reduce C={C}"]
    got = _run(case)
    assert all(v.dtype == np.int64 for v in got.values())


def test_expand_tile_constant_of_shape_range():
    for case in op_cases.copy_cases():
        _run(case)


@pytest.mark.parametrize("ctm", op_cases.op_ref.CTMS)
def test_nearest_resize_is_the_rational_index_map(ctm):
    """4 nearest modes x C in (8, 3) x 13 size pairs per coordinate mode; the input straight from the graph, deferred into Concat / Add / a convolution / a unary, and materialised"""
    cases = [c for c in op_cases.resize_nearest_cases() if c.name.startswith(f"nearest {ctm} /")]
    assert len(cases) == 8
    for case in cases:
        _run(case)


def test_linear_resize_at_single_element_axes_and_corner_modes():
    worst = []
    for case in op_cases.resize_linear_cases():
        _run(case, worst)
    print(f"linear Resize: largest |d| / max(1, |ref|.max()) over {len(worst)} outputs = {max(worst):.3g} (allowed {op_cases.TOL})")


def test_pad_crops_mixes_axes_and_reflects_a_single_element():
    for case in op_cases.pad_cases():
        _run(case)


def test_transpose_ranks_5_and_6():
    for case in op_cases.transpose_cases():
        _run(case)


def test_host_path_and_device_path_give_the_same_values():
    """the same node list on Shape-derived values (Planner::op_host, leaving as host outputs) and on graph inputs (the kernels): both equal op_ref"""
    names = [c.name for c in op_cases.twin_cases()]
    assert any(n.startswith("host path, int") for n in names) and any(n.startswith("host path, float") for n in names) and any(n.startswith("device path") for n in names)
    for case in op_cases.twin_cases():
        _run(case)


def test_plan_time_values_reach_device_only_operators_as_values():
    worst = []
    for case in op_cases.crossing_cases():
        _run(case, worst)
    print(f"Sigmoid / Softmax of a plan-time vector: largest relative |d| = {max(worst):.3g}")


def test_refusals_are_plan_time_errors_that_name_the_reason():
    for ec in op_cases.error_cases():
        with pytest.raises(api.OCRError) as e:
            api.OrtInfer(ec.model).infer(ec.feeds)
        assert e.value.code == getattr(api, ec.code) and ec.needle in e.value.message, (ec.name, e.value.code, e.value.message)


def test_a_plan_time_value_into_a_convolution_is_refused_by_name():
    g = GraphBuilder("host_conv", 17)
    g.add_input("x", [1, 2, 3, 4])
    s = g.op("Reshape", [g.op("Shape", ["x"]), g.init(np.array([1, 1, 2, 2], np.int64), "s")])
    y = g.op("Conv", [s, g.init(np.ones((1, 1, 1, 1), F32), "w")], kernel_shape=[1, 1])
    g.add_output(y, [1, 1, 2, 2])
    with pytest.raises(api.OCRError) as e:
        api.OrtInfer(g.model()).infer(np.zeros((1, 2, 3, 4), F32))
    assert e.value.code == api.OAR_UNSUPPORTED_OP and "Conv" in e.value.message and y in e.value.message


def test_bool_cast_of_a_mask_costs_no_launch_and_of_anything_else_one():
    def kernels(from_mask):
        g = GraphBuilder("castcost", 17)
        g.add_input("x", [4, 8])
        src = g.op("Less", ["x", g.init(np.array(0.5, F32), "c")]) if from_mask else "x"
        g.add_output(g.op("Cast", [g.op("Cast", [src], to=9)], to=1), [4, 8])
        eng = api.OrtInfer(g.model())
        try:
            return eng.cost((4, 8))[2]
        finally:
            eng.close()
    assert kernels(True) == 1 and kernels(False) == 1
