"""No GPU: what tests/test_hip_reduce.py rests on.  The packed reductions of csrc/wh_reduce.h add, at every node of
wave_sum's tree, the two operands wave_sum adds there, possibly in the other order; their totals are wave_sum's bit for bit
because a + b and b + a are the same double.  Here: the model of that tree (tests/_reduce_tree_model.py) does not notice
operands swapped at any node, and the inputs the GPU test feeds give another total under another association — so a tree
that paired other lanes would show."""
import numpy as np
import pytest

import _reduce_tree_model as M


@pytest.mark.parametrize("nt", [64, 256])
def test_totals_do_not_depend_on_the_operand_order_at_any_node(nt):
    rng = np.random.RandomState(nt)
    inputs = [M.scaled_normals(nt, k, seed=3) for k in range(8)] + [M.big_cancelling(nt, 1), M.signed_zeros(nt, 0),
                                                                    M.single_lane(nt, 2, 16)]
    for v in inputs:
        want = M.block_total(v)
        for _ in range(6):
            flips = rng.rand(nt // 64, len(M.SOURCES), 64) < 0.5
            assert M.bits(M.block_total(v, flips)) == M.bits(want)
        assert M.bits(M.block_total(v, np.ones((nt // 64, len(M.SOURCES), 64), bool))) == M.bits(want)


def test_the_tree_is_a_butterfly_over_the_lane_bits():
    """Lane 63's total pairs lanes l and l ^ 1, then pairs of pairs, ...: the same bits as a recursive halving sum."""
    def halving(v):
        while len(v) > 1:
            v = v[0::2] + v[1::2]
        return v[0]

    for k in range(5):
        v = M.scaled_normals(64, k, seed=4)
        assert M.bits(M.wave_total(v)) == M.bits(halving(v))


@pytest.mark.parametrize("nt", [64, 128, 256, 512])
def test_the_inputs_tell_the_tree_from_a_left_to_right_sum(nt):
    normals = [M.scaled_normals(nt, k) for k in range(5)]
    assert all(M.bits(M.block_total(v)) != M.bits(M.left_to_right(v)) for v in normals)
    # (1 + 1e16 - 1e16 in a row loses the 1 in either order for some rotations: one that differs is enough)
    assert any(M.bits(M.block_total(v)) != M.bits(M.left_to_right(v)) for v in [M.big_cancelling(nt, k) for k in range(5)])
    # a value in the wrong lane or summand shows: the single-lane patterns carry a value of their own per summand and wave
    seen = {int(M.bits(M.block_total(M.single_lane(nt, k, lane)))[0]) for k in range(5) for lane in M.SINGLE_LANES}
    assert len(seen) == 5
    assert len({M.single_lane(nt, k, 0)[64 * w] for k in range(5) for w in range(nt // 64)}) == 5 * (nt // 64)


def test_signed_zeros_and_nan():
    assert M.bits(M.block_total(M.signed_zeros(128, 0))) == M.bits(0.0)
    assert M.bits(M.wave_total(np.full(64, -0.0))) == M.bits(-0.0)  # (a wave of -0.0 stays -0.0: every add is a real one)
    v = M.scaled_normals(128, 0)
    v[77] = np.nan
    assert np.isnan(M.block_total(v))
