"""CPU: the host side of world/regrid.py — the destination grid of BatchEncoding.regrid and every ValueError the knot-list
checks raise.  Nothing here touches a device."""
import numpy as np
import pytest

from world import _tables
from world.regrid import check_source_times, destination_times, interp_contour_host, knot_lists


def test_destination_grid_identity_is_frame_times():
    for n in (1, 2, 61, 2001):
        t = _tables.frame_times(n, 5)
        assert np.array_equal(destination_times(t, 5), t)
    t = _tables.frame_times(401, 12.5)
    assert np.array_equal(destination_times(t, 12.5), t)


@pytest.mark.parametrize("period, count", ((10, 1001), (2.5, 4001), (12.5, 801)))
def test_destination_grid_counts(period, count):
    t = _tables.frame_times(2001, 5)  # 10 s
    g = destination_times(t, period)
    assert len(g) == count and np.array_equal(g, _tables.frame_times(count, period))
    assert g[-1] <= t[-1] < g[-1] + period / 1000
    odd = destination_times(_tables.frame_times(2000, 5), 10)  # last frame at 9.995 s: the grid ends at 9.99 s
    assert len(odd) == 1000 and odd[-1] == _tables.frame_times(1000, 10)[-1]


def test_destination_grid_of_a_stretched_utterance():
    t = _tables.frame_times(401, 5) * 1.7  # last frame at 3.4 s ...
    g = destination_times(t, 5)
    assert np.array_equal(g, _tables.frame_times(len(g), 5)) and g[-1] <= t[-1] < _tables.frame_times(len(g) + 1, 5)[-1]
    t = _tables.frame_times(38, 5) * 1.7  # ... and at 0.3145 s, no multiple of the period
    g = destination_times(t, 5)
    assert len(g) == 63 and g[-1] == _tables.frame_times(63, 5)[-1] and g[-1] < t[-1]
    # a first frame time that is not 0 shifts the grid
    s = destination_times(t + 0.25, 5)
    assert len(s) in (62, 63) and s[0] == t[0] + 0.25 and np.array_equal(s, (_tables.frame_times(len(s), 5) + 0.25))
    assert s[-1] <= t[-1] + 0.25


def test_one_frame_gives_one_frame():
    assert np.array_equal(destination_times(np.array([0.0]), 10), [0.0])
    assert np.array_equal(destination_times(np.array([0.37]), 2.5), [0.37])
    assert len(destination_times(np.zeros(0), 5)) == 0
    with pytest.raises(ValueError):
        destination_times(np.array([0.0, 0.005]), 0)


def test_knot_lists_layout():
    off, t, v = knot_lists([[0.0, 1.0], [0.5]], [[100.0, 200.0], [150.0]], 2)
    assert off.dtype == np.int64 and off.tolist() == [0, 2, 3] and t.tolist() == [0.0, 1.0, 0.5] and v.tolist() == [100.0, 200.0, 150.0]
    off, t, v = knot_lists(np.array([0.0, 1.0]), np.array([1.0, 2.0]), 3)  # one pair for every utterance
    assert off.tolist() == [0, 2, 4, 6] and t.tolist() == [0.0, 1.0] * 3
    off, t, v = knot_lists([([0.0], [7.0]), ([1.0, 2.0], [8.0, 9.0])], None, 2)  # (time, value) pairs
    assert off.tolist() == [0, 1, 3] and v.tolist() == [7.0, 8.0, 9.0]


@pytest.mark.parametrize("times, values, n_utt, what", (
    ([[0.0, 0.1, 0.1]], [[1.0, 2.0, 3.0]], 1, "strictly increasing"),
    ([[0.0, 0.2, 0.1]], [[1.0, 2.0, 3.0]], 1, "strictly increasing"),
    ([[0.0, np.nan]], [[1.0, 2.0]], 1, "finite"),
    ([[0.0, np.inf]], [[1.0, 2.0]], 1, "finite"),
    ([[0.0, 0.1]], [[1.0, 2.0, 3.0]], 1, "one length"),
    ([[0.0, 0.1], [0.0]], [[1.0, 2.0]], 2, "value list"),
    ([[0.0, 0.1]], [[1.0, 2.0]], 2, "for a batch of 2"),
    ([[0.0], [0.0], [0.0]], [[1.0], [1.0], [1.0]], 2, "for a batch of 2"),
    ([[], [0.0]], [[], [1.0]], 2, "no knots"),
))
def test_knot_list_checks_raise_value_error(times, values, n_utt, what):
    with pytest.raises(ValueError, match=what):
        knot_lists(times, values, n_utt)


def test_source_times_must_increase():
    check_source_times(np.array([0.0, 0.005, 0.0, 0.005]), [0, 2, 4])
    with pytest.raises(ValueError):
        check_source_times(np.array([0.0, 0.005, 0.005]), [0, 3])


def test_host_statement_of_the_voiced_rule():
    tp = _tables.frame_times(9, 5)
    f0, vuv = interp_contour_host(tp, [0.005, 0.02, 0.03], [100.0, 0.0, 200.0])
    assert vuv.tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 1] and f0[0] == 100.0 and f0[6] == 200.0 and f0[8] == 200.0
    assert np.array_equal(interp_contour_host(tp, [0.005, 0.02, 0.03], [100.0, 0.0, 200.0], voiced_rule=False),
                          np.interp(tp, [0.005, 0.02, 0.03], [100.0, 0.0, 200.0]))
