"""GPU: the packed workgroup reductions of csrc/wh_reduce.h (block_sum2 / block_sum3 / block_sum5, through
wh_reduce_probe) give, bit for bit, the totals of the routine they replaced — one wave_sum per value, the waves added in
ascending order — and of a NumPy model of that tree (tests/_reduce_tree_model.py), on inputs whose total depends on the
order of the additions, in every thread of the workgroup."""
import numpy as np
import pytest

import _reduce_tree_model as M

pytestmark = pytest.mark.gpu


def _probe(nt, values):
    """values [K][nt] -> (packed [nt][K], sequential [nt][K]): every thread's copy of the K totals."""
    from world import _hip

    rt = _hip.Runtime.get()
    k = values.shape[0]
    v_d = rt.to_device(values)
    out = rt.empty((nt, 2, k))
    _hip.check(rt.lib.wh_reduce_probe(rt.ctx, rt.stream(), nt, k, rt.ptr(v_d), rt.ptr(out)))
    out = out.cpu().numpy()
    return out[:, 0, :], out[:, 1, :]


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("nt", [64, 128, 256, 512])
def test_packed_totals_have_the_bits_of_wave_sum_and_of_the_model(nt, k):
    for name, values in M.input_sets(nt, k):
        packed, sequential = _probe(nt, values)
        model = np.array([M.block_total(values[j]) for j in range(k)])
        print(name, nt, k, packed[0], sequential[0], model)
        assert np.array_equal(M.bits(packed), M.bits(sequential)), name
        assert np.array_equal(M.bits(packed), np.broadcast_to(M.bits(model), (nt, k))), name


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("nt", [64, 128, 256, 512])
def test_a_nan_stays_in_its_own_total(nt, k):
    for j in range(k):
        values = np.stack([M.scaled_normals(nt, i, seed=5) for i in range(k)])
        values[j, (37 * (j + 1)) % nt] = np.nan
        packed, sequential = _probe(nt, values)
        clean = [i for i in range(k) if i != j]
        assert np.isnan(packed[:, j]).all() and np.isnan(sequential[:, j]).all()
        assert np.array_equal(M.bits(packed[:, clean]), M.bits(sequential[:, clean]))
        model = np.array([M.block_total(values[i]) for i in clean])
        assert np.array_equal(M.bits(packed[:, clean]), np.broadcast_to(M.bits(model), (nt, len(clean))))


def test_shapes_that_are_not_built_fail_with_a_message():
    from world import _hip

    rt = _hip.Runtime.get()
    buf = rt.zeros((4096,))
    assert rt.lib.wh_reduce_probe(rt.ctx, rt.stream(), 192, 2, rt.ptr(buf), rt.ptr(buf)) != 0
    assert rt.lib.wh_reduce_probe(rt.ctx, rt.stream(), 256, 4, rt.ptr(buf), rt.ptr(buf)) != 0
    assert b"wh_reduce_probe" in rt.lib.wh_last_error()
