"""CPU: the table of the table-driven exp and log (csrc/wh_math.h; built on the host by wh_api.hip, read back through
wh_math_table_read, no GPU) against extended-precision NumPy, entry by entry."""
import ctypes

import numpy as np

EXP0, LOG0, NODES, FIRST = 0, 128, 93, 90


def _table():
    from world import _hip

    lib = _hip.load_library()
    n = lib.wh_math_table_read(None, 0)
    assert n == LOG0 + 4 * NODES
    t = np.zeros(n)
    assert lib.wh_math_table_read(t.ctypes.data_as(ctypes.c_void_p), n) == 0
    assert lib.wh_math_table_read(t.ctypes.data_as(ctypes.c_void_p), n - 1) != 0
    return t


def _half_ulp(v):
    return 0.5 * np.spacing(np.abs(np.asarray(v, dtype=np.float64))).astype(np.longdouble)


def test_exp_entries():
    t = _table()
    ref = np.exp2(np.arange(128, dtype=np.longdouble) / 128)
    assert np.all(np.abs(t[EXP0:EXP0 + 128].astype(np.longdouble) - ref) <= _half_ulp(t[EXP0:EXP0 + 128]) * (1 + 2.0 ** -9))
    assert t[EXP0] == 1.0


def test_log_nodes():
    t = _table()[LOG0:].reshape(NODES, 4)
    inv, hi, lo = t[:, 0], t[:, 1], t[:, 2]
    c = (FIRST + np.arange(NODES)) / 128.0
    assert np.array_equal(inv, inv.astype(np.float32).astype(np.float64))           # 24 bits
    assert np.all(np.abs(inv * c - 1) <= 2.0 ** -24)
    assert np.array_equal(hi, np.round(hi * 2.0 ** 42) / 2.0 ** 42)                 # e ln2_hi + Lhi is exact
    ref = -np.log(inv.astype(np.longdouble))
    # the pair carries the value to half an ulp of its low part, and the high part is the value rounded at 2^-42
    assert np.all(np.abs(hi.astype(np.longdouble) - ref) <= 2.0 ** -43)
    assert np.all(np.abs(hi.astype(np.longdouble) + lo.astype(np.longdouble) - ref) <= np.maximum(_half_ulp(lo), np.longdouble(2.0) ** -64 * np.abs(ref)) * 1.01)
    assert np.all(t[:, 3] == 0.0)
    one = 128 - FIRST
    assert tuple(t[one]) == (1.0, 0.0, 0.0, 0.0)
    # the nodes cover [sqrt(1/2), sqrt(2)) with one to spare at either end
    assert c[0] < np.sqrt(0.5) - 1 / 256 and c[-1] > np.sqrt(2.0) + 1 / 256
