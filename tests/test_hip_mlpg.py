"""GPU: wh_delta_features and wh_mlpg (csrc/wh_mlpg.hip) through world.dynamics on made tracks, means and variances.  The
features, the tracks and the pivots of the factorisation are compared with tests/_mlpg_reference.py bit for bit; there is
no tolerance anywhere."""
import numpy as np
import pytest

import _mlpg_cases as mc
import _mlpg_reference as ref

pytestmark = pytest.mark.gpu


def _rt():
    from world import _hip

    return _hip.Runtime.get()


@pytest.fixture(autouse=True)
def flags_are_clear():
    yield
    assert _rt().take_flags() == [0] * 16


# ---- a. shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.kernel_cases(), ids=lambda c: c.name)
def test_equals_the_reference_bit_for_bit(case):
    """T at 1, 2, 3, 2L, 2L+1, 4L+1, 63, 64, 65 and 300 in one ragged batch; d = 1, 2, 39, 63, 64, 65, 130 (waves start and
    end inside an utterance); 1 .. 4 windows of half-width 0, 1 and 2, the HTS windows and an asymmetric one; rows inside
    wider tensors; one row of variances and a row per frame, over sixteen decades; 130 utterances of d = 1 in shared
    waves.  Features, tracks and pivots."""
    assert mc.compare(mc.run(_rt(), case), case) == []


def test_the_case_list_covers_what_it_says():
    cases = mc.kernel_cases()
    assert {c.d for c in cases} >= {1, 2, 39, 63, 64, 65, 130}
    assert {(c.half, c.n_win) for c in cases} >= {(h, n) for h in (0, 1, 2) for n in (1, 2, 3, 4)}
    for half in (0, 1, 2):
        assert {c.per_frame for c in cases if c.half == half} == {True, False}
        assert set(mc.edge_lengths(half)) >= {1, 2, 3, 2 * half + 1, 4 * half + 1, 63, 64, 65, 300}
    assert any(c.pad for c in cases) and any(c.d == 1 and len(c.lens) == 130 for c in cases)


# ---- b. the division on its own --------------------------------------------------------------------------------------
def test_one_frame_systems_equal_numpy_division():
    """4096 systems of one frame, static window only: c = r * (1 / R) with R = (1 * p) * 1, r = (1 * p) * mu,
    p = 1 / var — the device division alone, over twelve decades."""
    from world.dynamics import mlpg_device

    rt = _rt()
    rng = np.random.RandomState(5)
    var = 10.0 ** rng.uniform(-6, 6, size=(4096, 1))
    mu = rng.randn(4096, 1) * np.exp(rng.randn(4096, 1) * 3)
    off = np.arange(4097, dtype=np.int64)
    batch = rt.make_batch(np.zeros(4097, dtype=np.int64), off)
    p = 1.0 / var
    R = (1.0 * p) * 1.0
    want = ((1.0 * p) * mu) * (1.0 / R)
    for windows in (((1.0,),), ((0.0, 1.0, 0.0),), ((0.0, 0.0, 1.0, 0.0, 0.0),)):
        got, piv = mlpg_device(rt, batch, rt.to_device(mu), rt.to_device(var), windows, want_pivots=True)
        got, piv = got.cpu().numpy(), piv.cpu().numpy()
        assert got.tobytes() == want.tobytes(), "%d of 4096 differ" % np.sum(got != want)
        assert piv.tobytes() == R.tobytes()


# ---- c. batch invariance ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=(mc.RAGGED, mc.RAGGED_L2), ids=lambda c: c.name)
def ragged(request):
    return request.param, mc.run(_rt(), request.param)


def test_ragged_batch_with_empty_utterances_equals_the_reference(ragged):
    case, got = ragged
    assert mc.compare(got, case) == []
    assert got[1].shape == (sum(case.lens), case.d)


def test_an_utterance_alone_equals_the_utterance_in_the_batch(ragged):
    case, got = ragged
    rt = _rt()
    batch = mc.split(case, got)
    for u, T in enumerate(case.lens):
        if T == 0:
            continue
        alone = mc.split(case, mc.run(rt, case, only=u), only=u)[0]
        for key in mc.KEYS:
            assert mc.same_bits(alone[key], batch[u][key]), (u, key)


def test_two_runs_of_the_batch_are_equal(ragged):
    case, got = ragged
    again = mc.run(_rt(), case)
    for one, two in zip(got, again):
        assert mc.same_bits(one, two)


def test_workspace_groups_do_not_change_a_bit(ragged):
    from world.dynamics import plan_groups, workspace_bytes

    case, got = ragged
    need = [workspace_bytes(T, case.d, case.half) for T in case.lens]
    limit = (sum(need) + 2) // 3 + max(need) // 4
    assert len(plan_groups(case.lens, case.d, case.half, limit)) >= 3
    split = mc.run(_rt(), case._replace(max_ws=limit))
    assert mc.compare(split, case) == []
    for one, two in zip(got, split):
        assert mc.same_bits(one, two)


def test_an_empty_batch_is_no_error():
    from world.dynamics import delta_features_device, mlpg_device

    rt = _rt()
    batch = rt.make_batch([0, 0, 0], [0, 0, 0])
    x = rt.zeros((0, 3))
    assert tuple(delta_features_device(rt, batch, x).shape) == (0, 9)
    assert tuple(mlpg_device(rt, batch, rt.zeros((0, 9)), rt.zeros((9,)) + 1).shape) == (0, 3)


# ---- d. bad variances ------------------------------------------------------------------------------------------------
def test_bad_variances_raise_the_flag_and_touch_no_other_system():
    """A zero, a negative and a NaN variance, each in one system of a batch: the call returns, WH_FLAG_MLPG_PIVOT is
    reported, every other system has the bits it has in the clean batch, and the flags are clear afterwards."""
    from world import _hip
    from world.dynamics import mlpg_device

    rt = _rt()
    case = mc.Case("bad", (40, 70, 5), 39, 1, 3, seed=60)
    win = mc.case_windows(case)
    off, _, mean, var = mc.assemble(case)
    batch = rt.make_batch(np.zeros(len(off), dtype=np.int64), off)
    clean = mlpg_device(rt, batch, rt.to_device(mean), rt.to_device(var), win).cpu().numpy()
    assert rt.take_flags() == [0] * 16
    for value, (frame, column) in ((0.0, (3, 7)), (-1e-12, (40 + 69, 38)), (np.nan, (111, 0))):  # (-1e-12: a precision no neighbour outweighs)
        bad = np.array(var)
        for w in range(3):
            bad[frame, w * case.d + column] = value
        got = mlpg_device(rt, batch, rt.to_device(mean), rt.to_device(bad), win).cpu().numpy()
        flags = rt.take_flags()
        assert flags[_hip.FLAG_MLPG_PIVOT] == 1 and sum(flags) == 1, (value, flags)
        u = int(np.searchsorted(off, frame, side="right") - 1)
        mask = np.ones(got.shape, dtype=bool)
        mask[off[u]:off[u + 1], column] = False
        assert np.array_equal(got[mask].view(np.int64), clean[mask].view(np.int64)), value
        with pytest.raises(_hip.WorldHipError, match="MLPG"):
            mlpg_device(rt, batch, rt.to_device(mean), rt.to_device(bad), win)
            rt.check_flags("test")
        assert rt.take_flags() == [0] * 16


def test_arguments_the_library_refuses():
    """Behind the Python checks: the C entries fail with a message, before anything is launched."""
    import ctypes

    rt = _rt()
    batch = rt.make_batch([0, 0], [0, 4])
    x, y = rt.zeros((4, 9)) + 1, rt.zeros((4, 9))
    dp = ctypes.POINTER(ctypes.c_double)

    def feat(win, n_win, half, d=3, ldx=3, ldo=9):
        w = np.ascontiguousarray(win, dtype=np.float64)
        return rt.lib.wh_delta_features(rt.ctx, rt.stream(), batch.handle, rt.ptr(x), ldx, d, n_win, half,
                                        w.ctypes.data_as(dp), rt.ptr(y), ldo)

    def gen(win, n_win, half, d=3, ldm=9, ldv=9, ldo=3):
        w = np.ascontiguousarray(win, dtype=np.float64)
        return rt.lib.wh_mlpg(rt.ctx, rt.stream(), batch.handle, rt.ptr(x), ldm, rt.ptr(x), ldv, d, n_win, half,
                              w.ctypes.data_as(dp), rt.ptr(y), ldo, None)

    hts = ref.HTS_WINDOWS
    not_static = ((0.0, 0.5, 0.0),) + hts[1:]
    for call in (feat, gen):
        for args, kw, word in (((not_static, 3, 1), {}, b"static"), ((hts, 5, 1), {}, b"n_win"), ((hts, 3, 3), {}, b"half-width"),
                               ((hts, 3, 1), {"d": 0}, b"d must be"), ((hts, 3, 1), {"ldo": 2}, b"ldo")):
            assert call(*args, **kw) != 0
            assert word in rt.lib.wh_last_error(), (word, rt.lib.wh_last_error())
    assert feat(hts, 3, 1, ldx=2) != 0 and b"ldx" in rt.lib.wh_last_error()
    assert gen(hts, 3, 1, ldm=8) != 0 and b"ldm" in rt.lib.wh_last_error()
    assert gen(hts, 3, 1, ldv=5) != 0 and b"ldv" in rt.lib.wh_last_error()
    assert feat(hts, 3, 1) == 0 and gen(hts, 3, 1) == 0 and gen(hts, 3, 1, ldv=0) == 0
    rt.torch.cuda.synchronize()
