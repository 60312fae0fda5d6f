"""GPU: world.gmm.fit_device / posteriors_device / convert_device on synthetic parallel data, device and reference
(tests/_gmm_reference.py) in lock-step, then the chain encode -> compact -> align -> fit_compact -> convert_compact -> expand
-> decode on synthetic speech, and the NumPy-dict forms of World.

Lock-step: the parameters an iteration starts from are handed to the device one stage at a time — the E-step's ll against
the long-double ll of the same tables, its reduction against the reference's reduction of the DEVICE's ll, the statistics
against the reference's sums over the DEVICE's gamma, the host M-step against the long-double M-step of the DEVICE's
statistics — each within the bound derived in the reference from its own operands, so that no stage's error compounds
into the next one's bound; and fit_device(n_iter=1) from the same parameters returns exactly what the stages gave.  Ten
such steps are, bit for bit, fit_device(n_iter=10).

history[i + 1] >= history[i] - (tol_i + tol_(i+1)), tol_i the rounding bound of the mean: every ll of a row is within
E_n = max_m B_ll, the log-sum-exp moves by at most that, its own evaluation by B_rowll, and the mean of n such values adds
n u mean|rowll|.  The chain runs with reg_covar = 0 (the data is well conditioned): the regulariser is not part of EM's
ascent property — Sigma + reg I is off the M-step's maximiser by a second-order (reg / lambda_min)^2 per row, far above
rounding — and one further step checks the default reg_covar = 1e-6 against the reference.

Worst error / bound ratios seen on an MI355X over the ten steps (3000 rows, D = 16, M = 3; printed by every run):
    ll 0.090   gamma 0.49   rowll 0.71   s0 0.0093   s1 0.011   s2 0.018   weights 0.26   means 0.47   covariances 0.47
    (0.53 in the step with the default regulariser); posterior under the marginal of x: rowll 0.053, gamma 0.071;
    conversion: frame 0.23, mmse 0.15, the mean rows of mlpg 0.24 — and the MLPG track bit for bit.
"""
import numpy as np
import pytest

import _gmm_reference as ref
import _mlpg_reference as mref

pytestmark = pytest.mark.gpu

LD = ref.LD
WIN = mref.HTS_WINDOWS[:2]
N_UTT, T, DS, M = 12, 250, 4, 3


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


@pytest.fixture(scope="module")
def data():
    """x, y static tracks [3000][4], their static + delta rows fx, fy [3000][8] per utterance, z = [fx | fy]."""
    rng = np.random.RandomState(12)
    centres = 2.0 * rng.standard_normal((M, DS))
    maps = rng.standard_normal((M, DS, DS)) * 0.5 + np.eye(DS)
    shifts = rng.standard_normal((M, DS))
    xs, ys = [], []
    for _ in range(N_UTT):
        comp = np.repeat(rng.randint(0, M, size=T // 25), 25)
        noise = np.zeros((T, DS))
        for t in range(1, T):
            noise[t] = 0.8 * noise[t - 1] + 0.3 * rng.standard_normal(DS)
        x = centres[comp] + noise
        xs.append(x)
        ys.append(np.einsum("ti,tij->tj", x, maps[comp]) + shifts[comp] + 0.1 * rng.standard_normal((T, DS)))
    fx = np.concatenate([mref.delta_features(x, WIN) for x in xs])
    fy = np.concatenate([mref.delta_features(y, WIN) for y in ys])
    return {"x": np.concatenate(xs), "y": np.concatenate(ys), "fx": fx, "fy": fy, "z": np.concatenate([fx, fy], axis=1),
            "lens": (T,) * N_UTT}


def _staged_step(rt, z_d, z, w, mu, cov, reg):
    """One EM step on the device a stage at a time, every stage against the reference.  Returns the new parameters, the
    mean rowll and its rounding tolerance."""
    from world import gmm

    n, d = z.shape
    whiten, logc = gmm.cholesky_tables(w, mu, cov)
    mu_d = rt.to_device(mu)
    o = gmm.estep_device(rt, z_d, mu_d, rt.to_device(whiten), rt.to_device(logc), want=("ll", "gamma", "rowll", "best"))
    got = {k: v.cpu().numpy() for k, v in o.items()}
    ll, bll = ref.loglik(z, mu, whiten, logc, LD)
    ref.check("fit-ll", got["ll"], ll, bll)
    gamma, rowll, best, bg, br = ref.reduce(got["ll"], LD)
    ref.check("fit-gamma", got["gamma"], gamma, bg)
    ref.check("fit-rowll", got["rowll"], rowll, br)
    assert np.array_equal(got["best"], best)
    s = [t.cpu().numpy() for t in gmm.stats_device(rt, z_d, o["gamma"], mu_d)]
    e = ref.stats(z, got["gamma"], mu, LD)
    for k, name in enumerate(("fit-s0", "fit-s1", "fit-s2")):
        ref.check(name, s[k], e[k], e[k + 3])
    new = gmm.m_step(mu, s[0], s[1], s[2], reg)
    want = ref.m_step(mu, s[0], s[1], s[2], reg, LD)
    for k, name in enumerate(("fit-weights", "fit-means", "fit-covariances")):
        ref.check(name, new[k], want[k], want[k + 3] + ref.U * np.abs(want[k]))
    mean = float(np.sum(got["rowll"].astype(LD)) / n)
    tol = float(np.mean(np.max(bll, axis=1) + br) + n * ref.U * np.mean(np.abs(rowll)))
    return new, mean, tol


def test_default_initialisation(rt, data):
    from world import gmm

    z = data["z"]
    n, d = z.shape
    model, hist = gmm.fit_device(rt, rt.to_device(z), 8, M, 0, seed=5)
    assert hist == [] and np.all(model.weights == 1.0 / M)
    pick = np.sort(np.random.default_rng(5).choice(n, size=M, replace=False))
    assert len(set(pick.tolist())) == M and np.array_equal(model.means, z[pick])
    assert all(np.array_equal(model.covariances[0], c) for c in model.covariances)
    # the global covariance + reg I: centred statistics about a row, then delta; bound as for one component's m_step
    e = ref.stats(z, np.ones((n, 1)), z[pick[:1]], LD)
    want = ref.m_step(z[pick[:1]], e[0], e[1], e[2], 1e-6, LD)
    nk = e[0][0]
    delta = np.abs(e[1][0] / nk)
    bound = 2 * (e[5][0] / nk + np.add.outer(delta, delta) * (e[4][0].max() / nk) + np.abs(want[2][0]) * (e[3][0] / nk)) + want[5][0]
    ref.check("init-covariance", model.covariances[0], want[2][0], bound + ref.U * np.abs(want[2][0]))
    again, _ = gmm.fit_device(rt, rt.to_device(z), 8, M, 0, seed=5)
    assert again.covariances.tobytes() == model.covariances.tobytes()


@pytest.fixture(scope="module")
def chain(rt, data):
    """Ten lock-step iterations with reg_covar = 0 from the default initialisation: (init model, final parameters,
    history, tolerances)."""
    from world import gmm

    z = data["z"]
    z_d = rt.to_device(z)
    init, _ = gmm.fit_device(rt, z_d, 8, M, 0, seed=0)
    params, hist, tols = (init.weights, init.means, init.covariances), [], []
    for it in range(10):
        new, mean, tol = _staged_step(rt, z_d, z, *params, 0.0)
        one, h1 = gmm.fit_device(rt, z_d, 8, M, 1, reg_covar=0.0, init=gmm.JointGMM(*params, 8))
        for a, b in zip(new, (one.weights, one.means, one.covariances)):
            assert a.tobytes() == b.tobytes(), it
        assert abs(h1[0] - mean) <= len(z) * ref.U * abs(mean), it
        params = new
        hist.append(h1[0])
        tols.append(tol)
    return init, params, hist, tols


def test_ten_iterations_in_lock_step_are_fit_device(rt, data, chain):
    from world import gmm

    init, params, hist, _ = chain
    model, history = gmm.fit_device(rt, rt.to_device(data["z"]), 8, M, 10, reg_covar=0.0, init=init)
    assert history == hist
    for a, b in zip(params, (model.weights, model.means, model.covariances)):
        assert a.tobytes() == b.tobytes()
    assert model.dx == 8 and model.n_components == M and abs(np.sum(model.weights) - 1.0) < 1e-14
    print("worst ratios of the lock-step:", {k: v for k, v in ref.WORST.items() if k.startswith("fit-")})


def test_history_does_not_decrease(chain):
    _, _, hist, tols = chain
    assert len(hist) == 10 and hist[-1] > hist[0] + 0.1  # (EM did something)
    for i in range(9):
        assert hist[i + 1] >= hist[i] - (tols[i] + tols[i + 1]), (i, hist[i], hist[i + 1], tols[i])
    assert max(tols) < 1e-9


def test_one_step_with_the_default_regulariser(rt, data, chain):
    from world import gmm

    _, params, _, _ = chain
    z_d = rt.to_device(data["z"])
    new, _, _ = _staged_step(rt, z_d, data["z"], *params, 1e-6)
    one, _ = gmm.fit_device(rt, z_d, 8, M, 1, init=gmm.JointGMM(*params, 8))
    for a, b in zip(new, (one.weights, one.means, one.covariances)):
        assert a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def fitted(chain):
    from world import gmm
    return gmm.JointGMM(*chain[1], 8)


def test_conversion_modes_against_the_reference(rt, data, fitted):
    from world import gmm

    fx = data["fx"]
    x_d = rt.to_device(fx)
    batch = rt.make_batch(np.zeros(N_UTT + 1, dtype=np.int64), np.arange(N_UTT + 1, dtype=np.int64) * T)
    t = fitted.host_tables()
    gam_d, rowll_d, best_d = gmm.posteriors_device(rt, x_d, fitted)
    gam, best = gam_d.cpu().numpy(), best_d.cpu().numpy()
    # the posterior under the marginal of x: ll is not handed out by posteriors_device, so the whole E-step is compared
    # where the stages' bounds add: ll within B_ll moves log s by at most E = max_m B_ll and gamma by gamma (e^(2E) - 1)
    ll, bll = ref.loglik(fx, t["mu_x"], t["whiten_x"], t["logc_x"], LD)
    g, r, b, bg, br = ref.reduce(ll, LD)
    e_max = np.max(bll, axis=1)
    ref.check("posterior-rowll", rowll_d.cpu().numpy(), r, e_max + br)
    ref.check("posterior-gamma", gam, g, g * np.expm1(2 * e_max)[:, None] + bg)
    sure = np.sort(ll, axis=1)[:, -1] - (np.sort(ll, axis=1)[:, -2] if M > 1 else -np.inf) > 2 * e_max
    assert np.array_equal(best[sure], b[sure]) and np.mean(sure) > 0.99
    a_s, my_s = np.ascontiguousarray(t["a"][:, :, :DS]), np.ascontiguousarray(t["mu_y"][:, :DS])
    frame = gmm.convert_device(rt, batch, x_d, fitted, "frame", WIN).cpu().numpy()
    out, bnd = ref.convert_best(fx, t["mu_x"], a_s, my_s, best, LD)
    ref.check("convert-frame", frame, out, bnd)
    mmse = gmm.convert_device(rt, batch, x_d, fitted, "mmse", WIN).cpu().numpy()
    out, bnd = ref.convert_mmse(fx, t["mu_x"], a_s, my_s, gam, LD)
    ref.check("convert-mmse", mmse, out, bnd)
    # mlpg: the mean rows within their bound; then the reference's MLPG of the device's rows, bit for bit
    p = fitted.prepared(rt)
    mean = gmm.convert_rows_device(rt, x_d, p["mu_x"], p["a"], p["mu_y"], best=best_d).cpu().numpy()
    out, bnd = ref.convert_best(fx, t["mu_x"], t["a"], t["mu_y"], best, LD)
    ref.check("convert-mlpg-mean", mean, out, bnd)
    var = t["cvar"][best]
    assert np.all(var > 0)
    track = gmm.convert_device(rt, batch, x_d, fitted, "mlpg", WIN).cpu().numpy()
    want = np.concatenate([mref.mlpg(mean[u * T:(u + 1) * T], var[u * T:(u + 1) * T], WIN)[0] for u in range(N_UTT)])
    assert track.shape == want.shape == (N_UTT * T, DS) and track.tobytes() == want.tobytes()
    assert rt.take_flags() == [0] * 16
    # the float64 reference end to end agrees to rounding times conditioning (a sanity check of the reference's convert())
    for mode, got in (("frame", frame), ("mmse", mmse), ("mlpg", track)):
        full = ref.convert(fx, fitted.weights, fitted.means, fitted.covariances, 8, mode, WIN, data["lens"])
        assert np.max(np.abs(full - got)) <= 1e-8 * (1 + np.max(np.abs(got))), mode
    # and the point of it all: the converted static track is closer to the target than the source is
    src = np.mean((data["x"] - data["y"]) ** 2)
    for mode, got in (("frame", frame), ("mmse", mmse), ("mlpg", track)):
        assert np.mean((got - data["y"]) ** 2) < 0.5 * src, (mode, np.mean((got - data["y"]) ** 2), src)


def test_model_survives_the_npz_round_trip_on_the_device(rt, data, fitted, tmp_path):
    from world import gmm

    path = str(tmp_path / "m.npz")
    fitted.save_npz(path)
    again = gmm.JointGMM.load_npz(path)
    x_d = rt.to_device(data["fx"])
    for a, b in zip(gmm.posteriors_device(rt, x_d, fitted), gmm.posteriors_device(rt, x_d, again)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- synthetic speech end to end -------------------------------------------------------------------------------------------
FS, N0 = 16000, 13


@pytest.fixture(scope="module")
def speech(rt):
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    wb = WorldBatch(0)
    xa = [synth_utterance(80, FS, 0.5), synth_utterance(81, FS, 0.5)]
    xb = [synth_utterance(90, FS, 0.5), synth_utterance(91, FS, 0.5)]
    enc_a = wb.encode(xa, FS, f0_method="dio", want_coarse=True)
    enc_b = wb.encode(xb, FS, f0_method="dio", want_coarse=True)
    return wb, enc_a, enc_b


def test_end_to_end_on_compact_encodings(speech):
    import torch
    from world import gmm

    wb, enc_a, enc_b = speech
    ce_a, ce_b = enc_a.compact(n0=N0), enc_b.compact(n0=N0)
    al = enc_a.align(enc_b, n0=N0)
    model, hist = gmm.fit_compact(ce_a, ce_b, al, 2, n_iter=3, reg_covar=1e-4)
    assert model.dx == model.dy == 2 * (N0 - 1) and model.n_components == 2 and len(hist) == 3
    assert all(np.isfinite(hist)) and hist[-1] >= hist[0]
    out = gmm.convert_compact(ce_a, model)
    for name in ("f0", "vuv", "band_ap", "ap_gate", "temporal_positions"):
        assert torch.equal(getattr(out, name), getattr(ce_a, name)), name
    assert torch.equal(out.mcep[:, 0], ce_a.mcep[:, 0]) and out.mcep.shape == ce_a.mcep.shape
    assert bool(torch.isfinite(out.mcep).all()) and not torch.equal(out.mcep[:, 1:], ce_a.mcep[:, 1:])
    assert np.array_equal(out.frame_off, ce_a.frame_off) and out.n0 == N0
    y, y_off = wb.decode_device(out.expand(wb))
    _, want_off = wb.decode_device(ce_a.expand(wb))
    assert np.array_equal(np.asarray(y_off), np.asarray(want_off)) and int(np.asarray(y_off)[-1]) == int(y.shape[0])
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert wb.rt.take_flags() == [0] * 16
    with pytest.raises(ValueError):
        gmm.convert_compact(ce_a.to_host(), model)
    with pytest.raises(ValueError, match="windows"):
        gmm.convert_compact(ce_a, model, windows=mref.HTS_WINDOWS)


def test_numpy_dict_forms_give_what_the_device_forms_give(speech):
    from world import gmm
    from world.features import imcep_device
    from world.main import World

    wb, enc_a, enc_b = speech
    rt = wb.rt
    dats_a, dats_b = enc_a.to_dicts(), enc_b.to_dicts()
    W = World()
    model = W.fit_conversion(dats_a, dats_b, n_components=2, n0=N0, n_iter=3, reg_covar=1e-4)
    al = enc_a.align(enc_b, n0=N0)
    want, _ = gmm.fit_mceps(rt, enc_a.batch, enc_a.mcep(N0), enc_b.batch, enc_b.mcep(N0), al, 2, 3, reg_covar=1e-4)
    for a, b in ((model.weights, want.weights), (model.means, want.means), (model.covariances, want.covariances)):
        assert a.tobytes() == b.tobytes()
    conv = W.convert_voice(dats_a[0], model)
    mc = gmm.convert_mcep(rt, enc_a.batch, enc_a.mcep(N0), model)
    n0_frames = int(enc_a.batch.frame_off[1])
    spec = imcep_device(rt, mc, enc_a.fft_size)[:n0_frames].cpu().numpy().T
    assert conv["spectrogram"].shape == dats_a[0]["spectrogram"].shape and conv["spectrogram"].tobytes() == np.ascontiguousarray(spec).tobytes()
    for key in ("f0", "vuv", "aperiodicity", "temporal_positions"):
        assert np.array_equal(conv[key], dats_a[0][key]), key
    assert conv is not dats_a[0] and not np.array_equal(conv["spectrogram"], dats_a[0]["spectrogram"])
    out = W.decode(conv)
    assert np.all(np.isfinite(out["out"])) and len(out["out"]) > 0
