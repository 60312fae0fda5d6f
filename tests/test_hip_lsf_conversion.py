"""GPU: the voice-conversion chain over line spectral frequencies, end to end, at 16 kHz and at 48 kHz — where every one
of these calls raised before the chain took the kind 'lsf': encode -> compact(lsf_order) -> align_compact -> fit_compact ->
convert_compact -> expand -> decode on two synthetic speakers (a few hundred frames), each convenience call in lock-step
with the generic calls it is made of, bit for bit; then what a conversion must be: decodable rows no sharper than the
target's sharpest, finite audio of the right length, an aligned log-spectral distortion to the target that falls from the
source to the conversion, and a save / load round trip of model and encodings that reproduces it bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, M, SECONDS = 12, 2, 0.5


@pytest.fixture(scope="module", params=[16000, 48000], ids=["16k", "48k"])
def chain(request):
    from world import gmm
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    fs = request.param
    wb = WorldBatch(0)
    xa = [synth_utterance(80 + u, fs, SECONDS) for u in range(3)]
    xb = [synth_utterance(90 + u, fs, SECONDS + 0.05 * u) for u in range(3)]
    enc_a = wb.encode(xa, fs, f0_method="dio", want_coarse=True)
    enc_b = wb.encode(xb, fs, f0_method="dio", want_coarse=True)
    ce_a, ce_b = enc_a.compact(lsf_order=P), enc_b.compact(lsf_order=P)
    al = ce_a.align(ce_b)
    model, hist = gmm.fit_compact(ce_a, ce_b, al, M, n_iter=4)
    conv = gmm.convert_compact(ce_a, model)
    assert wb.rt.take_flags() == [0] * 16
    return {"fs": fs, "wb": wb, "rt": wb.rt, "enc_a": enc_a, "enc_b": enc_b, "ce_a": ce_a, "ce_b": ce_b, "al": al,
            "model": model, "hist": hist, "conv": conv}


def _batch(rt, ce):
    return rt.make_batch(np.zeros(ce.n_utt + 1, dtype=np.int64), ce.frame_off)


def test_dynamic_features_and_trajectories_are_the_generic_calls(chain):
    import torch
    from world import dynamics, lsf

    rt, ce = chain["rt"], chain["ce_a"]
    assert ce.kind == "lsf" and ce.fs == chain["fs"] and 200 <= ce.total_frames <= 400
    feats = ce.dynamic_features()
    assert sorted(feats) == ["band_ap", "lsf"]
    want = dynamics.delta_features_device(rt, _batch(rt, ce), ce.lsf, dynamics.HTS_WINDOWS)
    assert torch.equal(feats["lsf"], want) and tuple(want.shape) == (ce.total_frames, 3 * (P + 1))
    var = torch.ones(3 * (P + 1), dtype=torch.float64, device=rt.device)
    gap = 0.02
    out = ce.with_trajectories(lsf=(feats["lsf"], var), min_gap=gap)
    track = dynamics.mlpg_device(rt, _batch(rt, ce), feats["lsf"], var, dynamics.HTS_WINDOWS)
    assert torch.equal(out.lsf[:, 0], track[:, 0])
    assert torch.equal(out.lsf[:, 1:], lsf.repair_device(rt, track[:, 1:], gap))
    assert torch.equal(out.band_ap, ce.band_ap) and out.kind == "lsf" and out.lsf_order == P
    with pytest.raises(ValueError, match="mcep="):
        ce.with_trajectories(mcep=(feats["lsf"], var))
    with pytest.raises(ValueError, match="min_gap"):
        ce.with_trajectories(lsf=(feats["lsf"], var))
    assert rt.take_flags() == [0] * 16


def test_alignment_is_align_device_on_the_angles(chain):
    import torch
    from world.align import align_compact, align_device

    rt, ce_a, ce_b, al = chain["rt"], chain["ce_a"], chain["ce_b"], chain["al"]
    want = align_device(rt, _batch(rt, ce_a), ce_a.lsf[:, 1:], _batch(rt, ce_b), ce_b.lsf[:, 1:])
    again = align_compact(ce_a, ce_b)
    for name in ("path_a", "path_b", "path_len", "cost", "map_a2b", "map_b2a"):
        pos = al.valid_index()[0] if name.startswith("path_") and name != "path_len" else None
        a, b, c = (getattr(x, name) for x in (al, want, again))
        if pos is not None:
            a, b, c = a.index_select(0, pos), b.index_select(0, pos), c.index_select(0, pos)
        assert torch.equal(a, b) and torch.equal(a, c), name
    for u in range(al.n_utt):  # well-formed: from (0, 0) to (N - 1, M - 1) in steps of 0 or 1 on either side, never both 0
        i, j = al.pairs(u)
        n, m = np.diff(ce_a.frame_off)[u], np.diff(ce_b.frame_off)[u]
        assert (i[0], j[0], i[-1], j[-1]) == (0, 0, n - 1, m - 1)
        di, dj = np.diff(i), np.diff(j)
        assert set(di) <= {0, 1} and set(dj) <= {0, 1} and np.all(di + dj >= 1)
    banded = ce_a.align(ce_b, radius=40)
    assert int(banded.path_len.sum()) > 0
    other = chain["enc_b"].compact(lsf_order=P + 2)
    with pytest.raises(ValueError, match="order"):
        ce_a.align(other)
    with pytest.raises(ValueError, match="kind"):
        ce_a.align(chain["enc_b"].compact(n0=None))


def test_fit_and_conversion_are_the_generic_calls(chain):
    import torch
    from world import dynamics, gmm, lsf

    rt, ce_a, ce_b, al, model = chain["rt"], chain["ce_a"], chain["ce_b"], chain["al"], chain["model"]
    win = gmm.CONVERSION_WINDOWS
    fa = dynamics.delta_features_device(rt, _batch(rt, ce_a), ce_a.lsf[:, 1:], win)
    fb = dynamics.delta_features_device(rt, _batch(rt, ce_b), ce_b.lsf[:, 1:], win)
    z, _ = al.joint(fa, fb)
    want, hist = gmm.fit_device(rt, z, 2 * P, M, 4)
    for name in ("weights", "means", "covariances"):
        assert getattr(model, name).tobytes() == getattr(want, name).tobytes(), name
    assert hist == chain["hist"] and all(np.isfinite(hist)) and hist[-1] >= hist[0]
    assert (model.kind, model.lsf_order, model.dx, model.dy) == ("lsf", P, 2 * P, 2 * P)
    # lsf_min_gap: the definition, over the target's rows
    w = ce_b.lsf[:, 1:].cpu().numpy()
    brute = min(w[:, 0].min(), (float(np.pi) - w[:, -1]).min(), np.diff(w, axis=1).min())
    assert model.lsf_min_gap == brute and 0 < brute < np.pi / (P + 2)
    # the conversion: convert_device on the delta rows of the angles, log E carried over, then the repair
    conv = chain["conv"]
    y = gmm.convert_device(rt, _batch(rt, ce_a), fa, model, "mlpg", win)
    assert torch.equal(conv.lsf[:, 1:], lsf.repair_device(rt, y, model.lsf_min_gap))
    assert torch.equal(conv.lsf[:, 0], ce_a.lsf[:, 0])
    for name in ("f0", "vuv", "band_ap", "ap_gate", "temporal_positions"):
        assert torch.equal(getattr(conv, name), getattr(ce_a, name)), name
    assert conv.kind == "lsf" and conv.lsf_order == P and np.array_equal(conv.frame_off, ce_a.frame_off)
    wide = gmm.convert_compact(ce_a, model, min_gap=2 * model.lsf_min_gap)
    assert torch.equal(wide.lsf[:, 1:], lsf.repair_device(rt, y, 2 * model.lsf_min_gap))
    plain = gmm.JointGMM(model.weights, model.means, model.covariances, model.dx)
    with pytest.raises(ValueError, match="kind"):
        gmm.convert_compact(ce_a, plain)
    with pytest.raises(ValueError, match="order"):
        gmm.fit_compact(ce_a, chain["enc_b"].compact(lsf_order=P + 2), al, M)
    assert rt.take_flags() == [0] * 16


def test_converted_rows_decode_and_move_towards_the_target(chain):
    import torch

    rt, wb, ce_a, ce_b, al, conv, model = (chain[k] for k in ("rt", "wb", "ce_a", "ce_b", "al", "conv", "model"))
    w = conv.lsf[:, 1:].cpu().numpy()
    gap = model.lsf_min_gap
    # (w[i] <= fl(w[i+1] - gap): the difference is short of gap by at most that one rounding, 2^-53 pi, and its own)
    assert np.all(np.isfinite(w)) and np.all(w > 0) and np.all(w < np.pi) and np.all(np.diff(w, axis=1) > 0)
    assert np.all(np.diff(w, axis=1) >= gap - 2.0 ** -51) and w[:, 0].min() >= gap - 2.0 ** -51
    assert (np.pi - w[:, -1]).min() >= gap - 2.0 ** -51
    y, y_off = wb.decode_device(conv.expand(wb))
    _, want_off = wb.decode_device(ce_a.expand(wb))
    assert np.array_equal(np.asarray(y_off), np.asarray(want_off)) and int(np.asarray(y_off)[-1]) == int(y.shape[0])
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    before = al.lsd_db(ce_a.lsf, ce_b.lsf, ce_a.fft_size).cpu().numpy()
    after = al.lsd_db(conv.lsf, ce_b.lsf, ce_a.fft_size).cpu().numpy()
    print("fs %d: aligned LSD to the target, gain-free, dB per pair: source %s converted %s"
          % (chain["fs"], np.round(before, 3).tolist(), np.round(after, 3).tolist()))
    assert before.shape == (3,) and np.all(np.isfinite(before)) and np.all(after < before)
    # lsd_db is the mean over the path of distortion_device on the gathered rows
    from world.lsf import distortion_device
    i, j = al.pairs(1)
    ia = torch.from_numpy(i + int(ce_a.frame_off[1])).to(rt.device)
    ib = torch.from_numpy(j + int(ce_b.frame_off[1])).to(rt.device)
    cells = distortion_device(rt, ce_a.lsf, ce_b.lsf, ce_a.fft_size, ia, ib, gain=False)
    assert abs(float(cells.mean()) - before[1]) <= 1e-12 * before[1]
    with_gain = al.lsd_db(ce_a.lsf, ce_b.lsf, ce_a.fft_size, gain=True).cpu().numpy()
    assert np.all(with_gain >= before)  # the RMS about zero is at least the RMS about the mean
    assert rt.take_flags() == [0] * 16


def test_files_reproduce_the_conversion(chain, tmp_path):
    from world import gmm
    from world.compact import CompactEncoding

    rt, ce_a, conv, model = chain["rt"], chain["ce_a"], chain["conv"], chain["model"]
    model.save_npz(str(tmp_path / "model.npz"))
    ce_a.save_npz(str(tmp_path / "a.npz"))
    back = gmm.JointGMM.load_npz(str(tmp_path / "model.npz"))
    assert (back.kind, back.lsf_order, back.lsf_min_gap) == (model.kind, model.lsf_order, model.lsf_min_gap)
    again = gmm.convert_compact(CompactEncoding.load_npz(str(tmp_path / "a.npz")).to_device(rt), back)
    assert again.lsf.cpu().numpy().tobytes() == conv.lsf.cpu().numpy().tobytes()
    conv.save_npz(str(tmp_path / "conv.npz"))
    loaded = CompactEncoding.load_npz(str(tmp_path / "conv.npz"))
    assert loaded.kind == "lsf" and loaded.lsf.tobytes() == conv.lsf.cpu().numpy().tobytes()


def test_the_chain_against_the_cpu_record():
    """The chain on the rows of tests/_lsf_chain_e2e.py — the committed 48 kHz fixture and a second speaker made from it,
    the model fitted on the CPU by the references and handed over — against that module's record: the path and the best
    components are the reference's, every converted angle is within dw of the reference's, and the two aligned LSD values
    are within the derived tolerances of the recorded ones (source 3.653414 dB, converted 2.650187 dB; tolerances 7.2e-11
    and 8.0e-9 dB) and in the same order."""
    import torch

    import _lsf_chain_e2e as e2e
    from world import _hip, dynamics, gmm
    from world.compact import CompactEncoding, d4c_band_layout

    r = e2e.record()
    rt = _hip.Runtime.get()

    def encoding(rows):
        nf = len(rows)
        tp = np.arange(nf) * 0.005
        _, nap = d4c_band_layout(e2e.FS)
        return CompactEncoding(None, e2e.FS, e2e.FFT_SIZE, 5, False, None, 0, 8000, [0, nf], tp, np.full(nf, 120.0), np.ones(nf),
                               None, np.full((nf, nap), 0.1), np.ones(nf), tp_host=tp, lsf=np.array(rows)).to_device(rt)

    ce_a, ce_b = encoding(r["rows_a"]), encoding(r["rows_b"])
    al = ce_a.align(ce_b)
    pa, pb = al.pairs(0)
    assert np.array_equal(pa, r["path_a"]) and np.array_equal(pb, r["path_b"])
    model = r["model"]
    fa = dynamics.delta_features_device(rt, _batch(rt, ce_a), ce_a.lsf[:, 1:], gmm.CONVERSION_WINDOWS)
    assert np.array_equal(gmm.posteriors_device(rt, fa, model)[2].cpu().numpy(), r["best"])
    conv = gmm.convert_compact(ce_a, model)
    moved = np.abs(conv.lsf.cpu().numpy() - r["conv"])
    print("converted angles: worst |device - record| %.3g rad, bound %.3g" % (moved[:, 1:].max(), r["dw"]))
    assert np.all(moved[:, 0] == 0.0) and np.all(moved[:, 1:] <= r["dw"])
    before = float(al.lsd_db(ce_a.lsf, ce_b.lsf, e2e.FFT_SIZE)[0])
    after = float(al.lsd_db(conv.lsf, ce_b.lsf, e2e.FFT_SIZE)[0])
    print("aligned LSD, device - record: source %.3g dB (tolerance %.3g), converted %.3g dB (tolerance %.3g)"
          % (before - r["before"], r["tol_before"], after - r["after"], r["tol_after"]))
    assert abs(before - r["before"]) <= r["tol_before"]
    assert abs(after - r["after"]) <= r["tol_after"]
    assert after < before and r["after"] < r["before"]
    assert bool(torch.isfinite(conv.lsf).all()) and rt.take_flags() == [0] * 16


def test_numpy_dict_forms(chain):
    from world import gmm, lsf
    from world.main import World

    rt, enc_a, enc_b, model = chain["rt"], chain["enc_a"], chain["enc_b"], chain["model"]
    dats_a, dats_b = enc_a.to_dicts(), enc_b.to_dicts()
    w = World()
    fitted = w.fit_conversion(dats_a, dats_b, n_components=M, n_iter=4, lsf_order=P)
    for name in ("weights", "means", "covariances"):
        assert getattr(fitted, name).tobytes() == getattr(model, name).tobytes(), name
    assert (fitted.kind, fitted.lsf_order, fitted.lsf_min_gap) == ("lsf", P, model.lsf_min_gap)
    out = w.convert_voice(dats_a[0], fitted)
    n0 = int(enc_a.batch.frame_off[1])
    spec = lsf.ilsf_device(rt, chain["conv"].lsf[:n0], enc_a.fft_size).cpu().numpy().T
    assert out["spectrogram"].shape == dats_a[0]["spectrogram"].shape
    assert out["spectrogram"].tobytes() == np.ascontiguousarray(spec).tobytes()
    for key in ("f0", "vuv", "aperiodicity", "temporal_positions"):
        assert np.array_equal(out[key], dats_a[0][key]), key
    y = w.decode(out)
    assert np.all(np.isfinite(y["out"])) and len(y["out"]) > 0
    with pytest.raises(NotImplementedError):
        w.lsf_distortion(np.zeros((2, 13)), np.zeros((2, 13)), 1024, devices=[0])
