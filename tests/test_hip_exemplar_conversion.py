"""GPU: world.exemplar end to end on synthetic speech — four 0.5 s utterances per speaker at 16 kHz over the mel-cepstrum
(as tests/test_hip_gmm_fit.py) and at 48 kHz over line spectral frequencies of order 40: build_compact ->
convert_compact, both modes, leave-one-out, the NumPy-dict forms of World and the vocoder-free form.  Every comparison is
bit for bit: against the database's own rows, against mlpg_device applied by hand, against tests/_exemplar_reference.py
run on the downloaded features."""
import numpy as np
import pytest

import _exemplar_reference as xref

pytestmark = pytest.mark.gpu

N0, P, K = 13, 40, 6
CARRIED = ("f0", "vuv", "band_ap", "ap_gate", "temporal_positions")


def _chain(fs, **compact_kw):
    from world import exemplar
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    wb = WorldBatch(0)
    xa = [synth_utterance(80 + u, fs, 0.5) for u in range(4)]
    xb = [synth_utterance(90 + u, fs, 0.5) for u in range(4)]
    batch, x_d, tp_d = wb.upload(xa, fs)
    enc_a = wb.encode_device(batch, x_d, tp_d, fs, f0_method="dio", want_coarse=True)
    enc_b = wb.encode(xb, fs, f0_method="dio", want_coarse=True)
    ce_a, ce_b = enc_a.compact(**compact_kw), enc_b.compact(**compact_kw)
    al = ce_a.align(ce_b)
    db = exemplar.build_compact(ce_a, ce_b, al)
    assert wb.rt.take_flags() == [0] * 16
    return {"wb": wb, "rt": wb.rt, "batch": batch, "x_d": x_d, "enc_a": enc_a, "enc_b": enc_b, "ce_a": ce_a, "ce_b": ce_b, "al": al,
            "db": db, "key": "lsf" if "lsf_order" in compact_kw else "mcep"}


@pytest.fixture(scope="module")
def mcep16():
    return _chain(16000, n0=N0)


@pytest.fixture(scope="module")
def lsf48():
    return _chain(48000, lsf_order=P)


@pytest.fixture(scope="module", params=["mcep16", "lsf48"])
def chain(request):
    return request.getfixturevalue(request.param)


def test_the_database_is_the_targets_rows(chain):
    from world import exemplar
    from world.dynamics import delta_features_device

    rt, db, ce_a, ce_b, al, key = (chain[k] for k in ("rt", "db", "ce_a", "ce_b", "al", "key"))
    d = int(getattr(ce_b, key).shape[1]) - 1
    fb = delta_features_device(rt, exemplar._frames_batch(rt, ce_b.frame_off), getattr(ce_b, key)[:, 1:], db.windows).cpu().numpy()
    fa = delta_features_device(rt, exemplar._frames_batch(rt, ce_a.frame_off), getattr(ce_a, key)[:, 1:], db.windows).cpu().numpy()
    assert db.y.tobytes() == fb.tobytes() and db.x.tobytes() == fa[al.map_b2a.cpu().numpy()].tobytes()
    assert db.n_rows == ce_b.total_frames and db.n_static == d and db.kind == key
    assert np.array_equal(db.utt_off, ce_b.frame_off) and np.array_equal(db.succ, xref.chain_succ(ce_b.frame_off))
    assert db.scale_x.tobytes() == (1.0 / np.std(db.x, axis=0)).tobytes() and db.scale_y.tobytes() == (1.0 / np.std(db.y, axis=0)).tobytes()
    assert (db.lsf_order, db.lsf_min_gap is not None) == ((P, True) if key == "lsf" else (None, False))


def test_frames_mode_gives_rows_of_the_database_and_the_reference_selection(chain):
    import torch
    from world import exemplar
    from world.dynamics import delta_features_device

    rt, db, ce_a, key = (chain[k] for k in ("rt", "db", "ce_a", "key"))
    out, info = exemplar.convert_compact(ce_a, db, k=K, weight=1.0)
    sel, slot, idx = (info[n].cpu().numpy() for n in ("sel", "slot", "idx"))
    d = db.n_static
    rows = getattr(out, key).cpu().numpy()
    assert rows[:, 1:].tobytes() == np.ascontiguousarray(db.y[sel][:, :d]).tobytes()  # frames the target produced, unscaled
    assert torch.equal(getattr(out, key)[:, 0], getattr(ce_a, key)[:, 0])
    for name in CARRIED:
        assert torch.equal(getattr(out, name), getattr(ce_a, name)), name
    assert np.array_equal(out.frame_off, ce_a.frame_off) and (out.kind, out.lsf_order) == (ce_a.kind, ce_a.lsf_order)
    # the device against the reference on the downloaded features
    batch = exemplar._frames_batch(rt, ce_a.frame_off)
    q = delta_features_device(rt, batch, getattr(ce_a, key)[:, 1:], db.windows).cpu().numpy() * db.scale_x
    t = db.host_tables()
    want_idx, want_dist = xref.knn(q, t["x"], K)
    want_sel, want_slot, want_total, _ = xref.frame_select(ce_a.frame_off, want_idx, want_dist, t["y"][:, :d], db.succ, 1.0)
    assert idx.tobytes() == want_idx.tobytes() and sel.tobytes() == want_sel.tobytes() and slot.tobytes() == want_slot.tobytes()
    assert info["total"].cpu().numpy().tobytes() == want_total.tobytes()
    assert np.all(idx[:, 0] >= 0) and rt.take_flags() == [0] * 16


def test_selected_lsf_rows_decode_without_any_repair(lsf48):
    import torch
    from world import exemplar, lsf

    wb, rt, db, ce_a = (lsf48[k] for k in ("wb", "rt", "db", "ce_a"))
    out, _ = exemplar.convert_compact(ce_a, db, k=K)
    _, changed = lsf.repair_device(rt, out.lsf[:, 1:], db.lsf_min_gap, want_changed=True)
    assert int(changed.sum()) == 0  # never sharper than what the target produced
    y, y_off = wb.decode_device(out.expand(wb))
    assert int(np.asarray(y_off)[-1]) == int(y.shape[0]) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert rt.take_flags() == [0] * 16


def test_mlpg_mode_is_mlpg_device_over_the_same_selection(chain):
    import torch
    from world import exemplar
    from world.dynamics import mlpg_device

    rt, db, ce_a, key = (chain[k] for k in ("rt", "db", "ce_a", "key"))
    frames, info = exemplar.convert_compact(ce_a, db, k=K)
    out, info2 = exemplar.convert_compact(ce_a, db, k=K, mode="mlpg")
    assert torch.equal(info["sel"], info2["sel"])
    t = db.prepared(rt)
    track = mlpg_device(rt, exemplar._frames_batch(rt, ce_a.frame_off), t["y_raw"].index_select(0, info["sel"].to(torch.int64)),
                        t["var_y"], db.windows)
    if key == "lsf":
        from world.lsf import repair_device
        track = repair_device(rt, track, db.lsf_min_gap)
    assert torch.equal(getattr(out, key)[:, 1:], track) and torch.equal(getattr(out, key)[:, 0], getattr(ce_a, key)[:, 0])
    assert not torch.equal(getattr(out, key), getattr(frames, key)) and bool(torch.isfinite(getattr(out, key)).all())
    assert t["var_y"].cpu().numpy().tobytes() == np.var(db.y, axis=0).tobytes()
    assert rt.take_flags() == [0] * 16


def test_leave_one_out_selects_nothing_of_the_excluded_utterance(mcep16):
    from world import exemplar

    db, ce_a = mcep16["db"], mcep16["ce_a"]
    _, info_all = exemplar.convert_compact(ce_a, db, k=K)
    _, info = exemplar.convert_compact(ce_a, db, k=K, exclude=[0, 1, 2, 3])  # every training utterance without its own pair
    sel, idx, fo, ro = info["sel"].cpu().numpy(), info["idx"].cpu().numpy(), ce_a.frame_off, db.utt_off
    all_sel = info_all["sel"].cpu().numpy()
    inside = 0
    for u in range(4):
        s = slice(int(fo[u]), int(fo[u + 1]))
        assert not np.any((idx[s] >= ro[u]) & (idx[s] < ro[u + 1])) and not np.any((sel[s] >= ro[u]) & (sel[s] < ro[u + 1]))
        inside += int(np.count_nonzero((all_sel[s] >= ro[u]) & (all_sel[s] < ro[u + 1])))
    assert inside > 0  # (without the exclusion an utterance does find its own pair)
    _, some = exemplar.convert_compact(ce_a, db, k=K, exclude=[None, 1, None, None])
    some_sel = some["sel"].cpu().numpy()
    s1 = slice(int(fo[1]), int(fo[2]))
    keep = np.ones(len(sel), dtype=bool)
    keep[s1] = False
    assert np.array_equal(some_sel[s1], sel[s1]) and np.array_equal(some_sel[keep], all_sel[keep])
    with pytest.raises(ValueError):
        exemplar.convert_compact(ce_a, db, k=K, exclude=[0, 1])
    with pytest.raises(ValueError):
        exemplar.convert_compact(ce_a, db, k=K, exclude=[0, 1, 2, 4])


def test_world_forms_give_the_device_forms_bytes(mcep16):
    from world import exemplar
    from world.align import align_device
    from world.features import imcep_device
    from world.main import World

    rt, enc_a, enc_b = mcep16["rt"], mcep16["enc_a"], mcep16["enc_b"]
    dats_a, dats_b = enc_a.to_dicts(), enc_b.to_dicts()
    W = World()
    db = W.build_exemplars(dats_a, dats_b, n0=N0)
    ma, mb = enc_a.mcep(N0), enc_b.mcep(N0)
    al = align_device(rt, enc_a.batch, ma[:, 1:], enc_b.batch, mb[:, 1:])
    want = exemplar.build_rows(rt, enc_a.batch, ma, enc_b.batch, mb, al)
    for name in ("x", "y", "succ", "scale_x", "scale_y", "utt_off"):
        assert getattr(db, name).tobytes() == getattr(want, name).tobytes(), name
    conv = W.convert_voice_exemplar(dats_a[1], db, k=K, weight=0.5)
    from world.batch import BatchEncoding
    one = BatchEncoding.from_dicts(rt, [dats_a[1]])
    rows, _ = exemplar.convert_rows(rt, one.batch, one.mcep(N0), db, K, 0.5)
    spec = imcep_device(rt, rows, enc_a.fft_size).cpu().numpy().T
    assert conv["spectrogram"].tobytes() == np.ascontiguousarray(spec).tobytes()
    for key in ("f0", "vuv", "aperiodicity", "temporal_positions"):
        assert np.array_equal(conv[key], dats_a[1][key]), key
    assert np.all(np.isfinite(W.decode(conv)["out"]))
    with pytest.raises(NotImplementedError):
        W.build_exemplars(dats_a, dats_b, devices=[0])
    with pytest.raises(NotImplementedError):
        W.convert_voice_exemplar(dats_a[1], db, devices=[0])
    assert rt.take_flags() == [0] * 16


def test_convert_waveform_is_the_differential_filter_of_the_same_pair(chain):
    import torch
    from world import exemplar
    from world.specfilter import differential_device

    wb, rt, db, ce_a = (chain[k] for k in ("wb", "rt", "db", "ce_a"))
    y_d, conv, info = exemplar.convert_waveform(wb, chain["batch"], chain["x_d"], ce_a, db, k=K)
    want_conv, want_info = exemplar.convert_compact(ce_a, db, k=K)
    assert torch.equal(info["sel"], want_info["sel"]) and torch.equal(getattr(conv, chain["key"]), getattr(want_conv, chain["key"]))
    assert torch.equal(y_d, differential_device(wb, chain["batch"], chain["x_d"], ce_a, want_conv))
    assert y_d.shape == chain["x_d"].shape and bool(torch.isfinite(y_d).all())
    assert rt.take_flags() == [0] * 16
