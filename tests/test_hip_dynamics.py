"""GPU: the dynamic features and the parameter generation on encoded utterances (world/dynamics.py through
CompactEncoding.dynamic_features / with_trajectories and World.delta_features / World.mlpg): two short synthetic
utterances are encoded, compacted, turned into static + delta + delta-delta rows and back into tracks under unit
variances; the tracks equal tests/_mlpg_reference.py on the downloaded rows bit for bit, and the encoding that carries
them decodes."""
import numpy as np
import pytest

import _mlpg_cases as mc
import _mlpg_reference as ref

pytestmark = pytest.mark.gpu

FS = 16000


@pytest.fixture(scope="module")
def encoded():
    """(WorldBatch, CompactEncoding, its dynamic features, the encoding with the generated tracks); read-only."""
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    wb = WorldBatch(0)
    enc = wb.encode([synth_utterance(70, FS, 0.5), synth_utterance(71, FS, 0.62)], FS, f0_method="dio", want_coarse=True)
    ce = enc.compact(n0=40)
    feats = ce.dynamic_features()
    ones = {k: wb.rt.zeros((int(v.shape[1]),)) + 1 for k, v in feats.items()}
    gen = ce.with_trajectories(mcep=(feats["mcep"], ones["mcep"]), band_ap=(feats["band_ap"], ones["band_ap"]))
    return wb, ce, feats, gen


def test_features_and_tracks_equal_the_reference_bit_for_bit(encoded):
    wb, ce, feats, gen = encoded
    fo = ce.frame_off
    assert ce.n_utt == 2 and tuple(feats["mcep"].shape) == (ce.total_frames, 120)
    assert tuple(feats["band_ap"].shape) == (ce.total_frames, 3 * int(ce.band_ap.shape[1]))
    for key in ("mcep", "band_ap"):
        x, y, c = getattr(ce, key).cpu().numpy(), feats[key].cpu().numpy(), getattr(gen, key).cpu().numpy()
        assert c.shape == x.shape
        for u in range(2):
            rows = slice(int(fo[u]), int(fo[u + 1]))
            assert mc.same_bits(y[rows], ref.delta_features(x[rows], ref.HTS_WINDOWS)), (key, u)
            want, piv = ref.mlpg(y[rows], np.ones(y.shape[1]), ref.HTS_WINDOWS)
            assert np.all(piv > 0)
            assert mc.same_bits(c[rows], want), (key, u)
        assert np.max(np.abs(c - x)) <= 1e-9 * max(1.0, np.max(np.abs(x)))  # (unit variances: the track comes back)
    assert wb.rt.take_flags() == [0] * 16


def test_the_generated_encoding_carries_the_rest_over_and_decodes(encoded):
    import torch

    wb, ce, feats, gen = encoded
    for name in ("f0", "vuv", "ap_gate", "temporal_positions"):
        assert torch.equal(getattr(gen, name), getattr(ce, name)), name
    assert np.array_equal(gen.frame_off, ce.frame_off) and gen.n0 == ce.n0 and gen.fs == ce.fs
    only_mcep = ce.with_trajectories(mcep=(feats["mcep"], feats["mcep"] * 0 + 1))  # per-frame variances, band_ap kept
    assert only_mcep.band_ap is ce.band_ap and torch.equal(only_mcep.mcep, gen.mcep)
    y, y_off = wb.decode_device(gen.expand(wb))
    _, want_off = wb.decode_device(ce.expand(wb))
    assert np.array_equal(np.asarray(y_off), np.asarray(want_off)) and int(np.asarray(y_off)[-1]) == int(y.shape[0])
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert wb.rt.take_flags() == [0] * 16


def test_numpy_forms_give_the_device_forms_bits(encoded):
    from world.main import World

    wb, ce, feats, gen = encoded
    fo = ce.frame_off
    x = ce.mcep.cpu().numpy()
    parts = [x[int(fo[u]):int(fo[u + 1])] for u in range(2)]
    w = World()
    ys = w.delta_features(parts)
    assert mc.same_bits(np.concatenate(ys), feats["mcep"].cpu().numpy())
    assert mc.same_bits(w.delta_features(parts[1]), ys[1])
    cs = w.mlpg(ys, np.ones(120))
    assert mc.same_bits(np.concatenate(cs), gen.mcep.cpu().numpy())
    assert mc.same_bits(w.mlpg(ys[0], np.ones_like(ys[0])), cs[0])
    assert mc.same_bits(w.mlpg(ys, [np.ones_like(y) for y in ys])[1], cs[1])
    asym = mc.ASYMMETRIC
    got = w.delta_features(parts[0], windows=asym)
    assert mc.same_bits(got, ref.delta_features(parts[0], asym))
    assert wb.rt.take_flags() == [0] * 16
