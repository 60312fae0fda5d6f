"""CPU: the host side of the chain over line spectral frequencies: the two ABI entries are declared, bound and exported
and fail on wrong arguments without a device; the dB formulas of world.lsf.distortion_db (evaluated in NumPy) against the
definition — 10 log10 of the ratio of the two envelopes E / A2, RMS over the bins — in long double, within the bound the
reference derives; the argument checks of align_compact, fit_compact / convert_compact and with_trajectories; the .npz
forms of JointGMM both ways; and lsf_min_gap against its definition."""
import os
import re

import numpy as np
import pytest

import _lsf_chain_reference as cref
from test_lsf_host import _host_encoding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("wh_lsf_repair", 11), ("wh_lsf_distortion", 15))


def test_header_binding_and_exports():
    from world import _hip

    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    for name, n_args in ENTRIES:
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == n_args
    lib = _hip.load_library()
    assert lib.wh_version() >= 119
    for name, _ in ENTRIES:
        assert hasattr(lib, name)
    assert lib.wh_lsf_repair(None, None, None, 0, 24, 24, 0.01, 3.0, None, 24, None) != 0
    assert b"null" in lib.wh_last_error()
    assert lib.wh_lsf_distortion(None, None, None, 0, 25, None, 0, 25, 24, None, None, 0, None, 513, None) != 0


def test_the_unit_is_built_like_wh_lsf():
    from world import lsf

    src = open(os.path.join(ROOT, "python-world_amd", "csrc", "wh_lsf_chain.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert int(re.search(r"constexpr int kLsfMaxOrder = (\d+);", src).group(1)) == lsf.MAX_ORDER
    build = open(os.path.join(ROOT, "python-world_amd", "build.py")).read()
    assert "wh_lsf_chain" not in build and "-ffp-contract=off" in build  # the default flags, no entry of its own
    assert not re.search(r"\batomic\w*\s*\(", code) and not re.search(r"\bf(max|min)\s*\(", code)
    assert len(re.findall(r"\blog\s*\(", code)) == 1  # the distortion's one logarithm per bin


def _rows(n, p, seed):
    rng = np.random.RandomState(seed)
    w = np.sort(rng.uniform(0.05, np.pi - 0.05, size=(n, p)), axis=1)
    return np.concatenate([rng.uniform(-8.0, 2.0, size=(n, 1)), w], axis=1)


@pytest.mark.parametrize("p,k_bins", [(2, 129), (24, 513), (40, 1025)])
def test_db_formulas_against_the_envelopes_in_long_double(p, k_bins):
    from world import lsf

    rows_a = _rows(30, p, p)
    rows_b = np.array(rows_a)
    rows_b[:, 1:] = 0.7 * rows_a[:, 1:] + 0.3 * _rows(30, p, p + 1)[:, 1:]
    rows_b[:, 0] = _rows(30, p, p + 2)[:, 0]
    xa, xb = np.cos(rows_a[:, 1:]), np.cos(rows_b[:, 1:])
    ex_a, ex_b = np.concatenate([rows_a[:, :1], xa], axis=1), np.concatenate([rows_b[:, :1], xb], axis=1)
    s = cref.distortion(ex_a, ex_b, k_bins)
    t = cref.log_ratio(xa, xb, k_bins, cref.LD)
    b1, b2 = cref.sum_bounds(t, p)
    g = rows_a[:, 0] - rows_b[:, 0]
    assert lsf.LSD_SCALE == cref.LSD_SCALE
    for gain in (True, False):
        want = cref.lsd_long_double(rows_a, rows_b, k_bins, gain)
        got = lsf.distortion_db(np, g, s[:, 0], s[:, 1], k_bins, gain)
        # (the long-double definition takes exp of the two gains apart: 2^-64 relative on either envelope, far below)
        tol = cref.db_bound(g, s[:, 0], s[:, 1], b1, b2, k_bins, gain)
        assert np.all(np.abs(got.astype(cref.LD) - want) <= tol), gain
        assert got.tobytes() == cref.distortion_db(g, s[:, 0], s[:, 1], k_bins, gain).tobytes()
        # the sign of the cross term is the contract's: with the other sign the gain case is off by dB, not by rounding
        if gain:
            wrong = cref.LSD_SCALE * np.sqrt(np.maximum(g * g + 2.0 * g * s[:, 0] / k_bins + s[:, 1] / k_bins, 0.0))
            assert np.all(np.abs(wrong - want.astype(np.float64)) > 1e6 * tol)


def test_equal_angles_give_the_gain_difference():
    from world import lsf

    rows_a = _rows(20, 24, 3)
    rows_b = np.array(rows_a)
    rows_b[:, 0] = _rows(20, 24, 4)[:, 0]
    x = np.cos(rows_a[:, 1:])
    ex = np.concatenate([rows_a[:, :1], x], axis=1)
    s = cref.distortion(ex, ex, 513)
    assert np.all(s == 0.0)
    g = rows_a[:, 0] - rows_b[:, 0]
    assert np.array_equal(lsf.distortion_db(np, g, s[:, 0], s[:, 1], 513, True), lsf.LSD_SCALE * np.abs(g))
    assert np.all(lsf.distortion_db(np, g, s[:, 0], s[:, 1], 513, False) == 0.0)


def test_encodings_that_cannot_be_compared():
    from world.align import align_compact, check_compact_pair
    from world.compact import CompactEncoding

    lsf48, lsf16 = _host_encoding("lsf"), _host_encoding("lsf", 16000, 1024)
    mcep16, dense = _host_encoding("mcep", 16000, 1024), _host_encoding("spectrogram")
    assert check_compact_pair(lsf48, _host_encoding("lsf", seed=1)) == 24
    assert check_compact_pair(mcep16, _host_encoding("mcep", 16000, 1024, seed=1)) == 39
    with pytest.raises(ValueError, match="kind"):
        check_compact_pair(lsf16, mcep16)
    with pytest.raises(ValueError, match="kind"):
        check_compact_pair(dense, dense)
    with pytest.raises(ValueError, match="sampling rates"):
        check_compact_pair(lsf48, lsf16)
    short = CompactEncoding(None, 48000, 2048, 5, False, None, 0, 8000, lsf48.frame_off, lsf48.temporal_positions, lsf48.f0,
                            lsf48.vuv, None, lsf48.band_ap, lsf48.ap_gate, lsf=lsf48.lsf[:, :23])
    assert short.lsf_order == 22
    with pytest.raises(ValueError, match="order"):
        check_compact_pair(lsf48, short)
    with pytest.raises(ValueError, match="resident"):
        align_compact(lsf48, lsf48)
    with pytest.raises(ValueError, match="resident"):
        lsf48.align(lsf48)


def test_mixture_limits_and_kinds():
    from world import gmm

    gmm.check_lsf_width(40, gmm.CONVERSION_WINDOWS)
    with pytest.raises(ValueError, match="160 columns"):
        gmm.check_lsf_width(42, gmm.CONVERSION_WINDOWS)
    with pytest.raises(ValueError, match="160 columns"):
        gmm.fit_conversion_dicts([{"fs": 48000}], [{"fs": 48000}], 2, lsf_order=64)
    with pytest.raises(ValueError, match="sampling rates"):
        gmm.fit_conversion_dicts([{"fs": 48000}], [{"fs": 16000}], 2, lsf_order=24)
    with pytest.raises(ValueError, match="even"):
        gmm.fit_conversion_dicts([{"fs": 48000}], [{"fs": 48000}], 2, lsf_order=25)
    lsf48, mcep16 = _host_encoding("lsf"), _host_encoding("mcep", 16000, 1024)
    eye = np.eye(4)[None]
    model = gmm.JointGMM([1.0], np.zeros((1, 4)), eye, 2, "lsf", 24, 0.01)
    plain = gmm.JointGMM([1.0], np.zeros((1, 4)), eye, 2)
    assert (plain.kind, plain.lsf_order, plain.lsf_min_gap) == ("mcep", None, None)
    for ce, m in ((lsf48, plain), (mcep16, model)):  # (host encodings: the first check is the residence)
        with pytest.raises(ValueError):
            gmm.convert_compact(ce, m)
    for kw in (dict(kind="lsf"), dict(kind="lsf", lsf_order=24), dict(lsf_order=24, lsf_min_gap=0.1), dict(kind="other")):
        with pytest.raises(ValueError):
            gmm.JointGMM([1.0], np.zeros((1, 4)), eye, 2, **kw)


def test_with_trajectories_takes_the_encoding_s_own_kind():
    lsf48, mcep16 = _host_encoding("lsf"), _host_encoding("mcep", 16000, 1024)
    pair = (np.zeros((12, 75)), np.ones(75))
    with pytest.raises(ValueError, match="mcep= on an encoding that holds line spectral frequencies"):
        lsf48.with_trajectories(mcep=pair)
    with pytest.raises(ValueError, match="lsf= on an encoding that holds no line spectral frequencies"):
        mcep16.with_trajectories(lsf=pair, min_gap=0.01)
    with pytest.raises(ValueError, match="host"):
        lsf48.with_trajectories(lsf=pair, min_gap=0.01)


def test_joint_gmm_files_both_ways(tmp_path):
    from world import gmm

    rng = np.random.RandomState(0)
    a = rng.randn(2, 6, 6)
    cov = a @ a.transpose(0, 2, 1) + np.eye(6)[None]
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    model = gmm.JointGMM([0.25, 0.75], rng.randn(2, 6), cov, 2, "lsf", 40, 0.0123)
    model.save_npz(str(tmp_path / "lsf.npz"))
    back = gmm.JointGMM.load_npz(str(tmp_path / "lsf.npz"))
    assert (back.kind, back.lsf_order, back.lsf_min_gap, back.dx) == ("lsf", 40, 0.0123, 2)
    for name in ("weights", "means", "covariances"):
        assert getattr(back, name).tobytes() == getattr(model, name).tobytes()
    # a mel-cepstral model writes the file it always wrote, and such a file loads as it did
    plain = gmm.JointGMM(model.weights, model.means, model.covariances, 2)
    plain.save_npz(str(tmp_path / "mcep.npz"))
    with np.load(str(tmp_path / "mcep.npz")) as z:
        assert sorted(z.files) == ["covariances", "dx", "means", "weights"]
    np.savez(str(tmp_path / "old.npz"), weights=model.weights, means=model.means, covariances=model.covariances, dx=np.asarray(2))
    old = gmm.JointGMM.load_npz(str(tmp_path / "old.npz"))
    assert (old.kind, old.lsf_order, old.lsf_min_gap) == ("mcep", None, None) and old.means.tobytes() == model.means.tobytes()


def test_compact_encoding_files_both_ways(tmp_path):
    from world.compact import CompactEncoding

    h = _host_encoding("lsf")
    h.save_npz(str(tmp_path / "lsf.npz"))
    g = CompactEncoding.load_npz(str(tmp_path / "lsf.npz"))
    assert (g.kind, g.lsf_order, g.fs, g.fft_size) == ("lsf", 24, 48000, 2048) and g.lsf.tobytes() == h.lsf.tobytes()
    assert np.array_equal(g.frame_off, h.frame_off) and g.band_ap.tobytes() == h.band_ap.tobytes()
    # a mel-cepstral file as it was written before the kind existed (no 'lsf', no 'lsf_order') loads as it did, and a
    # mel-cepstral encoding still writes exactly those keys
    m = _host_encoding("mcep", 16000, 1024)
    m.save_npz(str(tmp_path / "mcep.npz"))
    with np.load(str(tmp_path / "mcep.npz")) as z:
        old = {k: z[k] for k in z.files}
    assert "lsf" not in old and "lsf_order" not in old
    np.savez(str(tmp_path / "old.npz"), **old)
    back = CompactEncoding.load_npz(str(tmp_path / "old.npz"))
    assert (back.kind, back.lsf, back.lsf_order, back.n0) == ("mcep", None, None, 40) and back.mcep.tobytes() == m.mcep.tobytes()
    # and the kinds do not compare
    from world.align import check_compact_pair
    with pytest.raises(ValueError, match="kind"):
        check_compact_pair(g, back)


def test_the_end_to_end_input_is_a_pair_on_which_conversion_helps():
    """The chain of tests/_lsf_chain_e2e.py on the CPU, from the references alone, on the committed 48 kHz fixture: the
    aligned gain-free LSD to the target falls from the source to the conversion.  Recorded: source 3.653414 dB, converted
    2.650187 dB (path of 101 cells, 2 components, 3 EM steps); a device run of the chain may be 7.2e-11 dB and 8.0e-9 dB
    from these (tolerances derived in that module's docstring; every converted angle within 4.1e-13 rad)."""
    import _lsf_chain_e2e as e2e

    r = e2e.record()
    print("end-to-end record: source %.9f dB, converted %.9f dB, tolerances %.3g / %.3g dB, dw %.3g rad"
          % (r["before"], r["after"], r["tol_before"], r["tol_after"], r["dw"]))
    assert r["after"] < r["before"]
    assert abs(r["before"] - 3.653414) < 1e-6 and abs(r["after"] - 2.650187) < 1e-6
    assert 0 < r["tol_before"] < 1e-9 and r["tol_before"] <= r["tol_after"] < 1e-6 and 0 < r["dw"] < 1e-10
    w = r["conv"][:, 1:]
    gap = r["model"].lsf_min_gap
    assert np.all(np.diff(w, axis=1) >= gap - 2.0 ** -51) and w[:, 0].min() >= gap - 2.0 ** -51
    assert (np.pi - w[:, -1]).min() >= gap - 2.0 ** -51 and r["conv"][:, 0].tobytes() == r["rows_a"][:, 0].tobytes()
    assert len(set(r["best"].tolist())) == 2  # both components are used


def test_lsf_min_gap_is_its_definition():
    import torch
    from world import gmm

    rng = np.random.RandomState(9)  # a made corpus: 24 angles pi / 25 apart, moved by up to 0.02 each
    rows = np.concatenate([rng.randn(201, 1), np.pi * (np.arange(24) + 1.0) / 25 + rng.uniform(-0.02, 0.02, (201, 24))], axis=1)
    rows[57, 8] = rows[57, 7] + 1e-4  # the sharpest pair of the corpus
    best = np.inf
    for r in rows:
        w = r[1:]
        best = min(best, w[0], float(np.pi) - w[-1], min(w[i + 1] - w[i] for i in range(len(w) - 1)))
    assert gmm.lsf_min_gap(rows) == best == rows[57, 8] - rows[57, 7]
    assert gmm.lsf_min_gap(torch.from_numpy(rows)) == best
    low = np.array(rows)
    low[3, 1] = 1e-5
    assert gmm.lsf_min_gap(low) == 1e-5
    high = np.array(rows)
    high[200, -1] = np.pi - 2e-5
    assert gmm.lsf_min_gap(high) == float(np.pi) - high[200, -1]
    nan = np.array(rows)
    nan[5, 5] = np.nan
    assert np.isnan(gmm.lsf_min_gap(nan))
