"""Helper of tests/test_hip_bounds.py: runs in a process whose WH_LIB is the BOUNDS build of the library
(tests/_variants.py, bounds; world/_hip.py loads WH_LIB).  The positive control, the CheapTrick fixtures, the f0, D4C and
decode sweeps, the off-regime signals, the whole pipelines and the probes."""
import os

import numpy as np

import _variants as V


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2) / np.mean(b ** 2)))


def main():
    from world import _hip
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch
    from world.cheaptrick import cheaptrick

    rt = _hip.Runtime.get()
    rep = V.Report(rt)

    def whole(key, rt):
        rep.set(key + "_flags", rt.take_flags())
        rep.set(key + "_record", list(_hip.bounds_last()))

    def oob(name, **fields):
        # the fixtures' and the probes' records carry the out-of-range flag alone: what tests/test_hip_bounds.py asks of them
        r = rep.record(name, **fields)
        r["flag"] = r.pop("flags")[_hip.FLAG_OOB]
        return r

    def taken(name, rc, y_d):
        r = oob(name, rc=rc)
        r["finite"] = bool(np.all(np.isfinite(y_d.cpu().numpy())))
        return r

    # ---- positive control: the checker sees a store one past a four-element buffer -----------------------------------
    _hip.check(rt.lib.wh_bounds_selftest(rt.ctx, rt.stream()))
    flags = rt.take_flags()
    rep.set("selftest_flag", flags[_hip.FLAG_OOB])
    rep.set("selftest_record", list(_hip.bounds_last()))
    rep.set("clean_after", (rt.take_flags()[_hip.FLAG_OOB], list(_hip.bounds_last())))
    # ---- the CheapTrick fixtures (reference outputs) -----------------------------------------------------------------
    fix = {}
    for tag in ("syn16k", "syn48k"):
        g = dict(np.load(os.path.join(V.HERE, "golden", "golden_%s.npz" % tag)))
        fs = int(g["fs"])
        src = {"f0": g["stonemask_f0"].copy(), "vuv": g["dio_vuv"].copy(), "temporal_positions": g["tp"].copy()}
        res = cheaptrick(g["x"], fs, src)
        fix[tag] = oob(tag, rel_rms=rel_rms(res["spectrogram"], g["ct_spectrogram"]))
    rep.set("fixtures", fix)
    # ---- f0 sweep: constant contours from far below the floor to beyond fs/2, three rates, transforms 512 ... 4096 ----
    sweep = []
    for fs, fft in ((16000, 1024), (16000, 512), (22050, 1024), (48000, 2048), (96000, 4096)):
        x = synth_utterance(5, fs, 0.6)
        n = int(1000 * len(x) / fs / 5 + 1)
        tp = np.arange(n) * 0.005
        for f0 in (1.0, 20.0, 47.0, 70.0, 71.0, 123.4, 250.0, 499.9, 800.0, 1500.0, 0.45 * fs, 0.4999 * fs, 0.5 * fs,
                   0.75 * fs, 1.5 * fs):
            src = {"f0": np.full(n, f0), "vuv": np.ones(n), "temporal_positions": tp.copy()}
            res = cheaptrick(x, fs, src, fft_size=fft)
            sweep.append(rep.record("cheaptrick", fs=fs, fft=fft, f0=f0, finite=bool(np.all(np.isfinite(res["spectrogram"])))))
    rep.set("sweep_bad", [s for s in sweep if s["flags"][_hip.FLAG_OOB] or not s["finite"]])
    rep.set("sweep_cases", len(sweep))
    # ---- D4C / D4C-Requiem / love-train (round 6, second half: their LDS blocks, waveform gathers, twiddle and window tables and
    # output rows are checked pointers too): the same constant contours, voiced everywhere, at every transform length
    # 512 ... 8192 the two entry points reach, fused and stand-alone gate
    from world.d4c import d4c
    from world.d4cRequiem import d4cRequiem
    dsweep = []
    for fs, req, fft in ((16000, False, None), (22050, False, None), (48000, False, None), (96000, False, None), (8000, False, None),
                         (16000, True, None), (16000, True, 512), (48000, True, None), (96000, True, 4096)):
        x = synth_utterance(6, fs, 0.4)
        n = int(1000 * len(x) / fs / 5 + 1)
        tp = np.arange(n) * 0.005
        for f0 in (1.0, 20.0, 47.0, 70.0, 71.0, 123.4, 250.0, 499.9, 800.0, 1500.0, 0.45 * fs, 0.4999 * fs, 0.5 * fs,
                   0.75 * fs, 1.5 * fs):
            src = {"f0": np.full(n, f0), "vuv": np.ones(n), "temporal_positions": tp.copy()}
            res = d4cRequiem(x, fs, src, fft_size=fft) if req else d4c(x, fs, src)
            dsweep.append(rep.record("d4c", fs=fs, requiem=req, fft=fft, f0=f0, nan=bool(np.any(np.isnan(res["aperiodicity"])))))
    rep.set("d4c_sweep_bad", [s for s in dsweep if s["flags"][_hip.FLAG_OOB]])
    rep.set("d4c_sweep_cases", len(dsweep))
    # ---- the off-regime signals of the fuzz tests through both pipelines (tone bursts between digital silence, noise, a
    # chirp, clicks, DC, a 0.2 s and a 1e-8 utterance, two tones, silence) -----------------------------------------------
    from _harvest_script import fuzz_inputs
    wbf = WorldBatch()
    for fs_f in (16000, 48000):
        _, xf = fuzz_inputs(fs_f)
        enc = wbf.encode(xf, fs_f, f0_method="dio")
        wbf.decode_device(enc, seed=2)
        enc = wbf.encode(xf, fs_f, f0_method="harvest", is_requiem=True)
        wbf.decode_device(enc)
    whole("fuzz", wbf.rt)
    # ---- decode sweep (round 6, second half: response_kernel's two chain buffers, padded response, noise block, ring and row,
    # req_filter_kernel's buffers, run accumulator and row, and the shared minimum-phase chain are checked pointers): frame
    # periods 1 / 5 / 10 ms (Requiem hops of 16 ... 480 samples), pulse rates from a quarter to eight times the contour's
    # (windows further apart than a transform; more pulses than the default capacity: the overflow retry), durations
    # halved and tripled, transforms 1024 ... 4096
    wbd = WorldBatch()
    dec_flags = [0] * 16
    dec_cases = 0
    for fs_d, period in ((16000, 1), (16000, 5), (16000, 10), (48000, 5), (48000, 10), (96000, 5)):
        xd = [synth_utterance(9, fs_d, 0.5), synth_utterance(10, fs_d, 0.3)]
        for req in (False, True):
            for pitch, dur in ((1.0, 1.0), (0.25, 1.0), (8.0, 1.0), (1.0, 0.5), (1.5, 3.0)):
                enc = wbd.encode(xd, fs_d, f0_method="dio", frame_period=period, is_requiem=req)
                if pitch != 1.0:
                    enc.scale_pitch(pitch)
                if dur != 1.0:
                    enc.scale_duration(dur)
                wbd.decode_device(enc, seed=4)  # (check=True: a pulse overflow is retried with the safe capacity)
                dec_flags = [a | b for a, b in zip(dec_flags, wbd.rt.take_flags())]
                dec_cases += 1
    rep.set("decode_sweep_flags", dec_flags)
    rep.set("decode_sweep_record", list(_hip.bounds_last()))
    rep.set("decode_sweep_cases", dec_cases)
    # ---- config 2 at full size: 64 x 10 s through every stage of the DIO path + decode, Harvest + Requiem on 8 ----------
    xs = [synth_utterance(u, 16000, 10.0) for u in range(64)]
    wb = WorldBatch()
    enc = wb.encode(xs, 16000, f0_method="dio", check=False)
    y, _ = wb.decode_device(enc, seed=3, check=False)
    whole("config2", wb.rt)
    enc = wb.encode(xs[:8], 16000, f0_method="harvest", is_requiem=True, check=False)
    y, _ = wb.decode_device(enc, check=False)
    whole("harvest", wb.rt)
    x48 = [synth_utterance(75, 48000, 3.0)]
    enc = wb.encode(x48, 48000, f0_method="harvest", check=False)
    y, _ = wb.decode_device(enc, seed=1, check=False)
    whole("cfg5", wb.rt)
    # ---- the transform probe: one launch each of a handful of shapes (kind, n, nt, snt, maxr, inverse) ------------------
    probe = {}
    for shape in ((2, 128, 64, 64, 8, 0), (0, 2048, 256, 512, 8, 0), (0, 8192, 512, 512, 8, 0), (1, 2048, 256, 256, 8, 0),
                  (2, 1024, 64, 64, 8, 0), (3, 4096, 512, 512, 8, 1)):
        kind, n = shape[0], shape[1]
        d_in, d_out = {0: (2 * n, 2 * n), 1: (2 * n, 2 * n), 2: (n, n + 2), 3: (n + 2, n)}[kind]
        x_d = rt.to_device(np.random.RandomState(n).standard_normal(37 * d_in))
        y_d = rt.empty((37 * d_out,))
        rc = rt.lib.wh_fft_engine_probe(rt.ctx, rt.stream(), *shape, rt.ptr(x_d), rt.ptr(y_d), 37)
        key = "-".join(str(v) for v in shape)
        probe[key] = taken(key, rc, y_d)
    rep.set("fft_probe", probe)
    # ---- the selection probe and the two spectral probes (csrc/wh_d4c_probe.hip, csrc/wh_spectral_probe.hip): one call per shape —
    # exponents over 39 octaves (every selection round) and all values equal (every refinement level, the whole row in the
    # ranked list); the replica with f0 around fs / 2 (every bin a node, the mirror branch of the LDS form) -----------------
    d4c_ft = {512: 256, 1024: 128, 2048: 256, 4096: 512, 8192: 512}
    sel = {}
    for n in sorted(d4c_ft):
        k = n // 2 + 1
        rng = np.random.RandomState(n)
        rows = np.concatenate([np.floor(2.0 ** rng.uniform(0.0, 39.0, (8, k))), np.full((2, k), 3.0)])
        x_d, y_d = rt.to_device(rows.reshape(-1)), rt.empty((2 * len(rows),))
        for layout in (0, 1):
            rc = rt.lib.wh_d4c_select_probe(rt.ctx, rt.stream(), n, layout, k - 22, rt.ptr(x_d), rt.ptr(y_d), len(rows))
            key = "%d-%d" % (n, layout)
            sel[key] = taken(key, rc, y_d)
    rep.set("select_probe", sel)
    spectral = {}
    for form, n, ft, fs in [("lds", 256, 128, 8000), ("lds", 512, 128, 16000), ("lds", 1024, 128, 16000), ("lds", 2048, 256, 48000),
                            ("lds", 4096, 256, 96000)] + [("runs", n, d4c_ft[n], 16000 if n <= 2048 else 12000 * (n // 1024))
                                                          for n in sorted(d4c_ft)]:
        k, df = n // 2 + 1, fs / n
        f0 = np.array([fs / 2 - 0.5 * df, fs / 2 - 0.5 * df, fs / 2 + 0.5 * df, fs / 2 + 0.5 * df, 0.75 * fs, 150.0])
        reach = np.array([f0[0] + df, 1.2 * f0[1], f0[2] + df, 1.2 * f0[3], 1.2 * f0[4], 1.2 * f0[5]])
        x_d = rt.to_device(np.random.RandomState(n).uniform(0.5, 1.5, len(f0) * k))
        f0_d, reach_d, y_d = rt.to_device(f0), rt.to_device(reach), rt.empty((len(f0) * k,))
        for which, rh_d in ((0, reach_d), (1, rt.to_device(f0 / 3))):
            if form == "lds":
                rc = rt.lib.wh_spectral_probe(rt.ctx, rt.stream(), n, ft, which, float(fs), rt.ptr(f0_d), rt.ptr(rh_d), rt.ptr(x_d),
                                              rt.ptr(y_d), len(f0))
            else:
                rc = rt.lib.wh_d4c_runs_probe(rt.ctx, rt.stream(), n, which, float(fs), rt.ptr(f0_d), rt.ptr(rh_d), rt.ptr(x_d),
                                              rt.ptr(y_d), len(f0))
            key = "%s-%d-%d" % (form, n, which)
            spectral[key] = taken(key, rc, y_d)
    rep.set("spectral_probes", spectral)
    rep.emit()


if __name__ == "__main__":
    main()
