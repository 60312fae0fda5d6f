"""Inputs, runner and reference shared by tests/test_hip_specfilter.py and tests/_specfilter_bounds_script.py: the case
list of wh_spectral_filter at the smallest shapes that reach every edge, the reference result of every case
(tests/_specfilter_reference.py, computed once per process and kept read-only) and the C entry called directly — the gain
rows inside wider tensors whose NaN guard bands must survive, the output between two guard samples.

A case is one CALL: a batch of utterances that share the transform length, the kind and the presence of a denominator;
hop, length, frame count and row map are per utterance."""
import collections
import functools

import numpy as np

import _specfilter_reference as sref

Case = collections.namedtuple("Case", "name n kind den p hops nys frames map_kind pad seed")

FFT_SIZES = (512, 1024, 2048, 4096)
WINDOWS = (2, 4, 5, 8, 9)  # around the run length of 4 (one window cannot occur: W = ceil(ny / H) + 1 >= 2 for ny >= 1)
ORDERS = (2, 24, 40, 64)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """Per N and hop in {1, 80, N / 2 (the largest with 2 H - 1 <= N)} one batch of ten utterances: W in WINDOWS, each at the
    shortest and the longest utterance with that many windows, (W - 2) H + 1 and (W - 1) H samples.  Up to N = 1024 the
    hops 1 and 80 take the run form (four windows per row), everything else one row per window."""
    cases = []
    for i, n in enumerate(FFT_SIZES):
        for j, hop in enumerate((1, 80, n // 2)):
            nys = tuple(ny for w in WINDOWS for ny in ((w - 2) * hop + 1, (w - 1) * hop))
            frames = tuple(sref.n_windows(ny, hop) for ny in nys)
            cases.append(Case("N=%d H=%d windows" % (n, hop), n, "spectrum", True, 0, (hop,) * len(nys), nys, frames,
                              "identity", (i + j) % 3, 10 * i + j))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def kind_cases():
    cases = [
        Case("ragged three: one frame, empty", 1024, "spectrum", True, 0, (80, 80, 80), (403, 0, 37), (6, 0, 1), "identity", 1, 100),
        Case("ragged three, mixed hops", 1024, "spectrum", True, 0, (80, 110, 1), (500, 333, 7), (7, 4, 3), "nearest", 0, 101),
        Case("spectrum without den", 1024, "spectrum", False, 0, (80, 80), (700, 161), (9, 3), "identity", 2, 102),
        Case("spectrum without den N=2048", 2048, "spectrum", False, 0, (240,), (1000,), (5,), "identity", 0, 103),
        Case("non-monotone map", 1024, "spectrum", True, 0, (80, 80), (900, 250), (5, 4), "shuffled", 1, 104),
        Case("non-monotone map lsf", 512, "lsf", True, 24, (40,), (411,), (6,), "shuffled", 0, 105),
        Case("lsf p=40 without den", 1024, "lsf", False, 40, (80, 80), (640, 81), (9, 2), "identity", 1, 106),
        Case("lsf p=40 N=2048", 2048, "lsf", True, 40, (240, 110), (1200, 500), (6, 5), "identity", 2, 107),
        Case("lsf p=24 N=4096 without den", 4096, "lsf", False, 24, (480,), (1500,), (4,), "identity", 0, 108),
        Case("lsf p=64 N=4096", 4096, "lsf", True, 64, (2048, 480), (4100, 1000), (3, 4), "identity", 1, 109),
        # hops on both sides of 3 H <= N in one call: each utterance keeps the form it has alone (run form / one row per window)
        Case("hops astride the run form N=1024", 1024, "spectrum", True, 0, (80, 400, 341, 342), (700, 1500, 1100, 1100), (9, 5, 5, 5),
             "identity", 1, 120),
        Case("hops astride the run form N=512 lsf", 512, "lsf", True, 24, (40, 200, 170, 171), (333, 700, 600, 600), (9, 5, 5, 5),
             "identity", 0, 121),
    ]
    for k, p in enumerate(ORDERS):
        cases.append(Case("lsf p=%d" % p, 1024, "lsf", True, p, (80, 80, 110), (500, 0, 1300), (7, 0, 4), "identity", k % 3, 110 + k))
    return tuple(cases)


def all_cases():
    return geometry_cases() + kind_cases()


def lsf_rows(frames, p, rng):
    """[frames][p + 1] = [log E, cos w_1 .. cos w_p]: ascending angles, evenly spread and moved by up to 0.35 of the spacing."""
    even = np.pi * (np.arange(p) + 1.0) / (p + 1)
    w = even[None, :] + rng.uniform(-0.35, 0.35, size=(frames, p)) * np.pi / (p + 1)
    return np.concatenate([rng.randn(frames, 1), np.cos(w)], axis=1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """{x: [per utterance], num, den, maps: [per utterance], x_off, frame_off} of a case."""
    rng = np.random.RandomState(7000 + case.seed)
    k_bins = case.n // 2 + 1
    f = int(sum(case.frames))
    if case.kind == "lsf":
        num, den = lsf_rows(f, case.p, rng), lsf_rows(f, case.p, rng)
    else:
        # a smooth log-envelope of +- 20 dB plus 1 dB of ripple per bin
        def rows():
            c = rng.randn(f, 6) * np.array([2.0, 1.5, 1.0, 0.7, 0.5, 0.3])[None, :]
            smooth = c @ np.cos(np.arange(6)[:, None] * np.linspace(0, np.pi, k_bins)[None, :])
            return np.exp(smooth + 0.1 * rng.randn(f, k_bins))
        num, den = rows(), rows()
    xs, maps = [], []
    for hop, ny, nf in zip(case.hops, case.nys, case.frames):
        xs.append(_frozen(rng.randn(ny)))
        n_win = sref.n_windows(ny, hop)
        if case.map_kind == "identity":
            m = np.minimum(np.arange(n_win), max(nf - 1, 0))
        elif case.map_kind == "nearest":
            m = sref.window_map(ny, nf, hop, 16000.0, 5.0)
        else:
            m = rng.randint(0, nf, size=n_win)
        maps.append(_frozen(m.astype(np.int32)))
    out = {"x": tuple(xs), "num": _frozen(num), "den": _frozen(den) if case.den else None, "maps": tuple(maps),
           "x_off": _frozen(np.concatenate([[0], np.cumsum(case.nys)]).astype(np.int64)),
           "frame_off": _frozen(np.concatenate([[0], np.cumsum(case.frames)]).astype(np.int64))}
    return out


def reference_utterance(case, u):
    inp = inputs(case)
    fo = inp["frame_off"]
    num = inp["num"][fo[u]:fo[u + 1]]
    den = None if inp["den"] is None else inp["den"][fo[u]:fo[u + 1]]
    if case.kind == "lsf":
        return sref.filter_lsf(inp["x"][u], num, den, inp["maps"][u], case.hops[u], case.n)
    return sref.filter_spectrum(inp["x"][u], num, den, inp["maps"][u], case.hops[u], case.n)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The reference's y per utterance."""
    return tuple(_frozen(reference_utterance(case, u)) for u in range(len(case.nys)))


def _wide(rt, a, pad):
    wide = np.full((a.shape[0], a.shape[1] + 2 * pad), np.nan)
    wide[:, pad:pad + a.shape[1]] = a
    return rt.to_device(wide)


def call(rt, n_utt, x_off, frame_off, map_off, h_map, hops, kind, num_d, ldn, den_d, ldd, width, fft_size, x_d, y_d, cos=True):
    """The C entry with host arrays made from lists; returns rc."""
    from world import _hip
    from world.lsf import bin_table

    x_off, frame_off, map_off = (np.ascontiguousarray(a, dtype=np.int64) for a in (x_off, frame_off, map_off))
    h_map = np.ascontiguousarray(h_map, dtype=np.int32)
    hops = np.ascontiguousarray(hops, dtype=np.int64)
    ctab = bin_table(int(fft_size) // 2 + 1) if cos and kind == 1 and fft_size in FFT_SIZES else None
    return rt.lib.wh_spectral_filter(
        rt.ctx, rt.stream(), n_utt, _hip.i64p(x_off), _hip.i64p(frame_off), _hip.i64p(map_off), _hip.i32p(h_map),
        _hip.i64p(hops), kind, num_d, ldn, den_d, ldd, width, _hip.f64p(ctab) if ctab is not None else None, fft_size, x_d, y_d)


def run(rt, case, only=None, num=None):
    """wh_spectral_filter on a case -> {y: [per utterance], guards, rc}.  ``only``: that utterance alone, as a batch of
    one (its own rows, map and samples).  ``num``: other numerator rows than the case's."""
    inp = inputs(case)
    utts = range(len(case.nys)) if only is None else [only]
    fo = inp["frame_off"]
    pick = np.concatenate([np.arange(fo[u], fo[u + 1]) for u in utts]).astype(np.int64) if len(utts) else np.zeros(0, np.int64)
    num_h = (inp["num"] if num is None else num)[pick]
    den_h = None if inp["den"] is None else inp["den"][pick]
    pad = case.pad
    cols = num_h.shape[1]
    num_w = _wide(rt, num_h, pad)
    den_w = None if den_h is None else _wide(rt, den_h, pad)
    xs = [inp["x"][u] for u in utts]
    x_off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    frame_off = np.concatenate([[0], np.cumsum([case.frames[u] for u in utts])]).astype(np.int64)
    maps = [inp["maps"][u] for u in utts]
    map_off = np.concatenate([[0], np.cumsum([len(m) for m in maps])]).astype(np.int64)
    total = int(x_off[-1])
    x_d = rt.to_device(np.concatenate(xs) if xs else np.zeros(0))
    y_w = rt.torch.full((total + 2,), -7.0, dtype=rt.torch.float64, device=rt.device)
    ld = cols + 2 * pad
    rc = call(rt, len(xs), x_off, frame_off, map_off, np.concatenate(maps) if maps else np.zeros(0), [case.hops[u] for u in utts],
              1 if case.kind == "lsf" else 0, rt.ptr(num_w[:, pad:]), ld, rt.ptr(den_w[:, pad:]) if den_w is not None else None,
              ld if den_w is not None else 0, case.p if case.kind == "lsf" else cols, case.n, rt.ptr(x_d), rt.ptr(y_w[1:]))
    host = y_w.cpu().numpy()
    guards = bool(host[0] == -7.0 and host[-1] == -7.0)
    for wide, src in ((num_w, num_h), (den_w, den_h)):
        if wide is not None:
            back = wide.cpu().numpy()
            guards = guards and bool(np.all(np.isnan(back[:, :pad])) and np.all(np.isnan(back[:, pad + cols:])))
            guards = guards and np.array_equal(back[:, pad:pad + cols], src, equal_nan=True)
    y = host[1:-1]
    return {"y": [y[x_off[i]:x_off[i + 1]].copy() for i in range(len(xs))], "guards": guards, "rc": rc}


def compare_case(case, got):
    """([what is wrong], worst relative RMS, worst sample error relative to max|y|) of a run of the whole case."""
    bad, rms, worst = [], 0.0, 0.0
    if got["rc"] != 0:
        return ["rc %d" % got["rc"]], rms, worst
    want = reference(case)
    for u, (g, w) in enumerate(zip(got["y"], want)):
        bad += ["utterance %d: %s" % (u, b) for b in sref.compare(g, w)]
        if np.all(np.isfinite(g)) and g.shape == w.shape:
            e = sref.errors(g, w)
            rms, worst = max(rms, e[0]), max(worst, e[1])
    if not got["guards"]:
        bad.append("a guard band was written")
    return bad, rms, worst
