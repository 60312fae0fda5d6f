"""Inputs, runner and reference shared by tests/test_hip_melcep_filter.py and tests/_melcep_bounds_script.py, modelled on
tests/_specfilter_cases.py: the case list of wh_melcep_filter at the smallest shapes that reach every edge, the reference
result of every case (tests/_melcep_reference.py, computed once per process and kept read-only) and the C entry called
directly — the rows inside wider tensors whose NaN guard bands must survive, the output between two guard samples.

A case is one CALL: a batch of utterances that share the transform length, the order, alpha and the presence of a
denominator; hop, length, frame count and row map are per utterance."""
import collections
import functools

import numpy as np

import _melcep_reference as mref
import _specfilter_reference as sref

Case = collections.namedtuple("Case", "name n order alpha den hops nys frames map_kind pad seed")

FFT_SIZES = (512, 1024, 2048, 4096)
WINDOWS = (2, 4, 5, 8, 9)  # around the run length of 4
ORDERS = (1, 24, 39, 59, 64)
ALPHAS = (0.0, 0.42, 0.554, -0.3)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """Per N and hop in {1, 80, N / 2} one batch of ten utterances: W in WINDOWS, each at the shortest and the longest
    utterance with that many windows.  Orders, alphas and the denominator go round over the twelve."""
    cases = []
    for i, n in enumerate(FFT_SIZES):
        for j, hop in enumerate((1, 80, n // 2)):
            nys = tuple(ny for w in WINDOWS for ny in ((w - 2) * hop + 1, (w - 1) * hop))
            frames = tuple(sref.n_windows(ny, hop) for ny in nys)
            c = 3 * i + j
            cases.append(Case("N=%d H=%d windows" % (n, hop), n, ORDERS[c % 5], ALPHAS[c % 4], c % 3 != 2, (hop,) * len(nys), nys,
                              frames, "identity", (i + j) % 3, 10 * i + j))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def kind_cases():
    cases = [
        Case("ragged three: one frame, empty", 1024, 24, 0.42, True, (80, 80, 80), (403, 0, 37), (6, 0, 1), "identity", 1, 100),
        Case("ragged three, mixed hops", 1024, 40, 0.42, True, (80, 110, 1), (500, 333, 7), (7, 4, 3), "nearest", 0, 101),
        Case("without den", 1024, 24, 0.42, False, (80, 80), (700, 161), (9, 3), "identity", 2, 102),
        Case("without den N=2048", 2048, 59, 0.554, False, (240,), (1000,), (5,), "identity", 0, 103),
        Case("non-monotone map", 1024, 39, 0.42, True, (80, 80), (900, 250), (5, 4), "shuffled", 1, 104),
        Case("non-monotone map N=512", 512, 24, -0.3, True, (40,), (411,), (6,), "shuffled", 0, 105),
        Case("m=59 N=2048", 2048, 59, 0.554, True, (240, 110), (1200, 500), (6, 5), "identity", 2, 107),
        Case("m=64 N=4096", 4096, 64, 0.554, True, (2048, 480), (4100, 1000), (3, 4), "identity", 1, 109),
        # hops on both sides of 3 H <= N in one call: each utterance keeps the form it has alone
        Case("hops astride the run form N=1024", 1024, 24, 0.42, True, (80, 400, 341, 342), (700, 1500, 1100, 1100), (9, 5, 5, 5),
             "identity", 1, 120),
        Case("hops astride the run form N=512", 512, 39, 0.0, False, (40, 200, 170, 171), (333, 700, 600, 600), (9, 5, 5, 5),
             "identity", 0, 121),
    ]
    for k, m in enumerate(ORDERS):
        for a, alpha in enumerate(ALPHAS):
            cases.append(Case("m=%d alpha=%g" % (m, alpha), 1024, m, alpha, (k + a) % 2 == 0, (80, 80, 110), (500, 0, 1300), (7, 0, 4),
                              "identity", (k + a) % 3, 130 + 4 * k + a))
    return tuple(cases)


def all_cases():
    return geometry_cases() + kind_cases()


def bounds_cases():
    """Six for the bounds build: one per N, one without den, the ragged one."""
    g, k = geometry_cases(), kind_cases()
    picked = (g[1], g[3], g[8], g[9], k[2], k[0])
    assert sorted(c.n for c in picked[:4]) == list(FFT_SIZES) and not picked[4].den and 0 in picked[5].nys
    return picked


@functools.lru_cache(maxsize=None)
def inputs(case):
    """{x: [per utterance], num, den, maps: [per utterance], x_off, frame_off} of a case."""
    rng = np.random.RandomState(9000 + case.seed)
    f = int(sum(case.frames))
    num, den = mref.random_rows(rng, f, case.order), mref.random_rows(rng, f, case.order)
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
    return {"x": tuple(xs), "num": _frozen(num), "den": _frozen(den) if case.den else None, "maps": tuple(maps),
            "x_off": _frozen(np.concatenate([[0], np.cumsum(case.nys)]).astype(np.int64)),
            "frame_off": _frozen(np.concatenate([[0], np.cumsum(case.frames)]).astype(np.int64))}


@functools.lru_cache(maxsize=None)
def reference(case):
    """The reference's y per utterance."""
    inp = inputs(case)
    fo = inp["frame_off"]
    out = []
    for u in range(len(case.nys)):
        den = None if inp["den"] is None else inp["den"][fo[u]:fo[u + 1]]
        out.append(_frozen(mref.filter_melcep(inp["x"][u], inp["num"][fo[u]:fo[u + 1]], den, inp["maps"][u], case.hops[u], case.n,
                                              case.alpha)))
    return tuple(out)


def _wide(rt, a, pad):
    wide = np.full((a.shape[0], a.shape[1] + 2 * pad), np.nan)
    wide[:, pad:pad + a.shape[1]] = a
    return rt.to_device(wide)


def call(rt, n_utt, x_off, frame_off, map_off, h_map, hops, num_d, ldn, den_d, ldd, order, alpha, fft_size, x_d, y_d, tables=(True, True)):
    """The C entry with host arrays made from lists; returns rc.  ``tables``: which of the two warp tables are handed in."""
    from world import _hip
    from world import melcep

    x_off, frame_off, map_off = (np.ascontiguousarray(a, dtype=np.int64) for a in (x_off, frame_off, map_off))
    h_map = np.ascontiguousarray(h_map, dtype=np.int32)
    hops = np.ascontiguousarray(hops, dtype=np.int64)
    k_bins = int(fft_size) // 2 + 1 if fft_size in FFT_SIZES else 513
    cos_b, sin_b = melcep.warp_tables(k_bins, float(alpha))
    return rt.lib.wh_melcep_filter(
        rt.ctx, rt.stream(), n_utt, _hip.i64p(x_off), _hip.i64p(frame_off), _hip.i64p(map_off), _hip.i32p(h_map), _hip.i64p(hops),
        num_d, ldn, den_d, ldd, order, _hip.f64p(cos_b) if tables[0] else None, _hip.f64p(sin_b) if tables[1] else None, fft_size,
        x_d, y_d)


def run(rt, case, only=None, num=None):
    """wh_melcep_filter on a case -> {y: [per utterance], guards, rc}.  ``only``: that utterance alone, as a batch of one
    (its own rows, map and samples).  ``num``: other numerator rows than the case's."""
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
              rt.ptr(num_w[:, pad:]), ld, rt.ptr(den_w[:, pad:]) if den_w is not None else None, ld if den_w is not None else 0,
              case.order, case.alpha, case.n, rt.ptr(x_d), rt.ptr(y_w[1:]))
    host = y_w.cpu().numpy()
    guards = bool(host[0] == -7.0 and host[-1] == -7.0)
    for wide, src in ((num_w, num_h), (den_w, den_h)):
        if wide is not None:
            back = wide.cpu().numpy()
            guards = guards and bool(np.all(np.isnan(back[:, :pad])) and np.all(np.isnan(back[:, pad + cols:])))
            guards = guards and np.array_equal(back[:, pad:pad + cols], src, equal_nan=True)
    y = host[1:-1]
    return {"y": [y[x_off[i]:x_off[i + 1]].copy() for i in range(len(xs))], "guards": guards, "rc": rc}


def compare(got, want):
    """[] when ``got`` is ``want`` within both bounds, else what is wrong."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return ["shape %s against %s" % (got.shape, want.shape)]
    if not np.all(np.isfinite(got)):
        return ["%d samples are not finite" % int(np.sum(~np.isfinite(got)))]
    rms, worst = sref.errors(got, want)
    bad = []
    if not rms <= sref.RMS_BOUND:
        bad.append("relative RMS %.3g over %.3g" % (rms, sref.RMS_BOUND))
    if not worst <= mref.SAMPLE_BOUND:
        bad.append("worst sample %.3g of max|y| over %.3g" % (worst, mref.SAMPLE_BOUND))
    return bad


def compare_case(case, got):
    """([what is wrong], worst relative RMS, worst sample error relative to max|y|) of a run of the whole case."""
    bad, rms, worst = [], 0.0, 0.0
    if got["rc"] != 0:
        return ["rc %d" % got["rc"]], rms, worst
    want = reference(case)
    for u, (g, w) in enumerate(zip(got["y"], want)):
        bad += ["utterance %d: %s" % (u, b) for b in compare(g, w)]
        if np.all(np.isfinite(g)) and g.shape == w.shape:
            e = sref.errors(g, w)
            rms, worst = max(rms, e[0]), max(worst, e[1])
    if not got["guards"]:
        bad.append("a guard band was written")
    return bad, rms, worst
