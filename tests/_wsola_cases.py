"""Inputs, runner and reference shared by tests/test_hip_wsola.py and tests/_wsola_bounds_script.py: the case list of
wh_wsola at the smallest shapes that reach every edge, the reference result of every case (tests/_wsola_reference.py,
computed once per process and kept read-only) and the C entry called directly — the output and the shifts between guard
values that must survive.

A case is one CALL: a hop, a tolerance and a batch of utterances; length, output length, position list and signal are per
utterance.  An utterance is (signal, n, positions, parameter):
    signals     noise; tone (three harmonics of a slowly falling pitch); silence; periodic (integer values, period 5: the
                scores of shifts 5 apart are the same bits); half_silent (noise behind digital silence); nan / inf (noise
                with one such sample in its middle).
    positions   ratio r: n_out = floor(r n + 0.5) and the uniform stretch's list; jitter n_out: ratio 1 moved by up to
                +- D per frame (the winner compensates it, so every lane's candidates win somewhere); shuffled n_out:
                anywhere from 3 H + D in front of the utterance to as far behind it, in no order; far n_out: the same
                with the ends of the int64 range and +- 2^62 among them."""
import collections
import functools

import numpy as np

import _wsola_reference as wref

Case = collections.namedtuple("Case", "name hop tol utts seed")

HOPS = (1, 2, 80, 176, 1024)
# 2 D + 1 candidates on 256 threads: D = 127 | 128, 255 | 256, 383 | 384, 511 | 512 are the last with k and the first with k + 1 per thread
TOLS = (0, 1, 127, 128, 255, 256, 383, 384, 511, 512)
RATIOS = (1.0, 0.8, 1.25, 1.5, 0.5)
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def hop_cases():
    """Every hop at a small and (H <= 176) a larger tolerance, all five ratios in one ragged batch."""
    cases = []
    for i, hop in enumerate(HOPS):
        n = {1: 40, 2: 61, 80: 700, 176: 1500, 1024: 3100}[hop]
        for tol in ((0, 3) if hop <= 2 else (1, 50) if hop <= 176 else (1,)):
            utts = tuple(("tone" if k % 2 else "noise", n + 7 * k, "ratio", r) for k, r in enumerate(RATIOS))
            cases.append(Case("H=%d D=%d ratios" % (hop, tol), hop, tol, utts, 10 * i + tol % 7))
    cases.append(Case("H=1024 D=512", 1024, 512, (("tone", 5000, "ratio", 0.8), ("noise", 3000, "jitter", 2500)), 60))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def tol_cases():
    """Every tolerance around the thread count's multiples, at hop 16: a jittered list, whose winners range over the lanes."""
    return tuple(Case("H=16 D=%d" % tol, 16, tol, (("noise", 2 * tol + 300, "jitter", 2 * tol + 280), ("tone", 400, "ratio", 1.25)),
                      100 + tol) for tol in TOLS)


@functools.lru_cache(maxsize=None)
def edge_cases():
    return (
        Case("empty, one sample, shorter than H", 80, 50, (("noise", 0, "ratio", 1.25), ("noise", 1, "ratio", 1.25), ("noise", 37, "ratio", 1.25),
                                                           ("noise", 79, "ratio", 0.8), ("noise", 500, "ratio", 1.5)), 200),
        Case("empty input, output asked for", 80, 50, (("noise", 0, "shuffled", 200), ("tone", 300, "ratio", 0.8)), 201),
        Case("output of one sample and of none", 80, 20, (("noise", 300, "shuffled", 1), ("noise", 300, "shuffled", 0), ("noise", 1, "ratio", 0.5)), 202),
        Case("non-monotone positions", 80, 50, (("tone", 900, "shuffled", 1000), ("noise", 333, "shuffled", 401)), 203),
        Case("positions out of range", 80, 50, (("noise", 600, "far", 2400), ("tone", 300, "far", 161)), 204),
        Case("positions out of range H=1 D=0", 1, 0, (("noise", 30, "far", 24),), 205),
        Case("digital silence", 80, 50, (("silence", 900, "ratio", 1.25), ("noise", 400, "ratio", 1.25)), 206),
        Case("periodic integers: exact ties", 8, 7, (("periodic", 400, "ratio", 1.25), ("periodic", 300, "jitter", 280), ("periodic", 300, "ratio", 0.8)), 207),
        Case("periodic integers: ties on two waves", 16, 200, (("periodic", 900, "jitter", 700),), 208),
        Case("silence next to signal", 80, 50, (("half_silent", 1200, "ratio", 1.25), ("half_silent", 1200, "ratio", 0.8)), 209),
        Case("ragged eight", 128, 80, tuple(("tone" if k % 3 else "noise", 150 * k + 5, "ratio", RATIOS[k % 5]) for k in range(8)), 210),
    )


def all_cases():
    return hop_cases() + tol_cases() + edge_cases()


def signal(kind, n, rng):
    t = np.arange(n, dtype=np.float64)
    if kind in ("noise", "nan", "inf"):
        x = rng.randn(n)
        if kind != "noise" and n:
            x[n // 2] = np.nan if kind == "nan" else np.inf
        return x
    if kind == "tone":
        phase = 2 * np.pi * np.cumsum(0.021 - 0.006 * t / max(n, 1))
        return np.sin(phase) + 0.5 * np.sin(2 * phase + 1.0) + 0.25 * np.sin(3 * phase + 2.0) + 0.01 * rng.randn(n)
    if kind == "silence":
        return np.zeros(n)
    if kind == "periodic":
        return np.tile(np.array([3.0, -1.0, 2.0, 0.0, -2.0]), n // 5 + 1)[:n]
    if kind == "half_silent":
        x = rng.randn(n)
        x[:n // 2] = 0.0
        return x
    raise ValueError(kind)


def position_list(kind, param, n, hop, tol, rng):
    """(n_out, int64 list)."""
    if kind == "ratio":
        n_out = int(np.floor(param * n + 0.5))
        return n_out, wref.positions(n_out, hop, param)
    n_out = int(param)
    m = wref.n_frames(n_out, hop)
    if kind == "jitter":
        # frame 0 rests, so the chain stays on the input's own time and frame m's winner is minus its jitter: the first
        # and the last candidate win at frames 3 and 5
        jit = rng.randint(-tol, tol + 1, size=m)
        jit[:1] = 0
        jit[3:4], jit[5:6] = tol, -tol
        return n_out, wref.positions(n_out, hop, 1.0) + jit
    reach = 3 * hop + tol
    pos = rng.randint(-reach, n + reach + 1, size=m).astype(np.int64)
    if kind == "far" and m:
        far = [INT64_MIN, INT64_MAX, -2 ** 62, 2 ** 62, INT64_MAX - hop, INT64_MIN + tol, -reach, n + reach, 2 ** 31, -2 ** 31 - 1]
        where = rng.permutation(m)[:len(far)]
        pos[where] = np.array(far[:len(where)], dtype=np.int64)
    return n_out, pos


@functools.lru_cache(maxsize=None)
def inputs(case):
    """{x: [per utterance], n_out: [..], pos: [per utterance]} of a case."""
    rng = np.random.RandomState(9000 + case.seed)
    xs, n_outs, poss = [], [], []
    for kind, n, pkind, param in case.utts:
        xs.append(_frozen(signal(kind, n, rng)))
        n_out, pos = position_list(pkind, param, n, case.hop, case.tol, rng)
        n_outs.append(n_out)
        poss.append(_frozen(np.ascontiguousarray(pos, dtype=np.int64)))
    return {"x": tuple(xs), "n_out": tuple(n_outs), "pos": tuple(poss)}


@functools.lru_cache(maxsize=None)
def reference(case):
    """The reference's (y, delta) per utterance."""
    inp = inputs(case)
    out = []
    for x, n_out, pos in zip(inp["x"], inp["n_out"], inp["pos"]):
        y, d = wref.wsola(x, n_out, [int(p) for p in pos], case.hop, case.tol)
        out.append((_frozen(y), _frozen(d)))
    return tuple(out)


def call(rt, n_utt, x_off, y_off, pos_off, pos, hop, tol, x_d, y_d, delta_d, win=True):
    """The C entry with host arrays made from lists (pointers pass as they are); returns rc."""
    from world import _hip

    x_off, y_off, pos_off, pos = (None if a is None else np.ascontiguousarray(a, dtype=np.int64) for a in (x_off, y_off, pos_off, pos))
    w = np.ascontiguousarray(wref.window(hop if 1 <= hop <= wref.MAX_HOP else 1)) if win else None
    return rt.lib.wh_wsola(rt.ctx, rt.stream(), n_utt, *(None if a is None else _hip.i64p(a) for a in (x_off, y_off, pos_off, pos)), hop, tol,
                           None if w is None else _hip.f64p(w), x_d, y_d, delta_d)


Y_GUARD, D_GUARD = -7.0, -77777


def run(rt, case, only=None, xs=None, want_delta=True):
    """wh_wsola on a case -> {y: [per utterance], delta: [per utterance] or None, guards, rc}.  ``only``: that utterance
    alone, as a batch of one.  ``xs``: other signals than the case's.  ``want_delta`` False: delta == NULL."""
    inp = inputs(case)
    utts = list(range(len(case.utts))) if only is None else [only]
    xs = [(inp["x"] if xs is None else xs)[u] for u in utts]
    poss = [inp["pos"][u] for u in utts]
    x_off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    y_off = np.concatenate([[0], np.cumsum([inp["n_out"][u] for u in utts])]).astype(np.int64)
    pos_off = np.concatenate([[0], np.cumsum([len(p) for p in poss])]).astype(np.int64)
    torch = rt.torch
    x_d = rt.to_device(np.concatenate(xs) if xs else np.zeros(0))
    y_w = torch.full((int(y_off[-1]) + 2,), Y_GUARD, dtype=torch.float64, device=rt.device)
    d_w = torch.full((int(pos_off[-1]) + 2,), D_GUARD, dtype=torch.int32, device=rt.device)
    rc = call(rt, len(xs), x_off, y_off, pos_off, np.concatenate(poss) if poss else np.zeros(0), case.hop, case.tol, rt.ptr(x_d),
              rt.ptr(y_w[1:]), rt.ptr(d_w[1:]) if want_delta else None)
    y_h, d_h = y_w.cpu().numpy(), d_w.cpu().numpy()
    guards = bool(y_h[0] == Y_GUARD and y_h[-1] == Y_GUARD and d_h[0] == D_GUARD and d_h[-1] == D_GUARD)
    if not want_delta:
        guards = guards and bool(np.all(d_h == D_GUARD))
    guards = guards and np.array_equal(x_d.cpu().numpy(), np.concatenate(xs) if xs else np.zeros(0), equal_nan=True)
    y, d = y_h[1:-1], d_h[1:-1]
    return {"y": [y[y_off[i]:y_off[i + 1]].copy() for i in range(len(xs))],
            "delta": [d[pos_off[i]:pos_off[i + 1]].copy() for i in range(len(xs))] if want_delta else None, "guards": guards, "rc": rc}


def same_bits(a, b):
    """Bit for bit, but any NaN equals any NaN (its sign and payload are no part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def compare_case(case, got):
    """[what is wrong] of a run of the whole case."""
    if got["rc"] != 0:
        return ["rc %d" % got["rc"]]
    bad = []
    for u, ((wy, wd), gy) in enumerate(zip(reference(case), got["y"])):
        if got["delta"] is not None and got["delta"][u].tobytes() != wd.tobytes():
            diff = np.flatnonzero(got["delta"][u] != wd) if got["delta"][u].shape == wd.shape else []
            bad.append("utterance %d: %d shifts differ, the first at frame %s" % (u, len(diff), diff[:1]))
        if not same_bits(gy, wy):
            bad.append("utterance %d: y differs in %s samples" % (u, np.count_nonzero(gy != wy) if gy.shape == wy.shape else "the count of"))
    if not got["guards"]:
        bad.append("a guard value was written or the input changed")
    return bad
