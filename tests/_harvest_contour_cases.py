"""Crafted candidate maps for Harvest's pruning and contour stages, and the packers that turn a dense [105][nf1] map into
the pools and per-frame lists hv_refine_kernel leaves (wh_hv_contour.hip: lst[frame] = (first slot << 8) | count).

Built deterministically, without a waveform: every case is named for the branch of world/harvest.py:215-559 it is meant
to take, and tests/test_harvest_contour_reference_host.py checks with tests/_harvest_contour_reference.py's counters
that it does.  How the maps are put together:

  * a TRACK is one candidate per frame at a constant frequency.  SearchF0Base takes it (it has the frame's best score),
    FixStep1 drops its first frame (nothing to continue from), so a track of L frames leaves a run of L - 1;
  * a ZIGZAG alternates between +2 % and -1 % of a frequency: every frame survives the 5 % pruning, is within the 18 % of
    the extension, and is dropped by FixStep1 (it continues neither the previous value nor the linear prediction to
    0.8 %) — candidates that only ExtendF0 ever uses;
  * FILLERS are low-score candidates at 600 Hz and up, all different and far from every track: they make lists long, and
    they die in the pruning unless the neighbouring frame holds them too.

Scores are multiples of 0.5 from 2.5 up (MergeF0's score sums are then exact in any order)."""
import collections

import numpy as np

ROWS = 105


class Map:
    def __init__(self, n):
        self.n = n
        self.c = np.zeros((ROWS, n))
        self.s = np.zeros((ROWS, n))

    def put(self, row, j, f, sc):
        assert 0 <= row < ROWS and 0 <= j < self.n and self.c[row, j] == 0, (row, j)
        assert sc >= 2.5 and sc * 2 == int(sc * 2)
        self.c[row, j] = f
        self.s[row, j] = sc

    def _row(self, row, j):
        if callable(row):
            return row(j)
        if self.c[row, j] == 0:
            return row
        return next(k for k in range(row, ROWS) if self.c[k, j] == 0)

    def track(self, a, b, f, row=0, sc=5.0, skip=()):
        """frames a .. b inclusive"""
        for j in range(a, b + 1):
            if j not in skip:
                self.put(self._row(row, j), j, f, sc)

    def zigzag(self, a, b, f, row=1, sc=2.5, skip=()):
        for j in range(a, b + 1):
            if j not in skip:
                self.put(self._row(row, j), j, f * (1.02 if j % 2 else 0.99), sc)

    def fill(self, j, count, f0=600.0, sc=2.5):
        """fillers in the free rows of frame j until it holds `count` candidates, spread over the whole column"""
        have = int(np.count_nonzero(self.c[:, j]))
        free = [k for k in range(ROWS) if self.c[k, j] == 0]
        need = count - have
        assert 0 <= need <= len(free), (j, count, have)
        pick = [free[(i * len(free)) // need] for i in range(need)] if need else []
        for k in pick:
            self.put(k, j, f0 + 1.75 * k, sc)


Case = collections.namedtuple("Case", "name cands scores hits")
_CASES = collections.OrderedDict()


def case(*hits):
    def deco(fn):
        _CASES[fn.__name__] = (fn, hits)
        return fn
    return deco


# ---- sections ---------------------------------------------------------------------------------------------------------
@case("step2_removed", "sec_total")
def runs_6_7():
    m = Map(64)
    m.track(5, 11, 400.0)    # 7 frames -> a run of 6 (last - first = 5): removed
    m.track(30, 37, 400.0)   # 8 frames -> a run of 7: kept (2200 / 400 = 5.5 < 6)
    return m


@case("sec_total", "fwd_clamped", "bwd_clamped")
def touches_ends():
    m = Map(40)
    m.track(0, 12, 410.0)
    m.track(27, 39, 380.0)
    return m


@case("merge_disjoint")
def seams_a():
    m = Map(300)
    m.track(49, 63, 420.0)    # run 50 .. 63
    m.track(99, 255, 400.0)   # run 100 .. 255
    m.track(256, 280, 520.0)  # run 257 .. 280 (the walk back from it takes frame 256 again)
    return m


@case("merge_disjoint")
def seams_b():
    m = Map(300)
    m.track(63, 80, 420.0)    # run 64 .. 80
    m.track(119, 256, 400.0)  # run 120 .. 256
    m.track(270, 290, 520.0)
    return m


@case("sec_total")
def run_longer_than_256():
    m = Map(400)
    m.track(9, 330, 233.0)
    return m


@case("no_section_kept", "sec_not_kept")
def none_kept():
    m = Map(120)
    for a in (10, 50, 90):
        m.track(a, a + 7, 101.0 + a)  # 7-frame runs near 100 Hz: 2200 / f0 > 6
    return m


@case("sec_not_kept", "merge_disjoint")
def one_kept_among_unkept():
    m = Map(200)
    m.track(10, 17, 111.0)
    m.track(40, 47, 123.0)
    m.track(80, 87, 400.0)   # the one that is kept
    m.track(120, 127, 97.0)
    m.track(150, 158, 131.0)
    m.track(170, 177, 390.0)
    return m


def _dense(n, f_a, f_b):
    m = Map(n)
    for k, a in enumerate(range(0, n - 8, 8)):
        m.track(a, a + 7, f_a if k % 2 == 0 else f_b, row=(7 * k) % ROWS, sc=2.5 + 0.5 * (k % 7))
    return m


@case("merge_disjoint")
def densest_sections():
    """7-frame runs one frame apart, too far apart in frequency to extend into each other"""
    return _dense(1203, 400.0, 500.0)


@case("tied_starts", "merge_partial_equal", "merge_covered")
def densest_sections_overlapping():
    """the same layout 10 % apart: every section extends 100 frames through its neighbours, the first dozen all to frame 1"""
    return _dense(420, 400.0, 440.0)


# ---- extension --------------------------------------------------------------------------------------------------------
@case("fwd_stop_miss", "bwd_stop_miss", "fwd_miss_at_step_mod4_0", "fwd_miss_at_step_mod4_1", "fwd_miss_at_step_mod4_2",
      "fwd_miss_at_step_mod4_3", "bwd_miss_at_step_mod4_0", "bwd_miss_at_step_mod4_1", "bwd_miss_at_step_mod4_2",
      "bwd_miss_at_step_mod4_3")
def extension_stops():
    m = Map(8 * 60 + 20)
    for q in range(4):
        a = 30 + 120 * q
        m.track(a, a + 9, 400.0 + 7 * q, sc=4.0)
        m.zigzag(a + 10, a + 10 + q, 400.0 + 7 * q)         # q + 1 hits, then the four misses ...
        m.zigzag(a + 15 + q, a + 16 + q, 400.0 + 7 * q)     # ... and candidates behind them that must not be taken
        a += 60
        m.track(a, a + 9, 300.0 + 7 * q, sc=4.5)
        m.zigzag(a - 1 - q, a - 1, 300.0 + 7 * q)
        m.zigzag(a - 7 - q, a - 6 - q, 300.0 + 7 * q)
    return m


@case("ext_three_miss_then_hit")
def three_misses_then_a_hit():
    m = Map(160)
    m.track(60, 72, 350.0)
    m.zigzag(73, 110, 350.0, skip=(75, 76, 77, 90, 91, 92, 100, 101, 102, 103))
    m.zigzag(30, 59, 350.0, skip=(55, 54, 53, 40, 39, 38, 37))
    return m


@case("fwd_stop_limit", "bwd_stop_limit")
def extension_to_the_limit():
    m = Map(420)
    m.track(200, 212, 180.0)
    m.zigzag(60, 199, 180.0, skip=(150, 151))
    m.zigzag(213, 400, 180.0, skip=(260,))
    return m


@case("fwd_clamped", "bwd_clamped", "fwd_stop_limit", "bwd_stop_limit")
def extension_to_the_clamps():
    m = Map(90)
    m.track(40, 50, 260.0)
    m.zigzag(0, 39, 260.0)
    m.zigzag(51, 89, 260.0)
    return m


# ---- picks ------------------------------------------------------------------------------------------------------------
TIE_ROWS = ((10, 70), (70, 10), (10, 20), (20, 10), (70, 80), (10, 74), (74, 10), (37, 101), (63, 64))


@case("pick_tie", "pick_multi", "pick_row_ge64")
def pick_ties():
    """reference 100 Hz with 90 and 110 (both 0.1 away, exactly) in (row of 90, row of 110): the later row wins.  Every
    other row of the two frames holds a filler, so that a candidate's list position is its row in both list forms."""
    m = Map(60 * len(TIE_ROWS) + 20)
    for q, (r90, r110) in enumerate(TIE_ROWS):
        a = 20 + 60 * q
        m.track(a, a + 30, 100.0, row=3)
        j = a + 31
        m.put(r90, j, 90.0, 2.5)
        m.put(r110, j, 110.0, 3.0)
        m.put(r90, j + 1, 91.0, 2.5)   # (what keeps the two alive in the pruning)
        m.put(r110, j + 1, 111.0, 3.0)
        m.fill(j, ROWS)
        m.fill(j + 1, ROWS)
    return m


@case("pick_at_limit")
def pick_at_the_allowed_range():
    """0.18 exactly is accepted (118 and 82 from 100), the next double above it is not"""
    m = Map(300)
    up = np.nextafter(118.0, np.inf)
    dn = np.nextafter(82.0, -np.inf)
    for a, f in ((20, 118.0), (90, up), (160, 82.0), (230, dn)):
        m.track(a, a + 30, 100.0)
        m.put(5, a + 31, f, 2.5)
        m.put(5, a + 32, f, 2.5)
        m.put(6, a + 32, 100.0, 3.0)  # (step 1 drops what would otherwise become a second run)
    return m


# ---- merge ------------------------------------------------------------------------------------------------------------
def _overlap(m, a, f1, f2, sc1, sc2, sc_mid1, sc_mid2, row1=0, row2=1):
    """two sections whose extensions overlap in a zone holding both lines of candidates: section 1 (f1) ends at a + 29, the
    zone is a + 30 .. a + 45, section 2 (f2, within 18 % of f1 so that each walk could take the other's line — it takes
    the nearer) starts at a + 46"""
    m.track(a, a + 29, f1, row=row1, sc=sc1)
    m.track(a + 46, a + 80, f2, row=row2, sc=sc2)
    m.zigzag(a + 30, a + 41, f1, row=row1, sc=sc_mid1)   # section 1 reaches a + 41
    m.zigzag(a + 36, a + 45, f2, row=row2, sc=sc_mid2)   # section 2 reaches back to a + 36


@case("merge_partial_first", "merge_partial_after_disjoint", "merge_disjoint")
def merge_partial_first_wins():
    m = Map(300)
    m.track(5, 20, 600.0)  # a disjoint merge first: the running range moves on
    _overlap(m, 60, 200.0, 300.0, 5.0, 5.0, 4.0, 3.0)
    return m


@case("merge_partial_second")
def merge_partial_second_wins():
    m = Map(200)
    _overlap(m, 20, 200.0, 300.0, 5.0, 5.0, 3.0, 4.0)
    return m


@case("merge_partial_equal")
def merge_partial_equal_scores():
    m = Map(200)
    _overlap(m, 20, 200.0, 300.0, 5.0, 5.0, 3.5, 3.5)
    return m


@case("merge_covered")
def merge_covered():
    m = Map(260)
    m.track(100, 130, 200.0, row=0, sc=6.0)
    m.zigzag(20, 99, 200.0, row=0)
    m.zigzag(131, 220, 200.0, row=0)
    m.track(150, 160, 320.0, row=2, sc=7.0)   # a section inside the first one's extended range
    return m


@case("tied_starts")
def tied_extended_starts():
    """two kept sections walk back along the same candidates to the same first frame"""
    m = Map(260)
    m.zigzag(10, 39, 210.0, row=0)
    m.track(40, 60, 210.0, row=0, sc=5.0)
    m.zigzag(61, 69, 210.0, row=0)
    m.track(70, 95, 210.0, row=0, sc=5.5)
    return m


# ---- step 4 -----------------------------------------------------------------------------------------------------------
@case("step4_bridged", "step4_left")
def gaps_8_9_1():
    m = Map(160)
    # (the walk back from a section takes its track's first frame, which step 1 dropped: the gaps are between tracks)
    m.track(9, 30, 400.0)
    m.track(39, 60, 520.0)    # a gap of 8: frames 31 .. 38
    m.track(70, 90, 400.0)    # a gap of 9
    m.track(92, 110, 520.0)   # a gap of 1
    return m


# ---- wide lists -------------------------------------------------------------------------------------------------------
WIDE = ((17, 105), (22, 33), (27, 64), (34, 96), (41, 65), (48, 105), (49, 105), (52, 105), (53, 96), (56, 33), (57, 105),
        (63, 96), (64, 65), (71, 64))


@case("prune_killed_word0", "prune_killed_word1", "prune_killed_word2", "prune_killed_word3", "base_row_ge64",
      "base_max_twice", "prune_kept_by_prev_only", "prune_kept_by_next_only", "pick_row_ge64", "merge_score_row_ge64")
def wide_lists():
    """frames of 33, 64, 65, 96 and 105 candidates between one-candidate frames; the track and the candidates of the
    extension sit in rows 64 and up in some of them and in rows 0 .. 31 in others"""
    m = Map(150)
    high = {17: 104, 27: 64, 41: 90, 48: 70, 49: 100, 52: 88, 53: 99, 63: 77, 71: 96}
    high_b = {52: 101, 53: 3, 56: 103, 57: 66}

    def row_a(j):
        return high.get(j, 2 + j % 30)

    def row_b(j):
        return high_b.get(j, 1)

    # section 1 (150 Hz) walks forward to frame 55, section 2 (230 Hz) back to frame 50: a partial overlap whose scores
    # are looked up in wide frames
    m.track(14, 43, 150.0, row=row_a, sc=6.0)
    m.zigzag(44, 55, 150.0, row=row_a, sc=3.0)
    m.zigzag(50, 59, 230.0, row=row_b, sc=3.5)
    m.track(60, 94, 230.0, row=row_a, sc=6.0)
    # the best score held twice: the first copy is the track's
    m.put(40, 30, 333.0, 6.0)     # another 32-entry word
    m.put(row_a(31) + 1, 31, 334.0, 6.0)  # the same word
    m.put(41, 31, 334.0, 2.5)
    m.put(41, 29, 333.0, 2.5)     # (what keeps them alive in the pruning)
    m.put(41, 32, 334.0, 2.5)
    for j, cnt in WIDE:
        m.fill(j, cnt)
    # fillers that survive: the neighbouring frame holds them too
    m.fill(100, 105)
    m.fill(101, 80)
    m.fill(102, 33)
    return m


# ---- shapes -----------------------------------------------------------------------------------------------------------
SHAPES = (2, 3, 4, 7, 8, 15, 16, 17, 33, 255, 256, 257)


def _shape(n):
    m = Map(n)
    if n >= 12:
        m.track(0, min(n - 1, 11), 400.0, sc=4.0)
    if n >= 30:
        m.track(n - 12, n - 1, 300.0, sc=3.5)
        m.zigzag(12, n - 13, 300.0, skip=tuple(range(20, n - 13, 7)))
    if n < 12:
        m.track(0, n - 1, 400.0)
        m.track(0, n - 1, 405.0, row=50, sc=3.0)
    return m


for _n in SHAPES:
    _CASES["shape_%d" % _n] = ((lambda n=_n: _shape(n)), ())

TIED = ("densest_sections_overlapping", "tied_extended_starts")


def names():
    return list(_CASES)


def get(name):
    fn, hits = _CASES[name]
    m = fn()
    return Case(name, m.c, m.s, hits)


def cases():
    return [get(n) for n in _CASES]


# ---- smoothing alone (mode 2 of the probe): step-4 contours FixF0Contour itself cannot leave ---------------------------
def smooth_rows():
    """name -> a step-4 row handed straight to SmoothF0"""
    out = collections.OrderedDict()
    n = 2600
    r = np.zeros(n)
    r[0::10] = 200.0 + 0.37 * np.arange(len(r[0::10]))   # 260 single-frame runs nine frames apart (a run in frame 0)
    out["single_frames_9_apart"] = r
    # 230 single frames and 27 runs of two different values (what a run left unsmoothed would show: a held single
    # frame passes the filter unchanged), nine frames apart: 257 runs, the last of them in the second tile of the run loop
    r = np.zeros(2597)
    r[0:2300:10] = 800.0 - 0.5 * np.arange(230)
    r[2300::11] = 300.0 + np.arange(27)
    r[2301::11] = 360.0 - np.arange(27)
    out["singles_and_pairs_9_apart"] = r
    out["one_run_over_everything"] = 240.0 + 30.0 * np.sin(np.arange(700) / 23.0)
    r = np.zeros(64)
    r[10:30] = np.linspace(100.0, 130.0, 20)
    r[31] = 555.0
    out["two_runs"] = r
    out["one_frame"] = np.array([321.0])
    return out


# The smoothed row is the one output with arithmetic in another order (hc_smooth_kernel holds a run's ends for 300 samples,
# the reference filters the whole padded contour).  Its tolerance comes from the CPU alone: SMOOTH_NOISE is the largest
# difference, over every case and row of this file, between SmoothF0 in float64 and the same recurrence in np.longdouble
# (measured 7.96e-12 Hz, at the 800 Hz row; tests/test_harvest_contour_reference_host.py measures it again), and the
# hold's truncation is |pole|^300 x the largest f0 = 4.32e-18 x 800 Hz.  1.3e-10 Hz in all: four orders below the
# 1e-6 Hz of the end-to-end tests.
SMOOTH_NOISE = 8.0e-12
SMOOTH_POLE_300 = 4.32e-18
SMOOTH_BOUND = 16 * SMOOTH_NOISE + SMOOTH_POLE_300 * 800.0


# ---- packers ----------------------------------------------------------------------------------------------------------
def pack(cands, scores, form):
    """dense map -> (pool_f0, pool_sc, lst, pos): lst[j] = (first slot << 8) | count; pos[j] = the rows listed, in order.
    form 'dense': every frame lists all 105 rows, zeros included; 'compact': only the non-zero rows, in row order."""
    assert form in ("dense", "compact")
    n = cands.shape[1]
    f0, sc, lst, pos = [], [], np.zeros(n, dtype=np.int64), []
    slot = 0
    for j in range(n):
        rows = np.arange(cands.shape[0]) if form == "dense" else np.flatnonzero(cands[:, j])
        f0.append(cands[rows, j])
        sc.append(scores[rows, j])
        lst[j] = (slot << 8) | len(rows)
        slot += len(rows)
        pos.append(rows)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
    return cat(f0), cat(sc), lst, pos


def unpack(pool_f0, pool_sc, lst, pos, rows=ROWS):
    c = np.zeros((rows, len(lst)))
    s = np.zeros((rows, len(lst)))
    for j, ent in enumerate(lst):
        slot, cnt = int(ent) >> 8, int(ent) & 255
        c[pos[j], j] = pool_f0[slot : slot + cnt]
        s[pos[j], j] = pool_sc[slot : slot + cnt]
    return c, s


def masks(alive, pos):
    """(rows, frames) boolean map -> the frames' 128-bit keep masks, [frames][4] uint32, bit k = list entry k"""
    out = np.zeros((alive.shape[1], 4), dtype=np.uint32)
    for j, rows in enumerate(pos):
        for k, row in enumerate(rows):
            if alive[row, j]:
                out[j, k >> 5] |= np.uint32(1 << (k & 31))
    return out


def unmask(words, pos, rows=ROWS):
    alive = np.zeros((rows, len(pos)), dtype=bool)
    for j, rr in enumerate(pos):
        for k, row in enumerate(rr):
            alive[row, j] = bool((int(words[j, k >> 5]) >> (k & 31)) & 1)
    return alive
