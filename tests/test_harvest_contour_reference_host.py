"""CPU: the stage-by-stage restatement of Harvest's pruning and contour stages (tests/_harvest_contour_reference.py) and
the crafted candidate maps of the GPU test (tests/_harvest_contour_cases.py), pinned without a GPU:
  * against oracle.pitch_harvest (prune_isolated, fix_contour, smooth_f0) on every case and on the refined map of a
    synthetic utterance, bit for bit;
  * against the UNMODIFIED reference's RemoveUnreliableCandidates, FixF0Contour and SmoothF0, recorded in
    tests/golden/golden_harvest_contour.npz (tests/golden/make_harvest_contour_golden.py), and — where the reference
    checkout is present — against a fresh run of it;
  * the conditions on the maps, with the reference side alone: every branch counter is hit, every case hits the branch it
    is named for, and the two order-dependent decisions (2200 / mean against the length, the merge's score sums) have the
    margins that make a bit-exact comparison with the kernels fair.

Branch counts (tests/_harvest_contour_reference.py names them), the crafted set (34 maps, 7 480 frames) against the
waveforms the suite runs Harvest on (synth_utterance 41 / 11 / 42 and tests/_harvest_script.py's inputs, inputs_22k and
fuzz_inputs but for the one the oracle cannot process: 23 610 frames, at most 32 candidates in a frame):

                                   crafted  waveforms |                                  crafted  waveforms
  prune_killed                         425       5321 | pick_multi                            15       7888
  prune_killed_word0 / 1         135 / 129 4747 / 574 | pick_tie                               9          0
  prune_killed_word2 / 3          129 / 32      0 / 0 | pick_row_ge64                       2893          0
  prune_kept                          7756     347087 | pick_at_limit                          2          0
  prune_kept_by_prev_only             1727      19689 | sec_total                            271        120
  prune_kept_by_next_only             1762      20666 | sec_not_kept                           7          1
  base_row_ge64                        540          0 | no_section_kept                        1          1
  base_max_twice                        11          0 | merge_disjoint                       180         31
  step1_drop                          1647       5940 | merge_covered                         14         15
  step2_removed                         11       1196 | merge_partial_first                    1         41
  fwd_stop_miss / limit           224 / 47    48 / 72 | merge_partial_second                   2         17
  bwd_stop_miss / limit           207 / 64    43 / 77 | merge_partial_equal                   39          2
  fwd_miss_at_step_mod4_0..3  1/13/3/207   11/9/6/22 | merge_partial_after_disjoint           1         14
  bwd_miss_at_step_mod4_0..3   197/2/6/2  12/10/8/13 | merge_score_row_ge64                4585          0
  fwd_clamped / bwd_clamped        61 / 67    14 / 18 | tied_starts                           14         21
  ext_three_miss_then_hit                3         35 | step4_bridged / left             49 / 30   102 / 26

(test_every_branch_is_taken_by_the_crafted_set prints the crafted column.)  What the waveforms never reach is everything
beyond list entry 31 — mask words 1 to 3 of a long list, the second candidate of a lane, a winner in rows 64 and up —,
a tie between different values, and an error exactly at the allowed range."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import _harvest_contour_cases as HC
import _harvest_contour_reference as HR
from conftest import GOLDEN
from oracle import pitch_harvest, refshim

FIXTURE = os.path.join(GOLDEN, "golden_harvest_contour.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_runs = {}


def run_of(name):
    if name not in _runs:
        c = HC.get(name)
        _runs[name] = (c, HR.run(c.cands, c.scores))
    return _runs[name]


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("name", HC.names())
def test_restatement_is_the_oracle_and_the_recorded_reference(recorded, name):
    c, r = run_of(name)
    oc, osc = pitch_harvest.prune_isolated(c.cands, c.scores)
    assert np.array_equal(_bits(oc), _bits(r.pruned_c)) and np.array_equal(_bits(osc), _bits(r.pruned_s))
    of0, ovuv = pitch_harvest.fix_contour(oc, osc)
    assert np.array_equal(_bits(of0), _bits(r.s4)) and np.array_equal(ovuv, r.vuv)
    assert np.max(np.abs(pitch_harvest.smooth_f0(of0) - r.smoothed)) <= HC.SMOOTH_BOUND
    # the unmodified reference's results
    rows, frames = recorded[name + ".rows"].astype(np.int64), recorded[name + ".frames"].astype(np.int64)
    pc, ps = np.zeros_like(c.cands), np.zeros_like(c.scores)
    pc[rows, frames] = recorded[name + ".f0"]
    ps[rows, frames] = recorded[name + ".score"]
    assert np.array_equal(_bits(pc), _bits(r.pruned_c)) and np.array_equal(_bits(ps), _bits(r.pruned_s))
    if name in HC.TIED and not bool(recorded[name + ".binding"]):
        return  # (the reference's unstable sort took another order where the fixture was made: DESIGN.md)
    assert np.array_equal(_bits(recorded[name + ".contour"]), _bits(r.s4))
    assert np.array_equal(np.unpackbits(recorded[name + ".vuv_bits"])[: c.cands.shape[1]], r.vuv.astype(np.uint8))
    assert np.max(np.abs(recorded[name + ".smoothed"] - r.smoothed)) <= HC.SMOOTH_BOUND


def test_tied_cases_bind_where_the_fixture_was_made(recorded):
    """Both cases with tied extended starts came out in the stable order on the authoring machine, so the fixture binds
    them; a regenerated fixture that says otherwise must be noticed (DESIGN.md gets a line then)."""
    assert all(bool(recorded[name + ".binding"]) for name in HC.TIED)
    assert all(run_of(name)[1].count["tied_starts"] >= 2 for name in HC.TIED)


def test_smoothing_rows_against_the_recorded_reference(recorded):
    for name, row in HC.smooth_rows().items():
        sm = HR.smooth(row)
        assert np.max(np.abs(recorded["smooth." + name] - sm)) <= HC.SMOOTH_BOUND, name
        assert np.max(np.abs(pitch_harvest.smooth_f0(row) - sm)) <= HC.SMOOTH_BOUND, name
        assert np.array_equal(sm == 0, row == 0)


def test_restatement_is_the_oracle_on_a_real_refined_map():
    from world._synthetic import synth_utterance

    aux = pitch_harvest.harvest_np(synth_utterance(11, 16000, 0.35), 16000, return_aux=True)["aux"]
    r = HR.run(aux["refined_f0"], aux["refined_score"])
    assert np.array_equal(_bits(r.pruned_c), _bits(aux["pruned_f0"]))
    assert np.array_equal(_bits(r.pruned_s), _bits(aux["pruned_score"]))
    assert np.array_equal(_bits(r.s4), _bits(aux["f0_1ms"]))
    assert np.max(np.abs(r.smoothed - aux["smoothed_1ms"])) <= HC.SMOOTH_BOUND
    assert r.count["sec_total"] >= 1 and r.count["prune_killed"] >= 1


COUNTERS = ("prune_killed", "prune_kept", "prune_killed_word0", "prune_killed_word1", "prune_killed_word2",
            "prune_killed_word3", "prune_kept_by_prev_only", "prune_kept_by_next_only", "base_row_ge64", "base_max_twice",
            "step1_drop", "step2_removed", "fwd_stop_miss", "fwd_stop_limit", "bwd_stop_miss", "bwd_stop_limit",
            "fwd_miss_at_step_mod4_0", "fwd_miss_at_step_mod4_1", "fwd_miss_at_step_mod4_2", "fwd_miss_at_step_mod4_3",
            "bwd_miss_at_step_mod4_0", "bwd_miss_at_step_mod4_1", "bwd_miss_at_step_mod4_2", "bwd_miss_at_step_mod4_3",
            "fwd_clamped", "bwd_clamped", "ext_three_miss_then_hit", "pick_multi", "pick_tie", "pick_row_ge64",
            "pick_at_limit", "sec_total", "sec_not_kept", "no_section_kept", "merge_disjoint", "merge_covered",
            "merge_partial_first", "merge_partial_second", "merge_partial_equal", "merge_partial_after_disjoint",
            "merge_score_row_ge64", "tied_starts", "step4_bridged", "step4_left", "smooth_runs")


def test_every_branch_is_taken_by_the_crafted_set():
    total = collections.Counter()
    for name in HC.names():
        total.update(run_of(name)[1].count)
    print(dict(sorted(total.items())))
    assert not [k for k in COUNTERS if total[k] == 0]
    assert set(total) <= set(COUNTERS), set(total) - set(COUNTERS)


@pytest.mark.parametrize("name", HC.names())
def test_every_case_takes_the_branch_it_is_named_for(name):
    c, r = run_of(name)
    assert not [h for h in c.hits if r.count[h] == 0]
    assert set(c.hits) <= set(COUNTERS)


def test_wide_lists_are_wide():
    """33, 64, 65, 96 and 105 candidates next to one-candidate frames, two of them in one wave of the pruning kernel (frames
    2 k - 1 and 2 k share one); more than 32 survive the pruning in some frame, and in some frame both neighbours do."""
    c, r = run_of("wide_lists")
    n = np.count_nonzero(c.cands, axis=0)
    assert {33, 64, 65, 96, 105} <= set(n.tolist())
    assert any(n[j] >= 96 and n[j + 1] == 1 and j % 2 == 1 for j in range(len(n) - 1))
    assert any(n[j] == 1 and n[j + 1] >= 96 and j % 2 == 1 for j in range(len(n) - 1))
    assert np.count_nonzero(r.pruned_c, axis=0).max() > 64
    c, r = run_of("pick_ties")
    assert np.count_nonzero(r.pruned_c, axis=0).max() == 105


def test_pick_ties_are_ties_between_different_values():
    """|100 - 90| / 100 and |100 - 110| / 100 are the same double, and so are 0.18 and |100 - 118| / 100, |100 - 82| / 100;
    the neighbouring doubles of 118 and 82 lie outside.  In every tie the later row's value is the one the contour takes."""
    assert abs(100.0 - 90.0) / 100.0 == abs(100.0 - 110.0) / 100.0
    assert abs(100.0 - 118.0) / 100.0 == 0.18 == abs(100.0 - 82.0) / 100.0
    assert abs(100.0 - np.nextafter(118.0, np.inf)) / 100.0 > 0.18 < abs(100.0 - np.nextafter(82.0, -np.inf)) / 100.0
    c, r = run_of("pick_ties")
    assert r.count["pick_tie"] == len(HC.TIE_ROWS)
    for q, (r90, r110) in enumerate(HC.TIE_ROWS):
        assert r.s4[20 + 60 * q + 31] == (110.0 if r110 > r90 else 90.0)
    c, r = run_of("pick_at_the_allowed_range")
    assert [r.s4[a + 31] for a in (20, 90, 160, 230)] == [118.0, 0.0, 82.0, 0.0]


def test_sections_of_the_named_cases():
    """what the section cases are named for, read off the restatement's section table"""
    assert [s[:2] for s in run_of("runs_6_7")[1].sections] == [(31, 37)]
    assert run_of("runs_6_7")[1].count["step2_removed"] == 1
    a = run_of("seams_a")[1].sections
    assert [s[:2] for s in a] == [(50, 63), (100, 255), (257, 280)]
    assert [s[:2] for s in run_of("seams_b")[1].sections][:2] == [(64, 80), (120, 256)]
    assert run_of("run_longer_than_256")[1].sections[0][1] - run_of("run_longer_than_256")[1].sections[0][0] > 256
    r = run_of("none_kept")[1]
    assert len(r.sections) == 3 and not any(s[4] for s in r.sections) and np.array_equal(r.s3, r.s2)
    r = run_of("one_kept_among_unkept")[1]
    assert [s[4] for s in r.sections] == [0, 0, 1, 0, 0, 1] and np.count_nonzero(r.s3) < np.count_nonzero(r.s2)
    r = run_of("densest_sections")[1]
    assert len(r.sections) == 149 and all(s[1] - s[0] == 6 and s[4] for s in r.sections)  # (frames 0 and 1 cost the first)
    assert all(b[0] - a[1] == 2 for a, b in zip(r.sections, r.sections[1:]))  # one unvoiced frame between the runs
    r = run_of("touches_ends")[1]
    assert r.sections[0][2] == 0 and r.sections[-1][3] == 39  # the walks reach the first and the last frame
    r = run_of("extension_to_the_limit")[1]
    assert r.sections == [(201, 212, 100, 313, 1)]  # (the walk from frame i fills frame i +- 1: 101 beyond the run)
    r = run_of("extension_to_the_clamps")[1]
    assert r.sections == [(41, 50, 0, 89, 1)]
    r = run_of("gaps_8_9_1")[1]
    gaps = [int(b[2] - a[3] - 1) for a, b in zip(r.sections, r.sections[1:])]
    assert gaps == [8, 9, 1] and r.count["step4_bridged"] == 2 and r.count["step4_left"] == 1
    assert np.all(r.s4[31:39] != 0) and np.all(r.s4[61:70] == 0) and r.s4[91] != 0
    r = run_of("tied_extended_starts")[1]
    assert r.sections[0][2] == r.sections[1][2] and r.sections[0][4] and r.sections[1][4]


def test_margins_that_make_an_exact_comparison_fair():
    """2200 / mean is more than 1e-9 (relative) away from the length it is compared with, for every section of every case
    (the kernel's wave sum and np.mean add in different orders); every score is a multiple of 0.5 and at least 2.5 (the
    merge's sums are exact in any order), and one partial merge has equal scores."""
    for name in HC.names():
        c, r = run_of(name)
        sc = c.scores[c.cands != 0]
        assert np.all(sc >= 2.5) and np.all(sc * 2 == np.round(sc * 2)) and np.all(c.scores[c.cands == 0] == 0)
        assert np.all(c.cands >= 0)
        for s, mean in zip(r.sections, r.means):
            length = s[3] - s[2]
            assert abs(2200 / mean - length) > 1e-9 * max(length, 1), (name, s)
    assert run_of("merge_partial_equal_scores")[1].count["merge_partial_equal"] == 1


def test_shortest_contours():
    """One frame: the reference (and the restatement, and the oracle) cannot index frame 1.  Two and three frames go through;
    two frames are unvoiced whatever they hold."""
    one = np.full((HC.ROWS, 1), 0.0)
    one[0, 0] = 400.0
    with pytest.raises(IndexError):
        HR.fix_contour(one, one)
    with pytest.raises(IndexError):
        pitch_harvest.fix_contour(one, one)
    assert not run_of("shape_2")[1].vuv.any() and not run_of("shape_2")[1].smoothed.any()
    assert len(run_of("shape_3")[1].s4) == 3


@pytest.mark.parametrize("name", ["wide_lists", "pick_ties", "shape_3", "extension_stops"])
def test_packers_round_trip(name):
    c, r = run_of(name)
    maps = {}
    for form in ("dense", "compact"):
        f0, sc, lst, pos = HC.pack(c.cands, c.scores, form)
        assert len(f0) == len(sc) == int(lst[-1] >> 8) + int(lst[-1] & 255)
        assert np.all((lst & 255) <= HC.ROWS)
        maps[form] = HC.unpack(f0, sc, lst, pos)
        assert np.array_equal(_bits(maps[form][0]), _bits(c.cands)) and np.array_equal(_bits(maps[form][1]), _bits(c.scores))
        alive = r.pruned_c != 0
        assert np.array_equal(HC.unmask(HC.masks(alive, pos), pos), alive)
    f0, sc, lst, pos = HC.pack(c.cands, c.scores, "dense")
    assert np.all((lst & 255) == HC.ROWS) and len(f0) == HC.ROWS * c.cands.shape[1]
    f0, sc, lst, pos = HC.pack(c.cands, c.scores, "compact")
    assert np.all(f0 != 0) and np.array_equal(lst & 255, np.count_nonzero(c.cands, axis=0))


def test_smoothing_tolerance_is_the_cpu_rounding_noise():
    """SMOOTH_NOISE bounds the difference between SmoothF0 in float64 and the same recurrence in np.longdouble over every
    case and every smoothing row; the bound the GPU test uses is 16 x that plus the hold's truncation, far below 1e-6 Hz."""
    worst, top = 0.0, 0.0
    rows = [run_of(name)[1].s4 for name in HC.names()] + list(HC.smooth_rows().values())
    for row in rows:
        worst = max(worst, float(np.max(np.abs(HR.smooth(row, dtype=np.longdouble) - HR.smooth(row)))))
        top = max(top, float(row.max()))
    print("smoothing noise %.3e Hz, bound %.3e Hz" % (worst, HC.SMOOTH_BOUND))
    assert 0 < worst <= HC.SMOOTH_NOISE and top <= 800.0
    assert np.abs(np.roots(HR.SMOOTH_A)).max() ** 300 <= HC.SMOOTH_POLE_300
    assert HC.SMOOTH_BOUND < 1e-9


def test_recorded_reference_is_reproduced_where_the_reference_is_present(tmp_path):
    """In the authoring container the fixture is generated again from the unmodified reference and compared; anywhere
    else there is nothing to run and the committed fixture (above) is the pin."""
    if not os.path.isdir(os.path.join(refshim.REFERENCE_ROOT, "world")):
        return
    out = str(tmp_path / "hc.npz")
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_harvest_contour_golden.py"), out], check=True,
                   stdout=subprocess.DEVNULL, timeout=300)
    fresh = dict(np.load(out))
    rec = dict(np.load(FIXTURE))
    assert set(fresh) == set(rec)
    for k in rec:
        assert fresh[k].dtype == rec[k].dtype and np.array_equal(fresh[k].view(np.uint8) if fresh[k].ndim else fresh[k],
                                                                 rec[k].view(np.uint8) if rec[k].ndim else rec[k]), k
