"""The profile records of the library's launches, name by name and in launch order.

Every kernel launch goes through one helper (wh::launch, csrc/wh_host.h) that brackets it for the profile under a record
name.  The names are a contract: bench.py keys its per-kernel byte table on them, the tools sum by them.  This test pins
the records of one small pass through the pipeline: a launch that gained or lost a record, or a name that drifted, fails
it.

The literal lists below were recorded by running `collect` against the build of the commit BEFORE the launch helper
replaced the hand-written bracket + launch + check idiom — not against the code under test."""
import pytest

pytestmark = pytest.mark.gpu

FS = 16000

# one window size of SWIPE' (the loudness matrices are feature products); five window sizes at 16 kHz
_SWIPE_WINDOW = ["swipe_stft_kernel", "feature_matmul_kernel", "swipe_normalise_kernel", "feature_matmul_kernel",
                 "swipe_accumulate_kernel"]

EXPECTED = {
    "encode_dio": [
        "iir_fwd_kernel", "iir_bwd_kernel", "lowcut_kernel", "band_events_kernel", "band_concat_kernel", "cand_kernel",
        "sort_kernel", "contour_kernel", "stonemask_tab_kernel", "stonemask_kernel", "cheaptrick_kernel", "d4c_kernel",
    ],
    "encode_harvest": [
        "hv_iir_fwd_kernel", "hv_iir_bwd_kernel", "hv_mean_kernel", "hv_mean_kernel", "hv_pad_kernel",
        "band_taps_fft_kernel", "band_tile_fft_kernel", "band_events_kernel", "hv_raw_kernel", "hv_detect_kernel",
        "hv_refine_kernel", "hv_prune_kernel", "hc_base_kernel", "hc_step1_kernel", "hc_sections_kernel",
        "hc_extend_kernel", "hc_merge_kernel", "hc_smooth_kernel", "hc_pick_kernel", "cheaptrick_kernel", "d4c_kernel",
    ],
    "encode_swipe": 5 * _SWIPE_WINDOW + [
        "swipe_pick_kernel", "cheaptrick_kernel", "d4c_kernel",
    ],
    "decode": [
        "prep_kernel", "phase_kernel", "pulse_mark_kernel", "pulse_scan_kernel", "pulse_emit_kernel",
        "pulse_finish_kernel", "pulse_base_kernel", "pulse_frames_kernel", "pulse_run_base_kernel", "pulse_rows_kernel",
        "response_kernel", "response_gather_kernel", "peak_max_kernel", "peak_scale_kernel",
    ],
    "encode_requiem": [
        "iir_fwd_kernel", "iir_bwd_kernel", "lowcut_kernel", "band_events_kernel", "band_concat_kernel", "cand_kernel",
        "sort_kernel", "contour_kernel", "stonemask_tab_kernel", "stonemask_kernel", "cheaptrick_kernel",
        "love_train_kernel", "d4c_kernel",
    ],
    "requiem_seeds": [
        "velvet_layout_kernel", "velvet_fill_kernel", "seed_pulse_kernel", "seed_noise_kernel", "seed_band0_dc_kernel",
    ],
    "decode_requiem": [
        "prep_kernel", "phase_kernel", "pulse_mark_kernel", "pulse_scan_kernel", "pulse_emit_kernel",
        "pulse_finish_kernel", "req_linap_kernel", "req_pulse_weights_kernel", "req_excite_kernel", "req_filter_kernel",
        "req_gather_kernel", "peak_max_kernel", "peak_scale_kernel",
    ],
    "flags": [],  # (the flag kernels leave no record)
}


def collect(wb):
    """[(step, [record name, ...]), ...] of the pass on the WorldBatch `wb`."""
    from world._synthetic import synth_utterance
    from world.get_seeds_signals import get_seeds_signals_device

    rt = wb.rt
    xs = [synth_utterance(70, FS, 0.3), synth_utterance(71, FS, 0.5)]
    out = []

    def step(name, fn):
        res = fn()
        out.append((name, [n for n, _ in rt.profile_collect()]))
        return res

    rt.profile(True)
    try:
        enc = None
        for method in ("dio", "harvest", "swipe"):
            enc = step("encode_" + method, lambda: wb.encode(xs, FS, f0_method=method))
        step("decode", lambda: wb.decode_device(enc))
        req = step("encode_requiem", lambda: wb.encode(xs, FS, f0_method="dio", is_requiem=True))
        seeds = step("requiem_seeds", lambda: get_seeds_signals_device(FS, seed=3, rt=rt))
        step("decode_requiem", lambda: wb.decode_device(req, seeds=seeds))
        step("flags", lambda: (rt.take_flags(), rt.post_flags()))
    finally:
        rt.profile_collect()
        rt.profile(False)
    return out


def test_profile_records_by_name_and_order():
    from world.batch import WorldBatch

    got = collect(WorldBatch(prefetch_timebase=False))
    assert [s for s, _ in got] == list(EXPECTED)
    for name, records in got:
        assert records == EXPECTED[name], name
