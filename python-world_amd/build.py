"""Build libworld_hip.so (gfx950) in-tree: hipcc per translation unit, then one shared link.

    python python-world_amd/build.py [--force]

No cmake/ninja: the library is a handful of .hip files.  Output: python-world_amd/lib/libworld_hip.so
(git-ignored, travels to the GPU box with the source snapshot).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
OBJ_DIR = os.path.join(HERE, "build")
LIB = os.path.join(OUT_DIR, "libworld_hip.so")
ARCH = "gfx950"
# -ffp-contract=off: the reference is NumPy float64 without FMA contraction; keeping mul/add
# separate keeps the discrete F0 decisions on the same side of their thresholds.
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]
# Per translation unit, appended after FLAGS (the last -ffp-contract wins; "fast-honor-pragmas", HIP's own default: plain
# "fast" lets the backend fuse across a `#pragma clang fp contract(off)`).  The SPECTRAL kernels may fuse a*b+c into one
# FP64 instruction: their outputs are compared with the reference at tolerances (1e-9 ... 1e-7).
#   * wh_cheaptrick.hip and wh_d4c.hip fuse as whole units; the two places of wh_d4c.hip where a discrete outcome is read
#     keep `#pragma clang fp contract(off)`: the output interpolation that must not exceed 0 dB, and the love-train powers,
#     sums and ratio of the voicing gate s1/s2 > 0.85 (d4c.py:86; the transform in front of the gate is fused — its rounding
#     differs from NumPy's pocketfft at the 1e-16 level with or without contraction, so a frame whose ratio lies within
#     ~1e-15 of the threshold can fall on either side either way).  Worth 1.1 % of the config-2 step (round 5: d4c
#     4.64 -> 4.56 ms, cheaptrick 1.14 -> 1.11, responses 3.45 -> 3.43).
#   * wh_apbands.hip (the expansion of stored band aperiodicity: wh_apbands.h, the interpolation it shares with d4c_kernel,
#     pins its own contraction) and wh_d4c_probe.hip (the test hooks of wh_d4c_select.h / wh_d4c_runs.h) were parts of
#     wh_d4c.hip and keep its flags: the code they hold is compiled as it was there.
#   * wh_synthesis.hip and wh_requiem.hip are built unfused (Philox, the Requiem excitation and the gathers round like the
#     reference) and fuse by `#pragma clang fp contract(fast)` inside min_phase_response (wh_minphase.h), response_pulse,
#     response_pair and noise_conv_groups only (wh_resp_pulse.h, wh_resp_pair.h).
#   * wh_specfilter.hip (the spectral filter of recordings: the Requiem filter's chain on another geometry) is built like
#     wh_requiem.hip: unfused — the products of its LSF gain are the contract's, rounded one by one — but for
#     min_phase_response's own pragma (and, for mel-cepstral rows, exponent_response's and the recurrence's in front of it).
#   * wh_wsola.hip (waveform-similarity overlap-add) has no entry below and no pragma: its scores are sums of products
#     rounded one by one, compared bit for bit with tests/_wsola_reference.py.
#   * wh_psola.hip (pitch-synchronous overlap-add) likewise: the scores and the window's cubic are rounded operation by
#     operation, compared bit for bit with tests/_psola_reference.py.
#   * wh_peak.hip and wh_philox_probe.hip were parts of wh_synthesis.hip, which has no entry below (it contracts by
#     pragma): they need none either.
# The F0 stages (DIO, StoneMask, Harvest — wh_harvest.hip, wh_hv_front.hip, wh_hv_refine.hip, wh_hv_contour.hip —, SWIPE') and the synthesis TIME BASE (wh_timebase.hip: no pragma anywhere in it)
# stay unfused: voicing decisions and pulse positions are bit-exact against the reference.  wh_hv_probe.hip (a test hook:
# Harvest's back end on caller-supplied candidate maps) has no entry below either: it is built like wh_hv_contour.hip.
TU_FLAGS = {
    "wh_d4c.hip": ["-ffp-contract=fast-honor-pragmas"],
    "wh_apbands.hip": ["-ffp-contract=fast-honor-pragmas"],
    "wh_d4c_probe.hip": ["-ffp-contract=fast-honor-pragmas"],  # (a test hook: the D4C headers as wh_d4c.hip compiles them)
    "wh_reduce_probe.hip": ["-ffp-contract=fast-honor-pragmas"],  # (a test hook: wh_reduce.h as wh_d4c.hip compiles it)
    "wh_cheaptrick.hip": ["-ffp-contract=fast-honor-pragmas"],
    "wh_fft_probe.hip": ["-ffp-contract=fast-honor-pragmas"],  # (a test hook: the transforms as most of their callers compile them)
    "wh_spectral_probe.hip": ["-ffp-contract=fast-honor-pragmas"],  # (a test hook: wh_spectral.h as wh_cheaptrick.hip compiles it)
}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _newer(src_list, target):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


def build(force=False, verbose=True):
    extra = os.environ.get("WH_EXTRA_FLAGS", "").split()  # tuning experiments, e.g. -DWH_FRAME_THREADS=64
    os.makedirs(OUT_DIR, exist_ok=True)
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    units = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "world_hip.h"))
    headers.append(os.path.abspath(__file__))  # (the flags live here)
    jobs = []
    objs = []
    for u in units:
        src = os.path.join(CSRC, u)
        obj = os.path.join(OBJ_DIR, u[:-4] + ".o")
        objs.append(obj)
        if force or _newer([src] + headers, obj):
            jobs.append((u, [hipcc] + FLAGS + TU_FLAGS.get(u, []) + extra + ["-c", src, "-o", obj]))

    def run(job):
        name, cmd = job
        r = subprocess.run(cmd, capture_output=True, text=True)
        return name, r.returncode, r.stdout + r.stderr

    if jobs:
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            for name, rc, log in ex.map(run, jobs):
                if verbose and log.strip():
                    print(log)
                if rc != 0:
                    raise RuntimeError("hipcc failed on %s\n%s" % (name, log))
                if verbose:
                    print("compiled", name)
    if force or jobs or _newer(objs, LIB):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed\n" + r.stdout + r.stderr)
        if verbose:
            print("linked", LIB)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
