"""The test variants of libworld_hip.so in one table, and both halves of the harness that runs a
case script against one.  A variant recompiles some translation units with other flags and links the rest from the
shipped build's objects (tools/build_variants.py); world/_hip.py loads it when WH_LIB names it.

The parent's half: path / stale / ensure build what is missing, run_script starts tests/<script> in a fresh child process
and returns the report it prints, report_fixture wraps the two in a module fixture.  The child's half: importing this
module makes the repository root, python-world_amd and tests importable, and Report collects per-case records and prints
them.  No pytest and no GPU at import: __graft_entry__.build() imports this module to build every variant."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "python-world_amd")
for p in (HERE, PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHIPPED = os.path.join(PKG, "lib", "libworld_hip.so")
MARKER = "VARIANT_JSON "


def _checked(*tus):
    # wh_bounds_build() and the record readers live in wh_api: a bounds variant without it reports bounds_build == False
    return {tu: ["-DWH_BOUNDS=1"] for tu in ("wh_api",) + tus}


# variant name -> {translation unit: [flags]}
VARIANTS = {
    "bounds": _checked("wh_cheaptrick", "wh_stonemask", "wh_harvest", "wh_hv_front", "wh_hv_refine", "wh_hv_contour",
                       "wh_timebase", "wh_synthesis", "wh_peak", "wh_requiem", "wh_d4c", "wh_apbands", "wh_d4c_probe",
                       "wh_fft_probe", "wh_spectral_probe"),
    "resample_bounds": _checked("wh_resample"),
    "manifold_bounds": _checked("wh_manifold"),
    "regrid_bounds": _checked("wh_regrid"),
    "dtw_bounds": _checked("wh_dtw"),
    "mlpg_bounds": _checked("wh_mlpg"),
    "gmm_bounds": _checked("wh_gmm"),
    "lsf_bounds": _checked("wh_lsf"),
    "lsf_chain_bounds": _checked("wh_lsf_chain"),
    "specfilter_bounds": _checked("wh_specfilter"),
    "wsola_bounds": _checked("wh_wsola"),
    "exemplar_bounds": _checked("wh_exemplar"),
    "psola_bounds": _checked("wh_psola"),
    # wh_fft_probe.hip compiled as wh_api.hip is, without contraction (tests/test_hip_fft_engine.py, d)
    "nocontract": {"wh_fft_probe": ["-ffp-contract=off"]},
}


def path(name):
    assert name in VARIANTS, name
    return os.path.join(PKG, "lib", "variants", "libworld_hip_%s.so" % name)


def stale(name):
    return not os.path.exists(path(name)) or os.path.getmtime(path(name)) < os.path.getmtime(SHIPPED)


def spec(name):
    """What tools/build_variants.py takes: name=tu:flag,flag;tu:flag"""
    return name + "=" + ";".join("%s:%s" % (tu, ",".join(flags)) for tu, flags in VARIANTS[name].items())


def ensure(*names):
    """Build the stale ones among names (none given: among all) in one run of tools/build_variants.py.  A child process:
    the tool does `import build`, not a name to have in a test process's sys.modules."""
    todo = [n for n in (names or VARIANTS) if stale(n)]
    if not todo:
        return
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variants.py")] + [spec(n) for n in todo],
                       capture_output=True, text=True, timeout=1500)
    done = r.stdout.splitlines()
    assert r.returncode == 0 and all(n + " ok" in done for n in todo), r.stdout[-2000:] + r.stderr[-2000:]


def run_script(script, variant=None, timeout=600):
    """tests/<script> in a fresh child process whose WH_LIB is the variant (None: unset, the shipped library); the report
    it printed."""
    env = dict(os.environ)
    env.pop("WH_LIB", None)
    if variant is not None:
        env["WH_LIB"] = path(variant)
    r = subprocess.run([sys.executable, os.path.join(HERE, script)], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(MARKER)][-1]
    return json.loads(line[len(MARKER):])


def report_fixture(variant, script, shipped=False, timeout=600):
    """A module fixture: the script's report under the variant; with shipped, the pair (that, its report under the shipped
    library)."""
    import pytest

    @pytest.fixture(scope="module")
    def report():
        ensure(variant)
        checked = run_script(script, variant, timeout)
        return (checked, run_script(script, None, timeout)) if shipped else checked

    return report


def digest(arrays):
    """sha256 of the arrays' bytes: what the dual-run tests compare between a variant and the shipped library."""
    import hashlib

    import numpy as np

    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


class Report:
    """The child's report: {"bounds_build", "cases": [...]} and whatever set() adds, printed by emit() as one line."""

    def __init__(self, rt):
        from world import _hip

        self.rt, self._hip = rt, _hip
        self.out = {"bounds_build": _hip.bounds_build(), "cases": []}

    def record(self, name, rt=None, **fields):
        """{"name", "flags", "record", **fields}: reads and clears the flags of rt (default: the report's) and the
        out-of-range record."""
        flags = (rt or self.rt).take_flags()
        return dict(name=name, flags=flags, record=list(self._hip.bounds_last()), **fields)

    def case(self, name, rt=None, **fields):
        """Close a case: append its record to "cases", and return it."""
        self.out["cases"].append(self.record(name, rt, **fields))
        return self.out["cases"][-1]

    def set(self, key, value):
        self.out[key] = value

    def emit(self):
        print(MARKER + json.dumps(self.out))
