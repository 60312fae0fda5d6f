"""CPU: the census of wh::rfft_frame_lds (csrc/wh_fft.h), the name under which the frame filters of recordings call
rfft_lds.  tests/test_fft_reference_host.py::test_call_site_tripwire lists, file by file, the calls of the shared
transforms by their own names and leaves wh_fft.h out; a call through rfft_frame_lds is therefore not in that list.  This
is its complement: every caller of the helper by file and count, the helper's one inner call, and every (N, threads) pair
its static_assert admits held against the shape lists of csrc/wh_fft_probe.hip and tests/test_hip_fft_engine.py — so that
the two lists together still name every unit that instantiates a shared transform, and no shape can come in unprobed."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-world_amd", "csrc")

CALLERS = {"wh_specfilter.hip": 1}
ADMITTED = ((512, 256), (1024, 256), (2048, 512), (4096, 512))


def _code(path):
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_callers_of_the_frame_transform():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        n = len(re.findall(r"(?<![A-Za-z0-9_])rfft_frame_lds<", _code(path)))
        if n and os.path.basename(path) != "wh_fft.h":
            found[os.path.basename(path)] = n
    assert found == CALLERS, ("the callers of wh::rfft_frame_lds have changed: %r now, %r in this test; a new caller's unit "
                              "belongs in CALLERS here" % (found, CALLERS))


def test_the_helper_admits_probed_shapes_only():
    text = _code(os.path.join(CSRC, "wh_fft.h"))
    body = text[text.index("void rfft_frame_lds("):]
    body = body[:body.index("\n}\n") + 3]
    assert len(re.findall(r"(?<![A-Za-z0-9_])rfft_lds<N, NT>\(", body)) == 1 and "fft_lds_wave" not in body
    pairs = tuple((int(a), int(b)) for a, b in re.findall(r"N == (\d+) && NT == (\d+)", body))
    assert pairs == ADMITTED
    probe = _code(os.path.join(CSRC, "wh_fft_probe.hip"))
    import test_hip_fft_engine as engine  # (its SHAPES are plain data; nothing in it touches the GPU on import)

    for n, nt in ADMITTED:  # kind 2 = rfft_lds<N, NT, SNT = NT, MAXR = 8>, forward
        assert re.search(r"X\(2, %d, %d, %d, 8, 0\)" % (n, nt, nt), probe), (n, nt)
        assert (2, n, nt, nt, 8, 0) in engine.SHAPES, (n, nt)
