"""Per-stage cycle counts inside response_kernel (build with WH_EXTRA_FLAGS=-DWH_RESP_STAGE_TIMER)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))
import torch
from world._synthetic import synth_utterance
from world.batch import WorldBatch

# tools/resp_stage_timer.py [fs] [utterances] [seconds] [pitch scale] [duration scale]   (config 5: 48000 16 60 1.5 2.0)
fs = int(sys.argv[1]) if len(sys.argv) > 1 else 16000
n_utt = int(sys.argv[2]) if len(sys.argv) > 2 else 64
secs = float(sys.argv[3]) if len(sys.argv) > 3 else 10.0
wb = WorldBatch(0)
xs = [synth_utterance(i, fs, secs) for i in range(n_utt)]
batch, x_d, tp_d = wb.upload(xs, fs)
enc = wb.encode_device(batch, x_d, tp_d, fs, f0_method="dio" if fs <= 16000 else "harvest")
if len(sys.argv) > 4:
    enc.scale_pitch(float(sys.argv[4]))
if len(sys.argv) > 5:
    enc.scale_duration(float(sys.argv[5]))
lib = wb.rt.lib
buf = (ctypes.c_ulonglong * 16)()
for it in range(3):
    y, _ = wb.decode_device(enc, seed=it)
    torch.cuda.synchronize()
    lib.wh_debug_resp_stages(buf, 1)
v = np.array(list(buf), dtype=np.float64)
# slot 5: from the pulse's start to the logs; slot 0: from there to the chains (with the wave roles of the 16 kHz shape the
# noise run and its mean are no longer here: the run is generated under the chains' first transform, and the mean
# is taken in front of the convolution, slot 3).  The chains' stage by the kind of pulse: slot 2 voiced (two chains side by
# side), slot 6 unvoiced (one chain), slot 7 two unvoiced pulses side by side (the 16 kHz shape).
# The slots are RespStage of csrc/wh_resp_types.h.
names = {5: "setup: pulse look-up, spectral rows, interpolation, logs", 0: "setup: noise run + mean in front of the chains",
         2: "minimum-phase chains, voiced pulses", 6: "minimum-phase chains, unvoiced pulses one by one",
         7: "minimum-phase chains, unvoiced pulses in pairs", 3: "response reorder + noise convolution",
         4: "DC sum + overlap-add into the run's ring"}
tot = v[:8].sum()
for i in (5, 0, 2, 6, 7, 3, 4):
    print("%-60s %6.1f %%  %.3e cycles" % (names[i], 100 * v[i] / tot, v[i]))
print("total cycles (sum over pulses) %.3e" % tot)
n_voiced, n_unv0, n_unv_rows, n_partner, n_pairs, n_all = (int(x) for x in v[8:14])
print("pulses %d: voiced %d, unvoiced with vuv == 0 %d, unvoiced by the aperiodicity rows only %d" % (n_all, n_voiced, n_unv0, n_unv_rows))
if n_pairs:
    print("pairs taken %d (%d of the %d vuv == 0 pulses)" % (n_pairs, 2 * n_pairs, n_unv0))
else:
    # (the shapes without pairs: resp_pairs<N>() is false) a pulse has a partner when its successor in the run has vuv == 0 too, the noise is the device
    # stream's and both runs fit nz together; pairs are disjoint, so a stretch of n such pulses in a row makes about n / 2
    per_pulse = v[6] / max(1, n_unv0 + n_unv_rows)
    print("vuv == 0 pulses whose successor in the run can share the chains with them: %d" % n_partner)
    print("unvoiced chain stage per pulse %.0f cycles; (pairable / 2) x that = %.3e cycles = %.1f %% of the total"
          % (per_pulse, n_partner / 2 * per_pulse, 100 * n_partner / 2 * per_pulse / tot))
