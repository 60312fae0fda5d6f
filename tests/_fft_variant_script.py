"""Helper of tests/test_hip_fft_engine.py (test d).  wh_fft_probe lives in wh_api.hip, which is compiled without
floating-point contraction; wh_fft_engine_probe lives in wh_fft_probe.hip, compiled like the spectral kernels, where the
compiler fuses a radix-8 butterfly's h * (x + y) into the additions behind it.  "The same plan, layout and twiddles: the same
bits" (wh_fft.h) can only be observed between the two hooks in a build that compiles both alike: the NOCONTRACT variant,
libworld_hip.so with wh_fft_probe.hip at -ffp-contract=off (tests/_variants.py, nocontract; never shipped).  With WH_LIB =
that variant it runs both hooks on the same 37 transforms of 512 points."""
import _variants as V


def main():
    import numpy as np

    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    cases = {}
    for nt, gt, snt in ((128, 128, 256), (64, 64, 64)):
        for inverse in (0, 1):
            x = np.random.RandomState(5 + inverse).standard_normal(37 * 1024)
            x_d = rt.to_device(x)
            a, b = rt.empty((x.size,)), rt.empty((x.size,))
            _hip.check(rt.lib.wh_fft_engine_probe(rt.ctx, rt.stream(), 0, 512, nt, nt, 8, inverse, rt.ptr(x_d), rt.ptr(a), 37))
            _hip.check(rt.lib.wh_fft_probe(rt.ctx, rt.stream(), 512, gt, snt, inverse, rt.ptr(x_d), rt.ptr(b), 37))
            a, b = a.cpu().numpy(), b.cpu().numpy()
            cases["nt%d-inv%d" % (nt, inverse)] = {"equal": bool(np.array_equal(a, b)), "differing": int(np.sum(a != b)),
                                                  "finite": bool(np.all(np.isfinite(a)))}
    rep.set("lib", _hip.LIB_PATH)
    rep.set("cases", cases)
    rep.emit()


if __name__ == "__main__":
    main()
