"""Helper of tests/test_hip_manifold_bounds.py: runs in a process whose WH_LIB is the bounds build of wh_manifold
(tests/_variants.py, manifold_bounds).  The random stacks of tests/test_hip_manifold.py, a tap with segments, the TIMIT
networks and a ragged batch."""
import os

import numpy as np

import _variants as V


def main():
    import test_hip_manifold as T

    from world import _hip
    from world.manifold import DenseStack, dense_stack_device, vae_device

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    rng = np.random.RandomState(3)

    def run(st, x, **kw):
        r = dense_stack_device(rt, rt.to_device(np.ascontiguousarray(x)), st, **kw)
        return tuple(t.cpu().numpy() for t in r) if isinstance(r, tuple) else r.cpu().numpy()

    # (a) random stacks: every activation, widths 12 / 39 / 17, row counts at the tile edges, windows 0 and 2, a mean
    for acts in (("relu", "relu", "linear"), ("tanh", "sigmoid", "tanh")):
        for dims, window in (((39, 256, 12, 39), 0), ((39 * 5, 100, 256, 12), 2), ((12, 39, 17, 256), 0),
                             ((2048, 64, 3), 0)):
            st = T.random_stack(rng, dims, acts)
            d = dims[0] // (2 * window + 1)
            for n in (1, 15, 16, 17, 129):
                x, mean = rng.randn(n, d), rng.randn(d)
                got = run(st, x, window=window, in_shift=mean)
                ok = T.relerr(got, T.forward(st, x, window=window, in_shift=mean)) <= 1e-12
                rep.case("%s %s n=%d" % (acts, dims, n), ok=bool(ok))
    # taps, kept columns, shifts, segments
    st = T.random_stack(rng, (39 * 5, 256, 12, 256, 39 * 5), ("relu", "linear", "relu", "linear"))
    x, mean = rng.randn(301, 39), rng.randn(39)
    seg = [0, 1, 2, 150, 150, 300, 301]
    z, y = run(st, x, window=2, seg_off=seg, in_shift=mean, out_cols=(78, 39), out_shift=mean, tap_layer=1)
    zr, yr = T.forward(st, x, window=2, seg=seg, in_shift=mean, out_cols=(78, 39), out_shift=mean, tap=1)
    rep.case("tap+segments", ok=bool(T.relerr(z, zr) <= 1e-12 and T.relerr(y, yr) <= 1e-12))
    # (b) the TIMIT networks on the stored MCEP
    g = dict(np.load(os.path.join(V.HERE, "golden", "golden_manifold.npz")))
    enc, dec = DenseStack.from_h5(T.ENC), DenseStack.from_h5(T.DEC)
    z_d, y_d = vae_device(rt, rt.to_device(np.ascontiguousarray(g["mcep"][:, 1:])), enc, dec, 0, g["mean"])
    ok = (np.max(np.abs(z_d.cpu().numpy() - g["zc"])) <= 1e-4 and np.max(np.abs(y_d.cpu().numpy() - g["yc"][:, 1:])) <= 1e-4)
    rep.case("timit", ok=bool(ok))
    # (d) a ragged batch with window 2
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    xs = [synth_utterance(300 + u, 16000, 0.12 + 0.05 * (u % 7)) for u in range(31)]
    wb = WorldBatch(0)
    be = wb.encode(xs, 16000, f0_method="dio")
    e = T.random_stack(rng, (39 * 5, 256, 256, 12), ("relu", "relu", "linear"))
    dd = T.random_stack(rng, (12, 256, 256, 39 * 5), ("relu", "relu", "linear"))
    z_d, y_d = be.vae(e, dd, mean * 0.1, n0=40, window=2)
    mc = be.mcep(40)
    fo = be.batch.frame_off
    ok = True
    for u in range(len(xs)):
        a, b = int(fo[u]), int(fo[u + 1])
        zu, yu = vae_device(wb.rt, mc[a:b, 1:].contiguous(), e, dd, window=2, mean=mean * 0.1)
        ok &= bool(np.array_equal(zu.cpu().numpy(), z_d[a:b].cpu().numpy())
                   and np.array_equal(yu.cpu().numpy(), y_d[a:b].cpu().numpy()))
    rep.case("ragged", rt=wb.rt, ok=ok)
    rep.emit()


if __name__ == "__main__":
    main()
