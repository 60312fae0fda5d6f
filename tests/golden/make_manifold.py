"""Generate tests/golden/golden_manifold.npz, the fixture of the manifold vocoder (World.encode_vae), by running the
UNMODIFIED reference.

Run only in the authoring container (needs /root/reference and the system HDF5 library):

    python tests/golden/make_manifold.py            # HDF5_LIB=/path/to/libhdf5.so if ctypes cannot find it

It copies the reference's trained TIMIT networks (manifold/timit_vae_{encoder,decoder}_0001: weights and a JSON
config, data) to tests/golden/manifold_timit_vae_{encoder,decoder}.h5 and records:
  * per dataset of both files: its shape and the SHA-256 of its little-endian float32 bytes, read with libhdf5 through
    ctypes (a reader independent of world.manifold's), and the bias vectors in full;
  * the reference's encode_mcep(spec.T, n0=40) of test-mwm.wav after a harvest encode, the mean of its coefficients
    1..39, and Zc / Yc of the reference's encode_vae with window 0, the Keras networks emulated by float32 NumPy
    (x @ W + b, ReLU on the hidden layers: Dense.predict in float32);
  * the two log-spectral distortions of test/spectralFeatures.py (MCEP only; through the VAE).
"""
import ctypes
import hashlib
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refshim  # noqa: E402

NETS = ("encoder", "decoder")


def hdf5_lib():
    """(libhdf5, libhdf5_hl): HDF5_LIB names the first, else the usual places of a system or conda install."""
    dirs = [os.path.join(p, "lib") for p in (os.environ.get("CONDA_PREFIX"), sys.prefix, "/opt/conda", "/usr") if p]
    dirs.append("/usr/lib/x86_64-linux-gnu")
    path = os.environ.get("HDF5_LIB") or next((os.path.join(d, "libhdf5.so") for d in dirs
                                               if os.path.exists(os.path.join(d, "libhdf5.so"))), None)
    if not path:
        raise SystemExit("libhdf5.so not found: set HDF5_LIB")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    return lib, ctypes.CDLL(path.replace("libhdf5.so", "libhdf5_hl.so"))


def read_datasets(path, names):
    """{name: float32 array} through H5Fopen + H5LTget_dataset_info + H5LTread_dataset_float."""
    lib, hl = hdf5_lib()
    hid = ctypes.c_int64  # hid_t (HDF5 >= 1.10)
    lib.H5open()
    lib.H5Fopen.restype = hid
    lib.H5Fopen.argtypes = [ctypes.c_char_p, ctypes.c_uint, hid]
    lib.H5Fclose.argtypes = [hid]
    hl.H5LTget_dataset_ndims.argtypes = [hid, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    hl.H5LTget_dataset_info.argtypes = [hid, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p,
                                        ctypes.c_void_p]
    hl.H5LTread_dataset_float.argtypes = [hid, ctypes.c_char_p, ctypes.c_void_p]
    f = lib.H5Fopen(path.encode(), 0, 0)  # H5F_ACC_RDONLY, H5P_DEFAULT
    assert f >= 0, path
    out = {}
    for name in names:
        rank = ctypes.c_int()
        assert hl.H5LTget_dataset_ndims(f, name.encode(), ctypes.byref(rank)) >= 0, name
        dims = (ctypes.c_uint64 * max(rank.value, 1))()
        assert hl.H5LTget_dataset_info(f, name.encode(), dims, None, None) >= 0, name
        shape = tuple(int(dims[i]) for i in range(rank.value))
        a = np.zeros(shape, dtype=np.float32)
        assert hl.H5LTread_dataset_float(f, name.encode(), a.ctypes.data_as(ctypes.c_void_p)) >= 0, name
        out[name] = a
    lib.H5Fclose(f)
    return out


def dense_layers(path):
    """[(W, b, activation)] in model order; the layer names and activations from the JSON config (read as bytes from
    the file: the config is the one variable-length string Keras writes at the root, located by its JSON text)."""
    raw = open(path, "rb").read()
    start = raw.index(b'{"class_name": "Model"')
    config, _ = json.JSONDecoder().raw_decode(raw[start:].decode("utf-8", "replace"))
    names, acts = [], []
    for spec in config["config"]["layers"]:
        if spec["class_name"] == "Dense":
            names.append(spec["config"]["name"])
            acts.append(spec["config"]["activation"])
    ds = read_datasets(path, ["/model_weights/%s/%s/%s:0" % (n, n, k) for n in names for k in ("kernel", "bias")])
    return [(ds["/model_weights/%s/%s/kernel:0" % (n, n)], ds["/model_weights/%s/%s/bias:0" % (n, n)], a)
            for n, a in zip(names, acts)], names, ds


class Float32Dense:
    """Keras Dense.predict restated in float32 NumPy."""

    def __init__(self, layers):
        self.layers = layers

    def predict(self, x, batch_size=None):
        h = np.asarray(x).astype(np.float32)
        for w, b, act in self.layers:
            h = h @ w + b
            if act == "relu":
                h = np.maximum(h, np.float32(0))
            else:
                assert act == "linear", act
        return h


def lsd(ori_spec, syn_spec):
    """test/spectralFeatures.py's log-spectral distortion (restated)."""
    a = ori_spec / np.sqrt(np.mean(ori_spec ** 2, axis=1)).reshape(-1, 1)
    b = syn_spec / np.sqrt(np.mean(syn_spec ** 2, axis=1)).reshape(-1, 1)
    return np.mean(np.mean((20 * np.log10(a) - 20 * np.log10(b)) ** 2, axis=1) ** 0.5)


def main():
    from scipy.io import wavfile

    R = refshim.load()
    out = {}
    nets = {}
    for net in NETS:
        src = os.path.join(refshim.REFERENCE_ROOT, "manifold", "timit_vae_%s_0001" % net)
        dst = os.path.join(HERE, "manifold_timit_vae_%s.h5" % net)
        shutil.copyfile(src, dst)
        layers, names, ds = dense_layers(dst)
        nets[net] = layers
        out["%s_datasets" % net] = np.array(sorted(ds))
        out["%s_shapes" % net] = np.array([list(ds[k].shape) + [0] * (2 - ds[k].ndim) for k in sorted(ds)])
        out["%s_sha256" % net] = np.array([hashlib.sha256(ds[k].astype("<f4").tobytes()).hexdigest() for k in sorted(ds)])
        out["%s_units" % net] = np.array([w.shape[1] for w, _, _ in layers])
        out["%s_activations" % net] = np.array([a for _, _, a in layers])
        for i, (_, b, _) in enumerate(layers):
            out["%s_bias%d" % (net, i)] = b
    fs, xi = wavfile.read(os.path.join(refshim.REFERENCE_ROOT, "test", "test-mwm.wav"))
    x = xi / (2 ** 15 - 1)
    W = R.main.World()
    data = W.encode(fs, x, f0_method="harvest")
    spec = data["spectrogram"].T
    mcep = W.encode_mcep(spec, n0=40)
    out["mcep"] = mcep.copy()
    m = np.mean(mcep[:, 1:], axis=0)
    out["mean"] = m
    energy = mcep[:, 0]
    xc = mcep[:, 1:40]  # a view: encode_vae's `Xc -= mean` writes through it, as in test/spectralFeatures.py
    zc, yc = W.encode_vae(xc, energy, encoder=Float32Dense(nets["encoder"]), decoder=Float32Dense(nets["decoder"]),
                          window=0, n0=40, batch_size=256, mean=m)
    assert np.array_equal(xc, out["mcep"][:, 1:] - m)  # the caller's array after `Xc -= mean`
    out["zc"] = zc
    out["yc"] = yc
    out["lsd_mcep"] = lsd(W.decode_mcep(out["mcep"], fft_size=1024), spec)
    out["lsd_vae"] = lsd(W.decode_mcep(yc, fft_size=1024), spec)
    np.savez_compressed(os.path.join(HERE, "golden_manifold.npz"), **out)
    print("manifold written: Zc %s %s, Yc %s; LSD %.5f dB (MCEP), %.5f dB (VAE)"
          % (zc.shape, zc.dtype, yc.shape, out["lsd_mcep"], out["lsd_vae"]))


if __name__ == "__main__":
    main()
