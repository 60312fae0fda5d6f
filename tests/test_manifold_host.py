"""CPU: the host half of world.manifold — the pure-Python HDF5 reader on the reference's TIMIT networks (every dataset's
SHA-256 as libhdf5 reads it, recorded by tests/golden/make_manifold.py), the Keras config and duck-typed model paths into
a DenseStack, and the argument checks that run before any device call."""
import hashlib
import json
import os

import numpy as np
import pytest

from world import manifold as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = ("encoder", "decoder")


def _path(net):
    return os.path.join(GOLDEN, "manifold_timit_vae_%s.h5" % net)


@pytest.mark.parametrize("net", NETS)
def test_h5_reader_reproduces_every_dataset(golden, net):
    g = golden("manifold")
    f = M.H5File(_path(net))
    for name, shape, sha in zip(g["%s_datasets" % net], g["%s_shapes" % net], g["%s_sha256" % net]):
        a = f.dataset(str(name))
        assert a.dtype == np.float32
        assert list(a.shape) + [0] * (2 - a.ndim) == list(shape)
        assert hashlib.sha256(a.astype("<f4").tobytes()).hexdigest() == sha, name


@pytest.mark.parametrize("net,units", [("encoder", [256, 256, 256, 12]), ("decoder", [256, 256, 256, 39])])
def test_from_h5_topology(golden, net, units):
    g = golden("manifold")
    st = M.DenseStack.from_h5(_path(net))
    assert st.units == units
    assert st.activations == ["relu", "relu", "relu", "linear"]
    assert list(g["%s_units" % net]) == units
    assert st.input_dim == (39 if net == "encoder" else 12)
    for i, b in enumerate(st.biases):
        assert np.array_equal(b, g["%s_bias%d" % (net, i)])
    cfg = json.loads(M.H5File(_path(net)).attrs("/")["model_config"])
    assert [lay["class_name"] for lay in cfg["config"]["layers"]] == ["InputLayer"] + ["Dense"] * 4


def test_truncated_file_is_refused(tmp_path):
    raw = open(_path("encoder"), "rb").read()
    for n in (4, 100, len(raw) // 2, len(raw) - 1000):
        p = tmp_path / ("cut%d.h5" % n)
        p.write_bytes(raw[:n])
        with pytest.raises((ValueError, KeyError)):
            M.DenseStack.from_h5(str(p))


def test_unsupported_hdf5_features_are_named(tmp_path):
    raw = bytearray(open(_path("encoder"), "rb").read())
    raw[8] = 2  # superblock version 2
    p = tmp_path / "v2.h5"
    p.write_bytes(bytes(raw))
    with pytest.raises(NotImplementedError, match="superblock version 2"):
        M.H5File(str(p))


def test_non_dense_layer_in_config_is_refused(tmp_path):
    raw = open(_path("encoder"), "rb").read()
    old = b'"class_name": "Dense", "config": {"name": "dense_2"'
    new = b'"class_name": "Lambda","config": {"name": "dense_2"'  # same length: the file stays valid
    assert raw.count(old) == 1 and len(old) == len(new)
    p = tmp_path / "lambda.h5"
    p.write_bytes(raw.replace(old, new))
    with pytest.raises(ValueError, match="Lambda"):
        M.DenseStack.from_h5(str(p))


class _Layer:
    def __init__(self, cfg, weights):
        self._cfg, self._w = cfg, weights
        self.name = cfg["name"]

    def get_config(self):
        return dict(self._cfg)

    def get_weights(self):
        return list(self._w)


class InputLayer(_Layer):
    pass


class Dense(_Layer):
    pass


class Dropout(_Layer):
    pass


class _Model:
    def __init__(self, layers):
        self.layers = layers


def test_from_keras_duck_typed():
    rng = np.random.RandomState(3)
    w1, b1 = rng.randn(5, 7).astype(np.float32), rng.randn(7).astype(np.float32)
    w2 = rng.randn(7, 3).astype(np.float32)
    model = _Model([InputLayer({"name": "in"}, []),
                    Dense({"name": "d1", "units": 7, "activation": "tanh", "use_bias": True}, [w1, b1]),
                    Dense({"name": "d2", "units": 3, "activation": "sigmoid", "use_bias": False}, [w2])])
    st = M.DenseStack.from_keras(model)
    assert st.units == [7, 3] and st.activations == ["tanh", "sigmoid"] and st.input_dim == 5
    assert np.array_equal(st.weights[0], w1) and np.array_equal(st.biases[0], b1)
    assert np.array_equal(st.biases[1], np.zeros(3, np.float32))
    assert M.as_stack(model).tag == st.tag
    with pytest.raises(ValueError, match="Dropout"):
        M.DenseStack.from_keras(_Model([Dense({"name": "d1", "units": 7, "activation": "relu"}, [w1, b1]),
                                        Dropout({"name": "x"}, [])]))
    with pytest.raises(ValueError, match="softmax"):
        M.DenseStack.from_keras(_Model([Dense({"name": "d1", "units": 7, "activation": "softmax"}, [w1, b1])]))


def test_stack_validation():
    rng = np.random.RandomState(0)
    w, b = rng.randn(4, 6), rng.randn(6)
    with pytest.raises(ValueError, match="at least one"):
        M.DenseStack([])
    with pytest.raises(ValueError, match="takes 5 inputs"):
        M.DenseStack([(w, b, "relu"), (rng.randn(5, 2), rng.randn(2), "linear")])
    with pytest.raises(ValueError, match="non-finite"):
        M.DenseStack([(np.where(w > 1, np.nan, w), b, "relu")])
    with pytest.raises(ValueError, match="non-finite"):
        M.DenseStack([(w, np.full(6, np.inf), "relu")])
    with pytest.raises(ValueError, match="elu"):
        M.DenseStack([(w, b, "elu")])
    with pytest.raises(ValueError, match="W must be"):
        M.DenseStack([(w, rng.randn(5), "relu")])
    with pytest.raises(ValueError, match="limit of 16"):
        M.DenseStack([(rng.randn(3, 3), rng.randn(3), "relu")] * 17)
    st = M.DenseStack([(w, b, None)])
    assert st.activations == ["linear"]
    assert M.DenseStack([(w, b, "relu")]).tag != M.DenseStack([(w, b, "tanh")]).tag
    with pytest.raises(TypeError):
        M.as_stack(42)


class _NoDevice:
    """Stands in for the runtime: any device call fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device touched before the arguments were checked: %s" % name)


class _Shape:
    def __init__(self, n, d):
        self.shape = (n, d)


def test_device_arguments_checked_before_any_device_call():
    rng = np.random.RandomState(1)
    wide = M.DenseStack([(rng.randn(4, 300), rng.randn(300), "relu"), (rng.randn(300, 2), rng.randn(2), "linear")])
    ok = M.DenseStack([(rng.randn(4, 8), rng.randn(8), "relu"), (rng.randn(8, 2), rng.randn(2), "linear")])
    rt, x = _NoDevice(), _Shape(10, 4)
    with pytest.raises(ValueError, match="limit is 256"):
        M.dense_stack_device(rt, x, wide)
    with pytest.raises(ValueError, match="takes 4 inputs"):
        M.dense_stack_device(rt, _Shape(10, 3), ok)
    with pytest.raises(ValueError, match="window 1"):
        M.dense_stack_device(rt, x, ok, window=1)
    with pytest.raises(ValueError, match="kept columns"):
        M.dense_stack_device(rt, x, ok, out_cols=(1, 2))
    with pytest.raises(ValueError, match="seg_off"):
        M.dense_stack_device(rt, x, ok, seg_off=[0, 5, 4, 10])
    with pytest.raises(ValueError, match="seg_off"):
        M.dense_stack_device(rt, x, ok, seg_off=[0, 9])
    with pytest.raises(ValueError, match="tap_layer"):
        M.dense_stack_device(rt, x, ok, tap_layer=1)
    with pytest.raises(ValueError, match="in_shift"):
        M.dense_stack_device(rt, x, ok, in_shift=np.zeros(3))
    big = M.DenseStack([(rng.randn(2100, 4), rng.randn(4), "relu")])
    with pytest.raises(ValueError, match="2048"):
        M.dense_stack_device(rt, _Shape(3, 2100), big)


def test_encode_vae_checks_before_the_device():
    from world import main

    W = main.World()
    rng = np.random.RandomState(2)
    enc = M.DenseStack([(rng.randn(39, 16), rng.randn(16), "relu"), (rng.randn(16, 12), rng.randn(12), "linear")])
    dec = M.DenseStack([(rng.randn(12, 16), rng.randn(16), "relu"), (rng.randn(16, 39), rng.randn(39), "linear")])
    x = rng.randn(5, 39)
    with pytest.raises(AssertionError):
        W.encode_vae(x, np.zeros(5), enc, dec, 0, 41, 256, 0.0)  # n0 mismatch: the reference's assert
    with pytest.raises(ValueError, match="energy"):
        W.encode_vae(x.copy(), np.zeros(4), enc, dec, 0, 40, 256, 0.0)
    y = x.copy()
    with pytest.raises(ValueError, match="mean"):
        W.encode_vae(y, np.zeros(5), enc, dec, 0, 40, 256, np.zeros(7))
    assert np.array_equal(y, x)  # refused before the caller's array is touched
