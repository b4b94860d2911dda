"""The wide output head (include/qlx.h "a wide output head") without a GPU: its entry points are declared
and exported, its argument errors are found on the host before any handle is read (so a handle that points at nothing
serves here), and the float64 restatement the GPU tests compare against (tests/wide_head_reference.py) gives, at width 3
with W4 and b4, the oracle's Q on the oracle's a4."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import wide_head_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")
E_INVALID = -1

ENTRY_POINTS = ["qlx_head_create", "qlx_head_destroy", "qlx_head_width", "qlx_head_iterations", "qlx_head_get_var",
                "qlx_head_set_var", "qlx_head_forward_dev", "qlx_head_backward_dev", "qlx_head_grads_dev",
                "qlx_head_copy_weights_dev"]


class StatesDev(C.Structure):   # qlx_states_dev
    _fields_ = [("obs", C.c_void_p), ("replay", C.c_void_p), ("indices", C.c_void_p), ("env", C.c_void_p),
                ("layout", C.c_int32), ("which", C.c_int32)]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libqlx.so not built (make lib)"
    L = C.CDLL(LIB)
    vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    L.qlx_last_error.restype = C.c_char_p
    for name, args in {
        "qlx_head_create": [vp, u32, u64, vp], "qlx_head_destroy": [vp], "qlx_head_get_var": [vp, i32, i32, vp],
        "qlx_head_set_var": [vp, i32, i32, vp], "qlx_head_forward_dev": [vp, vp, u32, vp, vp],
        "qlx_head_backward_dev": [vp, vp, vp, vp, u32, u64], "qlx_head_grads_dev": [vp, vp, vp],
        "qlx_head_copy_weights_dev": [vp, vp], "qlx_head_width": [vp],
    }.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = i32
    L.qlx_head_iterations.argtypes = [vp]
    L.qlx_head_iterations.restype = C.c_int64
    return L


def test_entry_points_are_declared_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qlx_[a-z0-9_]+)\s*\(", src))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+QLX_HEAD_MAX_WIDTH\s+1024\b", src)


def test_argument_errors_are_found_before_any_handle_is_read(lib):
    """every call below passes either a null pointer or a `handle` that is 4 KB of zeros: a check that read it after the
    argument checks would not return QLX_E_INVALID with the field's name"""
    blob = C.create_string_buffer(4096 + 16)
    fake = (C.addressof(blob) + 15) & ~15   # stands for a model, a head, a device array: never dereferenced
    out = C.c_void_p()
    src = StatesDev(obs=fake)
    nosrc = StatesDev()
    cnt = C.c_uint64()

    def invalid(status, field):
        msg = (lib.qlx_last_error() or b"").decode()
        assert status == E_INVALID, (status, msg)
        assert field in msg, (field, msg)

    invalid(lib.qlx_head_create(None, 4, 0, C.byref(out)), "model")
    invalid(lib.qlx_head_create(fake, 4, 0, None), "out")
    invalid(lib.qlx_head_create(fake, 0, 0, C.byref(out)), "width")
    invalid(lib.qlx_head_create(fake, 1025, 0, C.byref(out)), "width")
    assert out.value is None
    for fn in (lib.qlx_head_get_var, lib.qlx_head_set_var):
        invalid(fn(None, 0, 0, fake), "head")
        invalid(fn(fake, 0, 0, None), "out" if fn is lib.qlx_head_get_var else "in")
        invalid(fn(fake, 2, 0, fake), "var")
        invalid(fn(fake, -1, 0, fake), "var")
        invalid(fn(fake, 0, 3, fake), "which")
    invalid(lib.qlx_head_forward_dev(None, C.byref(src), 4, fake, None), "head")
    invalid(lib.qlx_head_forward_dev(fake, None, 4, fake, None), "src")
    invalid(lib.qlx_head_forward_dev(fake, C.byref(nosrc), 4, fake, None), "source")
    invalid(lib.qlx_head_forward_dev(fake, C.byref(src), 0, fake, None), "n must")
    invalid(lib.qlx_head_forward_dev(fake, C.byref(src), 8193, fake, None), "n must")
    invalid(lib.qlx_head_forward_dev(fake, C.byref(src), 4, None, None), "d_z")
    invalid(lib.qlx_head_backward_dev(None, C.byref(src), fake, None, 4, 0), "head")
    invalid(lib.qlx_head_backward_dev(fake, None, fake, None, 4, 0), "src")
    invalid(lib.qlx_head_backward_dev(fake, C.byref(src), None, None, 4, 0), "d_dz")
    invalid(lib.qlx_head_backward_dev(fake, C.byref(src), fake, None, 0, 0), "batch")
    invalid(lib.qlx_head_backward_dev(fake, C.byref(src), fake, None, 4097, 0), "batch")
    invalid(lib.qlx_head_grads_dev(None, C.byref(out), C.byref(cnt)), "head")
    invalid(lib.qlx_head_grads_dev(fake, None, C.byref(cnt)), "d_grads_out")
    invalid(lib.qlx_head_grads_dev(fake, C.byref(out), None), "count_out")
    invalid(lib.qlx_head_copy_weights_dev(None, fake), "dst")
    invalid(lib.qlx_head_copy_weights_dev(fake, None), "src")
    assert lib.qlx_head_width(None) == -1 and lib.qlx_head_iterations(None) == -1
    assert lib.qlx_head_destroy(None) == 0


def test_restatement_at_width_3_is_the_oracles_q():
    """Z of the restatement with Wh = W4, bh = b4 on the oracle's a4 against the oracle's fp32 Q (one fmaf chain over all
    512 k and the bias: 513 operations), within gamma(520) * sum |terms|"""
    net = O.QNet(seed=23, f32=True)
    _, _, _, _, x = O.envs_run(0x5EED, 6, 30, 7, want_tensors=True)
    q, acts = net.forward(x, acts=True)
    a4 = acts[3]
    assert a4.shape == (6, 512) and (a4 > 0).any()
    z, terms = R.forward(a4, net.get(8), net.get(9))
    err = np.abs(z - q.astype(np.float64))
    print("width-3 restatement against the oracle: max err / bound =", float((err / (R.gamma(520) * terms)).max()))
    assert (err <= R.gamma(520) * terms).all()
    assert np.abs(z).max() > 0


def test_restatement_gradients_are_the_derivatives():
    """the restatement's backward against central differences of its own forward (float64: exact to ~1e-9)"""
    rng = np.random.default_rng(3)
    B, width = 5, 7
    a4 = np.maximum(rng.normal(size=(B, 512)), 0).astype(np.float32)
    wh = rng.normal(size=(512, width)).astype(np.float32)
    bh = rng.normal(size=width).astype(np.float32)
    dz = rng.normal(size=(B, width)).astype(np.float32)
    w4 = rng.normal(size=(512, 3)).astype(np.float32)
    dq = rng.normal(size=(B, 3)).astype(np.float32)

    def loss(a, w, b):
        return float((R.forward(a, w, b)[0] * dz).sum() + ((R.f64(a) @ R.f64(w4)) * dq).sum())

    dwh, dbh, _, _ = R.weight_grads(a4, dz)
    dz4, _ = R.backward_data(a4, wh, dz, w4, dq)
    h = 1e-4
    for k, j in [(0, 0), (100, 3), (511, 6)]:
        e = np.zeros((512, width))
        e[k, j] = h
        assert abs((loss(a4, wh + e, bh) - loss(a4, wh - e, bh)) / (2 * h) - dwh[k, j]) < 1e-6
    e = np.zeros(width)
    e[2] = h
    assert abs((loss(a4, wh, bh + e) - loss(a4, wh, bh - e)) / (2 * h) - dbh[2]) < 1e-6
    for b, k in [(0, 1), (3, 200), (4, 511)]:
        e = np.zeros((B, 512))
        e[b, k] = h
        want = (loss(R.f64(a4) + e, wh, bh) - loss(R.f64(a4) - e, wh, bh)) / (2 * h)
        assert abs((want if a4[b, k] > 0 else 0.0) - dz4[b, k]) < 1e-6
