"""The distributional losses on the wide head (include/qlx.h "distributional losses on the wide head")
without a GPU: the entry points and the two QLX_DIST_* kinds are declared and exported, and every argument error is found on
the host before any handle is read, so 4 KB of zeros serve as every handle and device array here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")
E_INVALID = -1
QUANTILE, CATEGORICAL = 0, 1

ENTRY_POINTS = ["qlx_head_values_dev", "qlx_head_dist_loss_dev", "qlx_head_dist_train_dev"]


class StatesDev(C.Structure):   # qlx_states_dev
    _fields_ = [("obs", C.c_void_p), ("replay", C.c_void_p), ("indices", C.c_void_p), ("env", C.c_void_p),
                ("layout", C.c_int32), ("which", C.c_int32)]


class Dist(C.Structure):        # qlx_dist
    _fields_ = [("kind", C.c_int32), ("atoms", C.c_uint32), ("v_min", C.c_float), ("v_max", C.c_float)]


class DistBatch(C.Structure):   # qlx_dist_batch
    _fields_ = [(k, C.c_void_p) for k in ("actions", "returns", "discounts", "terminals", "z_next", "a_star", "weights")]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libqlx.so not built (make lib)"
    L = C.CDLL(LIB)
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    L.qlx_last_error.restype = C.c_char_p
    for name, args in {
        "qlx_head_values_dev": [vp, vp, vp, u32, vp, vp, vp],
        "qlx_head_dist_loss_dev": [vp, vp, vp, vp, u32, vp, vp, vp, vp],
        "qlx_head_dist_train_dev": [vp, vp, vp, vp, u32, vp, vp, vp, vp],
    }.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = i32
    return L


def test_entry_points_are_declared_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qlx_[a-z0-9_]+)\s*\(", src))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+QLX_DIST_QUANTILE\s+0\b", src)
    assert re.search(r"#define\s+QLX_DIST_CATEGORICAL\s+1\b", src)
    assert re.search(r"typedef struct qlx_dist\s*\{", src) and re.search(r"typedef struct qlx_dist_batch\s*\{", src)
    assert C.sizeof(Dist) == 16 and C.sizeof(DistBatch) == 56


def test_python_mirror_matches():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))
    import qlx
    assert [f[0] for f in qlx.Dist._fields_] == [f[0] for f in Dist._fields_] and C.sizeof(qlx.Dist) == 16
    assert [f[0] for f in qlx.DistBatch._fields_] == [f[0] for f in DistBatch._fields_] and C.sizeof(qlx.DistBatch) == 56
    assert (qlx.DIST_QUANTILE, qlx.DIST_CATEGORICAL, qlx.DIST_MAX_ATOMS) == (0, 1, 341)


def test_argument_errors_are_found_before_any_handle_is_read(lib):
    """every call below passes either a null pointer or a `handle` that is 4 KB of zeros: a check that read it after the
    argument checks would not return QLX_E_INVALID with the field's name"""
    blob = C.create_string_buffer(4096 + 16)
    fake = (C.addressof(blob) + 15) & ~15   # stands for a head, a replay, a device array: never dereferenced
    src = C.byref(StatesDev(obs=fake))
    nosrc = C.byref(StatesDev())
    good = C.byref(Dist(QUANTILE, 51, 0.0, 0.0))
    cat = C.byref(Dist(CATEGORICAL, 51, -10.0, 10.0))
    full = dict(actions=fake, returns=fake, discounts=fake, terminals=fake, z_next=fake)
    batch = C.byref(DistBatch(**full))
    inf, nan = float("inf"), float("nan")

    def invalid(status, field):
        msg = (lib.qlx_last_error() or b"").decode()
        assert status == E_INVALID, (status, msg)
        assert field in msg, (field, msg)

    bad_dists = [(Dist(2, 51, 0.0, 1.0), "kind"), (Dist(-1, 51, 0.0, 1.0), "kind"),
                 (Dist(QUANTILE, 0, 0.0, 0.0), "atoms"), (Dist(QUANTILE, 342, 0.0, 0.0), "atoms"),
                 (Dist(CATEGORICAL, 0, 0.0, 1.0), "atoms"), (Dist(CATEGORICAL, 1, 0.0, 1.0), "atoms"),
                 (Dist(CATEGORICAL, 342, 0.0, 1.0), "atoms"),
                 (Dist(CATEGORICAL, 51, 1.0, 1.0), "v_min"), (Dist(CATEGORICAL, 51, 2.0, 1.0), "v_min"),
                 (Dist(CATEGORICAL, 51, -inf, 1.0), "v_min"), (Dist(CATEGORICAL, 51, 0.0, inf), "v_min"),
                 (Dist(CATEGORICAL, 51, nan, 1.0), "v_min"), (Dist(CATEGORICAL, 51, 0.0, nan), "v_min"),
                 (Dist(CATEGORICAL, 51, -3e38, 3e38), "v_max")]

    # qlx_head_values_dev
    values = lib.qlx_head_values_dev
    invalid(values(None, good, fake, 4, fake, fake, fake), "head")
    invalid(values(fake, None, fake, 4, fake, fake, fake), "dist")
    for d, field in bad_dists:
        invalid(values(fake, C.byref(d), fake, 4, fake, fake, fake), field)
    invalid(values(fake, good, None, 4, fake, fake, fake), "d_z")
    invalid(values(fake, good, fake, 0, fake, fake, fake), "n must")
    invalid(values(fake, good, fake, 8193, fake, fake, fake), "n must")
    invalid(values(fake, cat, fake, 4, None, None, None), "all null")

    # qlx_head_dist_loss_dev
    loss = lib.qlx_head_dist_loss_dev
    invalid(loss(None, good, fake, batch, 4, fake, None, None, None), "head")
    invalid(loss(fake, None, fake, batch, 4, fake, None, None, None), "dist")
    for d, field in bad_dists:
        invalid(loss(fake, C.byref(d), fake, batch, 4, fake, None, None, None), field)
    invalid(loss(fake, good, None, batch, 4, fake, None, None, None), "d_z")
    invalid(loss(fake, good, fake, None, 4, fake, None, None, None), "batch_in")
    for missing in full:
        part = DistBatch(**{k: v for k, v in full.items() if k != missing})
        invalid(loss(fake, good, fake, C.byref(part), 4, fake, None, None, None), missing)
    invalid(loss(fake, good, fake, batch, 0, fake, None, None, None), "batch must")
    invalid(loss(fake, good, fake, batch, 4097, fake, None, None, None), "batch must")
    invalid(loss(fake, cat, fake, batch, 4, None, None, None, None), "d_dz")

    # qlx_head_dist_train_dev
    train = lib.qlx_head_dist_train_dev
    invalid(train(None, good, src, batch, 4, fake, fake, None, None), "head")
    invalid(train(fake, None, src, batch, 4, fake, fake, None, None), "dist")
    for d, field in bad_dists:
        invalid(train(fake, C.byref(d), src, batch, 4, fake, fake, None, None), field)
    invalid(train(fake, good, None, batch, 4, fake, fake, None, None), "src")
    invalid(train(fake, good, nosrc, batch, 4, fake, fake, None, None), "source")
    invalid(train(fake, good, src, None, 4, fake, fake, None, None), "batch_in")
    for missing in full:
        part = DistBatch(**{k: v for k, v in full.items() if k != missing})
        invalid(train(fake, good, src, C.byref(part), 4, fake, fake, None, None), missing)
    invalid(train(fake, good, src, batch, 0, fake, fake, None, None), "batch must")
    invalid(train(fake, good, src, batch, 4097, fake, fake, None, None), "batch must")
    invalid(train(fake, cat, src, batch, 4, None, fake, None, None), "d_z_work")
    invalid(train(fake, cat, src, batch, 4, fake, None, None, None), "d_dz_work")
