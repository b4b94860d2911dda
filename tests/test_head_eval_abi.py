"""Acting with, evaluating and checkpointing a distributional head (include/qlx.h "acting with, evaluating and checkpointing a
distributional head") without a GPU: the five entry points are declared and exported, the Python mirror
agrees, and every argument error is found on the host before any handle is read, so 4 KB of zeros serve as every handle and
device array here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
INTERNAL = os.path.join(ROOT, "q-learning_amd", "csrc", "qlx_internal.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")
E_INVALID = -1
QUANTILE, CATEGORICAL = 0, 1

ENTRY_POINTS = ["qlx_head_select_dev", "qlx_head_act_dev", "qlx_evaluator_run_head", "qlx_head_write_checkpoint",
                "qlx_head_read_checkpoint"]


class StatesDev(C.Structure):   # qlx_states_dev
    _fields_ = [("obs", C.c_void_p), ("replay", C.c_void_p), ("indices", C.c_void_p), ("env", C.c_void_p),
                ("layout", C.c_int32), ("which", C.c_int32)]


class Dist(C.Structure):        # qlx_dist
    _fields_ = [("kind", C.c_int32), ("atoms", C.c_uint32), ("v_min", C.c_float), ("v_max", C.c_float)]


vp, i32, u32, u64, f64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_double
SIGNATURES = {
    "qlx_head_select_dev": [vp, vp, vp, u32, f64, u64, u32, vp, vp, vp],
    "qlx_head_act_dev": [vp, vp, vp, u32, f64, u64, u32, vp, vp, vp, vp],
    "qlx_evaluator_run_head": [vp, vp, vp, vp],
    "qlx_head_write_checkpoint": [vp, C.c_char_p],
    "qlx_head_read_checkpoint": [vp, C.c_char_p],
}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libqlx.so not built (make lib)"
    L = C.CDLL(LIB)
    L.qlx_last_error.restype = C.c_char_p
    for name, args in SIGNATURES.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = i32
    return L


def test_entry_points_are_declared_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qlx_[a-z0-9_]+)\s*\(", src))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
    # the declared parameter counts are the ones this file calls with
    for name, args in SIGNATURES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == len(args), name
    assert re.search(r"\bP_ACT_DEV\s*=\s*9\b", open(INTERNAL).read())


def test_python_mirror_matches():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))
    import qlx
    assert qlx.P_ACT_DEV == 9
    L = qlx.lib()
    ptr = lambda t: getattr(t, "_type_", None)
    for name, args in SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is i32, name
        assert len(fn.argtypes) == len(args), name
        for got, want in zip(fn.argtypes, args):
            if want in (u32, u64, f64, C.c_char_p):
                assert got is want, (name, got, want)
            else:   # a pointer: void* or a typed pointer to the mirror's structure
                assert got is vp or ptr(got) in (qlx.Dist, qlx.StatesDev, qlx.EvalSummary), (name, got)
    for cls, method in ((qlx.Evaluator, "run_head"), (qlx.WideHead, "select_dev"), (qlx.WideHead, "act_dev"),
                        (qlx.WideHead, "write_checkpoint"), (qlx.WideHead, "read_checkpoint")):
        assert callable(getattr(cls, method)), (cls, method)


def test_argument_errors_are_found_before_any_handle_is_read(lib):
    """every call below passes either a null pointer or a `handle` that is 4 KB of zeros: a check that read it after the
    argument checks would not return QLX_E_INVALID with the field's name"""
    blob = C.create_string_buffer(4096 + 16)
    fake = (C.addressof(blob) + 15) & ~15   # stands for a head, an evaluator, a device array: never dereferenced
    src = C.byref(StatesDev(obs=fake))
    nosrc = C.byref(StatesDev())
    good = C.byref(Dist(QUANTILE, 51, 0.0, 0.0))
    cat = C.byref(Dist(CATEGORICAL, 51, -10.0, 10.0))
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
    bad_eps = [nan, inf, -inf, -0.25, 1.5]

    # qlx_head_select_dev
    select = lib.qlx_head_select_dev
    invalid(select(None, good, fake, 4, 0.1, 1, 0, fake, fake, fake), "head")
    invalid(select(fake, None, fake, 4, 0.1, 1, 0, fake, fake, fake), "dist")
    for d, field in bad_dists:
        invalid(select(fake, C.byref(d), fake, 4, 0.1, 1, 0, fake, fake, fake), field)
    invalid(select(fake, good, None, 4, 0.1, 1, 0, fake, fake, fake), "d_z")
    invalid(select(fake, good, fake, 0, 0.1, 1, 0, fake, fake, fake), "n must")
    invalid(select(fake, good, fake, 8193, 0.1, 1, 0, fake, fake, fake), "n must")
    for eps in bad_eps:
        invalid(select(fake, cat, fake, 4, eps, 1, 0, fake, fake, fake), "epsilon")
    invalid(select(fake, cat, fake, 4, 0.1, 1, 0, None, fake, fake), "d_actions")

    # qlx_head_act_dev
    act = lib.qlx_head_act_dev
    invalid(act(None, good, src, 4, 0.1, 1, 0, fake, fake, fake, fake), "head")
    invalid(act(fake, None, src, 4, 0.1, 1, 0, fake, fake, fake, fake), "dist")
    for d, field in bad_dists:
        invalid(act(fake, C.byref(d), src, 4, 0.1, 1, 0, fake, fake, fake, fake), field)
    invalid(act(fake, good, None, 4, 0.1, 1, 0, fake, fake, fake, fake), "src")
    invalid(act(fake, good, nosrc, 4, 0.1, 1, 0, fake, fake, fake, fake), "source")
    invalid(act(fake, good, src, 0, 0.1, 1, 0, fake, fake, fake, fake), "n must")
    invalid(act(fake, good, src, 8193, 0.1, 1, 0, fake, fake, fake, fake), "n must")
    for eps in bad_eps:
        invalid(act(fake, cat, src, 4, eps, 1, 0, fake, fake, fake, fake), "epsilon")
    invalid(act(fake, cat, src, 4, 0.1, 1, 0, None, fake, fake, fake), "d_actions")
    invalid(act(fake, cat, src, 4, 0.1, 1, 0, fake, fake, fake, None), "d_z_work")

    # qlx_evaluator_run_head
    run = lib.qlx_evaluator_run_head
    invalid(run(None, fake, good, fake), "evaluator")
    invalid(run(fake, None, good, fake), "head")
    invalid(run(fake, fake, None, fake), "dist")
    for d, field in bad_dists:
        invalid(run(fake, fake, C.byref(d), fake), field)
    invalid(run(fake, fake, cat, None), "out")

    # the checkpoint calls
    for call in (lib.qlx_head_write_checkpoint, lib.qlx_head_read_checkpoint):
        invalid(call(None, b"/nonexistent/head.ckpt"), "head")
        invalid(call(fake, None), "path")
