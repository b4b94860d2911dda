"""The Q-net's separate backward and optimizer calls (include/qlx.h "a caller's own loss") without a GPU: the
four names are declared and exported, the step flag of the ctypes mirror is the header's, and every host check is made
before a handle is read (a block of zero bytes stands in for the handles and is left alone)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")

NEW = ["qlx_model_forward_ticket", "qlx_model_backward_dev", "qlx_model_step_dev", "qlx_model_grads_dev"]
E_INVALID, E_STATE = -1, -4


def test_new_names_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qlx_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    dyn = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NEW:
        assert n in declared, n
        assert n in dyn, n


def test_step_flag_matches_header():
    import qlx
    m = re.search(r"#define\s+QLX_STEP_GRADS_WRITTEN\s+(\d+)u?\b", open(HEADER).read())
    assert m and int(m.group(1)) == qlx.STEP_GRADS_WRITTEN == 1


def _err(L):
    return L.qlx_last_error().decode()


class _Fakes:
    """zeroed stand-ins for a model, an env and a replay, and pointers that are never dereferenced"""

    def __init__(self):
        self.blocks = [C.create_string_buffer(4096) for _ in range(3)]
        self.m, self.env, self.rb = (C.cast(b, C.c_void_p) for b in self.blocks)
        self.ptr = C.c_void_p(0x10000)   # 16-byte aligned

    def untouched(self):
        return all(bytes(b) == bytes(4096) for b in self.blocks)


def test_argument_errors_need_no_device():
    import qlx
    L = qlx.lib()
    f = _Fakes()
    m, p = f.m, f.ptr
    S = qlx.StatesDev
    ok = S(obs=p.value, layout=1)
    t = C.c_uint64(77)
    out, cnt = C.c_void_p(), C.c_uint64()

    assert L.qlx_model_forward_ticket(None, C.byref(t)) == E_INVALID and "null model" in _err(L)
    assert L.qlx_model_forward_ticket(m, None) == E_INVALID and "ticket_out" in _err(L)
    assert L.qlx_model_grads_dev(None, C.byref(out), C.byref(cnt)) == E_INVALID and "null model" in _err(L)
    assert L.qlx_model_grads_dev(m, None, C.byref(cnt)) == E_INVALID and "d_grads_out" in _err(L)
    assert L.qlx_model_grads_dev(m, C.byref(out), None) == E_INVALID and "count_out" in _err(L)
    assert L.qlx_model_step_dev(None, 0) == E_INVALID and "null model" in _err(L)
    for bad in (2, 3, 0x80000000):
        assert L.qlx_model_step_dev(m, bad) == E_INVALID and "flags" in _err(L)

    def back(model, src, dq=p, batch=4, ticket=0):
        return L.qlx_model_backward_dev(model, None if src is None else C.byref(src), dq, batch, ticket)

    assert back(None, ok) == E_INVALID and "null model" in _err(L)
    assert back(m, None) == E_INVALID and "null src" in _err(L)
    assert back(m, ok, dq=None) == E_INVALID and "d_dq" in _err(L)
    # zero or more than one source
    assert back(m, S(layout=1)) == E_INVALID and "no state source" in _err(L)
    assert back(m, S(obs=p.value, env=f.env.value)) == E_INVALID and "more than one" in _err(L)
    assert back(m, S(obs=p.value, replay=f.rb.value, indices=p.value)) == E_INVALID and "more than one" in _err(L)
    assert back(m, S(env=f.env.value, replay=f.rb.value, indices=p.value)) == E_INVALID and "more than one" in _err(L)
    # indices and replay go together
    assert back(m, S(indices=p.value)) == E_INVALID and "indices without" in _err(L)
    assert back(m, S(replay=f.rb.value)) == E_INVALID and "replay without" in _err(L)
    for lay in (2, -1):
        assert back(m, S(obs=p.value, layout=lay)) == E_INVALID and "layout" in _err(L)
    for which in (2, -1):
        assert back(m, S(obs=p.value, which=which)) == E_INVALID and "which" in _err(L)
    for off in (1, 4, 8):
        assert back(m, S(obs=p.value + off)) == E_INVALID and "obs" in _err(L) and "aligned" in _err(L)
    for bad in (0, 4097):
        for ticket in (0, 5):
            assert back(m, ok, batch=bad, ticket=ticket) == E_INVALID and "batch" in _err(L)
    assert t.value == 77 and out.value is None and cnt.value == 0
    assert f.untouched()   # nothing wrote into the stand-ins


def test_calls_before_a_reserve_or_a_gradient_are_refused():
    """an otherwise valid backward on a model that never reserved (the zeroed block), and a step on a model whose gradient
    buffer nothing has filled: QLX_E_STATE, nothing launched"""
    import qlx
    L = qlx.lib()
    f = _Fakes()
    p = f.ptr
    for src in (qlx.StatesDev(obs=p.value, layout=0), qlx.StatesDev(obs=p.value, layout=1),
                qlx.StatesDev(replay=f.rb.value, indices=p.value, layout=1, which=1), qlx.StatesDev(env=f.env.value)):
        for batch, ticket in ((4, 0), (4096, 0), (4, 9)):
            assert L.qlx_model_backward_dev(f.m, C.byref(src), p, batch, ticket) == E_STATE and "reserve" in _err(L)
    for flags in (0, qlx.STEP_GRADS_WRITTEN):
        assert L.qlx_model_step_dev(f.m, flags) == E_STATE and "gradient" in _err(L)
    assert f.untouched()
