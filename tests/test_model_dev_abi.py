"""The Q-net's device-tensor calls (include/qlx.h "Q-network on device tensors") without a GPU: the names are
declared and exported, the header compiles as C and C++ with the struct size the ABI states, the ctypes mirror agrees, and
every host check is made before a handle is read (a block of zero bytes stands in for the handles and is left alone)."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")

NEW = ["qlx_model_stream", "qlx_model_share_stream", "qlx_model_reserve", "qlx_model_q_dev", "qlx_model_train_dev",
       "qlx_model_copy_weights_dev", "qlx_states_dev"]
E_INVALID, E_STATE = -1, -4


def test_new_names_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qlx_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    dyn = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NEW[:-1]:
        assert n in declared, n
        assert n in dyn, n
    assert re.search(r"\}\s*qlx_states_dev\s*;", src), "the struct is a typedef of the header"


def test_header_compiles_with_the_abi_size(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cxx and cc, "no host compiler"
    body = '#include "qlx.h"\n'
    (tmp_path / "t.cpp").write_text(body + 'static_assert(sizeof(qlx_states_dev) == 40, "ABI size");\n'
                                    "int main() { qlx_states_dev s = {}; return s.obs != nullptr || s.which != 0; }\n")
    (tmp_path / "t.c").write_text(body + '_Static_assert(sizeof(qlx_states_dev) == 40, "ABI size");\n'
                                  "int main(void) { qlx_states_dev s = {0}; return s.layout != 0; }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / "t.cpp")], check=True)
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / "t.c")], check=True)


def test_ctypes_struct_matches_header():
    import qlx
    assert C.sizeof(qlx.StatesDev) == 40
    assert [k for k, _ in qlx.StatesDev._fields_] == ["obs", "replay", "indices", "env", "layout", "which"]
    assert [getattr(qlx.StatesDev, k).offset for k, _ in qlx.StatesDev._fields_] == [0, 8, 16, 24, 32, 36]
    assert (qlx.OBS_NHWC_SLOT, qlx.OBS_NCHW_TIME) == (0, 1)


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
    out = C.c_void_p()

    assert L.qlx_model_stream(None, C.byref(out)) == E_INVALID and "null model" in _err(L)
    assert L.qlx_model_stream(m, None) == E_INVALID and "hip_stream_out" in _err(L)
    assert L.qlx_model_share_stream(None, f.env) == E_INVALID and "null model" in _err(L)
    assert L.qlx_model_share_stream(m, None) == E_INVALID and "null env" in _err(L)
    assert L.qlx_model_reserve(None, 16) == E_INVALID and "null model" in _err(L)
    for bad in (0, 8193):
        assert L.qlx_model_reserve(m, bad) == E_INVALID and "max_n" in _err(L)
    assert L.qlx_model_copy_weights_dev(None, m) == E_INVALID and "null dst" in _err(L)
    assert L.qlx_model_copy_weights_dev(m, None) == E_INVALID and "null src" in _err(L)

    def q(model, src, n=4, outs=(p, p, p)):
        return L.qlx_model_q_dev(model, None if src is None else C.byref(src), n, *outs)

    def train(model, src, actions=p, y=p, w=None, batch=4, loss=None, td=None):
        return L.qlx_model_train_dev(model, None if src is None else C.byref(src), actions, y, w, batch, loss, td)

    for call in (q, train):
        assert call(None, ok) == E_INVALID and "null model" in _err(L)
        assert call(m, None) == E_INVALID and "null src" in _err(L)
        # zero or more than one source
        assert call(m, S(layout=1)) == E_INVALID and "no state source" in _err(L)
        assert call(m, S(obs=p.value, env=f.env.value)) == E_INVALID and "more than one" in _err(L)
        assert call(m, S(obs=p.value, replay=f.rb.value, indices=p.value)) == E_INVALID and "more than one" in _err(L)
        assert call(m, S(env=f.env.value, replay=f.rb.value, indices=p.value)) == E_INVALID and "more than one" in _err(L)
        # indices and replay go together
        assert call(m, S(indices=p.value)) == E_INVALID and "indices without" in _err(L)
        assert call(m, S(replay=f.rb.value)) == E_INVALID and "replay without" in _err(L)
        for lay in (2, -1):
            assert call(m, S(obs=p.value, layout=lay)) == E_INVALID and "layout" in _err(L)
        for which in (2, -1):
            assert call(m, S(obs=p.value, which=which)) == E_INVALID and "which" in _err(L)
        for off in (1, 4, 8):
            assert call(m, S(obs=p.value + off)) == E_INVALID and "obs" in _err(L) and "aligned" in _err(L)
    for bad in (0, 8193):
        assert q(m, ok, n=bad) == E_INVALID and "n must be" in _err(L)
    assert q(m, ok, outs=(None, None, None)) == E_INVALID and "d_q" in _err(L) and "null" in _err(L)
    for bad in (0, 4097):
        assert train(m, ok, batch=bad) == E_INVALID and "batch" in _err(L)
    assert train(m, ok, actions=None) == E_INVALID and "d_actions" in _err(L)
    assert train(m, ok, y=None) == E_INVALID and "d_y" in _err(L)
    assert f.untouched()   # nothing wrote into the stand-ins


def test_calls_before_a_reserve_are_refused():
    """an otherwise valid call on a model that never reserved (the zeroed block): QLX_E_STATE, nothing launched"""
    import qlx
    L = qlx.lib()
    f = _Fakes()
    p = f.ptr
    for src in (qlx.StatesDev(obs=p.value, layout=0), qlx.StatesDev(obs=p.value, layout=1),
                qlx.StatesDev(replay=f.rb.value, indices=p.value, layout=1, which=1), qlx.StatesDev(env=f.env.value)):
        assert L.qlx_model_q_dev(f.m, C.byref(src), 4, p, None, None) == E_STATE and "reserve" in _err(L)
        assert L.qlx_model_q_dev(f.m, C.byref(src), 8192, None, p, p) == E_STATE and "reserve" in _err(L)
        assert L.qlx_model_train_dev(f.m, C.byref(src), p, p, None, 4, None, None) == E_STATE and "reserve" in _err(L)
        assert L.qlx_model_train_dev(f.m, C.byref(src), p, p, p, 4096, p, p) == E_STATE and "reserve" in _err(L)
    assert f.untouched()
