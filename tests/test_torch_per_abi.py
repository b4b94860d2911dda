"""The replay's prioritized device calls (include/qlx.h "Prioritized replay on device tensors") without a GPU:
the names are declared and exported, the header still compiles as C11 and C++17, every host argument check fails with
QLX_E_INVALID and names its field before any device is needed, priorities not enabled is QLX_E_STATE after those checks, and
the numpy restatement's tree total is the oracle sampler's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import per_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")

NEW = ["qlx_replay_per_enable", "qlx_replay_per_sample_dev", "qlx_replay_per_update_dev", "qlx_replay_per_get"]
E_INVALID, E_STATE = -1, -4


def test_new_names_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qlx_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    dyn = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NEW:
        assert n in declared, n
        assert n in dyn, n


def test_header_compiles_as_cxx_and_c(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cxx and cc, "no host compiler"
    call = ("qlx_replay_per_enable(0); qlx_replay_per_sample_dev(0, 1, 0, 0, 4, 0.4f, 0, 0); "
            "qlx_replay_per_update_dev(0, 0, 0, 0, 0.6f, 1e-6f); return qlx_replay_per_get(0, 0, 0, 0, 0, 0, 0);")
    (tmp_path / "t.cpp").write_text('#include "qlx.h"\nint f() { ' + call + " }\n")
    (tmp_path / "t.c").write_text('#include "qlx.h"\nint f(void) { ' + call + " }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / "t.cpp")], check=True)
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / "t.c")], check=True)


def _err(L):
    L.qlx_last_error.restype = C.c_char_p
    return L.qlx_last_error().decode()


def test_argument_errors_need_no_device():
    """Every check below is made before anything of the device is touched, so a block of zero bytes can stand in for a
    replay: it reads as an empty replay (len 0) without priorities."""
    import qlx
    L = qlx.lib()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    idx, w, td = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)   # never dereferenced: the calls fail first
    f = C.c_float
    nan, inf = float("nan"), float("inf")

    assert L.qlx_replay_per_enable(None) == E_INVALID and "null replay" in _err(L)

    assert L.qlx_replay_per_sample_dev(None, 1, 0, 0, 4, f(0.4), idx, w) == E_INVALID and "null replay" in _err(L)
    assert L.qlx_replay_per_sample_dev(h, 1, 0, 0, 4, f(0.4), None, w) == E_INVALID and "d_out_indices" in _err(L)
    for bad in (0, 4097):
        assert L.qlx_replay_per_sample_dev(h, 1, 0, 0, bad, f(0.4), idx, w) == E_INVALID and "batch" in _err(L)
    for bad in (nan, inf, -inf, -0.5):
        assert L.qlx_replay_per_sample_dev(h, 1, 0, 0, 4, f(bad), idx, w) == E_INVALID and "beta" in _err(L)
    # a zeroed replay holds nothing: len == 0, with and without the optional weights
    assert L.qlx_replay_per_sample_dev(h, 1, 0, 0, 4, f(0.4), idx, w) == E_INVALID and "len" in _err(L)
    assert L.qlx_replay_per_sample_dev(h, 1, 0, 0, 4, f(0.0), idx, None) == E_INVALID and "len" in _err(L)

    assert L.qlx_replay_per_update_dev(None, idx, td, 4, f(0.6), f(1e-6)) == E_INVALID and "null replay" in _err(L)
    assert L.qlx_replay_per_update_dev(h, idx, td, 4097, f(0.6), f(1e-6)) == E_INVALID and "n must" in _err(L)
    assert L.qlx_replay_per_update_dev(h, None, td, 4, f(0.6), f(1e-6)) == E_INVALID and "d_indices" in _err(L)
    assert L.qlx_replay_per_update_dev(h, idx, None, 4, f(0.6), f(1e-6)) == E_INVALID and "d_td_abs" in _err(L)
    for bad in (nan, inf, -inf, -0.1):
        assert L.qlx_replay_per_update_dev(h, idx, td, 4, f(bad), f(1e-6)) == E_INVALID and "alpha" in _err(L)
    for bad in (nan, inf, -inf, -1e-6, 0.0):
        assert L.qlx_replay_per_update_dev(h, idx, td, 4, f(0.6), f(bad)) == E_INVALID and "eps" in _err(L)

    assert L.qlx_replay_per_get(None, None, None, None, None, None, None) == E_INVALID and "null replay" in _err(L)

    # priorities not enabled: after the argument checks, still without a device
    assert L.qlx_replay_per_update_dev(h, idx, td, 4, f(0.6), f(1e-6)) == E_STATE and "not enabled" in _err(L)
    assert L.qlx_replay_per_update_dev(h, None, None, 0, f(0.6), f(1e-6)) == E_STATE and "not enabled" in _err(L)
    assert L.qlx_replay_per_update_dev(h, idx, td, 4, f(0.0), f(1e-6)) == E_STATE   # alpha 0 is allowed
    total = C.c_float()
    assert L.qlx_replay_per_get(h, None, None, None, C.byref(total), None, None) == E_STATE and "not enabled" in _err(L)
    assert bytes(fake) == bytes(4096)   # nothing wrote into the stand-in


def test_python_methods_exist():
    import qlx
    for m in ("per_enable", "per_sample_dev", "per_update_dev", "per_get"):
        assert callable(getattr(qlx.ReplayBuffer, m))


@pytest.mark.parametrize("cap", [1, 2, 3, 100, 2049, 5000])
def test_restatement_tree_total_is_the_oracle_samplers(cap):
    rng = np.random.default_rng(cap)
    leaves = ((rng.gamma(0.4, 1.0, cap) + 1e-6).astype(np.float32) ** np.float32(0.6)).astype(np.float32)
    t = P.build_tree(leaves)
    L = P.leaves_pow2(cap)
    assert t.shape == (2 * L,) and np.array_equal(t[L:L + cap], leaves) and not t[L + cap:].any()
    _, _, total = O.per_sample(leaves, 1, 0, 1, 0, cap, 0.4, 1)
    assert t[1] == np.float32(total) if L > 1 else t[1] == leaves[0]


def test_restatement_push_update_and_mapping():
    ref = P.PerRef(5, total=3)
    assert ref.len == 3 and ref.start == 0 and ref.leaves.tolist() == [1, 1, 1, 0, 0]
    bad = ref.update([0, 2, 0], np.array([3.0, 1.0, 0.5], np.float32), 0.6, 1e-6)
    pr = O.det_powf(np.array([3.0, 1.0, 0.5], np.float32) + np.float32(1e-6), 0.6)
    assert not bad and ref.leaves[0] == pr[2] and ref.leaves[2] == pr[1] and ref.per_max == pr[0]   # the last writer wins
    ref.push(4)   # slots 3, 4, 0, 1 at per_max; the ring has wrapped
    assert ref.len == 5 and ref.start == 2 and (ref.leaves[[3, 4, 0, 1]] == pr[0]).all() and ref.leaves[2] == pr[1]
    assert ref.to_physical([0, 1, 4]).tolist() == [2, 3, 1] and ref.to_logical([2, 3, 1]).tolist() == [0, 1, 4]
    before, pmax = ref.leaves.copy(), ref.per_max
    with np.errstate(invalid="ignore"):
        bad = ref.update([5, -1, 0, 1, 2, 3], np.array([1, 1, np.nan, np.inf, -1, 9], np.float32), 0.6, 1e-6)
    assert bad and ref.leaves[ref.to_physical([3])[0]] == O.det_powf(np.float32(9) + np.float32(1e-6), 0.6)[()]
    keep = np.ones(5, bool)
    keep[ref.to_physical([3])[0]] = False
    assert np.array_equal(ref.leaves[keep], before[keep]) and ref.per_max > pmax
    t = ref.tree()
    assert all(t[i] == np.float32(t[2 * i] + t[2 * i + 1]) for i in range(1, 8))
