"""The device-tensor env / replay calls (include/qlx.h) without a GPU: the names are declared and exported,
the header still compiles as C++, argument errors are found on the host before any device is needed, qlx_torch keeps one
HIP runtime in the process, and the numpy restatement of NCHW_TIME agrees with the oracle env."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import obs_layout_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")
PKG = os.path.join(ROOT, "q-learning_amd")

NEW = ["qlx_env_stream", "qlx_replay_stream", "qlx_replay_share_stream", "qlx_replay_sync", "qlx_env_obs_dev",
       "qlx_env_reset_dev", "qlx_replay_sample_distinct_dev", "qlx_replay_batch_dev"]
E_INVALID = -1


def test_new_names_declared_and_exported():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(qlx_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    dyn = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NEW:
        assert n in declared, n
        assert n in dyn, n
    assert re.search(r"#define\s+QLX_OBS_NHWC_SLOT\s+0\b", src) and re.search(r"#define\s+QLX_OBS_NCHW_TIME\s+1\b", src)
    assert "qlx_batch_dev" in src


def test_header_compiles_as_cxx_and_c(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cxx and cc, "no host compiler"
    body = '#include "qlx.h"\n'
    (tmp_path / "t.cpp").write_text(body + 'static_assert(sizeof(qlx_batch_dev) == 8 * sizeof(void*), "eight pointers");\n'
                                    "int main() { qlx_batch_dev b = {}; return b.s != nullptr; }\n")
    (tmp_path / "t.c").write_text(body + "int main(void) { qlx_batch_dev b = {0}; return b.steps != 0; }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / "t.cpp")], check=True)
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / "t.c")], check=True)


def test_ctypes_struct_matches_header():
    import qlx
    assert C.sizeof(qlx.BatchDev) == 64
    assert [k for k, _ in qlx.BatchDev._fields_] == ["s", "s_next", "actions", "returns", "discounts", "terminals",
                                                    "last_indices", "steps"]
    assert (qlx.OBS_NHWC_SLOT, qlx.OBS_NCHW_TIME) == (0, 1)


def _err(L):
    L.qlx_last_error.restype = C.c_char_p
    return L.qlx_last_error().decode()


def test_argument_errors_need_no_device():
    """Every check below fails before the handle is read, so a block of zero bytes can stand in for one."""
    import qlx
    L = qlx.lib()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    p = C.c_void_p()
    o = qlx.BatchDev()
    idx = C.c_void_p(0x1000)   # never dereferenced: the calls fail first
    ok_state = 0x10000
    assert L.qlx_env_stream(None, C.byref(p)) == E_INVALID and "null env" in _err(L)
    assert L.qlx_env_stream(h, None) == E_INVALID and "hip_stream_out" in _err(L)
    assert L.qlx_replay_stream(None, C.byref(p)) == E_INVALID
    assert L.qlx_replay_share_stream(None, h) == E_INVALID and "null replay" in _err(L)
    assert L.qlx_replay_share_stream(h, None) == E_INVALID and "null env" in _err(L)
    assert L.qlx_replay_sync(None) == E_INVALID
    assert L.qlx_env_obs_dev(None, 0, ok_state) == E_INVALID
    assert L.qlx_env_obs_dev(h, 0, None) == E_INVALID and "d_out" in _err(L)
    assert L.qlx_env_obs_dev(h, 2, ok_state) == E_INVALID and "layout" in _err(L)
    assert L.qlx_env_obs_dev(h, -1, ok_state) == E_INVALID and "layout" in _err(L)
    assert L.qlx_env_obs_dev(h, 1, ok_state + 4) == E_INVALID and "aligned" in _err(L)
    assert L.qlx_env_reset_dev(None, None) == E_INVALID
    assert L.qlx_replay_sample_distinct_dev(None, 1, 0, 0, 4, idx) == E_INVALID
    assert L.qlx_replay_sample_distinct_dev(h, 1, 0, 0, 4, None) == E_INVALID and "d_out_indices" in _err(L)
    for bad in (0, 4097):
        assert L.qlx_replay_sample_distinct_dev(h, 1, 0, 0, bad, idx) == E_INVALID and "batch" in _err(L)
    # a zeroed replay holds nothing: batch > len, still without a device
    assert L.qlx_replay_sample_distinct_dev(h, 1, 0, 0, 4, idx) == E_INVALID and "len" in _err(L)
    gamma = C.c_float(0.99)
    assert L.qlx_replay_batch_dev(None, idx, 4, 1, gamma, 1, C.byref(o)) == E_INVALID and "null replay" in _err(L)
    assert L.qlx_replay_batch_dev(h, idx, 4, 1, gamma, 1, None) == E_INVALID and "null out" in _err(L)
    assert L.qlx_replay_batch_dev(h, None, 4, 1, gamma, 1, C.byref(o)) == E_INVALID and "d_indices" in _err(L)
    assert L.qlx_replay_batch_dev(h, idx, 4, 1, gamma, 2, C.byref(o)) == E_INVALID and "layout" in _err(L)
    for bad in (0, 4097):
        assert L.qlx_replay_batch_dev(h, idx, bad, 1, gamma, 1, C.byref(o)) == E_INVALID and "batch" in _err(L)
    for bad in (0, 33):
        assert L.qlx_replay_batch_dev(h, idx, 4, bad, gamma, 1, C.byref(o)) == E_INVALID and "n_step" in _err(L)
    o.s = ok_state + 8
    assert L.qlx_replay_batch_dev(h, idx, 4, 1, gamma, 0, C.byref(o)) == E_INVALID and "out->s " in _err(L)
    o.s, o.s_next = ok_state, ok_state + 1
    assert L.qlx_replay_batch_dev(h, idx, 4, 1, gamma, 0, C.byref(o)) == E_INVALID and "out->s_next" in _err(L)
    assert bytes(fake) == bytes(4096)   # nothing wrote into the stand-in


def _child(code):
    return subprocess.run([sys.executable, "-c", code, PKG], capture_output=True, text=True, timeout=240)


def test_qlx_torch_first_keeps_one_hip_runtime():
    r = _child("import sys; sys.path.insert(0, sys.argv[1])\n"
               "import qlx_torch\n"
               "rts = qlx_torch.mapped_hip_runtimes()\n"
               "maps = open('/proc/self/maps').read()\n"
               "assert 'libqlx.so' in maps\n"
               "print(len(rts))\n")
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-1] == "1", r.stdout


def test_qlx_before_qlx_torch_is_refused():
    r = _child("import sys; sys.path.insert(0, sys.argv[1])\n"
               "import qlx\n"
               "qlx.lib()\n"
               "try:\n"
               "    import qlx_torch\n"
               "except qlx.QlError as e:\n"
               "    print('QlError:', e)\n"
               "else:\n"
               "    print('imported')\n")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "QlError:" in r.stdout and "qlx_torch must be imported before any other use of qlx" in r.stdout, r.stdout


@pytest.fixture(scope="module")
def oracle_walk():
    """one oracle env stepped 9 times: after each step its tensor view, next_slot and the frame that step drew"""
    import oracle as O
    env = O.Env(0x51A5EED, 0)
    rows = [(env.tensor(), int(env.state()["next_slot"]), None)]
    for t in range(1, 10):
        env.step(t % 3)
        ns = int(env.state()["next_slot"])
        rows.append((env.tensor(), ns, env.frame((ns + 3) & 3).T.copy()))   # the oracle keeps frames [y][x]
    return rows


@pytest.mark.parametrize("steps", [1, 2, 5, 9])
def test_restatement_against_oracle_env(oracle_walk, steps):
    tensor, ns, drawn = oracle_walk[steps]
    assert ns == steps & 3
    got = R.env_nchw_time(tensor[None], [ns])[0]
    assert got.shape == (4, 84, 84) and got.dtype == np.uint8
    assert drawn.any() and np.array_equal(got[3], drawn), "the newest channel is the frame the last step drew"
    for c in range(4):
        m = steps - 3 + c   # the episode step channel c shows
        if m < 1:
            assert not got[c].any(), f"channel {c} is older than the episode"
        else:
            assert np.array_equal(got[c], oracle_walk[m][2]), f"channel {c} is the frame of step {m}"
    # the replay's two definitions over the same ring: s' of the transition of step k is the env's state after k steps,
    # s is its state after k - 1
    assert np.array_equal(R.replay_nchw_time(tensor[None], [steps], True)[0], got)
    prev, pns, _ = oracle_walk[steps - 1]
    # s is read from the ring as it stands after step k, minus the newest frame: compare with the state one step earlier
    s = R.env_nchw_time(prev[None], [pns])[0]
    assert np.array_equal(s[1:], got[:3])


def test_restatement_is_a_permutation_of_slots():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (6, 84, 84, 4), dtype=np.uint8)
    first = np.array([0, 1, 2, 3, 5, -1])
    y = R.nchw_time(x, first)
    for i in range(6):
        for c in range(4):
            assert np.array_equal(y[i, c], x[i, :, :, (first[i] + c) & 3])
