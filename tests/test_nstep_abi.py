"""The n-step return surface without a GPU: include/qlx.h declares qlx_replay_nstep and QLX_NSTEP_MAX, libqlx.so exports
the entry point, and qlx_params / qlx.Params carry n_step in what was tail padding (the ABI size stays 408)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")


def _header():
    return open(HEADER).read()


def test_header_declares_nstep():
    src = _header()
    assert re.search(r"^#define QLX_NSTEP_MAX 32\s*$", src, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint32_t\s+qlx_replay_nstep\s*\(", code)
    body = re.search(r"typedef struct qlx_params \{(.*?)\} qlx_params;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\d+\])?;", body)
    assert fields[-1] == "n_step" and fields[-2] == "episode_reward_goal", fields[-3:]
    assert "sizeof(qlx_params) == 408" in code


def test_library_exports_nstep():
    assert os.path.exists(LIB), "libqlx.so not built (make lib)"
    assert hasattr(ctypes.CDLL(LIB), "qlx_replay_nstep")


def test_params_mirror():
    import qlx
    names = [f[0] for f in qlx.Params._fields_]
    assert names[-1] == "n_step"
    assert ctypes.sizeof(qlx.Params) == 408
    assert qlx.Params.n_step.offset == 404 and qlx.Params.episode_reward_goal.offset == 400
    assert qlx.Parameter().n_step == 1
    assert qlx.Parameter(n_step=3).n_step == 3
    assert qlx.Params().n_step == 0   # a zero-filled struct selects the 1-step target
    assert qlx.NSTEP_MAX == 32


def test_params_default_reads_zero():
    import qlx
    p = qlx.Params()
    p.n_step = 7
    qlx.lib().qlx_params_default(ctypes.byref(p))
    assert p.n_step == 0
    assert callable(qlx.ReplayBuffer.nstep)
