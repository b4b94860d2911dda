"""The policy-evaluation surface without a GPU: include/qlx.h declares the six entry points and QLX_EVAL_MAX_ENVS,
libqlx.so exports them, the ctypes mirrors have the header's sizes and field order, an invalid config is refused with
the field named before any device is touched, and a valid one reports the missing device.  qlx_params is unchanged."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")

ENTRY_POINTS = ["qlx_evaluator_create", "qlx_evaluator_destroy", "qlx_evaluator_run", "qlx_evaluator_episodes",
                "qlx_evaluator_env", "qlx_learner_evaluate"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _code(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = re.sub(r"^\w+\s+", "", decl)   # drop the type: "a, b, c" or "action_counts[3]"
        out += [re.sub(r"\[\d+\]", "", n).strip() for n in names.split(",")]
    return out


def test_header_declares_the_evaluator():
    src = open(HEADER).read()
    assert "Policy evaluation (beyond the reference)" in src
    assert re.search(r"^#define QLX_EVAL_MAX_ENVS 8192\b", src, flags=re.M)
    code = _code()
    for n in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % n, code), n
    assert "sizeof(qlx_eval_config) == 48" in code and "sizeof(qlx_eval_summary) == 96" in code
    assert "sizeof(qlx_params) == 408" in code


def test_library_exports_the_evaluator():
    assert os.path.exists(LIB), "libqlx.so not built (make lib)"
    L = ctypes.CDLL(LIB)
    assert not [n for n in ENTRY_POINTS if not hasattr(L, n)]


def test_mirrors_match_the_header():
    import qlx
    assert ctypes.sizeof(qlx.EvalConfig) == 48 and ctypes.sizeof(qlx.EvalSummary) == 96
    assert [f[0] for f in qlx.EvalConfig._fields_] == _struct_fields("qlx_eval_config")
    assert [f[0] for f in qlx.EvalSummary._fields_] == _struct_fields("qlx_eval_summary")
    offs = {k: getattr(qlx.EvalConfig, k).offset for k, _ in qlx.EvalConfig._fields_}
    assert offs == dict(n_envs=0, episodes_per_env=4, max_steps_per_episode=8, epsilon=16, env_seed=24, policy_seed=32,
                        poll_steps=40, flags=44)
    offs = {k: getattr(qlx.EvalSummary, k).offset for k, _ in qlx.EvalSummary._fields_}
    assert offs == dict(episodes=0, env_steps=8, vector_steps=16, forward_samples=24, terminal_episodes=32,
                        action_counts=40, mean_return=64, mean_length=72, mean_max_q=80, min_return=88, max_return=92)
    assert qlx.EVAL_MAX_ENVS == 8192
    assert ctypes.sizeof(qlx.Params) == 408
    assert callable(qlx.SelfDrivingQLearner.evaluate)


@pytest.mark.parametrize("kw, field", [
    (dict(n_envs=0), "n_envs"), (dict(n_envs=8193), "n_envs"),
    (dict(n_envs=4, episodes_per_env=0), "episodes_per_env"),
    (dict(n_envs=4, max_steps_per_episode=0), "max_steps_per_episode"),
    (dict(n_envs=4, epsilon=-0.1), "epsilon"), (dict(n_envs=4, epsilon=1.5), "epsilon"),
    (dict(n_envs=4, epsilon=float("nan")), "epsilon"),
    (dict(n_envs=4, flags=1), "flags"),
    (dict(n_envs=8192, episodes_per_env=2049), "episodes_per_env"),   # n_envs * K above 1 << 24
])
def test_invalid_config_names_the_field(kw, field):
    """argument errors come before the device is touched, so they read the same with and without a GPU"""
    import qlx
    with pytest.raises(qlx.QlError, match=field) as ei:
        qlx.Evaluator(**kw)
    assert "status -1" in str(ei.value)   # QLX_E_INVALID


def test_valid_config_without_gpu_reports_the_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the device path is covered by the -m gpu tests")
    import qlx
    with pytest.raises(qlx.QlError, match="device"):
        qlx.Evaluator(4)
