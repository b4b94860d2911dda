"""The training-metrics surface without a GPU: include/qlx.h declares the six learner entry points and
qlx_metrics_td_bin, libqlx.so exports them, the ctypes mirror and the numpy dtype of qlx_update_metrics have the header's
size, field order and offsets, the host bin function agrees with a frexp restatement at every edge, and a learner still
cannot be created without a device (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")

LEARNER_ENTRY_POINTS = [p + s for p in ("qlx_learner_metrics_", "qlx_bg_learner_metrics_") for s in ("enable", "info", "read")]
ENTRY_POINTS = LEARNER_ENTRY_POINTS + ["qlx_metrics_td_bin"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _row_fields():
    """(name, length) of every member of qlx_update_metrics in header order (length 1 for scalars)"""
    body = re.search(r"typedef struct qlx_update_metrics \{(.*?)\} qlx_update_metrics;", _code(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for n in re.sub(r"^\w+\s+", "", decl).split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
            out.append((m.group(1), int(m.group(2) or 1)))
    return out


def test_header_declares_the_metrics_surface():
    code = _code()
    for n in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % n, code), n
    assert re.search(r"typedef struct qlx_update_metrics \{", code)
    assert "sizeof(qlx_update_metrics) == 256" in code
    assert "sizeof(qlx_params) == 408" in code


def test_library_exports_the_metrics_surface():
    assert os.path.exists(LIB), "libqlx.so not built (make lib)"
    L = ctypes.CDLL(LIB)
    assert not [n for n in ENTRY_POINTS if not hasattr(L, n)]


def test_mirrors_match_the_header():
    import qlx
    assert ctypes.sizeof(qlx.UpdateMetrics) == 256 and qlx.UPDATE_METRICS_DTYPE.itemsize == 256
    assert ctypes.sizeof(qlx.Params) == 408
    fields = _row_fields()
    assert [f[0] for f in qlx.UpdateMetrics._fields_] == [n for n, _ in fields]
    assert list(qlx.UPDATE_METRICS_DTYPE.names) == [n for n, _ in fields]
    for name, length in fields:
        c = getattr(qlx.UpdateMetrics, name)
        np_type, np_off = qlx.UPDATE_METRICS_DTYPE.fields[name][:2]
        assert c.offset == np_off and c.size == np_type.itemsize, name
        assert (np_type.shape or (1,)) == (length,), name
    assert qlx.UpdateMetrics.loss.offset == 40 and qlx.UpdateMetrics.argmax_counts.offset == 96
    assert qlx.UpdateMetrics.grad_norm.offset == 128 and qlx.UpdateMetrics.td_hist.offset == 192
    for cls in (qlx.SelfDrivingQLearner, qlx.BallGameLearner):
        for name in ("metrics_enable", "metrics_info", "metrics"):
            assert callable(getattr(cls, name))


def _bin_restated(x):
    """bin 0: |td| < 2^-11; bin k = 1..14: 2^(k-12) <= |td| < 2^(k-11); bin 15: >= 8, inf, NaN"""
    x = np.float32(x)
    if not np.isfinite(x):
        return 15
    if x == 0:
        return 0
    _, e = np.frexp(x)   # x = m * 2^e, m in [0.5, 1): 2^(e-1) <= x < 2^e
    return int(min(max(int(e) + 11, 0), 15))


def test_td_bin_matches_a_frexp_restatement():
    import qlx
    f = np.float32
    edges = [f(0), f(1e-45), np.nextafter(f(2.0 ** -11), f(0)), f(2.0 ** -11), f(1.0), np.nextafter(f(8), f(0)), f(8),
             f(np.inf), f(np.nan)]
    assert [qlx.metrics_td_bin(x) for x in edges] == [0, 0, 0, 1, 12, 14, 15, 15, 15]
    more = [f(2.0 ** k) for k in range(-14, 6)] + [np.nextafter(f(2.0 ** k), f(0)) for k in range(-14, 6)] + [f(1.5), f(0.3)]
    for x in edges + more:
        assert qlx.metrics_td_bin(x) == _bin_restated(x), float(x)


def test_null_arguments_are_invalid():
    import qlx
    L = qlx.lib()
    n = ctypes.c_uint64()
    row = qlx.UpdateMetrics()
    for prefix in ("qlx_learner", "qlx_bg_learner"):
        assert getattr(L, prefix + "_metrics_enable")(None, 4) == -1
        assert getattr(L, prefix + "_metrics_info")(None, None, None, None) == -1
        assert getattr(L, prefix + "_metrics_read")(None, ctypes.byref(row), 1, ctypes.byref(n), ctypes.byref(n)) == -1


def test_no_cpu_fallback():
    """Without a GPU a learner cannot be created (QlError), as before; with one, metrics are off until enabled and
    reading them is a state error - either way nothing is computed on the host."""
    import torch
    import qlx
    p = qlx.Parameter(n_envs=16, batch_size=32, history_buffer_len=1000)
    if not torch.cuda.is_available():
        with pytest.raises(qlx.QlError):
            qlx.SelfDrivingQLearner(p)
        with pytest.raises(qlx.QlError):
            qlx.BallGameLearner(p)
        return
    L = qlx.SelfDrivingQLearner(p)
    with pytest.raises(qlx.QlError, match="status -4"):
        L.metrics_info()
    with pytest.raises(qlx.QlError, match="status -4"):
        L.metrics()
