"""The snapshot surface without a GPU: include/qlx.h declares the seven entry points and the constants, libqlx.so exports
them, the ctypes mirror of qlx_snapshot_info has the header's size and field order, and qlx_snapshot_info_read reports
a missing file and a file that is no snapshot as QLX_E_IO with no device.  qlx_params is unchanged."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qlx.h")
LIB = os.path.join(ROOT, "q-learning_amd", "lib", "libqlx.so")

ENTRY_POINTS = ["qlx_snapshot_info_read", "qlx_learner_save", "qlx_learner_load", "qlx_replay_save", "qlx_replay_load",
                "qlx_frame_codec_roundtrip"]
CONSTANTS = dict(QLX_SNAPSHOT_VERSION=1, QLX_SNAPSHOT_LEARNER=1, QLX_SNAPSHOT_REPLAY=2, QLX_FRAME_CODEC_RAW=0,
                 QLX_FRAME_CODEC_BITMAP=1)


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _info_fields():
    body = re.search(r"typedef struct qlx_snapshot_info \{(.*?)\} qlx_snapshot_info;", _code(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [n.strip() for n in re.sub(r"^\w+\s+", "", decl).split(",")]
    return out


def test_header_declares_the_snapshot_surface():
    src = open(HEADER).read()
    assert "Snapshots (beyond the reference)" in src
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s\s+%d\b" % (name, value), src, flags=re.M), name
    code = _code()
    for n in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % n, code), n
    assert re.search(r"typedef struct qlx_snapshot_info \{", code)     # the seventh declaration: the info struct
    assert "sizeof(qlx_snapshot_info) == 504" in code
    assert "sizeof(qlx_params) == 408" in code


def test_library_exports_the_snapshot_surface():
    assert os.path.exists(LIB), "libqlx.so not built (make lib)"
    L = ctypes.CDLL(LIB)
    assert not [n for n in ENTRY_POINTS if not hasattr(L, n)]


def test_mirror_matches_the_header():
    import qlx
    assert ctypes.sizeof(qlx.SnapshotInfo) == 504
    assert ctypes.sizeof(qlx.Params) == 408
    assert [f[0] for f in qlx.SnapshotInfo._fields_] == _info_fields()
    assert qlx.SnapshotInfo.step_count.offset == 16 and qlx.SnapshotInfo.frames.offset == 64
    assert qlx.SnapshotInfo.file_bytes.offset == 88 and qlx.SnapshotInfo.params.offset == 96
    assert (qlx.SNAPSHOT_VERSION, qlx.SNAPSHOT_LEARNER, qlx.SNAPSHOT_REPLAY) == (1, 1, 2)
    assert (qlx.FRAME_CODEC_RAW, qlx.FRAME_CODEC_BITMAP) == (0, 1)
    for name in ("save", "load"):
        assert callable(getattr(qlx.SelfDrivingQLearner, name)) and callable(getattr(qlx.ReplayBuffer, name))
    assert callable(qlx.snapshot_info) and callable(qlx.frame_codec_roundtrip)


def test_info_read_reports_bad_files_without_a_device(tmp_path):
    import qlx
    with pytest.raises(qlx.QlError, match="status -6") as ei:
        qlx.snapshot_info(tmp_path / "missing.qlx")
    assert "missing.qlx" in str(ei.value)
    zeros = tmp_path / "zeros.qlx"
    zeros.write_bytes(bytes(64))
    with pytest.raises(qlx.QlError, match="magic") as ei:
        qlx.snapshot_info(zeros)
    assert "status -6" in str(ei.value)
    short = tmp_path / "short.qlx"
    short.write_bytes(b"QLXSNAP1")
    with pytest.raises(qlx.QlError, match="status -6"):
        qlx.snapshot_info(short)


def test_argument_errors_are_invalid():
    import qlx
    L = qlx.lib()
    info = qlx.SnapshotInfo()
    assert L.qlx_snapshot_info_read(None, ctypes.byref(info)) == -1
    assert L.qlx_learner_save(None, b"x") == -1 and L.qlx_replay_save(None, b"x") == -1
    h = ctypes.c_void_p()
    assert L.qlx_learner_load(None, 0, ctypes.byref(h)) == -1 and L.qlx_replay_load(None, 0, ctypes.byref(h)) == -1
