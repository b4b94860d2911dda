"""The snapshot container and the host reference of the bitmap frame codec (q-learning_amd/csrc/snapshot_format.cpp, host
code with no HIP call) on the CPU: scripts/snapshot_host_check.cpp, a program of its own compiled host-only with
AddressSanitizer and UBSan linked in, writes a small container with both frame codecs, reads it back equal and must get a
clean error, and no sanitizer report, for truncated and corrupted copies.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_container_and_codec_reject_bad_files_cleanly(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "snapshot_host_check")
    csrc = os.path.join(ROOT, "q-learning_amd", "csrc")
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    os.path.join(ROOT, "scripts", "snapshot_host_check.cpp"), os.path.join(csrc, "snapshot_format.cpp"),
                    "-o", exe], check=True, capture_output=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "ok"
