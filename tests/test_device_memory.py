"""DeviceBuffer / PinnedBuffer (q-learning_amd/csrc/device_memory.h), the owners of all device and pinned memory of the
library: ownership, moves, reserve / reset and above all the failed-allocation paths are run on the CPU
(scripts/devmem_host_check.hip, compiled host-only with AddressSanitizer and UBSan linked into the program) over
malloc / free stand-ins of the four allocation functions that count live allocations and fail on request.  No GPU
needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_buffers_own_and_fail_cleanly(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "devmem_host_check")
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-I", os.path.join(ROOT, "q-learning_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-g", "-O1", os.path.join(ROOT, "scripts", "devmem_host_check.hip"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "ok"
