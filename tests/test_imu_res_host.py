"""use_imu_res on the host, without a GPU: which observations the CPI table serves (cpi_servable) and what cpi_attach makes of a pool
(pl-viwo_amd/csrc/camera_tracks.hpp), as a stand-alone program under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpi_validity_and_attach_under_sanitizers(tmp_path):
    """tests/host_sanitize/cpi_attach_check.cpp: every kind of query time against a hand-made table (stored record, between records of
    one clone, between the records of two clones, before the first and beyond the last record, records of a clone that left the
    window), then point and line pools through cpi_attach with and without covariances — every view ends in the pool or in what
    returns to the database, in order, and every kept one carries the index of its own time; tables plv_cpi_poses refuses are refused
    with the pool untouched."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cpi_attach_check")
    src = os.path.join(ROOT, "tests", "host_sanitize", "cpi_attach_check.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert r.returncode == 0 and "ok: the table's misses leave the pool" in r.stdout, (r.stdout[-3000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
