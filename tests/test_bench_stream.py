"""bench.py's stream: a plain run renders and plays the frames up to the end of its timed segment only, on the drive a --full run
plays (same IMU and wheel streams, same messages and images up to the last frame it plays).  Runs in a fresh interpreter: the
stream sets the renderer's camera and mount module-wide."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check():
    sys.path.insert(0, ROOT)
    import bench

    wl = bench.WORKLOADS["C"]
    full = bench.build_stream(wl, 12, 1)
    plain = bench.build_stream(wl, 12, 1, n_render=4)
    assert len(full["imgs"]) == 12 and len(plain["imgs"]) == 4
    np.testing.assert_array_equal(plain["imu"], full["imu"])
    np.testing.assert_array_equal(plain["wheel"], full["wheel"])
    cams = [m for m in plain["msgs"] if m[1] == bench.CAM]
    assert [m[2] for m in cams] == [0, 1, 2, 3]
    last = plain["msgs"].index(cams[-1])
    assert plain["msgs"][:last + 1] == full["msgs"][:last + 1]
    for a, b in zip(plain["imgs"], full["imgs"]):
        np.testing.assert_array_equal(a, b)


def test_plain_run_plays_the_first_frames_of_the_full_drive():
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]


if __name__ == "__main__":
    check()
