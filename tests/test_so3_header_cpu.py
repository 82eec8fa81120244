"""pl-viwo_amd/csrc/so3.hpp — the one copy of the 3x3 / SO(3) / JPL-quaternion arithmetic that host code and kernels share — compiled as
plain C++ with g++ (no HIP headers, no GPU) and held to bits recorded before the header existed.

tests/golden/so3_bits.json holds a few hundred inputs with the outputs of the copies the header replaced (the Jacobian kernels'
prelude, the between-frame kernels' helper header, the evaluator's and the initialisers' local helpers), as hex doubles.  Inputs: random
cases, rotation angles 0, 1e-8, 1e-7, 1e-6 and pi - 1e-9, rotations by exactly pi about axes that reach each of log_so3's three
branches (trace + 1 < 1e-10), quaternions with w < 0, w = 0 and each component dominant (rot_2_quat's four branches), dth = 0.
  * quat_2_Rot, rot_2_quat, quat_multiply, quatnorm, omega_times, jpl_left_update, inv3, mm, mv use + - * / sqrt only: IEEE fixes their
    results, so tests/host/so3_check.cpp must reproduce every recorded bit (built -ffp-contract=off, like the library).
  * exp_so3, log_so3 and Jl_so3 call the host's sin / cos / acos; the fixture holds them on the branches that call none.  On the
    general branch the program asserts exp_so3(log_so3(R)) == R and log_so3(exp_so3(w)) == w to 1e-12, for angles in [0.01, 2.5] rad:
    there acos((tr - 1) / 2) turns one ulp of the trace into at most 1.1e-16 / sin(0.01) ~ 1e-14 rad and theta / (2 sin theta) is far
    from its pole at pi, so 1e-12 leaves two orders of magnitude over the rounding of a correct implementation.
  * exp_and_Jl equals exp_so3 and Jl_so3 bit for bit (same libm calls, same order), at every input above.
  * Host / device twin: the chained line launch needs the library's plv_jpl_left_update (host) and the function the kernel calls to form
    the same bits.  Both are so3.hpp's jpl_left_update now; the test calls the library on the fixture's inputs and compares with what
    the g++ program printed, and with the fixture."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "so3_check.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "so3_bits.json")


def bits(values):
    return [struct.pack("<d", float(v)) for v in values]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("so3") / "so3_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=120)
    return r


def test_header_reproduces_the_recorded_bits(check_output):
    r = check_output
    tail = "\n".join(line for line in r.stdout.split("\n") if not line.startswith("jpl "))[-3000:]
    assert r.returncode == 0 and "ok: " in r.stdout, (tail, r.stderr[-2000:])
    records = json.load(open(FIXTURE))
    assert f"ok: {len(records)} records reproduced bit for bit" in r.stdout, tail
    # the fixture covers what it claims to
    fns = {rec["fn"] for rec in records}
    assert fns == {"quat_2_Rot", "rot_2_quat", "quat_multiply", "quatnorm", "omega_times", "jpl_left_update", "inv3", "mm", "mv", "exp_so3", "log_so3", "Jl_so3"}
    quats = [[float.fromhex(v) for v in rec["in"]] for rec in records if rec["fn"] == "quat_2_Rot"]
    assert any(q[3] < 0 for q in quats) and any(q[3] == 0 for q in quats)
    assert all(any(abs(q[k]) == max(map(abs, q)) for q in quats) for k in range(4))
    dths = [[float.fromhex(v) for v in rec["in"][4:]] for rec in records if rec["fn"] == "jpl_left_update"]
    assert any(d == [0, 0, 0] for d in dths) and any(d != [0, 0, 0] for d in dths)
    logs = [np.array([float.fromhex(v) for v in rec["in"]]).reshape(3, 3) for rec in records if rec["fn"] == "log_so3"]
    near_pi = [R for R in logs if np.trace(R) + 1.0 < 1e-10]
    assert any(abs(R[2, 2] + 1) > 1e-5 for R in near_pi)
    assert any(abs(R[2, 2] + 1) <= 1e-5 and abs(R[1, 1] + 1) > 1e-5 for R in near_pi)
    assert any(abs(R[2, 2] + 1) <= 1e-5 and abs(R[1, 1] + 1) <= 1e-5 for R in near_pi)


def test_host_update_and_the_kernels_function_are_one(check_output):
    r = check_output
    assert r.returncode == 0, r.stdout[-2000:]
    printed = [[float.fromhex(v) for v in line.split()[1:]] for line in r.stdout.split("\n") if line.startswith("jpl ")]
    records = [rec for rec in json.load(open(FIXTURE)) if rec["fn"] == "jpl_left_update"]
    assert len(printed) == len(records) > 50
    pkg = ge.load_pkg()
    # one call per record, and all of them as one stack
    Q = np.array([[float.fromhex(v) for v in rec["in"][:4]] for rec in records])
    D = np.array([[float.fromhex(v) for v in rec["in"][4:]] for rec in records])
    Qs, Rs = Q.copy(), np.zeros((len(records), 9))
    pkg.jpl_left_update(Qs, D, Rs)
    for i, rec in enumerate(records):
        q, R = Q[i:i + 1].copy(), np.zeros((1, 9))
        pkg.jpl_left_update(q, D[i:i + 1], R)
        got = bits(q[0]) + bits(R[0])
        assert got == bits(printed[i]), (i, rec["in"])
        assert got == bits(float.fromhex(v) for v in rec["out"]), (i, rec["in"])
        assert got == bits(Qs[i]) + bits(Rs[i]), i
