"""plv_traj_rpe, plv_traj_nees and plv_traj_ate_2d on the GPU, through the C ABI, against the numpy restatement of the
reference's routines (tests/eval_metrics_ref.py, itself checked against closed forms in tests/test_eval_metrics_cpu.py).

Tolerances are tests/test_gpu_eval.py's for the same arithmetic: 1e-10 on position errors and their statistics, 1e-8 degrees on
orientation errors; the NEES, a quadratic form over the inverse of a well-conditioned 3x3, a relative 1e-9.  End indices are
compared as integers, everywhere, with no case left out."""
import ctypes as C
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import eval_oracle as eo  # noqa: E402
import eval_metrics_ref as em  # noqa: E402

pytestmark = pytest.mark.gpu
METHODS = ("posyaw", "posyawsingle", "se3", "se3single", "sim3", "none")
POS_TOL, ORI_TOL, NEES_RTOL = 1e-10, 1e-8, 1e-9
# The NEES bound is relative, and a relative bound says nothing about a value that is itself rounding noise: the single-pose
# alignments map pose 0 of the ground truth onto pose 0 of the estimate exactly, so its errors are a few 1e-17 and its NEES a few
# 1e-34 (orientation) and 1e-31 (position) on the toy fixture, where the library and numpy measured 6.7e-3 apart, relatively.
# A perturbation d of an error near zero moves e^T P^-1 e by d^2 / lambda_min(P): with d = 1e-15 (tens of ulps of a rotation
# matrix entry) and lambda_min >= 5e-4 (the covariances drawn below) that is 2e-27.  NEES_ATOL = 1e-20 covers it with room and is
# twenty orders below any NEES one would read.
NEES_ATOL = 1e-20


def _nees_close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool((np.abs(got - ref) <= NEES_RTOL * np.abs(ref) + NEES_ATOL).all())


def _toy():
    with open(os.path.join(ROOT, "tests", "golden", "ate_toy.json")) as f:
        d = json.load(f)
    return d, np.array(d["gt"]), np.array(d["est"])


def _stats_close(got, ref, tol, what):
    for k, v in ref.items():
        if k in ("std", "ninetynine") and math.isnan(v):   # one valid value: the reference divides by n - 1
            assert math.isnan(got[k]), (what, k, got[k])
        else:
            assert abs(got[k] - v) < tol, (what, k, got[k], v)


def _check_rpe(got, ref, what):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        w = (what, r["length"])
        assert np.array_equal(g["end_idx"], r["end_idx"]), (w, np.flatnonzero(g["end_idx"] != r["end_idx"])[:10])
        ok = r["end_idx"] >= 0
        assert g["n"] == r["n"] == int(ok.sum()), w
        assert np.isnan(g["pos_err"][~ok]).all() and np.isnan(g["ori_err"][~ok]).all(), w   # untouched where there is no segment
        if ok.any():
            dp, do = np.abs(g["pos_err"][ok] - r["pos_err"][ok]).max(), np.abs(g["ori_err"][ok] - r["ori_err"][ok]).max()
            print(f"rpe {what} L={r['length']:g}: n={r['n']} max |pos diff| {dp:.3e} m, max |ori diff| {do:.3e} deg")
            assert dp < POS_TOL and do < ORI_TOL, (w, dp, do)
        _stats_close(g["pos"], r["pos"], POS_TOL, w + ("pos",))
        _stats_close(g["ori"], r["ori"], ORI_TOL, w + ("ori",))


def _perturbed(gt, rng, sig_p=0.03, sig_r=0.01):
    """A noisy estimate in another frame: rigid transform of gt plus position and orientation noise."""
    from make_ate_toy import transform
    Rz, t = eo.rot_z(0.7), np.array([3.0, -1.0, 0.5])
    est = transform(gt, Rz.T, -Rz.T @ t)
    est[:, :3] += rng.normal(0, sig_p, (len(gt), 3))
    for i in range(len(gt)):
        dq = np.append(0.5 * rng.normal(0, sig_r, 3), 1.0)
        est[i, 3:] = eo.quat_multiply(dq / np.linalg.norm(dq), est[i, 3:])
    return est


def _path(acc_steps, rng, heading_rate=0.15):
    """Poses whose consecutive ground-truth distances are acc_steps (to rounding): a planar drive with a turning heading."""
    n = len(acc_steps) + 1
    gt = np.zeros((n, 7))
    th = 0.0
    for i in range(n):
        if i:
            th += heading_rate * acc_steps[i - 1]
            gt[i, :3] = gt[i - 1, :3] + acc_steps[i - 1] * np.array([math.cos(th), math.sin(th), 0.05])
        gt[i, 3:] = eo.rot_2_quat(eo.rot_z(th).T)
    return gt


def test_rpe_matches_restatement_on_fixture(ctx):
    """tests/golden/ate_toy.json (40 poses, 10.59 m): 37 / 33 / 26 / 13 / 0 segments of 1, 2, 4, 8, 16 m; the 16 m case is the
    'no segment' case and must leave n == 0 and every statistic zero, as the reference's empty Statistics does."""
    _, gt, est = _toy()
    seg = [1.0, 2.0, 4.0, 8.0, 16.0]
    for m in METHODS:
        got, ref = ctx.traj_rpe(est, gt, seg, m), em.calculate_rpe(est, gt, seg, m)
        assert [r["n"] for r in ref] == [37, 33, 26, 13, 0]
        _check_rpe(got, ref, m)
        assert got[4]["n"] == 0 and (got[4]["end_idx"] == -1).all()
        assert all(v == 0 for v in got[4]["pos"].values()) and all(v == 0 for v in got[4]["ori"].values())
    # one valid value: NaN std / ninetynine on both sides (10.59 m of path: only from the first pose is its end within 0.5 m of 11 m)
    got, ref = ctx.traj_rpe(est, gt, [11.0], "posyaw"), em.calculate_rpe(est, gt, [11.0], "posyaw")
    assert ref[0]["n"] == 1 and math.isnan(ref[0]["pos"]["std"])
    _check_rpe(got, ref, "single")


def test_rpe_nullable_outputs_and_bad_arguments(pkg, ctx):
    _, gt, est = _toy()
    lib = ctx.lib
    seg = np.array([2.0, 16.0])
    nv = np.zeros(2, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = lib.plv_traj_rpe(ctx.h, 0, len(gt), dp(est), dp(gt), 2, dp(seg), None, None, None, nv.ctypes.data_as(C.POINTER(C.c_int)), None, None)
    assert rc == 0 and list(nv) == [33, 0]
    assert lib.plv_traj_rpe(ctx.h, 0, len(gt), dp(est), dp(gt), 0, None, None, None, None, None, None, None) == 0
    assert lib.plv_traj_rpe(ctx.h, 0, len(gt), dp(est), None, 2, dp(seg), None, None, None, None, None, None) == pkg.PLV_E_BADARG
    assert lib.plv_traj_rpe(ctx.h, 0, len(gt), dp(est), dp(gt), 2, None, None, None, None, None, None, None) == pkg.PLV_E_BADARG


def test_rpe_ties_standing_stretch_and_gap(ctx):
    """End indices where the reference's scan is decided by its tie rule: exact ties between neighbours (0.25 m spacing, lengths
    k / 8), the limit itself (1 m spacing, length 0.5: the best error is exactly 0.5, not below it), a standing vehicle (repeated
    positions: runs of equal accumulated distance, the first of a run wins), and gaps wider than 0.5 m (starts before them find no
    end).  n is deliberately not a multiple of 64."""
    rng = np.random.default_rng(5)
    cases = {
        "quarter_metre": np.full(70, 0.25),
        "one_metre": np.full(33, 1.0),
        "standing": rng.choice([0.0, 0.0, 0.0, 0.125, 0.25, 0.375], size=330),
        "gaps": rng.uniform(0.01, 0.3, size=201),
    }
    cases["gaps"][[40, 120]] = [0.9, 2.5]
    seg = [0.0, 0.125, 0.375, 0.5, 1.0, 1.5, 2.0, 7.875]
    for name, steps in cases.items():
        if name in ("quarter_metre", "one_metre"):   # along one axis so that the accumulated distances are exact in binary
            gt = np.zeros((len(steps) + 1, 7))
            gt[1:, 0] = np.cumsum(steps)
            gt[:, 6] = 1.0
        else:
            gt = _path(steps, rng)
        assert len(gt) % 64 != 0
        est = _perturbed(gt, rng)
        ref = em.calculate_rpe(est, gt, seg, "se3")
        _check_rpe(ctx.traj_rpe(est, gt, seg, "se3"), ref, name)
        by_len = {r["length"]: r for r in ref}
        if name == "quarter_metre":
            assert by_len[0.125]["end_idx"][0] == 0 and by_len[0.375]["end_idx"][0] == 1      # the earlier index wins the tie
        if name == "one_metre":
            assert by_len[0.5]["n"] == 0 and by_len[1.5]["n"] == 0 and by_len[1.0]["n"] == len(gt) - 1
        if name == "standing":
            acc = em.accumulated_distances(gt)
            assert (np.diff(acc) == 0).sum() > 100                                           # the runs are there
        if name == "gaps":
            # the pose before the 2.5 m gap is 1 m short of its target and the one after it 1.5 m beyond; the 0.9 m gap leaves
            # an end within 0.45 m on one of its sides
            assert by_len[1.0]["end_idx"][120] == -1 and (by_len[1.0]["end_idx"][:100] >= 0).all()


@pytest.mark.parametrize("n", [5000, 4999])
def test_rpe_many_starts(ctx, n):
    """More starts than one workgroup holds, 2 cm apart, n a multiple of 8 but not of 64 / odd: every (length, start) pair against
    the reference's rule (its inner loop as one numpy reduction per start, pinned to the literal loop in the CPU tests and, here,
    on a 400-pose stretch)."""
    rng = np.random.default_rng(n)
    steps = np.full(n - 1, 0.02) + rng.uniform(-0.002, 0.002, n - 1)
    gt = _path(steps, rng, heading_rate=0.05)
    est = _perturbed(gt, rng, 0.01, 0.002)
    seg = [1.0, 2.0, 4.0, 8.0, 16.0]
    ref = em.calculate_rpe(est, gt, seg, "posyaw", search=em.comparison_indices_fast)
    acc = em.accumulated_distances(gt)
    for L in seg:
        assert np.array_equal(em.comparison_indices(acc[:400], L), em.comparison_indices_fast(acc[:400], L))
    assert all(r["n"] > n - 1000 for r in ref)
    _check_rpe(ctx.traj_rpe(est, gt, seg, "posyaw"), ref, f"n={n}")


def _random_spd(rng, n, scale):
    out = np.zeros((n, 3, 3))
    for i in range(n):
        A = rng.normal(size=(3, 3))
        out[i] = scale * (A @ A.T + 0.5 * np.eye(3))
    return out


def test_nees_matches_restatement(pkg, ctx):
    _, gt, est = _toy()
    rng = np.random.default_rng(9)
    n = len(gt)
    co, cp = _random_spd(rng, n, 1e-3), _random_spd(rng, n, 1e-2)
    for m in METHODS:
        got, ref = ctx.traj_nees(est, gt, co, cp, m), em.calculate_nees(est, gt, co, cp, m)
        assert got["n"] == ref["n"] == n
        big = (ref["nees_ori"] > 1e-6) & (ref["nees_pos"] > 1e-6)
        ro = np.abs(got["nees_ori"] / ref["nees_ori"] - 1)[big].max()
        rp = np.abs(got["nees_pos"] / ref["nees_pos"] - 1)[big].max()
        print(f"nees {m}: max relative diff ori {ro:.3e}, pos {rp:.3e} over {big.sum()} of {n} poses; the others: "
              f"{got['nees_ori'][~big]} vs {ref['nees_ori'][~big]}, {got['nees_pos'][~big]} vs {ref['nees_pos'][~big]}")
        assert _nees_close(got["nees_ori"], ref["nees_ori"]) and _nees_close(got["nees_pos"], ref["nees_pos"]), (m, ro, rp)
        for k in ref["ori"]:
            assert _nees_close(got["ori"][k], ref["ori"][k]) and _nees_close(got["pos"][k], ref["pos"][k]), (m, k)
    # a pose with a NaN covariance is skipped and counted out; the statistics are those of the rest
    co[11] = np.nan
    got, ref = ctx.traj_nees(est, gt, co, cp, "posyaw"), em.calculate_nees(est, gt, co, cp, "posyaw")
    assert got["n"] == ref["n"] == n - 1
    assert np.isnan(got["nees_ori"][11]) and np.isnan(got["nees_pos"][11]) and np.isnan(got["nees_ori"]).sum() == 1
    for k in ref["ori"]:
        assert _nees_close(got["ori"][k], ref["ori"][k]) and _nees_close(got["pos"][k], ref["pos"][k]), k
    # sizes around the workgroup: 1, 257 poses
    for n2 in (1, 257):
        gt2 = _path(np.full(n2 - 1, 0.1), rng)
        est2 = _perturbed(gt2, rng)
        co2, cp2 = _random_spd(rng, n2, 1e-3), _random_spd(rng, n2, 1e-2)
        got, ref = ctx.traj_nees(est2, gt2, co2, cp2, "none"), em.calculate_nees(est2, gt2, co2, cp2, "none")
        assert got["n"] == n2
        assert _nees_close(got["nees_ori"], ref["nees_ori"]) and _nees_close(got["nees_pos"], ref["nees_pos"])


def test_nees_without_covariance_is_refused(pkg, ctx):
    _, gt, est = _toy()
    cp = _random_spd(np.random.default_rng(1), len(gt), 1e-2)
    for co_, cp_ in ((None, cp), (cp, None), (None, None)):
        with pytest.raises(pkg.PlvError) as e:
            ctx.traj_nees(est, gt, co_, cp_)
        assert e.value.code == pkg.PLV_E_BADARG
        assert b"plv_traj_nees" in ctx.lib.plv_last_error() and b"covariance" in ctx.lib.plv_last_error()


def test_ate_2d_matches_restatement_and_3d_is_unmoved(ctx):
    d, gt, est = _toy()
    for m in METHODS:
        got, ref = ctx.traj_ate_2d(est, gt, m), em.calculate_ate_2d(est, gt, m)
        assert np.abs(got["pos_err"] - ref["pos_err"]).max() < POS_TOL, m
        assert np.abs(got["ori_err"] - ref["ori_err"]).max() < ORI_TOL, m
        _stats_close(got["pos"], ref["pos"], POS_TOL, (m, "pos"))
        _stats_close(got["ori"], ref["ori"], ORI_TOL, (m, "ori"))
        assert (got["ori_err"] < 0).any() or (ref["ori_err"] >= 0).all()      # signed, not a norm
        # the 3-D path on the same input, after the 2-D call on the same context: the recorded results of the fixture
        r, rec = ctx.traj_ate(est, gt, m), d["results"][m]
        assert np.abs(r["R"] - np.array(rec["R"])).max() < 1e-11 and np.abs(r["t"] - np.array(rec["t"])).max() < 1e-10
        assert np.abs(r["pos_err"] - np.array(rec["pos_err"])).max() < POS_TOL
        assert np.abs(r["ori_err"] - np.array(rec["ori_err"])).max() < ORI_TOL
        for k, v in rec["pos"].items():
            assert abs(r["pos"][k] - v) < POS_TOL, (m, k)
    assert np.array_equal(ctx.traj_ate_2d(est, gt, "posyaw", n_aligned=1)["pos_err"], ctx.traj_ate_2d(est, gt, "posyawsingle")["pos_err"])


def test_replay_tool_reports_rpe_and_nees(pkg, ctx, tmp_path):
    """tools/replay.py --synthetic 8 --rpe 2,4,8 --nees end to end: the filter's logged 6x6 marginal, written by plv_traj_format and
    read back by plv_traj_load, is invertible at every logged pose (n_valid == the number of associated poses: no NaN), and every
    RPE / NEES entry is finite.  That the restatement finds segments of these lengths on this drive's ground truth is checked
    here, not assumed.  No band is asserted for the mean NEES: it had never been measured (profiles/eval_metrics_synthetic.json
    records it; a consistent filter gives 3 per block)."""
    out, keep = str(tmp_path / "res.json"), str(tmp_path / "data")
    lengths = [2.0, 4.0, 8.0, 1000.0]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--synthetic", "8", "--rpe", ",".join(f"{x:g}" for x in lengths),
                        "--nees", "--out", out, "--keep", keep], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    et, ep, co, cp = pkg.traj_load(res["trajectory"])
    gt_t, gt_p = pkg.traj_load(os.path.join(keep, "gt.txt"))[:2]
    ei, gi = pkg.traj_associate(et, gt_t)
    n = len(ei)
    assert n == res["ate"]["n"] >= 70 and len(co) == len(et)
    ref = em.calculate_rpe(ep[ei], gt_p[gi], lengths, "posyaw")
    assert all(s["n"] >= 10 for s in ref[:3]) and ref[3]["n"] == 0
    assert [s["n"] for s in res["rpe"]] == [s["n"] for s in ref] and [s["length_m"] for s in res["rpe"]] == lengths
    for got, want in zip(res["rpe"][:3], ref[:3]):
        assert all(math.isfinite(v) for v in got["pos"].values()) and all(math.isfinite(v) for v in got["ori"].values())
        assert abs(got["pos"]["rmse"] - want["pos"]["rmse"]) < POS_TOL and abs(got["ori"]["rmse"] - want["ori"]["rmse"]) < ORI_TOL
    assert all(v == 0 for v in res["rpe"][3]["pos"].values())                   # a length with no segment: n 0, not an error
    nees = res["nees"]
    assert nees["n"] == nees["n_poses"] == n, nees                              # the logged marginal inverts at every pose
    assert all(math.isfinite(v) and v >= 0 for v in nees["pos"].values()) and all(math.isfinite(v) and v >= 0 for v in nees["ori"].values())
    want = em.calculate_nees(ep[ei], gt_p[gi], co[ei], cp[ei], "posyaw")
    assert abs(nees["pos"]["mean"] / want["pos"]["mean"] - 1) < NEES_RTOL and abs(nees["ori"]["mean"] / want["ori"]["mean"] - 1) < NEES_RTOL
    print("synthetic 8 s drive: mean NEES ori %.3f pos %.3f (3 expected of a consistent filter), RPE pos rmse %s m" %
          (nees["ori"]["mean"], nees["pos"]["mean"], [round(s["pos"]["rmse"], 4) for s in res["rpe"][:3]]))
    # the CPU oracle's replay of the same dataset (tests/replay_vs_cpu.py's route), scored the same way and printed beside it
    import oracle_context as oc
    import synth_dataset as sd
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    traj = str(tmp_path / "cpu" / "traj.txt")
    rp.replay(options.load_options(sd.write_config(str(tmp_path / "config_cpu"), keep, traj)), context_factory=oc.OracleContext,
              iw_initializer_factory=oc.OracleIwInitializer)
    ct, cpo, cco, ccp = pkg.traj_load(traj)
    ci, cgi = pkg.traj_associate(ct, gt_t)
    c = ctx.traj_nees(cpo[ci], gt_p[cgi], cco[ci], ccp[ci], "posyaw")
    print("CPU oracle on the same drive: mean NEES ori %.3f pos %.3f over %d of %d poses" % (c["ori"]["mean"], c["pos"]["mean"], c["n"], len(ci)))
