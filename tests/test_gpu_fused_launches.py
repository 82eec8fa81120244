"""The fused point and line launches (jacobian_nullspace_kernel and its line twin: triangulation, FEJ Jacobians with pose
interpolation, null-space projection and chi-square gate in one launch) held to the CPU oracle over the case matrix of
tests/fused_cases.py — off-clone times, first estimates that differ from the estimates, every noise option, calibration columns,
NaN blocks, blocks with nothing left after the projection — by verdict, by dx and P', and by the value of every chi2 and
projected-residual norm the gate looked at.

Largest differences measured on an MI355X (relative to the largest entry of the reference; the bounds asserted are the project's
own for these paths — lines: dx 1e-7 of max(1, |dx|), P' 1e-8 of the prior's largest entry; points: 1e-9 — and, for the gate values,
max(1e-8, 1e3 x the case's oracle-against-QR spread)).  The device's line chi2 had not been measured against the oracle's before:
2.4e-11 at worst, on lines whose chi2 reaches 1e5; the residual norm 1.4e-13; point chi2 2.4e-15.

build_*_jacobians_resident + msckf_update_resident   | fused launch against the oracle | against the unfused device route
  lines  easiest                      79/80  | dx 3.2e-14 P' 1.1e-15  | dx 1.5e-14 P' 4.6e-16
  lines  a-13ms-fej-dt-pol            56/80  | dx 5.6e-14 P' 9.7e-16  | dx 9.6e-15 P' 4.9e-16
  lines  b-37ms-fej-pol               31/40  | dx 1.3e-14 P' 3.2e-16  | dx 1.1e-14 P' 4.3e-16
  lines  c3-13ms-fej-dt-imucov       100/150 | dx 7.2e-15 P' 1.7e-15  | dx 4.0e-15 P' 2.2e-16
  lines  a-37ms-fej-imucov            58/80  | dx 6.3e-15 P' 6.5e-16  | dx 3.8e-15 P' 1.2e-16
  lines  b-13ms-fej-dt-respose        40/40  | dx 1.1e-14 P' 2.0e-14  | dx 6.1e-15 P' 8.2e-16
  lines  short-37ms-fej-dt-respose    60/65  | dx 1.0e-14 P' 3.1e-15  | dx 1.3e-14 P' 2.3e-15
  lines  a-camdt-fej-dt               77/80  | dx 1.6e-14 P' 5.7e-15  | dx 1.0e-14 P' 1.9e-15
  lines  c3-camdt                    150/150 | dx 4.1e-13 P' 8.4e-14  | dx 4.0e-13 P' 1.5e-13
  lines  one-13ms-fej-dt               1/1   | dx 2.7e-14 P' 1.2e-16  | dx 7.2e-15 P' 4.9e-17
  lines  one-37ms-fej                  1/1   | dx 2.7e-14 P' 1.1e-16  | dx 1.2e-14 P' 2.8e-17
  lines  short-37ms-pol               41/65  | dx 1.8e-12 P' 1.2e-15  | dx 3.4e-14 P' 1.4e-15
  lines  c3-13ms-fej-pol              99/150 | dx 1.2e-14 P' 1.1e-15  | dx 1.6e-14 P' 6.7e-16
  lines  b-fej-dt                     40/40  | dx 1.3e-13 P' 1.7e-14  | dx 5.7e-14 P' 1.1e-15
  lines  short-13ms-imucov            40/65  | dx 2.5e-13 P' 1.5e-15  | dx 3.2e-13 P' 2.6e-15
  points easiest                      80/80  | dx 7.3e-15 P' 2.9e-15  | dx 5.2e-15 P' 1.2e-16
  points a-13ms-fej-all-pol           68/80  | dx 8.5e-15 P' 1.0e-15  | dx 2.0e-15 P' 1.3e-16
  points b-37ms-fej-pol               40/40  | dx 4.6e-15 P' 1.8e-15  | dx 3.2e-15 P' 7.9e-16
  points c3-13ms-fej-all-imucov      108/150 | dx 7.9e-15 P' 1.4e-15  | dx 3.5e-15 P' 2.3e-16
  points a-37ms-fej-ext-imucov        66/80  | dx 4.8e-15 P' 7.9e-16  | dx 5.8e-15 P' 3.4e-16
  points b-13ms-fej-dt-respose        34/40  | dx 2.9e-14 P' 1.3e-15  | dx 7.8e-15 P' 2.6e-16
  points short-37ms-fej-all-respose   65/65  | dx 5.2e-14 P' 8.8e-16  | dx 4.5e-14 P' 2.8e-16
  points a-camdt-fej-all              80/80  | dx 1.3e-14 P' 9.4e-16  | dx 4.2e-15 P' 2.7e-16
  points c3-camdt-ext                128/150 | dx 9.1e-15 P' 4.2e-15  | dx 4.2e-15 P' 3.6e-16
  points one-13ms-fej-all              1/1   | dx 1.8e-14 P' 1.2e-16  | dx 2.5e-14 P' 1.2e-16
  points one-37ms-fej                  1/1   | dx 6.8e-15 P' 2.9e-17  | dx 4.2e-15 P' 2.9e-17
  points short-2px-outliers           58/65  | dx 5.4e-14 P' 7.7e-16  | dx 6.3e-14 P' 2.2e-16
  points a-equi-strong-13ms-fej-all   80/80  | (no fisheye oracle)    | dx 2.4e-15 P' 2.6e-16
  points b-equi-strong-37ms-fej       34/40  | (no fisheye oracle)    | dx 1.4e-14 P' 1.4e-16
  points c3-37ms-fej-dt-pol          150/150 | dx 1.2e-14 P' 1.8e-15  | dx 4.9e-15 P' 2.5e-16

one-call updates, per feature at the gate            | chi2    residual norm  (spread)  | dx      P'      | triangulation
  lines  wide-easiest                  6/22  | 2.4e-11 1.4e-13        (1.4e-11) | 8.8e-13 1.7e-12 | line_FinG 0.0e+00
  lines  wide-130ms-fej-dt             5/22  | 1.7e-12 1.1e-13        (3.6e-12) | 4.9e-13 2.6e-13 | line_FinG 0.0e+00
  lines  wide-370ms-fej-pol            4/5   | 8.9e-15 4.4e-15        (2.2e-14) | 6.9e-15 1.5e-17 | line_FinG 1.7e-16
  lines  wide-camdt-fej-dt             3/20  | 1.3e-11 5.8e-14        (5.8e-12) | 1.5e-14 4.5e-15 | line_FinG 0.0e+00
  points easiest                      45/45  | 8.1e-16 2.0e-16        (9.3e-16) | 1.9e-13 2.1e-15 | cond / depths / reprojection 5.9e-12
  points a-13ms-fej-all-pol           40/40  | 2.4e-15 8.6e-16        (6.3e-16) | 4.3e-15 8.9e-16 | cond / depths / reprojection 7.1e-12
  points b-37ms-fej                   30/30  | 9.9e-16 5.1e-16        (4.2e-16) | 1.8e-14 9.8e-16 | cond / depths / reprojection 7.1e-12
  points c3-camdt-fej-ext             75/75  | 8.0e-16 3.2e-16        (8.7e-16) | 1.5e-14 2.8e-15 | cond / depths / reprojection 3.0e-12
  points a-2px-outliers-13ms-fej-dt   35/40  | 7.2e-16 2.2e-16        (7.7e-16) | 2.1e-14 8.8e-16 | cond / depths / reprojection 4.0e-12
  lines  try_update (unchained)        3/24  | 9.2e-12 2.9e-14        (5.6e-12) | 1.3e-12 2.9e-12 | line_FinG 0.0e+00

(accepted / features; for the one-call updates accepted / features that reached the gate.  The module runs in 3.2 s.)

Each check was shown to bite on one-line changes of the fused launches' own code (scratch builds, not kept): the new tests that
failed, and whether test_gpu_lines.py / test_gpu_jacobian.py / test_gpu_update_frame.py as they stood before noticed —
  line_rows_split takes dli_dI at the estimate pose            12 resident line cases with FEJ noise, 3 one-call, try_update | no
  the fused point launch takes the residual at the FEJ pose     10 resident point cases with FEJ noise, 4 one-call, try_update | one (test_camera_update_points_with_cpi_poses)
  res_Q / res_clone of the line's first observation for all     the 3 resident line cases with the CPI covariance             | no
  the fused line launch interpolates at obs_time without cam_dt the 2 resident + 1 one-call line cases with cam_dt != 0        | no
  the fused line launch's time offset column x (1 + 1e-4)       the 7 resident + 2 one-call line cases that calibrate it      | no"""
import numpy as np
import pytest

import fused_cases as fc
import oracle_lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


def _rel(a, b):
    """largest difference relative to the largest entry of the reference"""
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _build(ctx, b, resident=False):
    pts = b["case"].kind == "points"
    if resident:
        return (ctx.build_jacobians_resident if pts else ctx.build_line_jacobians_resident)
    return (ctx.build_jacobians if pts else ctx.build_line_jacobians)


def _check_update(b, got, ref, what):
    """accepted and n_rows identical; dx and P' to the bounds the project holds these paths to (test_gpu_lines.py: 1e-7 of max(1, |dx|)
    and 1e-8 of the prior's largest entry for lines; test_fused_build_project_paths_agree: 1e-9 for points)"""
    (rc, dx, acc, nrows, Pn), (rc_r, dx_r, acc_r, nrows_r, P_r) = got, ref
    assert rc == rc_r == 0, what
    assert np.array_equal(acc, acc_r), (what, np.nonzero(acc != acc_r)[0])
    assert nrows == nrows_r, what
    assert np.isfinite(dx).all() and np.isfinite(Pn).all(), what
    if b["case"].kind == "lines":
        assert np.abs(dx - dx_r).max() <= 1e-7 * max(1.0, np.abs(dx_r).max()), what
        assert np.abs(Pn - P_r).max() <= 1e-8 * np.abs(b["P"]).max(), what
    else:
        assert np.abs(dx - dx_r).max() <= 1e-9 * max(1.0, np.abs(dx_r).max()), what
        assert np.abs(Pn - P_r).max() <= 1e-9 * np.abs(P_r).max(), what
    return _rel(dx, dx_r), _rel(Pn, P_r)


@pytest.mark.parametrize("case", fc.LINE_CASES + fc.POINT_CASES, ids=lambda c: f"{c.kind}-{c.name}")
def test_resident_build_and_update(pkg, ctx, oracle, jo, case):
    """build_*_jacobians_resident + msckf_update_resident (the fused launch) against the oracle's build + msckf_update, and against the
    unfused device route (build_*_jacobians to the host, msckf_update): the split pieces form the values the unsplit ones form."""
    b = fc.build(pkg, case)
    st, tr, n, P, ld, s2, gate = b["st"], b["tr"], b["n"], b["P"], b["ld"], b["sigma2"], b["res_norm_gate"]
    ctx.set_camera_model(case.model)
    try:
        cols = (ctx.jacobian_columns if case.kind == "points" else ctx.line_jacobian_columns)(st, tr)
        # the unfused device route
        rows, Hf, Hx, res = _build(ctx, b)(st, tr, cols, ld)
        rc_u, P_u, dx_u, acc_u, nr_u = ctx.msckf_update(P, rows, Hf, Hx, res, cols, s2, res_norm_gate=gate)
        # the fused launch
        ctx.cov_upload(P)
        _build(ctx, b, resident=True)(st, tr, cols, ld)
        rc, dx, acc, nrows = ctx.msckf_update_resident(n, s2, res_norm_gate=gate)
        Pn = ctx.cov_download(n)
    finally:
        ctx.set_camera_model("radtan")
    got = (rc, dx, acc, nrows, Pn)
    line = f"{case.kind:6s} {case.name:28s} accepted {int(acc.sum()):3d} of {case.F:3d}"
    if b["has_oracle"]:
        systems = fc.oracle_systems(jo, b)
        assert np.array_equal(cols, systems[0]) and np.array_equal(rows, systems[1])
        up = fc.oracle_update(oracle, b, systems)
        nan = np.array([np.isnan(systems[3][f]).any() or np.isnan(systems[4][f]).any() for f in range(case.F)])
        assert not acc[nan].any()                               # a NaN block is rejected (and dx, P' are finite: _check_update)
        d = _check_update(b, got, (up["rc"], up["dx"], up["accepted"], up["n_rows"], up["P"]), "fused launch against the oracle")
        line += f" | against the oracle: dx {d[0]:.1e} P' {d[1]:.1e}"
    else:
        assert acc.sum() >= 0.5 * case.F and (case.outlier_px == 0 or (acc == 0).sum() >= 0.1 * case.F)
    d = _check_update(b, got, (rc_u, dx_u, acc_u, nr_u, P_u), "fused launch against the unfused device route")
    print(line + f" | against the unfused route: dx {d[0]:.1e} P' {d[1]:.1e}")


def _by_id(ids, vals):
    return {int(i): v for i, v in zip(ids, vals)}


def _compare_gate_values(ids, dev, orc, bound, what):
    """chi2 (0), threshold (1), residual norm (2) per feature: threshold exactly, NaN on one side means NaN on the other, values to
    `bound` relative.  Returns the largest differences (chi2, residual norm)."""
    worst = [0.0, 0.0]
    for i in ids:
        a, o = dev[int(i)], orc[int(i)]
        assert np.array_equal(np.isnan(a), np.isnan(o)), (what, int(i), a, o)
        if np.isnan(o[0]):
            continue
        assert a[1] == o[1], (what, int(i), a, o)
        for j, col in enumerate((0, 2)):
            rel = abs(a[col] - o[col]) / max(abs(o[col]), 1e-300)
            worst[j] = max(worst[j], rel)
            assert rel <= bound, (what, int(i), ("chi2", "residual norm")[j], a[col], o[col], rel, bound)
    return worst


@pytest.mark.parametrize("case", fc.ONE_CALL_LINE_CASES + fc.ONE_CALL_POINT_CASES, ids=lambda c: f"{c.kind}-{c.name}")
def test_one_call_update_by_value(pkg, oracle, jo, case):
    """camera_update_points / camera_update_lines (databases -> pool -> triangulation in the launch -> Jacobians -> gate -> update) with
    the decision trace on, against the compiled CPU frame on the same databases: every feature that reaches the gate, accepted or not,
    has the oracle's threshold exactly and its chi2 and residual norm to max(1e-8, 1e3 x the case's oracle-against-QR spread)."""
    fo = oracle_lib.load_front()
    b = fc.build(pkg, case)
    tracks, used = fc.one_call_tracks(b, fo.undistort)
    r = fc.one_call_oracle(pkg, b, tracks, used)
    ref = r["out"]
    b2, systems = fc.one_call_systems(pkg, jo, b, tracks, ref)
    s = fc.spread(fc.gate_values_oracle(oracle, b2, systems), fc.gate_values_qr(b2, systems))
    bound = fc.value_bound(s)
    c = pkg.Context(pkg.default_config(b["sc"]["w"], b["sc"]["h"]))
    try:
        c.decision_trace(True)
        fc.fill_databases(c, case.kind, tracks, used, device=True)
        c.cov_upload(b["P"])
        args, kw = fc.one_call_args(b)
        out = (c.camera_update_points if case.kind == "points" else c.camera_update_lines)(*args, **kw)
        ids, vals = c.last_point_decisions() if case.kind == "points" else c.last_line_decisions()
        Pn = c.cov_download(b["n"])
    finally:
        c.close()
    assert out["status"] == ref["status"] == 0 and out["n_pool"] == ref["n_pool"]
    assert np.array_equal(out["ids"], ref["ids"]) and np.array_equal(out["accepted"], ref["accepted"]) and out["n_rows"] == ref["n_rows"]
    assert set(int(i) for i in ids) == set(int(i) for i in r["ids"])
    dev, orc = _by_id(ids, vals), _by_id(r["ids"], r["vals"])
    if case.kind == "points":
        assert np.abs(out["p_FinG"] - ref["p_FinG"]).max() < 1e-6
        assert not np.isnan([dev[int(i)][3] for i in ids]).any()         # (gate_passed is recorded by the fused route only)
        worst_tri = 0.0
        for i in ids:                                                    # the whole pool: reprojection error, condition number, depths, baseline ratio
            a, o = dev[int(i)][[2, 4, 5, 6, 7]], orc[int(i)][[2, 4, 5, 6, 7]]
            assert np.array_equal(np.isnan(a), np.isnan(o)), (int(i), a, o)
            fin = ~np.isnan(o)
            rel = np.abs(a[fin] - o[fin]) / np.maximum(np.abs(o[fin]), 1e-300)
            worst_tri = max(worst_tri, rel.max() if fin.any() else 0.0)
            assert (rel <= 1e-8).all(), (int(i), a, o)
        gate_cols = [8, 9, 10]
        dev, orc = {i: v[gate_cols] for i, v in dev.items()}, {i: v[gate_cols] for i, v in orc.items()}
        extra = f" triangulation values {worst_tri:.1e}"
    else:
        assert np.abs(out["line_FinG"] - ref["line_FinG"]).max() <= 1e-9 * max(1.0, np.abs(ref["line_FinG"]).max())
        extra = f" line_FinG {_rel(out['line_FinG'], ref['line_FinG']):.1e}"
    worst = _compare_gate_values(ids, dev, orc, bound, case.name)
    d = _check_update(b, (0, out["dx"], out["accepted"], out["n_rows"], Pn), (0, ref["dx"], ref["accepted"], ref["n_rows"], r["P"]), "one-call update")
    n_gate = sum(1 for i in ids if not np.isnan(orc[int(i)][0]))
    print(f"{case.kind:6s} {case.name:28s} at the gate {n_gate:3d}, accepted {int(out['accepted'].sum()):3d} | chi2 {worst[0]:.1e} residual norm {worst[1]:.1e} "
          f"(spread {s:.1e}, bound {bound:.0e}) | dx {d[0]:.1e} P' {d[1]:.1e} |{extra}")


def test_try_update_line_half_unchained_and_chained(pkg, oracle, jo):
    """Both halves of camera_try_update in one call, on a window the point update moves.  Unchained (knob 2048) the lines are
    triangulated on the state before the point correction and linearised on the corrected one — two views of one window in one
    launch; chained (knob 4096) the launch sits behind the point update on the stream and forms x (+) dx itself.  The unchained form
    against the compiled CPU frame's try_update by line_FinG, verdicts, per-line values, dx and P'; the chained form equals the
    unchained bit for bit."""
    fo = oracle_lib.load_front()
    S = fc.try_update_scene(pkg, fo.undistort)
    b = S["b"]
    t, n = b["sc"]["t"], b["n"]
    MAX_MSCKF, MOBS = 80, b["case"].M                                   # (the cap above the pool: what a chained launch asks for)
    kw = dict(t_prev_frame=float(t[-2]), state_time=float(t[-1]), window_full=True, lines=True, **fc.TRI)
    # ---- the oracle
    st_o, plus_o, keep_o = S["make_state"]()
    fr = oracle_lib.FrameOracle(pkg, pkg.default_config(b["sc"]["w"], b["sc"]["h"]), fc.q95_table())
    fr.set_intrinsics(b["K8"])
    fc.fill_databases(fr, "points", S["tracks"], {}, device=False)
    fc.fill_databases(fr, "lines", S["ltracks"], S["used"], device=False)
    P_o = np.array(b["P"], dtype=np.float64, order="F")
    pts_o, lns_o, _ = fr.try_update(P_o, st_o, dict(plus=plus_o, n=n, max_msckf=MAX_MSCKF, max_obs=MOBS, **kw))
    lid_o, lval_o = fr.last_line_decisions()
    fr.close()
    assert pts_o["status"] == lns_o["status"] == 0 and pts_o["accepted"].sum() >= 20 and np.abs(pts_o["dx"]).max() > 1e-5   # the state moves
    assert len(lns_o["ids"]) >= 20 and lns_o["accepted"].sum() >= 2
    # the spread of the line values on the batch the oracle gated: Jacobians on the state and the covariance the line half saw, which
    # are the ones the point half alone leaves behind
    st_p, plus_p, keep_p = S["make_state"]()
    P_mid = np.array(b["P"], dtype=np.float64, order="F")
    fr2 = oracle_lib.FrameOracle(pkg, pkg.default_config(b["sc"]["w"], b["sc"]["h"]), fc.q95_table())
    fr2.set_intrinsics(b["K8"])
    fc.fill_databases(fr2, "points", S["tracks"], {}, device=False)
    fr2.try_update(P_mid, st_p, dict(plus=plus_p, n=n, max_msckf=MAX_MSCKF, max_obs=MOBS, **dict(kw, lines=False)))
    fr2.close()
    lb = dict(b, case=b["case"]._replace(kind="lines"), st=st_p, fdim=6, min_rows=5, res_norm_gate=0.0)
    b2, systems = fc.one_call_systems(pkg, jo, lb, S["ltracks"], lns_o)
    b2["P"] = P_mid
    vo = fc.gate_values_oracle(oracle, b2, systems)
    pos = {int(i): q for q, i in enumerate(lid_o)}
    fv = np.array([lval_o[pos[int(i)]] for i in lns_o["ids"]])
    assert fc.rel_diff(fv[:, 0], vo[:, 0]) < 1e-12 and fc.rel_diff(fv[:, 2], vo[:, 2]) < 1e-12   # (the composition is the frame's)
    s = fc.spread(vo, fc.gate_values_qr(b2, systems))
    bound = fc.value_bound(s)
    # ---- the device, both forms
    runs = {}
    before = pkg.debug_knobs()
    try:
        for form, knob in (("unchained", 2048), ("chained", 4096)):
            pkg.debug_knobs(knob)
            chains0 = pkg.chain_count()
            st, plus, keep = S["make_state"]()
            c = pkg.Context(pkg.default_config(b["sc"]["w"], b["sc"]["h"]))
            try:
                c.decision_trace(True)
                fc.fill_databases(c, "points", S["tracks"], {}, device=True)
                fc.fill_databases(c, "lines", S["ltracks"], S["used"], device=True)
                c.cov_upload(b["P"])
                pts, lns, _ = c.camera_try_update(st, plus, n, MAX_MSCKF, MOBS, **kw)
                lid, lval = c.last_line_decisions()
                runs[form] = dict(pts=pts, lns=lns, lid=lid, lval=lval, P=c.cov_download(n), R=st.R.copy(), p=st.p.copy(), chains=pkg.chain_count() - chains0)
            finally:
                c.close()
    finally:
        pkg.debug_knobs(before)
    u, ch = runs["unchained"], runs["chained"]
    assert u["chains"] == 0 and ch["chains"] == 1, (u["chains"], ch["chains"])
    # unchained against the oracle
    assert np.array_equal(u["pts"]["ids"], pts_o["ids"]) and np.array_equal(u["pts"]["accepted"], pts_o["accepted"])
    assert np.abs(u["pts"]["dx"] - pts_o["dx"]).max() <= 1e-9 * max(1.0, np.abs(pts_o["dx"]).max())
    assert u["lns"]["status"] == 0 and u["lns"]["n_pool"] == lns_o["n_pool"]
    assert np.array_equal(u["lns"]["ids"], lns_o["ids"]) and np.array_equal(u["lns"]["accepted"], lns_o["accepted"]) and u["lns"]["n_rows"] == lns_o["n_rows"]
    assert np.abs(u["lns"]["line_FinG"] - lns_o["line_FinG"]).max() <= 1e-9 * max(1.0, np.abs(lns_o["line_FinG"]).max())
    worst = _compare_gate_values(lid_o, _by_id(u["lid"], u["lval"]), _by_id(lid_o, lval_o), bound, "try_update, unchained")
    d = _check_update(lb, (0, u["lns"]["dx"], u["lns"]["accepted"], u["lns"]["n_rows"], u["P"]),
                      (0, lns_o["dx"], lns_o["accepted"], lns_o["n_rows"], P_o), "try_update, unchained, line half")
    assert np.abs(u["R"] - st_o.R).max() < 1e-9 and np.abs(u["p"] - st_o.p).max() < 1e-9
    print(f"lines  try_update (unchained)       at the gate {int((~np.isnan(lval_o[:, 0])).sum()):3d}, accepted {int(lns_o['accepted'].sum()):3d} | chi2 {worst[0]:.1e} "
          f"residual norm {worst[1]:.1e} (spread {s:.1e}, bound {bound:.0e}) | dx {d[0]:.1e} P' {d[1]:.1e} | line_FinG {_rel(u['lns']['line_FinG'], lns_o['line_FinG']):.1e}")
    # chained against unchained: bit for bit
    for key in ("dx", "ids", "accepted", "line_FinG"):
        assert np.array_equal(ch["lns"][key], u["lns"][key]), key
    assert np.array_equal(ch["pts"]["dx"], u["pts"]["dx"]) and ch["lns"]["n_rows"] == u["lns"]["n_rows"]
    assert np.array_equal(ch["lid"], u["lid"]) and np.array_equal(ch["lval"], u["lval"], equal_nan=True)
    assert np.array_equal(ch["P"], u["P"]) and np.array_equal(ch["R"], u["R"]) and np.array_equal(ch["p"], u["p"])
