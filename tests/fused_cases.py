"""The case matrix of the fused point and line launches (test infrastructure; tests/test_fused_cases_cpu.py states what the cases
must contain, tests/test_gpu_fused_launches.py runs them on the device).

jacobian_nullspace_kernel and its line twin build the Jacobians, project them on the left null space of Hf and gate them in one
launch; the pieces are the ones the unfused launches run, the code around them (four waves, LDS slots, the window tables instead of
`interpolate`, LDS copies of the observations) is not.  The cases below walk the inputs on which that code decides something:

  shape       (n_clones, F or L, M): (15, 80, 15), (11, 40, 11), (20, 150, 20), (15, 1, 15), (15, 65, 6) — 65 is one past a wave, and
              with M = 6 the shortest line tracks have 6 rows = fdim: nothing is left after the projection; ld = 2 M and 2 M + 2
  obs_offset  0, 13 ms, 37 ms behind the clone times (dt_clone = 50 ms): the interpolation and the window tables; `cam_dt` puts the
              same offset into the state view instead of the stamps
  fej_noise   0, 1e-3, 2e-3: first estimates that are not the estimates
  calib       time offset (both kinds); extrinsics, intrinsics (points)
  model       radtan, equidistant with the strong coefficient set (points; the CPU oracle has no fisheye model: such a case is held to
              the unfused device route only)
  noise       "pol": use_pol_cov = 1, intr_ori_cov = 1e-5, intr_pos_cov = 2e-5 (always with off-clone times: an observation on a clone
              time takes no interpolation noise);  "imu_cov": use_imu_cov = 1 with res_R / res_p / res_Q / res_clone on the tracks
              (LINE_Q_SCALE below);  "res_pose": res_R / res_p alone
  outlier_px  (points) extra pixel noise on 15 % of the tracks, so that the gate decides both ways

Not the full product: every value of every axis occurs at least twice per kind, and every noise option occurs at least once together
with off-clone times AND first-estimate noise (the combination in which a kernel that reads the wrong one of two poses, or the noise of
the wrong observation, shows).

chi2 and the norm of the projected residual do not depend on the basis the null space is projected with, so they can be compared by
value although the device projects with Householder reflections and the oracle with Givens rotations: gate_values_qr() restates them
with LAPACK's QR and numpy.linalg.solve, and spread() says how far that restatement is from the oracle's own values — how much the
value moves under rounding-sized perturbations of its arithmetic."""
from collections import namedtuple

import numpy as np

import synth

SIGMA_PIX = 1.5
DT_CLONE = 0.05
STRONG = np.array([350.0, 348.0, 370.0, 245.0, -0.35, 0.12, -0.03, 0.004])     # test_gpu_equidistant.STRONG

# The reference inverts the 2 x 2 noise of an observation through the Cholesky factor of its Cholesky factor, which is NaN once the
# two rows are strongly correlated; H Q H^T with a line's H (|H| 1e4 .. 1e7) is.  With the CPI covariance at the scale the point
# tests use (factors of 2e-3 / 8e-3), 28 of the 40 lines of test_line_jacobians_with_the_cpi_covariance_as_noise hold such an
# observation, and 60 .. 85 % of the lines of the cases below: the gate would see less than half of a batch.  At 0.3 of that scale
# 27 .. 34 % of the lines are NaN — NaN blocks next to healthy ones, as in the "pol" cases — and 62 .. 72 % pass the gate.
LINE_Q_SCALE = 0.3

Case = namedtuple("Case", "kind name n_clones F M ld_extra obs_offset cam_dt fej_noise calib_dt calib_ext calib_intr model noise outlier_px seed dt_clone")


def _line(name, shape, ld_extra, obs_offset, fej_noise, calib_dt, noise="none", cam_dt=0.0, seed=5, dt_clone=DT_CLONE):
    return Case("lines", name, shape[0], shape[1], shape[2], ld_extra, obs_offset, cam_dt, fej_noise, calib_dt, False, True, "radtan", noise, 0.0, seed,
                dt_clone)


def _point(name, shape, ld_extra, obs_offset, fej_noise, calib_dt, calib_ext, calib_intr, noise="none", cam_dt=0.0, model="radtan", outlier_px=0.0, seed=3,
           dt_clone=DT_CLONE):
    return Case("points", name, shape[0], shape[1], shape[2], ld_extra, obs_offset, cam_dt, fej_noise, calib_dt, calib_ext, calib_intr, model, noise,
                outlier_px, seed, dt_clone)


A, B, C3, ONE, SHORT = (15, 80, 15), (11, 40, 11), (20, 150, 20), (15, 1, 15), (15, 65, 6)

LINE_CASES = [
    _line("easiest", A, 0, 0.0, 0.0, False),
    _line("a-13ms-fej-dt-pol", A, 2, 0.013, 1e-3, True, "pol"),
    _line("b-37ms-fej-pol", B, 0, 0.037, 2e-3, False, "pol", seed=6),
    _line("c3-13ms-fej-dt-imucov", C3, 0, 0.013, 2e-3, True, "imu_cov"),
    _line("a-37ms-fej-imucov", A, 2, 0.037, 1e-3, False, "imu_cov", seed=7),
    _line("b-13ms-fej-dt-respose", B, 2, 0.013, 1e-3, True, "res_pose"),
    _line("short-37ms-fej-dt-respose", SHORT, 0, 0.037, 2e-3, True, "res_pose"),
    _line("a-camdt-fej-dt", A, 0, 0.013, 1e-3, True, cam_dt=0.013, seed=8),
    _line("c3-camdt", C3, 2, 0.037, 0.0, False, cam_dt=0.037),
    _line("one-13ms-fej-dt", ONE, 0, 0.013, 1e-3, True),
    _line("one-37ms-fej", ONE, 2, 0.037, 2e-3, False, seed=9),
    _line("short-37ms-pol", SHORT, 2, 0.037, 0.0, False, "pol"),
    _line("c3-13ms-fej-pol", C3, 0, 0.013, 1e-3, False, "pol", seed=6),
    _line("b-fej-dt", B, 0, 0.0, 1e-3, True),
    _line("short-13ms-imucov", SHORT, 0, 0.013, 0.0, False, "imu_cov", seed=7),
]

POINT_CASES = [
    _point("easiest", A, 0, 0.0, 0.0, False, False, True),
    _point("a-13ms-fej-all-pol", A, 2, 0.013, 1e-3, True, True, True, "pol", outlier_px=4.0),
    _point("b-37ms-fej-pol", B, 0, 0.037, 2e-3, False, False, False, "pol", seed=4),
    _point("c3-13ms-fej-all-imucov", C3, 0, 0.013, 2e-3, True, True, True, "imu_cov", outlier_px=9.0),
    _point("a-37ms-fej-ext-imucov", A, 2, 0.037, 1e-3, False, True, False, "imu_cov", seed=5),
    _point("b-13ms-fej-dt-respose", B, 2, 0.013, 1e-3, True, False, True, "res_pose", outlier_px=4.0),
    _point("short-37ms-fej-all-respose", SHORT, 0, 0.037, 2e-3, True, True, True, "res_pose"),
    _point("a-camdt-fej-all", A, 0, 0.013, 1e-3, True, True, True, cam_dt=0.013, seed=6),
    _point("c3-camdt-ext", C3, 2, 0.037, 0.0, False, True, False, cam_dt=0.037, outlier_px=9.0),
    _point("one-13ms-fej-all", ONE, 0, 0.013, 1e-3, True, True, True),
    _point("one-37ms-fej", ONE, 2, 0.037, 2e-3, False, False, False, seed=7),
    _point("short-2px-outliers", SHORT, 2, 0.0, 0.0, False, False, True, outlier_px=2.0),
    _point("a-equi-strong-13ms-fej-all", A, 0, 0.013, 1e-3, True, True, True, model="equidistant"),
    _point("b-equi-strong-37ms-fej", B, 2, 0.037, 2e-3, False, False, True, model="equidistant", outlier_px=4.0, seed=4),
    _point("c3-37ms-fej-dt-pol", C3, 0, 0.037, 1e-3, True, False, True, "pol", seed=8),
]

CASES = {"lines": LINE_CASES, "points": POINT_CASES}

# The one-call entry points (camera_update_points / camera_update_lines: databases -> pool -> triangulation -> fused launch -> update)
# take no residual poses on the tracks, and with a CPI table they leave the fused launch for the two-step route: the cases that
# reach the fused launches through them vary what the state view carries.  Lines are triangulated in the launch itself: on the
# 50 ms window only the lines with an anchor point (D > 0 and a triangulated point of theirs) come through, and what the launch
# triangulates there is conditioned badly enough for chi2 to move by 1e-8 .. 1e-7 under rounding alone (spread(): 1.3e-8 and 1.4e-7
# measured on two such scenes) — no ground to compare two implementations by value on.  The cases use the wide baseline
# (dt_clone = 0.5 s, offsets scaled with it), where plane pairs pass the 8 degree gate as well and the spread stays below 2e-11
# (a 20-clone window at that spacing is a 10 s drive, |H| reaches 5e8 and the spread 3e-10 .. 1e-9 on five seeds: not used).
ONE_CALL_LINE_CASES = [
    _line("wide-easiest", (15, 50, 15), 0, 0.0, 0.0, False, dt_clone=0.5, seed=6),
    _line("wide-130ms-fej-dt", (15, 50, 15), 0, 0.13, 1e-3, True, dt_clone=0.5, seed=6),
    _line("wide-370ms-fej-pol", (11, 40, 11), 0, 0.37, 2e-3, False, "pol", dt_clone=0.5, seed=7),
    _line("wide-camdt-fej-dt", (15, 50, 15), 0, 0.13, 1e-3, True, cam_dt=0.13, dt_clone=0.5, seed=8),
]
ONE_CALL_POINT_CASES = [
    _point("easiest", (15, 90, 15), 0, 0.0, 0.0, False, False, True, outlier_px=9.0, seed=9),
    _point("a-13ms-fej-all-pol", A, 0, 0.013, 1e-3, True, True, True, "pol", outlier_px=4.0),
    _point("b-37ms-fej", B, 0, 0.037, 2e-3, False, False, False, seed=4),
    _point("c3-camdt-fej-ext", C3, 0, 0.013, 2e-3, False, True, True, cam_dt=0.013, outlier_px=9.0),
    _point("a-2px-outliers-13ms-fej-dt", A, 0, 0.013, 1e-3, True, False, True, outlier_px=2.0, seed=5),
]
ONE_CALL_CASES = {"lines": ONE_CALL_LINE_CASES, "points": ONE_CALL_POINT_CASES}
# the triangulation gates of the one-call point update, opened as test_camera_update_points opens them (the default condition-number
# gate rejects most landmarks of the 50 ms window)
TRI = dict(max_cond=1e7, max_dist=100.0, max_baseline=1e3)


_Q95 = []


def q95_table():
    """The 95 % chi-square quantiles the oracle gates with in this module: the library's own host function (plv_chi2_quantile95, the
    table every context uploads; held to scipy's to 1e-11 by tests/test_oracle_update.py), not scipy's.  The two differ in the last
    two or three bits (36.41502850180729 against ...731 at 24 degrees of freedom), and the threshold a gate value was held against is
    compared exactly: with one table on both sides that comparison says the launch looked up the right number of rows."""
    if not _Q95:
        import __graft_entry__ as ge
        lib = ge.load_pkg().load_library()
        _Q95.append(np.array([0.0] + [lib.plv_chi2_quantile95(i) for i in range(1, 1024)]))
    return _Q95[0]


# ------------------------------------------------------------------ scenes
def _scene(case, noise_px):
    """synth.vio_scene with the case's window, observations `obs_offset` behind the clone times (true times; the stamps the tracks carry
    are these minus cam_dt)."""
    w, h = (1280, 720) if case.n_clones == 20 else (752, 480)
    sc = synth.vio_scene(n_clones=case.n_clones, F=case.F if case.kind == "points" else 4, M=case.M, seed=case.seed, noise_px=noise_px,
                         dt_clone=case.dt_clone, obs_offset=case.obs_offset, calib_int=case.calib_intr, fej_noise=case.fej_noise, w=w, h=h)
    sc["w"], sc["h"] = w, h
    return sc


def _residual_poses(case, sc, t_true, rng):
    """res_R / res_p (and, for "imu_cov", res_Q / res_clone) per observation, as test_line_jacobians_with_the_cpi_covariance_as_noise
    makes them: the trajectory's pose at the observation's time, disturbed by 1e-3; an SPD 6 x 6 and a clone index."""
    if case.noise not in ("imu_cov", "res_pose"):
        return {}
    nobs = len(t_true)
    out = dict(res_R=np.array([synth._exp_so3(rng.normal(0, 1e-3, 3)) @ sc["pose_fn"](t)[0] for t in t_true]),
               res_p=np.array([sc["pose_fn"](t)[1] + rng.normal(0, 1e-3, 3) for t in t_true]))
    if case.noise == "imu_cov":
        Aq = rng.normal(0, 1.0, (nobs, 6, 6)) * np.array([2e-3] * 3 + [8e-3] * 3)[None, :, None] * (LINE_Q_SCALE if case.kind == "lines" else 1.0)
        out["res_Q"] = (Aq @ np.transpose(Aq, (0, 2, 1))).reshape(nobs, 36)
        out["res_clone"] = rng.integers(0, len(sc["t"]), nobs).astype(np.int32)
    return out


def _state_view(pkg, case, sc, K8):
    n = sc["n_state"]
    kw = {}
    if case.calib_ext:
        kw["extrinsic_state_id"], n = n, n + 6
    if case.calib_dt:
        kw["dt_state_id"], n = n, n + 1
    if case.noise == "pol":
        kw.update(use_pol_cov=1, intr_ori_cov=1e-5, intr_pos_cov=2e-5)
    if case.noise == "imu_cov":
        kw.update(use_imu_cov=1, intr_err_mlt=3.0)
    st = pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], sc["R_ItoC"], sc["p_IinC"], K8, clone_R_fej=sc["Rf"], clone_p_fej=sc["pf"],
                       intrinsic_state_id=sc["intr_id"], sigma_pix=SIGMA_PIX, cam_dt=case.cam_dt, **kw)
    return st, n


def _line_scene(case, sc, L, seed, **kw):
    """synth.line_scene with the observations at the true (off-clone) times: line_scene reads the poses and times of the scene it is
    handed, so it is handed the trajectory's poses at the observation times"""
    off = np.where(np.arange(case.n_clones) < case.n_clones - 1, case.obs_offset, 0.0)
    t_obs = sc["t"] + off
    poses = [sc["pose_fn"](t) if o else (sc["R"][i], sc["p"][i]) for i, (t, o) in enumerate(zip(t_obs, off))]
    sc_obs = dict(sc, t=t_obs, R=np.array([q[0] for q in poses]), p=np.array([q[1] for q in poses]))
    return synth.line_scene(sc_obs, L=L, M=case.M, seed=seed, noise_px=0.4, w=sc["w"], h=sc["h"], **kw)


def build(pkg, case):
    """The case as the C-ABI takes it: dict(case, sc, st, tr, n, P, ld, fdim, min_rows, sigma2, res_norm_gate, has_oracle, K8)."""
    rng = np.random.default_rng(1000 + case.seed)
    K8 = STRONG if case.model == "equidistant" else synth.EUROC_K8
    if case.kind == "points":
        sc = _scene(case, noise_px=0.4)
        t_true = sc["obs_time"]
        uv = sc["obs_uv"].astype(np.float64)
        if case.model == "equidistant":
            import cam_equi
            uvn = np.zeros((len(t_true), 2))
            for f in range(case.F):
                for o in range(sc["obs_ptr"][f], sc["obs_ptr"][f + 1]):
                    R, p = sc["pose_fn"](t_true[o])
                    pc = sc["R_ItoC"] @ (R @ (sc["pts"][f] - p)) + sc["p_IinC"]
                    uvn[o] = pc[:2] / pc[2]
            uv = cam_equi.distort(K8, uvn).astype(np.float64) + rng.normal(0, 0.4, uvn.shape)
        outlier = np.zeros(case.F, dtype=bool)
        if case.outlier_px > 0:
            outlier[rng.choice(case.F, size=max(1, int(round(0.15 * case.F))), replace=False)] = True
            for f in np.nonzero(outlier)[0]:
                a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
                uv[a:b] += rng.normal(0, case.outlier_px, (b - a, 2))
        extra = _residual_poses(case, sc, t_true, rng)
        st, n = _state_view(pkg, case, sc, K8)
        tr = pkg.Tracks(sc["obs_ptr"], t_true - case.cam_dt, uv.astype(np.float32), sc["pts"], **extra)
        fdim, min_rows, gate = 3, 4, 3.0
        more = dict(outlier=outlier)
    else:
        sc = _scene(case, noise_px=1.0)
        ls = _line_scene(case, sc, case.F, case.seed)
        t_true = ls["obs_time"]
        extra = _residual_poses(case, sc, t_true, rng)
        st, n = _state_view(pkg, case, sc, K8)
        tr = pkg.LineTracks(ls["obs_ptr"], t_true - case.cam_dt, ls["seg_uv"], seg_uvn=ls["seg_uvn"], line_FinG=ls["lines"], **extra)
        fdim, min_rows, gate = 6, 5, 0.0
        more = dict(ls=ls)
    P = synth.spd_cov(n, seed=4 + case.seed) * 1e-4
    return dict(case=case, sc=sc, st=st, tr=tr, n=n, P=P, ld=2 * case.M + case.ld_extra, fdim=fdim, min_rows=min_rows, sigma2=SIGMA_PIX ** 2,
                res_norm_gate=gate, has_oracle=case.model == "radtan", K8=K8, **more)


# ------------------------------------------------------------------ the oracle's answers
def oracle_systems(jo, b):
    """(cols, rows, Hf, Hx, res) of the case from the oracle's unfused build"""
    if b["case"].kind == "points":
        cols = jo.columns(b["st"], b["tr"])
        return (cols,) + tuple(jo.build_jacobians(b["st"], b["tr"], cols, b["ld"]))
    cols = jo.line_columns(b["st"], b["tr"])
    return (cols,) + tuple(jo.build_line_jacobians(b["st"], b["tr"], cols, b["ld"]))


def oracle_update(oracle, b, systems):
    """dict(rc, P, dx, accepted, n_rows) of oracle.msckf_update on the case's covariance"""
    cols, rows, Hf, Hx, res = systems
    rc, P, dx, acc, nrows = oracle.msckf_update(b["P"], rows, Hf, Hx, res, cols, b["sigma2"], q95_table(), res_norm_gate=b["res_norm_gate"])
    return dict(rc=rc, P=P, dx=dx, accepted=acc, n_rows=nrows)


def reaches_gate(b, rows):
    """the features the update hands to the gate (REF UpdaterCamera.cpp:228 / :406, and at least one row left after the projection)"""
    rows = np.asarray(rows)
    return (rows >= b["min_rows"]) & (rows - b["fdim"] >= 1)


def gate_values_oracle(oracle, b, systems):
    """[F][3] = chi2, threshold, norm of the projected residual as the oracle's pieces (nullspace_batch with Givens rotations in the
    reference's order, chi2_batch) form them; NaN where the feature does not reach the gate"""
    cols, rows, Hf, Hx, res = systems
    reach = reaches_gate(b, rows)
    out = np.full((len(rows), 3), np.nan)
    if not reach.any():
        return out
    q95 = q95_table()
    idx = np.nonzero(reach)[0]           # (the oracle's pieces take every block they are handed: hand them the ones the gate sees)
    _, Hx_n, res_n = oracle.nullspace_batch(rows[idx], Hf[idx], Hx[idx], res[idx])
    r_out = (rows[idx] - b["fdim"]).astype(np.int32)
    chi = oracle.chi2_batch(b["P"], r_out, Hx_n, res_n, cols, b["sigma2"])
    for q, f in enumerate(idx):
        m = r_out[q]
        out[f] = chi[q], q95[m], np.sqrt(np.sum(res_n[q, :m] ** 2))
    return out


def gate_values_qr(b, systems):
    """The same values restated: LAPACK's QR of Hf for the left null space, numpy.linalg.solve for chi2 = r^T (H P H^T + sigma^2 I)^-1 r"""
    cols, rows, Hf, Hx, res = systems
    reach = reaches_gate(b, rows)
    q95 = q95_table()
    Ps = b["P"][np.ix_(cols, cols)]
    out = np.full((len(rows), 3), np.nan)
    for f in np.nonzero(reach)[0]:
        r, fd = int(rows[f]), b["fdim"]
        out[f, 1] = q95[r - fd]
        A, H, y = Hf[f, :, :r].T, Hx[f, :, :r].T, res[f, :r]
        if not (np.isfinite(A).all() and np.isfinite(H).all() and np.isfinite(y).all()):
            continue
        Q, _ = np.linalg.qr(A, mode="complete")
        N = Q[:, fd:]
        Hn, yn = N.T @ H, N.T @ y
        S = Hn @ Ps @ Hn.T + b["sigma2"] * np.eye(r - fd)
        out[f, 0], out[f, 2] = yn @ np.linalg.solve(S, yn), np.linalg.norm(yn)
    return out


def rel_diff(a, b):
    """largest relative difference of two arrays of positive test values; inf where exactly one side is NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    na, nb = np.isnan(a), np.isnan(b)
    if (na != nb).any():
        return np.inf
    ok = ~na
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.maximum(np.abs(a[ok]), np.abs(b[ok])), 1e-300)))


def spread(vals_oracle, vals_qr):
    """`s`: the largest relative difference of chi2 / residual norm between the oracle's values and their restatement, over the features
    that reach the gate with numbers (a NaN block is NaN on both sides: checked by the caller through rel_diff's inf)"""
    return max(rel_diff(vals_oracle[:, 0], vals_qr[:, 0]), rel_diff(vals_oracle[:, 2], vals_qr[:, 2]))


def value_bound(s):
    """The bound on chi2 and residual norm between the device and the oracle: 1e-8 is the project's own bound for recorded test values
    on identical input (decision_trace.check_tie's first_tol); 1e3 x s allows for the device building the Jacobians in another order
    where the value is ill-conditioned enough for that to matter (s only measures rounding-sized perturbations)."""
    return max(1e-8, 1e3 * s)


# ------------------------------------------------------------------ the one-call entry points
def one_call_tracks(b, undistort):
    """What the databases hold before the one-call update of a built case: (tracks, used).  points: tracks[id] = (t, uv, uvn);
    lines: tracks[id] = (t, seg_uv, seg_uvn, D, point ids) and used[point id] = (p_FinG, newest time) — a point ON the line for every
    third line, the reference's anchor of a classified line (D > 0)."""
    case, tr = b["case"], b["tr"]
    rng = np.random.default_rng(2000 + case.seed)
    tracks, used = {}, {}
    if case.kind == "points":
        for f in range(case.F):
            a, e = tr.ptr[f], tr.ptr[f + 1]
            tracks[f + 1] = (tr.t[a:e].copy(), tr.uv[a:e].copy(), undistort(b["K8"], tr.uv[a:e]))
        return tracks, used
    D = rng.integers(0, 4, case.F)
    newest = float(b["sc"]["t"][-1])
    for l in range(case.F):
        a, e = tr.ptr[l], tr.ptr[l + 1]
        tracks[l + 2] = (tr.t[a:e].copy(), tr.uv[a:e].copy(), tr.uvn[a:e].copy(), int(D[l]), [1000 + l, 2000 + l])
        if l % 3 == 1:
            nG, vG = b["ls"]["lines"][l, :3], b["ls"]["lines"][l, 3:]
            used[2000 + l] = (np.cross(vG, nG) + rng.uniform(-1, 1) * vG + rng.normal(0, 0.01, 3), newest)
    return tracks, used


def fill_databases(c, kind, tracks, used, device):
    """the same database contents into a device Context (device=True) or an oracle_lib.FrameOracle"""
    for fid, e in tracks.items():
        if kind == "points":
            (c.db_append_measurements if device else c.db_append)(fid, *e)
        else:
            (c.line_db_append_measurements if device else c.line_db_append)(fid, e[0], e[1], e[2], D=e[3], point_ids=e[4])
    for pid, (p, newest) in used.items():
        (c.point_used_insert if device else c.used_insert)(pid, p, newest)


def one_call_args(b):
    case, t = b["case"], b["sc"]["t"]
    kw = dict(t_prev_frame=float(t[-2]), state_time=float(t[-1]), window_full=True)
    if case.kind == "points":
        return (b["st"], b["n"], max(40, case.F // 2), case.M), dict(kw, **TRI)
    return (b["st"], b["n"], case.M), kw


def one_call_oracle(pkg, b, tracks, used):
    """The compiled CPU frame (oracle/frame_oracle.cpp: pool, triangulation, Jacobians, gate, update) on the same databases:
    dict(out, P, ids, vals) with (ids, vals) = last_point_decisions / last_line_decisions."""
    import oracle_lib
    sc, case = b["sc"], b["case"]
    cfg = pkg.default_config(sc["w"], sc["h"])
    fr = oracle_lib.FrameOracle(pkg, cfg, q95_table())
    fr.set_intrinsics(b["K8"])
    fill_databases(fr, case.kind, tracks, used, device=False)
    P = np.array(b["P"], dtype=np.float64, order="F")
    args, kw = one_call_args(b)
    if case.kind == "points":
        st, n, max_msckf, max_obs = args
        out = fr.update_points(P, st, max_msckf, max_obs, kw["t_prev_frame"], kw["state_time"], True, 1.0, 0.1, TRI["max_dist"], TRI["max_cond"], TRI["max_baseline"])
        ids_, vals = fr.last_point_decisions()
    else:
        st, n, max_obs = args
        out = fr.update_lines(P, st, max_obs, kw["t_prev_frame"], kw["state_time"], True)
        ids_, vals = fr.last_line_decisions()
    fr.close()
    return dict(out=out, P=P, ids=ids_, vals=vals)


def one_call_systems(pkg, jo, b, tracks, out):
    """The batch the one-call update gated, rebuilt from its own outputs (ids, triangulated features) with the oracle's unfused build:
    what gate_values_oracle / gate_values_qr / spread take.  Every observation of these scenes has bounding clones, so a selected track
    enters whole."""
    case = b["case"]
    sel = [int(i) for i in out["ids"]]
    ptr = np.concatenate([[0], np.cumsum([len(tracks[i][0]) for i in sel])]).astype(np.int32)
    cat = lambda j: np.concatenate([tracks[i][j] for i in sel])
    if case.kind == "points":
        tr = pkg.Tracks(ptr, cat(0), cat(1), out["p_FinG"])
    else:
        tr = pkg.LineTracks(ptr, cat(0), cat(1), line_FinG=out["line_FinG"])
    b2 = dict(b, tr=tr, ld=2 * case.M)
    return b2, oracle_systems(jo, b2)


# ------------------------------------------------------------------ both halves in one call (camera_try_update)
TRY_UPDATE_CASE = _point("try-update-130ms-fej-ext", (15, 60, 15), 0, 0.13, 1e-3, False, True, True, dt_clone=0.5, seed=12)
TRY_UPDATE_LINES = 50


def try_update_scene(pkg, undistort):
    """A window on which the point update moves the state before the line update linearises on it: off-clone times, first-estimate
    noise, extrinsics and intrinsics calibrated; the time offset is not (a launch chained behind the point update forms x (+) dx
    itself, and does so for poses, extrinsics and intrinsics).  Returns dict(b, tracks, used, ltracks, make_state)."""
    case = TRY_UPDATE_CASE
    b = build(pkg, case)
    tracks, _ = one_call_tracks(b, undistort)
    ls = _line_scene(case, b["sc"], TRY_UPDATE_LINES, 6, depth=(4.0, 14.0))
    lcase = case._replace(kind="lines", F=TRY_UPDATE_LINES)
    lb = dict(b, case=lcase, ls=ls, tr=pkg.LineTracks(ls["obs_ptr"], ls["obs_time"] - case.cam_dt, ls["seg_uv"], seg_uvn=ls["seg_uvn"], line_FinG=ls["lines"]))
    ltracks, used = one_call_tracks(lb, undistort)
    return dict(b=b, tracks=tracks, ltracks=ltracks, used=used, make_state=lambda: _moving_state(pkg, b))


def _moving_state(pkg, b):
    """(state view, BoxPlus, arrays to keep) of a built case with every variable of the view in the list the library moves: clone
    orientations (JPL quaternions, the view's rotation matrices their output), clone positions, extrinsics, intrinsics."""
    import ctypes as C
    from vio_sequence import rot_2_quat
    sc, st0 = b["sc"], b["st"]
    N = len(sc["t"])
    q = np.array([rot_2_quat(R) for R in sc["R"]])
    R = np.zeros((N, 9))
    pkg.jpl_left_update(q, None, R)                       # the view's matrices are the quaternions' own, bit for bit
    qe = rot_2_quat(sc["R_ItoC"]).reshape(1, 4)
    Re = np.zeros((1, 9))
    pkg.jpl_left_update(qe, None, Re)
    c0 = st0.c
    st = pkg.StateView(sc["t"].copy(), R, sc["p"].copy(), sc["ids"].copy(), Re.reshape(3, 3), sc["p_IinC"], b["K8"], clone_R_fej=sc["Rf"].copy(),
                       clone_p_fej=sc["pf"].copy(), cam_dt=c0.cam_dt, extrinsic_state_id=c0.extrinsic_state_id, intrinsic_state_id=c0.intrinsic_state_id,
                       dt_state_id=c0.dt_state_id, sigma_pix=c0.sigma_pix)
    base = C.addressof(st.c)
    off = lambda name: base + getattr(pkg.PlvStateView, name).offset
    K, pe = np.array(b["K8"], dtype=np.float64), np.array(sc["p_IinC"], dtype=np.float64)
    ent = []
    for i in range(N):
        ent += [("quat", int(st.ids[i]), q[i], st.R[i], None), ("vec", int(st.ids[i]) + 3, st.p[i], None, None)]
    if c0.extrinsic_state_id >= 0:
        ent += [("quat", c0.extrinsic_state_id, qe[0], Re[0], off("R_ItoC")), ("vec", c0.extrinsic_state_id + 3, pe, None, off("p_IinC"))]
    if c0.intrinsic_state_id >= 0:
        ent.append(("vec", c0.intrinsic_state_id, K, None, off("intrinsics")))
    return st, pkg.BoxPlus(ent), (q, qe, Re, K, pe)
