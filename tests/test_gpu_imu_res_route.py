"""est.use_imu_res on the one-submission updates (plv_update_options::cpi through plv_camera_update_points / _lines): which
observations the CPI table serves is decided on the host from times alone (cpi_servable), the poses of the distinct observation
times are formed by cpi_pose_kernel on the stream in front of the fused launch and read through JacParams::res_pose_of, and the
update takes the synchronisations it takes without a table.

Points: the composition of oracle pieces of test_gpu_update_frame.py::test_camera_update_points_with_cpi_poses (jo.cpi_poses, drop
unserved, jo.triangulate_batch, selection, jo.columns, jo.build_jacobians, oracle.msckf_update) and its bounds — ids, accepted set and
n_rows identical, p_FinG to 1e-6, dx to 1e-7 max(1, |dx|), P' to 1e-8 max|P| — on the shapes of that test (8 clones, 60 tracks of up
to 8 views).  Lines: jo.triangulate_lines on the state before a point correction, jo.build_line_jacobians on the state after it,
both with the table's poses of their own state, to the line bounds of test_gpu_fused_launches.py::_check_update.

Measured on an MI355X (largest absolute differences; pool / selected / accepted by the oracle composition):
  points a-between-records            50 / 50 / 50 | p_FinG 0.0e+00  dx 1.0e-18 of 1.3e-04  P' 4.2e-22 of 9.8e-07
  points b-track-left-with-one-view   50 / 49 / 49 | p_FinG 0.0e+00  dx 8.8e-19 of 1.2e-04  P' 5.3e-22 of 9.8e-07
  points c-pool-above-the-cap         50 / 20 / 20 | p_FinG 0.0e+00  dx 6.7e-19 of 1.4e-04  P' 8.5e-22 of 9.8e-07
  points d-imu-cov                    50 / 50 / 50 | p_FinG 0.0e+00  dx 7.6e-19 of 2.2e-05  P' 8.5e-22 of 9.8e-07
  points e-on-clone-times             50 / 50 / 50 | p_FinG 7.1e-15  dx 8.8e-19 of 1.0e-04  P' 6.4e-22 of 9.8e-07
  lines  wide-easiest                 36 / 32 /  6 | line_FinG 0.0e+00  dx 2.0e-15 of 2.6e-03  P' 1.4e-18 of 7.1e-07
  lines  wide-130ms-fej-dt            36 / 32 /  5 | line_FinG 0.0e+00  dx 3.4e-16 of 6.7e-04  P' 1.0e-19 of 8.7e-07
On the commit before this route the synchronisation test fails (the table cost the point and the line update extra
synchronisations) and so do the line cases (one pose set, the corrected state's, served triangulation and rows alike).  The module
runs in about 3 s."""
import numpy as np
import pytest

import fused_cases as fc
import oracle_lib
import synth

pytestmark = pytest.mark.gpu

TRI = dict(max_cond=1e7, max_dist=100.0, max_baseline=1e3)
MOBS = 10
DT_EXP = 0.01          # pkg.StateView's default: the margin of the window tests


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


# ------------------------------------------------------------------ points
# name: (obs_offset, max_msckf, what is done to the tracks)
POINT_VARIANTS = {
    "a-between-records": (0.0125, 64, "late"),          # pool below the cap: triangulation inside the fused launch
    "b-track-left-with-one-view": (0.0125, 64, "starved"),
    "c-pool-above-the-cap": (0.0125, 20, "late"),       # the device's selection loop cuts the pool
    "d-imu-cov": (0.0125, 64, "late"),
    "e-on-clone-times": (0.0, 64, "none"),              # the record stored at t: nothing is interpolated
    "edges": (0.0125, 64, "edges"),                     # before the first record, between the records of two clones
    "left-window": (0.0125, 64, "left"),                # records of a clone that is no longer in the window
}
_RUNS = {}


def _noise_of(tab, clone_times, tq):
    """res_Q / res_clone of served query times, restated: the stored record's covariance, or the blend of its two neighbours'"""
    Q, ci = np.zeros((len(tq), 36)), np.zeros(len(tq), dtype=np.int32)
    for j, t in enumerate(tq):
        e = int(np.searchsorted(tab.t, t))
        if e < len(tab.t) and tab.t[e] == t:
            Q[j], ct = tab.Q[e], tab.clone_t[e]
        else:
            lam = (t - tab.t[e - 1]) / (tab.t[e] - tab.t[e - 1])
            Q[j], ct = (1 - lam) * tab.Q[e - 1] + lam * tab.Q[e], tab.clone_t[e - 1]
        ci[j] = int(np.flatnonzero(clone_times == ct)[0])
    return Q, ci


def _points_run(pkg, oracle, jo, name):
    """One variant, once: the device's update on a fresh context and the oracle composition on the same databases."""
    if name in _RUNS:
        return _RUNS[name]
    fo = oracle_lib.load_front()
    offset, MAX, edit = POINT_VARIANTS[name]
    imu_cov = name == "d-imu-cov"
    sc = synth.vio_scene(n_clones=8, F=60, M=8, noise_px=0.4, seed=12, obs_offset=offset)
    cp = synth.cpi_scene(sc)
    K8, n = sc["K8"], sc["n_state"]
    rng = np.random.default_rng(5)
    Qtab = None
    if imu_cov:
        A = rng.normal(0, 1.0, (len(cp["t"]), 6, 6)) * np.array([2e-3] * 3 + [8e-3] * 3)[None, :, None]
        Qtab = (A @ np.transpose(A, (0, 2, 1))).reshape(-1, 36)
    tab = pkg.CpiTable(cp["t"], cp["clone_t"], cp["R"], cp["alpha"], cp["v"], gravity=cp["gravity"], Q=Qtab)
    view_kw = dict(use_imu_cov=1, intr_err_mlt=3.0) if imu_cov else {}
    if edit == "left":       # the window has lost its oldest clone; the table still holds that clone's records
        sc_v = dict(sc, t=sc["t"][1:], R=sc["R"][1:], p=sc["p"][1:], Rf=sc["Rf"][1:], pf=sc["pf"][1:], ids=sc["ids"][1:])
    else:
        sc_v = sc
    st, _ = synth.scene_views(pkg, sc_v, **view_kw)
    t = sc_v["t"]
    tracks = {}
    for f in range(60):
        a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
        uv = sc["obs_uv"][a:b].astype(np.float32)
        tracks[f + 1] = [sc["obs_time"][a:b].copy(), uv, fo.undistort(K8, uv)]
    late = float(cp["t"][-1] + 0.004)      # beyond the table's last record: nothing to interpolate towards
    full = [fid for fid in sorted(tracks) if len(tracks[fid][0]) == 8 and fid != 5]
    special = {}
    if edit in ("late", "starved"):
        tracks[5][0][-1] = late
        special[5] = [late]
    if edit == "starved":
        fid = full[3]
        tracks[fid][0][1:] = late + 0.001 * np.arange(1, 8)
        special[fid] = list(tracks[fid][0][1:])
    if edit == "edges":
        before_first = float(cp["t"][0] - 0.5 * DT_EXP)                 # inside the window's margin, before the first record
        last_of_2 = float(cp["t"][cp["clone_t"] == sc["t"][2]][-1])
        two_clones = 0.5 * (last_of_2 + float(sc["t"][3]))              # between the last record of clone 2 and the first of clone 3
        for fid, (i, tm) in zip(full[2:4], ((0, before_first), (3, two_clones))):
            tracks[fid][0][i] = tm
            special[fid] = [tm]
    if edit == "left":
        gone = float(cp["t"][cp["clone_t"] == sc["t"][0]][-1])          # the last record of clone 0, stored at exactly this time
        assert sc["t"][1] - DT_EXP < gone < sc["t"][1]                  # (inside the window's margin)
        for fid in full[2:4]:
            tracks[fid][0][0] = gone
            special[fid] = [gone]
    state_time = late + 0.1
    window_full = edit not in ("edges", "left")     # (the clean-up of a full window drops what is older than the oldest clone: the returned views would be gone)
    P = synth.spd_cov(n, seed=4) * 1e-4

    ctx = pkg.Context(pkg.default_config(752, 480))
    try:
        for fid, (tt, uv, uvn) in tracks.items():
            ctx.db_append_measurements(fid, tt, uv, uvn)
        ctx.cov_upload(P)
        s0 = pkg.counters()["syncs"]
        out = ctx.camera_update_points(st, n, MAX, MOBS, t_prev_frame=t[-2], state_time=state_time, window_full=window_full, cpi=tab, **TRI)
        syncs = pkg.counters()["syncs"] - s0
        P_dev = ctx.cov_download(n)
        ids_all = np.array(sorted(tracks), dtype=np.uint64)
        ptr_db, t_db, _, _ = ctx.db_export(ids_all)
        db = {int(fid): np.sort(t_db[ptr_db[j]:ptr_db[j + 1]]) for j, fid in enumerate(ids_all)}
        # ---- the window's trim (CamHelper.cpp:740-775), then the pool in the update's order
        pool_all = [fid for fid, (tt, _, _) in sorted(tracks.items()) if (tt < t[1]).any() or not (tt > t[-2]).any()]
        win = {}
        for fid in pool_all:
            tt = tracks[fid][0]
            assert not (tt > state_time + DT_EXP).any()
            m = ~(tt < t[0] - DT_EXP)
            win[fid] = tuple(x[m] for x in tracks[fid])
        pool = [fid for fid in pool_all if len(win[fid][0]) >= 2]
        pool.sort(key=lambda fid: -len(win[fid][0]))
        tq = np.concatenate([win[f][0] for f in pool])
        # ---- which of them the table serves: the device's own answer (plv_cpi_poses' ok), and the oracle's
        _, _, ok_dev = ctx.cpi_poses(st, tab, tq)
    finally:
        ctx.close()
    Rq, pq, okq = jo.cpi_poses(st, tab, tq)
    ptr = np.concatenate([[0], np.cumsum([len(win[f][0]) for f in pool])])
    kept = {}
    for j, f in enumerate(pool):
        m = okq[ptr[j]:ptr[j + 1]].astype(bool)
        kept[f] = (win[f][0][m], win[f][1][m], win[f][2][m], Rq[ptr[j]:ptr[j + 1]][m], pq[ptr[j]:ptr[j + 1]][m])
    cand = [f for f in pool if len(kept[f][0]) >= 2]      # (fewer than two views left: never a candidate, CamHelper.cpp:656-661)
    kptr = np.concatenate([[0], np.cumsum([len(kept[f][0]) for f in cand])]).astype(np.int32)
    cat = lambda i: np.concatenate([kept[f][i] for f in cand])
    tr_all = pkg.Tracks(kptr, cat(0), cat(1), np.zeros((len(cand), 3)), obs_uvn=cat(2), res_R=cat(3), res_p=cat(4))
    p_o, ok_o, err_o = jo.triangulate_batch(st, tr_all, **TRI)
    passing = [q for q in range(len(cand)) if ok_o[q] and err_o[q] < 3.0]
    sel = passing[:MAX]
    sptr = np.concatenate([[0], np.cumsum([len(kept[cand[q]][0]) for q in sel])]).astype(np.int32)
    scat = lambda i: np.concatenate([kept[cand[q]][i] for q in sel])
    noise = {}
    if imu_cov:
        noise["res_Q"], noise["res_clone"] = _noise_of(tab, t, scat(0))
    tr_sel = pkg.Tracks(sptr, scat(0), scat(1), p_o[sel], res_R=scat(3), res_p=scat(4), **noise)
    cols = jo.columns(st, tr_sel)
    rows, Hf, Hx, res = jo.build_jacobians(st, tr_sel, cols, 2 * MOBS)
    rc_o, P_o, dx_o, acc_o, nrows_o = oracle.msckf_update(P, rows, Hf, Hx, res, cols, st.c.sigma_pix ** 2, synth.q95_table())
    _RUNS[name] = dict(out=out, P_dev=P_dev, P=P, db=db, pool_all=pool_all, pool=pool, win=win, tq=tq, ptr=ptr, ok_dev=ok_dev, okq=okq, passing=passing,
                       sel=sel, cand=cand, t=t, p_o=p_o, rc_o=rc_o, P_o=P_o, dx_o=dx_o, acc_o=acc_o, nrows_o=nrows_o, special=special, MAX=MAX, syncs=syncs, tracks=tracks,
                       late=late)
    return _RUNS[name]


@pytest.mark.parametrize("name", [k for k in POINT_VARIANTS if k[1] == "-"])
def test_point_update_with_cpi_poses_against_the_oracle(pkg, oracle, jo, name):
    r = _points_run(pkg, oracle, jo, name)
    out, sel, pool, cand, acc_o, dx_o = r["out"], r["sel"], r["pool"], r["cand"], r["acc_o"], r["dx_o"]
    # the oracle composition alone: enough accepted for the comparison to show something
    assert r["rc_o"] == 0 and acc_o.sum() >= 15, (r["rc_o"], int(acc_o.sum()))
    if name.startswith("a") or name.startswith("c") or name.startswith("d"):
        assert (r["okq"] == 0).sum() == 1 and not r["okq"][np.flatnonzero(r["tq"] == r["late"])[0]]
    if name.startswith("c"):
        assert len(pool) > r["MAX"] and len(r["passing"]) > r["MAX"] == len(sel)      # the cap cuts the pool
    else:
        assert len(pool) <= r["MAX"]
    if name.startswith("e"):
        assert r["okq"].all() and np.isin(r["tq"], r["t"]).all()           # every view on a clone time, every one served
    print(f"{name}: pool {len(pool)}, selected {len(sel)}, accepted {int(acc_o.sum())}, p_FinG {np.abs(out['p_FinG'] - r['p_o'][sel]).max():.1e}, "
          f"dx {np.abs(out['dx'] - dx_o).max():.1e} of {np.abs(dx_o).max():.1e}, P' {np.abs(r['P_dev'] - r['P_o']).max():.1e} of {np.abs(r['P']).max():.1e}")
    assert out["status"] == 0 and out["n_pool"] == len(r["pool_all"])
    assert np.array_equal(out["ids"], np.array([cand[q] for q in sel], dtype=np.uint64))
    assert np.array_equal(out["accepted"], acc_o) and out["n_rows"] == r["nrows_o"]
    assert np.abs(out["p_FinG"] - r["p_o"][sel]).max() < 1e-6
    assert np.abs(out["dx"] - dx_o).max() <= 1e-7 * max(1.0, np.abs(dx_o).max())
    assert np.abs(r["P_dev"] - r["P_o"]).max() <= 1e-8 * np.abs(r["P"]).max()
    if name.startswith("b"):      # the starved track: one view left, not selected, every view of it back in the database
        fid = [f for f in r["special"] if f != 5][0]
        assert fid in pool and fid not in cand and fid not in [int(i) for i in out["ids"]]
        assert np.array_equal(r["db"][fid], np.sort(r["tracks"][fid][0]))


@pytest.mark.parametrize("name", ["a-between-records", "b-track-left-with-one-view", "e-on-clone-times", "edges", "left-window"])
def test_host_validity_rule_equals_the_pose_kernels(pkg, oracle, jo, name):
    """cpi_servable (host, times only) drops what cpi_pose_kernel reports as ok == 0, and nothing else: a consumed track leaves exactly
    its unserved views in the database, every other pool track is back whole."""
    r = _points_run(pkg, oracle, jo, name)
    out, pool, ptr, ok_dev = r["out"], r["pool"], r["ptr"], r["ok_dev"]
    assert np.array_equal(ok_dev, r["okq"])                      # (the kernel's rule is the oracle's)
    n_unserved = {"a-between-records": 1, "b-track-left-with-one-view": 8, "e-on-clone-times": 0, "edges": 2, "left-window": 2}[name]
    assert (ok_dev == 0).sum() == n_unserved, (ok_dev == 0).sum()
    consumed = {int(i) for i, a in zip(out["ids"], out["accepted"]) if a}
    seen = 0
    for j, fid in enumerate(pool):
        tt, ok = r["win"][fid][0], ok_dev[ptr[j]:ptr[j + 1]].astype(bool)
        for tm in r["special"].get(fid, []):
            assert not ok[np.flatnonzero(tt == tm)[0]], (fid, tm)
        if fid in consumed:
            assert np.array_equal(r["db"][fid], np.sort(tt[~ok])), (fid, r["db"][fid], tt[~ok])
            seen += int((~ok).sum())
        else:
            assert np.array_equal(r["db"][fid], np.sort(tt)), (fid, r["db"][fid], tt)
    if name != "b-track-left-with-one-view":
        assert seen == n_unserved, (seen, n_unserved)            # every unserved view sat on a track the update consumed: the exact set was seen
    else:
        assert seen == 1


# ------------------------------------------------------------------ lines
def _moved(pkg, b, rng):
    """the state view of a built case after a point correction: clone orientations and positions moved by ~1e-3, first estimates kept"""
    sc, c0 = b["sc"], b["st"].c
    R = np.array([synth._exp_so3(rng.normal(0, 1e-3, 3)) @ Ri for Ri in sc["R"]])
    p = sc["p"] + rng.normal(0, 1e-3, sc["p"].shape)
    return pkg.StateView(sc["t"], R, p, sc["ids"], sc["R_ItoC"], sc["p_IinC"], b["K8"], clone_R_fej=sc["Rf"], clone_p_fej=sc["pf"],
                         intrinsic_state_id=c0.intrinsic_state_id, dt_state_id=c0.dt_state_id, sigma_pix=c0.sigma_pix, cam_dt=c0.cam_dt)


def _line_case(pkg, case):
    fo = oracle_lib.load_front()
    b = fc.build(pkg, case)
    tracks, used = fc.one_call_tracks(b, fo.undistort)
    cp = synth.cpi_scene(b["sc"], imu_dt=0.05)                  # (clones 0.5 s apart: ten records each)
    tab = pkg.CpiTable(cp["t"], cp["clone_t"], cp["R"], cp["alpha"], cp["v"], gravity=cp["gravity"])
    return b, tracks, used, tab


@pytest.mark.parametrize("case", [c for c in fc.ONE_CALL_LINE_CASES if c.name in ("wide-easiest", "wide-130ms-fej-dt")], ids=lambda c: c.name)
def test_line_update_with_cpi_poses_against_the_oracle(pkg, oracle, jo, case):
    """camera_get_line_features on the state before a point correction, camera_update_lines with the table on the state after it: the
    lines are triangulated on the table's poses of the first, the rows taken at the table's poses of the second."""
    b, tracks, used, tab = _line_case(pkg, case)
    st_pre, n, t, M = b["st"], b["n"], b["sc"]["t"], case.M
    st_post = _moved(pkg, b, np.random.default_rng(77))
    kw = dict(t_prev_frame=float(t[-2]), state_time=float(t[-1]), window_full=True)
    c = pkg.Context(pkg.default_config(b["sc"]["w"], b["sc"]["h"]))
    try:
        fc.fill_databases(c, "lines", tracks, used, device=True)
        c.cov_upload(b["P"])
        c.camera_get_line_features(st_pre)
        out = c.camera_update_lines(st_post, n, M, cpi=tab, **kw)
        P_dev = c.cov_download(n)
    finally:
        c.close()
    # ---- the oracle composition (test_gpu_update_frame.py::test_camera_update_lines, with res_R / res_p)
    pool = [k for k in sorted(tracks) if (tracks[k][0] < t[1]).any() or not (tracks[k][0] > t[-2]).any()]
    order = sorted(pool, key=lambda k: -len(tracks[k][0]))
    ptr = np.concatenate([[0], np.cumsum([len(tracks[k][0]) for k in order])]).astype(np.int32)
    tq = np.concatenate([tracks[k][0] for k in order]) + case.cam_dt
    R0, p0, ok0 = jo.cpi_poses(st_pre, tab, tq)
    R1, p1, ok1 = jo.cpi_poses(st_post, tab, tq)
    assert ok0.all() and ok1.all() and np.abs(R0 - R1).max() > 1e-4          # every view served; two different pose sets
    has = np.array([1 if 2000 + (k - 2) in used else 0 for k in order], dtype=np.uint8)
    anchor = np.array([used[2000 + (k - 2)][0] if 2000 + (k - 2) in used else np.zeros(3) for k in order])
    cat = lambda j: np.concatenate([tracks[k][j] for k in order])
    lt_all = pkg.LineTracks(ptr, cat(0), cat(1), seg_uvn=cat(2), D=[tracks[k][3] for k in order], anchor_pt=anchor, has_pt=has, res_R=R0, res_p=p0)
    lg_o, ok_o = jo.triangulate_lines(st_pre, lt_all)
    lg_wrong, _ = jo.triangulate_lines(st_pre, pkg.LineTracks(ptr, cat(0), cat(1), seg_uvn=cat(2), D=[tracks[k][3] for k in order], anchor_pt=anchor,
                                                              has_pt=has, res_R=R1, res_p=p1))
    sel = [q for q in range(len(order)) if ok_o[q]]
    assert len(sel) >= 5 and np.abs(lg_wrong[sel] - lg_o[sel]).max() > 1e-6 * np.abs(lg_o[sel]).max()      # (the other pose set would show)
    sptr = np.concatenate([[0], np.cumsum([len(tracks[order[q]][0]) for q in sel])]).astype(np.int32)
    pick = np.concatenate([np.arange(ptr[q], ptr[q + 1]) for q in sel])
    scat = lambda j: np.concatenate([tracks[order[q]][j] for q in sel])
    lt = pkg.LineTracks(sptr, scat(0), scat(1), line_FinG=lg_o[sel], res_R=R1[pick], res_p=p1[pick])
    cols = jo.line_columns(st_post, lt)
    rows, Hf, Hx, res = jo.build_line_jacobians(st_post, lt, cols, 2 * M)
    rc_o, P_o, dx_o, acc_o, nrows_o = oracle.msckf_update(b["P"], rows, Hf, Hx, res, cols, b["sigma2"], fc.q95_table(), res_norm_gate=0.0)
    assert rc_o == 0 and acc_o.sum() >= 1
    print(f"lines {case.name}: pool {len(pool)}, triangulated {len(sel)}, accepted {int(acc_o.sum())}, line_FinG {np.abs(out['line_FinG'] - lg_o[sel]).max():.1e}, "
          f"dx {np.abs(out['dx'] - dx_o).max():.1e} of {np.abs(dx_o).max():.1e}, P' {np.abs(P_dev - P_o).max():.1e} of {np.abs(b['P']).max():.1e}")
    assert out["status"] == 0 and out["n_pool"] == len(pool)
    assert np.array_equal(out["ids"], np.array([order[q] for q in sel], dtype=np.uint64))
    assert np.abs(out["line_FinG"] - lg_o[sel]).max() <= 1e-9 * max(1.0, np.abs(lg_o).max())
    assert np.array_equal(out["accepted"], acc_o) and out["n_rows"] == nrows_o
    assert np.isfinite(out["dx"]).all() and np.isfinite(P_dev).all()
    assert np.abs(out["dx"] - dx_o).max() <= 1e-7 * max(1.0, np.abs(dx_o).max())
    assert np.abs(P_dev - P_o).max() <= 1e-8 * np.abs(b["P"]).max()


# ------------------------------------------------------------------ the route
def test_cpi_updates_take_the_synchronisations_of_the_polynomial_ones(pkg, oracle, jo):
    """Twin contexts, same tracks and covariance: the update with a CPI table synchronises the host as often as the one without.  (On
    the two-step route the table cost a synchronisation for the poses and one for the triangulation on top.)"""
    fo = oracle_lib.load_front()
    # ---- points: every view on a clone time, so that both calls see the same pool
    sc = synth.vio_scene(n_clones=8, F=60, M=8, noise_px=0.4, seed=12, obs_offset=0.0)
    cp = synth.cpi_scene(sc)
    tab = pkg.CpiTable(cp["t"], cp["clone_t"], cp["R"], cp["alpha"], cp["v"], gravity=cp["gravity"])
    st, _ = synth.scene_views(pkg, sc)
    t, n = sc["t"], sc["n_state"]
    P = synth.spd_cov(n, seed=4) * 1e-4
    syncs, outs = {}, {}
    for with_cpi in (False, True):
        c = pkg.Context(pkg.default_config(752, 480))
        try:
            for f in range(60):
                a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
                uv = sc["obs_uv"][a:b].astype(np.float32)
                c.db_append_measurements(f + 1, sc["obs_time"][a:b], uv, fo.undistort(sc["K8"], uv))
            c.cov_upload(P)
            c.synchronize()
            s0 = pkg.counters()["syncs"]
            outs[with_cpi] = c.camera_update_points(st, n, 64, MOBS, t_prev_frame=t[-2], state_time=float(t[-1]), window_full=True,
                                                    cpi=tab if with_cpi else None, **TRI)
            syncs[with_cpi] = pkg.counters()["syncs"] - s0
        finally:
            c.close()
    assert outs[True]["n_accepted"] >= 15 and outs[False]["n_accepted"] >= 15 and np.array_equal(outs[True]["ids"], outs[False]["ids"])
    assert syncs[True] == syncs[False] >= 1, syncs
    # ---- lines
    case = [x for x in fc.ONE_CALL_LINE_CASES if x.name == "wide-easiest"][0]
    b, tracks, used, tab = _line_case(pkg, case)
    t = b["sc"]["t"]
    for with_cpi in (False, True):
        c = pkg.Context(pkg.default_config(b["sc"]["w"], b["sc"]["h"]))
        try:
            fc.fill_databases(c, "lines", tracks, used, device=True)
            c.cov_upload(b["P"])
            c.synchronize()
            s0 = pkg.counters()["syncs"]
            outs[with_cpi] = c.camera_update_lines(b["st"], b["n"], case.M, t_prev_frame=float(t[-2]), state_time=float(t[-1]), window_full=True,
                                                   cpi=tab if with_cpi else None)
            syncs[with_cpi] = pkg.counters()["syncs"] - s0
        finally:
            c.close()
    assert outs[True]["n_lines"] >= 5 and np.array_equal(outs[True]["ids"], outs[False]["ids"])
    assert syncs[True] == syncs[False] >= 1, syncs
