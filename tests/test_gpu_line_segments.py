"""The line map on the device: plv_line_segments (csrc/line_map_kernels.hip) against its numpy restatement
(tests/line_segments_ref.py, DESIGN.md "The line map"), plv_camera_used_lines behind a line update, the mode switch's promise that
"off" changes nothing, and the driver's map getters over a short replay."""
import importlib

import numpy as np
import pytest

import line_segments_ref as ref
import synth
import synth_dataset as sd

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ plv_line_segments
@pytest.fixture(scope="module")
def scene():
    """ref.gpu_scene() and its reference results, once: with polynomial poses and with res_R / res_p on the tracks"""
    sc, ls = ref.gpu_scene()
    rng = np.random.default_rng(5)
    t_in = np.clip(ls["obs_time"], sc["t"][0], sc["t"][-1])      # (an observation outside the window still needs some pose in the array)
    res_R = np.array([synth._exp_so3(rng.normal(0, 2e-3, 3)) @ sc["pose_fn"](t)[0] for t in t_in])
    res_p = np.array([sc["pose_fn"](t)[1] + rng.normal(0, 2e-3, 3) for t in t_in])
    out = {}
    for poses, kw in (("polynomial", {}), ("res", dict(res_R=res_R, res_p=res_p))):
        out[poses] = (kw, ref.line_segments(sc["t"], sc["R"], sc["p"], sc["R_ItoC"], sc["p_IinC"], 0.0, 0.01, ls["obs_ptr"], ls["obs_time"],
                                             ls["seg_uvn"], ls["lines"], **kw))
    return sc, ls, out


@pytest.mark.parametrize("poses", ["polynomial", "res"])
@pytest.mark.parametrize("L", [1, 4, 5, 67])      # one wave, a full workgroup, one wave into the next workgroup, many workgroups
def test_line_segments_match_the_restatement(ctx, pkg, scene, L, poses):
    sc, ls, refs = scene
    kw, (ep_r, ext_r, nv_r, ok_r) = refs[poses]
    n = ls["obs_ptr"][L]
    st, _ = synth.scene_views(pkg, sc)
    lt = pkg.LineTracks(ls["obs_ptr"][:L + 1], ls["obs_time"][:n], ls["seg_uv"][:n], seg_uvn=ls["seg_uvn"][:n], line_FinG=ls["lines"][:L],
                        **{k: v[:n] for k, v in kw.items()})
    ep, ext, nv, ok = ctx.line_segments(st, lt)
    print(f"L={L} {poses}: n_views {nv.tolist()[:8]}..., |end points - ref| max {np.abs(ep - ep_r[:L]).max():.3g}, |extent - ref| max "
          f"{np.abs(ext - ext_r[:L]).max():.3g}")
    assert np.array_equal(ok, ok_r[:L]) and np.array_equal(nv, nv_r[:L])
    assert (np.abs(ep - ep_r[:L]) <= 1e-9 * np.maximum(1.0, np.abs(ep_r[:L]))).all()
    assert (np.abs(ext - ext_r[:L]) <= 1e-9 * np.maximum(1.0, np.abs(ext_r[:L]))).all()
    if L == 67:      # the scene holds what the test is after (tests/test_line_segments_cpu.py asserts it of the restatement)
        assert {1, 2, 3, 63, 64}.issubset(set(nv.tolist())) and np.diff(ls["obs_ptr"]).max() >= 65 and (nv < np.diff(ls["obs_ptr"])).sum() >= 10


def test_a_line_without_a_counted_view_returns_exact_zeros(ctx, pkg, scene):
    sc, ls, _ = scene
    st, _ = synth.scene_views(pkg, sc)
    L, n = 6, ls["obs_ptr"][6]
    t = ls["obs_time"][:n].copy()
    t[ls["obs_ptr"][1]:ls["obs_ptr"][2]] = sc["t"][-1] + 5.0      # line 1: every view outside the window
    lines = ls["lines"][:L].copy()
    lines[2, 3:] = 0.0                                             # line 2: no direction
    lines[4, 1] = np.nan                                           # line 4: not finite
    lt = pkg.LineTracks(ls["obs_ptr"][:L + 1], t, ls["seg_uv"][:n], seg_uvn=ls["seg_uvn"][:n], line_FinG=lines)
    ep, ext, nv, ok = ctx.line_segments(st, lt)
    assert ok.tolist() == [1, 0, 0, 1, 0, 1] and nv[[1, 2, 4]].tolist() == [0, 0, 0]
    for l in (1, 2, 4):
        assert ep[l].tobytes() == bytes(48) and ext[l].tobytes() == bytes(16)
    ep_r, ext_r, nv_r, ok_r = ref.segments_of(st, lt)
    assert np.array_equal(ok, ok_r) and np.array_equal(nv, nv_r)


# ------------------------------------------------------------------------------------------------ plv_camera_used_lines
def _filled_context(pkg, sc, ls, D, pts):
    """a context with the scene's line tracks in its database (as tests/test_gpu_update_frame.py builds it)"""
    ctx = pkg.Context(pkg.default_config(752, 480))
    tracks = {}
    for l in range(len(D)):
        a, b = ls["obs_ptr"][l], ls["obs_ptr"][l + 1]
        pid = [1000 + l, 2000 + l]
        tracks[l + 2] = (ls["obs_time"][a:b].copy(), ls["seg_uv"][a:b].copy(), ls["seg_uvn"][a:b].copy())
        ctx.line_db_append_measurements(l + 2, *tracks[l + 2], D=int(D[l]), point_ids=pid)
        if l % 3 == 1:
            ctx.point_used_insert(2000 + l, pts[l], sc["t"][-1])
    ctx.cov_upload(synth.spd_cov(sc["n_state"], seed=4) * 1e-4)
    return ctx, tracks


def _databases(ctx):
    """every byte the update can leave in the context's two track databases: the line tracks (times, raw and normalised segments,
    direction class, point ids) in id order, and the point database's size (the scene puts no point tracks in)"""
    ids = np.sort(ctx.line_db_ids())
    ex = ctx.line_db_export(ids)
    return dict(ids=ids.tobytes(), points=ctx.db_size(), **{k: np.ascontiguousarray(v).tobytes() for k, v in ex.items()})


@pytest.fixture(scope="module")
def updates(pkg):
    """The same two line updates in a row on three contexts: map mode on / switched on and off again beforehand / never touched.
    Returns what each returned and left behind.  The second update runs on what the first handed back — the returned tracks, the
    covariance, and point_used (which the C ABI does not export: its entries anchor the lines with a direction class, so a change
    there shows in the second update's line_FinG).  For the context with the mode on, what plv_camera_used_lines returned between
    the two updates is kept as well."""
    sc = synth.vio_scene(F=4, calib_int=True, dt_clone=0.5, seed=2)
    ls = synth.line_scene(sc, L=50, noise_px=0.3, depth=(4.0, 14.0), seed=6)
    st, _ = synth.scene_views(pkg, sc)
    rng = np.random.default_rng(3)
    D, pts = rng.integers(0, 4, 50), rng.normal(size=(50, 3)) * 4 + np.array([0, 0, 8.0])
    t, n = sc["t"], sc["n_state"]
    runs = {}
    for name in ("on", "toggled", "plain"):
        ctx, tracks = _filled_context(pkg, sc, ls, D, pts)
        r = runs[name] = dict(ctx=ctx, tracks=tracks)
        if name == "on":
            assert ctx.line_map_mode() is False
            ctx.line_map_mode(True)
            assert ctx.line_map_mode() is True and len(ctx.camera_used_lines(st)["ids"]) == 0      # no update yet
        elif name == "toggled":
            ctx.line_map_mode(True), ctx.line_map_mode(False)
        r["out"] = ctx.camera_update_lines(st, n, 15, t_prev_frame=t[-2], state_time=t[-1], window_full=True)
        r["P"], r["db"] = ctx.cov_download(n), _databases(ctx)
        r["used"] = [ctx.camera_used_lines(st), ctx.camera_used_lines(st)]
        r["P_read"], r["db_read"] = ctx.cov_download(n), _databases(ctx)
        r["out2"] = ctx.camera_update_lines(st, n, 15, t_prev_frame=t[-2], state_time=t[-1], window_full=True)
        r["P2"], r["db2"] = ctx.cov_download(n), _databases(ctx)
    yield sc, st, runs
    for r in runs.values():
        r["ctx"].close()


def test_used_lines_are_the_updates_batch_with_the_restatements_end_points(pkg, updates):
    sc, st, runs = updates
    r = runs["on"]
    ctx, out, n = r["ctx"], r["out"], sc["n_state"]
    assert out["status"] == 0 and out["n_lines"] > 20 and out["n_accepted"] >= 1
    ul, again = r["used"]
    assert ul["ids"].tobytes() == out["ids"].tobytes() and ul["accepted"].tobytes() == out["accepted"].tobytes()
    assert ul["line_FinG"].tobytes() == out["line_FinG"].tobytes()
    # the end points: the restatement on the tracks the update saw (every view of this scene lies inside the window)
    tr = [r["tracks"][int(i)] for i in ul["ids"]]
    ptr = np.concatenate([[0], np.cumsum([len(x[0]) for x in tr])]).astype(np.int32)
    lt = pkg.LineTracks(ptr, np.concatenate([x[0] for x in tr]), np.concatenate([x[1] for x in tr]), seg_uvn=np.concatenate([x[2] for x in tr]),
                        line_FinG=out["line_FinG"])
    ep_r, _, nv_r, ok_r = ref.segments_of(st, lt)
    print(f"used lines: {len(ul['ids'])}, ok {int(ul['ok'].sum())}, |end points - ref| max {np.abs(ul['end_points'] - ep_r).max():.3g}")
    assert np.array_equal(ul["ok"], ok_r) and ok_r.sum() > 20
    assert (np.abs(ul["end_points"] - ep_r) <= 1e-9 * np.maximum(1.0, np.abs(ep_r))).all()
    # read-only: the same bytes again, the filter and both databases as before the calls
    assert all(again[k].tobytes() == ul[k].tobytes() for k in ul)
    assert r["P_read"].tobytes() == r["P"].tobytes() and r["db_read"] == r["db"]
    # the contexts without the mode return nothing
    assert all(len(u["ids"]) == 0 for name in ("plain", "toggled") for u in runs[name]["used"])
    # a new update replaces the record
    now = ctx.camera_used_lines(st)
    assert now["ids"].tobytes() == r["out2"]["ids"].tobytes() and now["line_FinG"].tobytes() == r["out2"]["line_FinG"].tobytes()
    # too little room: PLV_E_CAPACITY with the count
    import ctypes as C
    cnt = C.c_int()
    assert len(now["ids"]) > 1
    assert ctx.lib.plv_camera_used_lines(ctx.h, C.byref(st.c), 1, C.byref(cnt), None, None, None, None, None) == pkg.PLV_E_CAPACITY
    assert cnt.value == len(now["ids"])
    # the mode switched off: nothing is kept
    ctx.line_map_mode(False)
    assert len(ctx.camera_used_lines(st)["ids"]) == 0
    ctx.line_map_mode(True)
    assert len(ctx.camera_used_lines(st)["ids"]) == 0


def test_the_mode_changes_nothing_in_the_update(updates):
    """dx, covariance and databases of the twins bit for bit, after the update and after a second one that runs on what the first
    left behind (the tracks it handed back, point_used)."""
    _, _, runs = updates
    a = runs["plain"]
    for name in ("toggled", "on"):
        b = runs[name]
        for out in ("out", "out2"):
            for k in ("dx", "ids", "accepted", "line_FinG"):
                assert b[out][k].tobytes() == a[out][k].tobytes(), (name, out, k)
            for k in ("n_pool", "n_lines", "n_accepted", "n_rows", "n_returned", "status", "n_truncated"):
                assert b[out][k] == a[out][k], (name, out, k)
        for k in ("P", "P_read", "P2"):
            assert b[k].tobytes() == a[k].tobytes(), (name, k)
        for k in ("db", "db_read", "db2"):
            assert b[k] == a[k], (name, k, [f for f in a[k] if a[k][f] != b[k][f]])
    assert np.abs(a["out"]["dx"]).max() > 0
    # the databases hold something to compare, and the second update had a pool to work on (the first one's returned tracks)
    assert len(a["db"]["obs_time"]) > 8 * 20 and a["db"]["pt_ids"] and a["out2"]["n_pool"] > 10 and a["out2"]["n_lines"] > 0
    print(f"second update: pool {a['out2']['n_pool']}, triangulated {a['out2']['n_lines']}, accepted {a['out2']['n_accepted']}; "
          f"line database after the first {len(a['db']['obs_time']) // 8} observations")


def test_used_lines_behind_an_update_with_a_cpi_table(pkg):
    """plv_update_options::cpi (use_imu_res) with the mode on: the record carries the table's poses as the update formed them (the
    fused route has them on the device only and fetches them when the mode is on), so the end points are the restatement's on
    res_R / res_p = plv_cpi_poses of the update's state — and the update itself is the twin's without the mode, bit for bit."""
    sc = synth.vio_scene(F=4, calib_int=True, dt_clone=0.5, seed=2)
    ls = synth.line_scene(sc, L=50, noise_px=0.3, depth=(4.0, 14.0), seed=6)
    # (views 20 ms behind the clones, between two records of the table: at a clone time the table's pose IS the clone's and the
    # polynomial's, and the two pose sets could not be told apart)
    ls["obs_time"] = ls["obs_time"] + np.where(ls["obs_time"] < sc["t"][-1], 0.02, 0.0)
    cp = synth.cpi_scene(sc, imu_dt=0.05)
    tab = pkg.CpiTable(cp["t"], cp["clone_t"], cp["R"], cp["alpha"], cp["v"], gravity=cp["gravity"])
    st, _ = synth.scene_views(pkg, sc)
    rng = np.random.default_rng(3)
    D, pts = rng.integers(0, 4, 50), rng.normal(size=(50, 3)) * 4 + np.array([0, 0, 8.0])
    t, n = sc["t"], sc["n_state"]
    runs = {}
    for name in ("on", "plain"):
        ctx, tracks = _filled_context(pkg, sc, ls, D, pts)
        try:
            ctx.line_map_mode(name == "on")
            out = ctx.camera_update_lines(st, n, 15, t_prev_frame=t[-2], state_time=t[-1], window_full=True, cpi=tab)
            runs[name] = dict(out=out, P=ctx.cov_download(n), db=_databases(ctx), used=ctx.camera_used_lines(st), tracks=tracks)
            if name == "on":
                tq = np.concatenate([tracks[int(i)][0] for i in out["ids"]])
                runs[name]["poses"] = ctx.cpi_poses(st, tab, tq)
        finally:
            ctx.close()
    a, b = runs["plain"], runs["on"]
    for k in ("dx", "ids", "accepted", "line_FinG"):
        assert b["out"][k].tobytes() == a["out"][k].tobytes(), k
    assert b["P"].tobytes() == a["P"].tobytes() and b["db"] == a["db"] and len(a["used"]["ids"]) == 0
    out, ul = b["out"], b["used"]
    assert out["status"] == 0 and out["n_lines"] > 20
    assert ul["ids"].tobytes() == out["ids"].tobytes() and ul["line_FinG"].tobytes() == out["line_FinG"].tobytes()
    R, p, ok = b["poses"]
    tr = [b["tracks"][int(i)] for i in ul["ids"]]
    cnt = np.array([len(x[0]) for x in tr])
    served = ok.astype(bool)                                       # (views the table cannot serve left their tracks before the update)
    ptr = np.concatenate([[0], np.cumsum([served[s:e].sum() for s, e in zip(np.cumsum(cnt) - cnt, np.cumsum(cnt))])]).astype(np.int32)
    cat = lambda j: np.concatenate([x[j] for x in tr])[served]
    lt = pkg.LineTracks(ptr, cat(0), cat(1), seg_uvn=cat(2), line_FinG=out["line_FinG"], res_R=R[served], res_p=p[served])
    ep_r, _, _, ok_r = ref.segments_of(st, lt)
    ep_poly = ref.segments_of(st, pkg.LineTracks(ptr, cat(0), cat(1), seg_uvn=cat(2), line_FinG=out["line_FinG"]))[0]
    print(f"cpi: used lines {len(ul['ids'])}, ok {int(ul['ok'].sum())}, |end points - ref| max {np.abs(ul['end_points'] - ep_r).max():.3g}, "
          f"|ref with the table's poses - ref with the polynomial's| max {np.abs(ep_r - ep_poly).max():.3g}")
    assert np.array_equal(ul["ok"], ok_r) and ok_r.sum() > 20
    assert (np.abs(ul["end_points"] - ep_r) <= 1e-9 * np.maximum(1.0, np.abs(ep_r))).all()
    assert np.abs(ep_r - ep_poly).max() > 1e-7                     # (the other pose set would show: a hundred times the tolerance)


# ------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def street_runs(pkg, tmp_path_factory):
    """the street drive of tests/test_gpu_replay.py (6 s at 10 Hz, lines on) through the driver without and with the map"""
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    d = tmp_path_factory.mktemp("street")
    sd.make_dataset(str(d / "data"), seconds=6.0, cam_hz=10.0, style="street", workers=16)
    runs = {}
    for name in ("off", "on"):
        op = options.load_options(sd.write_config(str(d / "config"), str(d / "data"), str(d / f"traj_{name}.txt")))
        op.est.cam.use_lines = True
        acc = rp.MapAccumulator()
        second = []

        def after(system, frame, t, acc=acc, second=second):
            acc.after_camera(system, frame, t)
            second.append((len(system.get_used_msckf()), len(system.get_used_lines())))      # a second read: empty
        runs[name] = rp.replay(op, after_camera=after, line_map=(name == "on")) + (acc, second)
    return runs


def test_the_driver_collects_the_map_and_leaves_the_trajectory_alone(street_runs):
    (s0, t0, p0, m0, _), (s1, t1, p1, m1, second) = street_runs["off"], street_runs["on"]
    assert np.array_equal(t1, t0) and p1.tobytes() == p0.tobytes()
    for key in s0:
        if not key.startswith("time"):
            assert s1[key] == s0[key], (key, s1[key], s0[key])
    assert s0["lines_accepted"] >= 10 and s0["cam_accepted"] >= 500
    pts, lms, seg = m1.arrays()
    print(f"map: {len(pts)} MSCKF points (cam_accepted {s1['cam_accepted']}), {len(seg)} segments (lines_accepted {s1['lines_accepted']}), "
          f"segment length p50 {m1.stats()['map_line_length_p50']:.2f} m")
    assert len(pts) == s1["cam_accepted"] and len(seg) == s1["lines_accepted"]
    assert np.isfinite(pts).all() and np.isfinite(seg).all()
    assert all(x == (0, 0) for x in second)
    off = m0.arrays()
    assert len(off[0]) == 0 and len(off[2]) == 0                  # without line_map nothing is collected
    # Every segment lies inside the street.  The renderer's corridor (synth_dataset.Renderer, style "street") is |y| <= 9 m and
    # 0 <= z <= 7 m around a drive down the x axis, its end walls at most 150 m from the camera.  The filter's frame starts at the first
    # IMU pose (0.9 m above the ground, synth_dataset.P_IINO), gravity aligned, its x axis within 0.055 rad of the corridor's (the
    # weave's slope 0.25 * 2 pi / 45 = 0.035 plus the mount's 0.02): in that frame the corridor is |x| <= drive + 150, |y| <= 9 + 0.25 (weave
    # amplitude) + 0.055 |x|, -0.9 <= z <= 6.1.  Margin 1 m: an end point lies where an image ray meets the triangulated line, and a
    # line seen over the window's 1.2 s (3 m of travel) at the 25 m beyond which these facades' segments fall below the detector's
    # 40 px has a depth error of d^2 / (b f) * sigma_px = 625 / (3 * 458) * 1 px = 0.45 m: 1 m is two sigma of the farthest lines.
    x_max = np.abs(p1[:, 0]).max() + 150.0
    ends = seg.reshape(-1, 3)
    assert (np.abs(ends[:, 0]) <= x_max).all()
    assert (np.abs(ends[:, 1]) <= 9.25 + 0.055 * np.abs(ends[:, 0]) + 1.0).all(), np.abs(ends[:, 1]).max()
    assert ((ends[:, 2] >= -0.9 - 1.0) & (ends[:, 2] <= 7.0 - 0.9 + 1.0)).all(), (ends[:, 2].min(), ends[:, 2].max())
