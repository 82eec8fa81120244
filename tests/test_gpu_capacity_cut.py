"""The batch-capacity cut of the camera updates (plv_update_options::max_obs, counted in plv_update_result::n_truncated): a track with
more usable views than a batch entry has rows sends the update down the two-step route, leaves out its oldest usable views, and gets
ALL its usable views back when the gate rejects it.  plv_camera_update_points / plv_camera_update_lines against the whole-call oracle
(oracle/frame_oracle.cpp) on the same database: results, and the database afterwards track by track.

The scenes are small on purpose — 8 clones, a dozen tracks, max_obs = 4 (ld = 8) — and the seeds were chosen on the CPU with the
oracle alone; every test first asserts on the oracle's output that the scene still exercises the cut (conditions below)."""
import numpy as np
import pytest

import oracle_lib
import synth

N_CLONES, MAX_OBS, MAX_MSCKF = 8, 4, 40


def point_case():
    """12 point tracks of 3 .. 8 views over 8 clones, every third cut to its newest 3 or 4; the image points of every fourth carry 2 px
    of extra noise: consistent enough to triangulate below the 3 px limit, too far off for the chi2 gate"""
    fo = oracle_lib.load_front()
    sc = synth.vio_scene(n_clones=N_CLONES, F=12, M=8, noise_px=0.4, dt_clone=0.2, seed=21)
    rng = np.random.default_rng(3)
    tracks = {}
    for f in range(12):
        a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
        if f % 3 == 2:
            a = b - (3 + f % 2)   # within the capacity: the newest 3 or 4 views
        uv = sc["obs_uv"][a:b].astype(np.float32)
        if f % 4 == 1:
            uv = uv + rng.normal(0, 2.0, uv.shape).astype(np.float32)
        tracks[f + 1] = (sc["obs_time"][a:b].copy(), uv, fo.undistort(sc["K8"], uv))
    tri = dict(min_dist=0.1, max_dist=100.0, max_cond=1e7, max_baseline=1e3, refine=True)   # (short baseline: the default gates reject most)
    return sc, tracks, tri


def line_case():
    """14 line tracks of 3 .. 8 views, every third cut to its newest 3 or 4, on the wide-baseline scene of test_camera_update_lines
    (without it the reference's plane-pair gate rejects everything); a triangulated point on every third line"""
    sc = synth.vio_scene(n_clones=N_CLONES, F=4, calib_int=True, dt_clone=0.5, seed=2)
    L = 14
    ls = synth.line_scene(sc, L=L, M=8, noise_px=0.3, depth=(4.0, 14.0), seed=6)
    rng = np.random.default_rng(3)
    D = rng.integers(0, 4, L)
    pts = rng.normal(size=(L, 3)) * 4 + np.array([0, 0, 8.0])
    tracks, anchors = {}, {}
    for l in range(L):
        a, b = ls["obs_ptr"][l], ls["obs_ptr"][l + 1]
        if l % 3 == 2:
            a = b - (3 + l % 2)   # within the capacity: the newest 3 or 4 views
        tracks[l + 2] = (ls["obs_time"][a:b].copy(), ls["seg_uv"][a:b].copy(), ls["seg_uvn"][a:b].copy(), int(D[l]), [1000 + l, 2000 + l])
        if l % 3 == 1:
            anchors[2000 + l] = pts[l]
    return sc, tracks, anchors


def oracle_points(pkg, sc, tracks, tri, P):
    fr = oracle_lib.FrameOracle(pkg, pkg.default_config(752, 480), synth.q95_table())
    fr.set_intrinsics(sc["K8"])
    for fid, tr in tracks.items():
        fr.db_append(fid, *tr)
    st, _ = synth.scene_views(pkg, sc)
    Po = np.array(P, dtype=np.float64, order="F")
    t_last = float(sc["t"][-1])
    ref = fr.update_points(Po, st, MAX_MSCKF, MAX_OBS, t_last + 1.0, t_last, True, 1.0, tri["min_dist"], tri["max_dist"], tri["max_cond"],
                           tri["max_baseline"], tri["refine"])
    ids, _ = fr.db_ids()
    db = {int(i): fr.db_track(i) for i in ids}
    fr.close()
    return ref, Po, db


def oracle_lines(pkg, sc, tracks, anchors, P):
    fr = oracle_lib.FrameOracle(pkg, pkg.default_config(752, 480), synth.q95_table())
    fr.set_intrinsics(sc["K8"])
    t_last = float(sc["t"][-1])
    for lid, (tt, uv, uvn, D, pid) in tracks.items():
        fr.line_db_append(lid, tt, uv, uvn, D=D, point_ids=pid)
    for pid, p in anchors.items():
        fr.used_insert(pid, p, t_last)
    st, _ = synth.scene_views(pkg, sc)
    Po = np.array(P, dtype=np.float64, order="F")
    ref = fr.update_lines(Po, st, MAX_OBS, t_last + 1.0, t_last, True)
    ids, _ = fr.db_ids(lines=True)
    db = {int(i): fr.line_db_track(i) for i in ids}
    fr.close()
    return ref, Po, db


def exercises_the_cut(ref, tracks):
    """the conditions on the oracle's output: n_truncated >= 2, a truncated track accepted, a truncated track rejected, and tracks
    within the capacity selected next to them (every view of these scenes is usable: truncated = more than MAX_OBS views)"""
    long_ = np.array([len(tracks[int(i)][0]) > MAX_OBS for i in ref["ids"]])
    acc = ref["accepted"] > 0
    return ref["status"] == 0 and ref["n_truncated"] >= 2 and ref["n_truncated"] == long_.sum() and (long_ & acc).any() and (long_ & ~acc).any() and (~long_).any()


def same_tracks(name, got, want, width):
    """the database afterwards, track by track: times and image points"""
    assert set(got) == set(want), (name, sorted(got), sorted(want))
    for i in sorted(want):
        assert np.array_equal(got[i][0], want[i][0]), (name, i, "times", got[i][0], want[i][0])
        assert np.array_equal(got[i][1].reshape(-1, width), want[i][1].reshape(-1, width)), (name, i, "image points")
        assert np.array_equal(got[i][2].reshape(-1, width), want[i][2].reshape(-1, width)), (name, i, "normalised points")


@pytest.mark.gpu
def test_points_update_cut_to_the_batch_capacity(pkg):
    sc, tracks, tri = point_case()
    n = sc["n_state"]
    P = synth.spd_cov(n, seed=4) * 1e-4
    ref, P_o, db_o = oracle_points(pkg, sc, tracks, tri, P)
    assert exercises_the_cut(ref, tracks), (ref["n_truncated"], ref["ids"], ref["accepted"])
    st, _ = synth.scene_views(pkg, sc)
    t_last = float(sc["t"][-1])
    ctx = pkg.Context(pkg.default_config(752, 480))
    try:
        for fid, tr in tracks.items():
            ctx.db_append_measurements(fid, *tr)
        ctx.cov_upload(P)
        out = ctx.camera_update_points(st, n, MAX_MSCKF, MAX_OBS, t_prev_frame=t_last + 1.0, state_time=t_last, window_full=True, **tri)
        P_d = ctx.cov_download(n)
        ids = ctx.db_select(1, 1e18)
        ptr, tt, uv, uvn = ctx.db_export(ids)
        db = {int(i): (tt[ptr[q]:ptr[q + 1]], uv[ptr[q]:ptr[q + 1]], uvn[ptr[q]:ptr[q + 1]]) for q, i in enumerate(ids)}
        assert ctx.db_size() == len(ids)
    finally:
        ctx.close()
    assert out["status"] == ref["status"] and out["n_pool"] == ref["n_pool"] and out["n_truncated"] == ref["n_truncated"]
    assert np.array_equal(out["ids"], ref["ids"]) and np.array_equal(out["accepted"], ref["accepted"])
    d_dx, d_P = np.abs(out["dx"] - ref["dx"]).max(), np.abs(P_d - P_o).max()
    print(f"points: n_truncated {ref['n_truncated']}, selected {len(ref['ids'])}, accepted {int(ref['accepted'].sum())} | dx {d_dx:.2e} (|dx| {np.abs(ref['dx']).max():.2e}) P {d_P:.2e} (|P| {np.abs(P).max():.2e})")
    assert d_dx <= 1e-7 * max(1.0, np.abs(ref["dx"]).max())    # (test_camera_update_points' tolerances)
    assert d_P <= 1e-8 * np.abs(P).max()
    same_tracks("points", db, db_o, 2)


@pytest.mark.gpu
def test_lines_update_cut_to_the_batch_capacity(pkg):
    sc, tracks, anchors = line_case()
    n = sc["n_state"]
    P = synth.spd_cov(n, seed=4) * 1e-4
    ref, P_o, db_o = oracle_lines(pkg, sc, tracks, anchors, P)
    assert exercises_the_cut(ref, tracks), (ref["n_truncated"], ref["ids"], ref["accepted"])
    st, _ = synth.scene_views(pkg, sc)
    t_last = float(sc["t"][-1])
    ctx = pkg.Context(pkg.default_config(752, 480))
    try:
        for lid, (tt, uv, uvn, D, pid) in tracks.items():
            ctx.line_db_append_measurements(lid, tt, uv, uvn, D=D, point_ids=pid)
        for pid, p in anchors.items():
            ctx.point_used_insert(pid, p, t_last)
        ctx.cov_upload(P)
        out = ctx.camera_update_lines(st, n, MAX_OBS, t_prev_frame=t_last + 1.0, state_time=t_last, window_full=True)
        P_d = ctx.cov_download(n)
        ids = ctx.line_db_ids()
        ex = ctx.line_db_export(ids)
        ptr = ex["obs_ptr"]
        db = {int(i): (ex["obs_time"][ptr[q]:ptr[q + 1]], ex["seg_uv"][ptr[q]:ptr[q + 1]], ex["seg_uvn"][ptr[q]:ptr[q + 1]]) for q, i in enumerate(ids)}
    finally:
        ctx.close()
    assert out["status"] == ref["status"] and out["n_pool"] == ref["n_pool"] and out["n_truncated"] == ref["n_truncated"]
    assert np.array_equal(out["ids"], ref["ids"]) and np.array_equal(out["accepted"], ref["accepted"])
    d_dx, d_P = np.abs(out["dx"] - ref["dx"]).max(), np.abs(P_d - P_o).max()
    print(f"lines: n_truncated {ref['n_truncated']}, selected {len(ref['ids'])}, accepted {int(ref['accepted'].sum())} | dx {d_dx:.2e} (|dx| {np.abs(ref['dx']).max():.2e}) P {d_P:.2e} (|P| {np.abs(P).max():.2e})")
    assert d_dx <= 1e-6 * max(1.0, np.abs(ref["dx"]).max())    # (test_camera_update_lines' tolerances)
    assert d_P <= 1e-6 * np.abs(P).max()
    same_tracks("lines", db, db_o, 4)
