"""The stereo point update on the device — plv_triangulate_stereo, plv_build_jacobians_stereo, plv_stereo_update_points — against the
restatement composed of oracle pieces (tests/stereo_update_ref.py; tests/test_stereo_update_ref_cpu.py pins it and the scene).
Tolerances are the monocular tests': positions 1e-9 x max(1, largest entry) and the reprojection error 1e-7 relative
(tests/triangulation_cases.py point_tolerances; 1e-6 absolute where a camera of the pair is equidistant, as tests/test_gpu_equidistant.py holds
the monocular fisheye error: the restatement's arctan is numpy's), Jacobians 1e-9 x max(1, largest entry) per array
(tests/test_gpu_jacobian.py), the update p 1e-6, dx 1e-7, P 1e-8 (tests/test_gpu_update_frame.py test_camera_update_points).
The pairings (camera 0, camera 1): radtan-radtan, radtan-equidistant, equidistant-radtan, equidistant-equidistant.  Camera 0's model
is the context's (plv_set_camera_model), camera 1's comes with its plv_camera_side; tests/test_stereo_update_ref_cpu.py shows that a
scene with camera 0 equidistant, read with camera 0 as radtan, gives other verdicts."""
import numpy as np
import pytest

import cam_equi
import oracle_lib
import stereo_update_ref as sr
import synth

pytestmark = pytest.mark.gpu

W, H = 752, 480
_REF = {}


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


@pytest.fixture(scope="module")
def fo():
    return oracle_lib.load_front()


@pytest.fixture(scope="module")
def dev(pkg):
    c = pkg.Context(pkg.default_config(W, H))
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev_equi(pkg):
    c = pkg.Context(pkg.default_config(W, H))
    c.set_camera_model("equidistant")
    yield c
    c.close()


def _dev_of(pair, dev, dev_equi):
    """the context whose model is camera 0's"""
    return dev_equi if pair.cams[0].model == sr.EQUI else dev


def _update_ref(pkg, jo, fo, oracle, model1, model0=sr.RADTAN):
    """(scene, pair, tracks, names, options, P, the restatement's first update), computed once per pairing and left unchanged"""
    if (model0, model1) not in _REF:
        sc, pair, tracks, names, opt = sr.update_scene(pkg, fo.undistort, model1=model1, model0=model0)
        P = synth.spd_cov(sc["n_state"], seed=4) * 1e-4
        _REF[model0, model1] = (sc, pair, tracks, names, opt, P, sr.update_points(jo, oracle, pair, tracks, P, **opt))
    return _REF[model0, model1]


def _stereo_ctx(pkg, pair):
    c = pkg.Context(pkg.default_config(W, H))
    if pair.cams[0].model == sr.EQUI:
        c.set_camera_model("equidistant")
    c.stereo_configure(pair.cams[1].K8, pair.cams[1].model)
    return c


def _fill(c, tracks):
    for fid, ft in tracks.items():
        for cam, o in ft.items():
            if len(o[0]):
                c.stereo_db_append_measurements(fid, cam, o[0], o[1], o[2])


def _db(c):
    ids = c.stereo_db_ids()
    out = {int(i): {} for i in ids}
    for cam in (0, 1):
        ptr, t, uv, uvn = c.stereo_db_export(ids, cam)
        for q, i in enumerate(ids):
            if ptr[q + 1] > ptr[q]:
                out[int(i)][cam] = (t[ptr[q]:ptr[q + 1]], uv[ptr[q]:ptr[q + 1]], uvn[ptr[q]:ptr[q + 1]])
    return out


# ------------------------------------------------------------------ 1. triangulation
@pytest.mark.parametrize("case", ["radtan", "equidistant", "res-poses", "time-offset", "equi-radtan", "equi-equi"])
def test_triangulate_stereo(pkg, dev, dev_equi, jo, fo, case):
    model1 = sr.EQUI if case in ("equidistant", "equi-equi") else sr.RADTAN
    model0 = sr.EQUI if case in ("equi-radtan", "equi-equi") else sr.RADTAN
    sc, pair, tracks, names, _ = sr.update_scene(pkg, fo.undistort, model1=model1, model0=model0, dt=0.003 if case == "time-offset" else 0.0)
    dev = _dev_of(pair, dev, dev_equi)
    ids = sorted(tracks)
    feats = [tracks[i] for i in ids]
    if case == "res-poses":
        feats = sr.with_res_poses(sc, feats)
    fl = sr.flatten(feats)
    p, ok, err = dev.triangulate_stereo(pair.views[0], pair.side, sr.stereo_tracks(pkg, fl, np.zeros((len(feats), 3))), **sr.TRI)
    p_o, ok_o, err_o, _, anchors, nv = sr.triangulate_batch(jo, pair, feats)
    assert np.array_equal(ok, ok_o) and ok_o.sum() >= 25 and (ok_o == 0).any()
    bad = ok_o == 0
    assert not p[bad].any() and not err[bad].any()
    tol_p = 1e-9 * max(1.0, np.abs(p_o).max())

    def close(sel, what):
        sel = [q for q in sel if ok_o[q]]
        assert sel, what
        dp = np.abs(p[sel] - p_o[sel]).max()
        de = np.abs(err[sel] - err_o[sel])
        print(f"{case:12s} {what:22s} {len(sel):2d} features | p {dp:.1e} (tolerance {tol_p:.1e}) | error {de.max():.1e}")
        assert dp <= tol_p, (what, dp)
        assert (de <= 1e-6).all() if sr.EQUI in (model0, model1) else (de <= 1e-7 * err_o[sel]).all(), (what, de.max())

    # the anchor: camera 1 on a tie, else the camera with more usable observations
    close([q for q in range(len(ids)) if nv[q][0] == nv[q][1] and anchors[q] == 1], "anchor: tie")
    close([q for q in range(len(ids)) if nv[q][0] > nv[q][1] > 0 and anchors[q] == 0], "anchor: majority 0")
    close([q for q in range(len(ids)) if nv[q][1] > nv[q][0] > 0 and anchors[q] == 1], "anchor: majority 1")
    close([q for q in range(len(ids)) if min(nv[q]) == 0], "one camera only")
    close(range(len(ids)), "all")
    # the mean over the cameras, not over the observations
    q = ids.index(names["camera-averaged"])
    assert abs(err[q] - err_o[q]) <= 1e-6 and (err[q] < 3.0 or case not in ("radtan", "equidistant", "equi-radtan", "equi-equi"))


# ------------------------------------------------------------------ 2. Jacobians
JAC_CASES = {
    "all-blocks": dict(calib="all"),
    "camera-1-off": dict(calib="cam0"),
    "camera-0-off": dict(calib="cam1"),
    "time-offset": dict(calib="all", dt=0.003),
    "pol-cov": dict(calib="all", scene_kw=dict(obs_offset=0.017), use_pol_cov=1, intr_ori_cov=1e-6, intr_pos_cov=1e-6),
    "mixed-models": dict(calib="all", model1=sr.EQUI),
    "res-poses": dict(calib="all", res=True),
    "long-40+30": dict(calib="all", long=True),
    "over-ld": dict(calib="all", ld=40),
    # camera 0 equidistant: the intrinsic columns of both cameras carry dzeta; res poses; the second 64-lane chunk and a camera
    # change inside it
    "equi-radtan": dict(calib="all", model0=sr.EQUI),
    "equi-equi": dict(calib="all", model0=sr.EQUI, model1=sr.EQUI),
    "equi-equi-res-poses": dict(calib="all", model0=sr.EQUI, model1=sr.EQUI, res=True),
    "equi-equi-long-40+30": dict(calib="all", model0=sr.EQUI, model1=sr.EQUI, long=True),
}


@pytest.mark.parametrize("case", sorted(JAC_CASES))
def test_build_jacobians_stereo(pkg, dev, dev_equi, jo, fo, case):
    kw = dict(JAC_CASES[case])
    res, long, ld = kw.pop("res", False), kw.pop("long", False), kw.pop("ld", 62)
    sc, pair, obs = sr.stereo_scene(pkg, fo.undistort, F=12, **kw)
    dev = _dev_of(pair, dev, dev_equi)
    n = sc["n_state"]
    feats = [obs[0], sr.cut(obs[1], None, ()), sr.cut(obs[2], (), None), sr.cut(obs[3], slice(0, 9), None), sr.cut(obs[5], None, slice(3, 15)), obs[6], obs[7]]
    pts = [sc["pts"][f] for f in (0, 1, 2, 3, 5, 6, 7)]
    # an observation without bounding clones in camera 1 only (in front of the window)
    early = tuple(a.copy() for a in feats[0][1])
    early[0][2] = sc["t"][0] - 5.0
    feats[0] = {0: feats[0][0], 1: early}
    if long:  # 40 + 30 observations at distinct times: the second 64-lane chunk; and 66 + 10: the camera changes inside that chunk
        feats += [sr.long_feature(sc, pair, fo.undistort, sc["pts"][8], 40, 30), sr.long_feature(sc, pair, fo.undistort, sc["pts"][9], 66, 10, seed=4)]
        pts += [sc["pts"][8], sc["pts"][9]]
        ld = 2 * 80
    if res:
        feats = sr.with_res_poses(sc, feats)
    p = np.array(pts) + np.random.default_rng(1).normal(0, 0.02, (len(pts), 3))
    fl = sr.flatten(feats)
    trk = sr.stereo_tracks(pkg, fl, p)
    cols = dev.stereo_jacobian_columns(pair.views[0], pair.side, trk)
    cols_o = sr.columns(jo, pair, feats)
    assert np.array_equal(cols, cols_o), (cols, cols_o)
    rows, Hf, Hx, rs = dev.build_jacobians_stereo(pair.views[0], pair.side, trk, cols, ld)
    rows_o, Hf_o, Hx_o, rs_o = sr.build_jacobians(jo, pair, feats, p, cols_o, ld)
    assert np.array_equal(rows, rows_o) and rows[0] == 2 * (len(feats[0][0][0]) + len(feats[0][1][0]) - 1)
    if case == "over-ld":
        assert rows.max() > ld
    worst = {}
    for name, a, b in (("Hf", Hf, Hf_o), ("Hx", sr.by_state(cols, Hx, n), sr.by_state(cols_o, Hx_o, n)), ("res", rs, rs_o)):
        worst[name] = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    print(f"{case:14s} k {len(cols):3d} rows {rows.tolist()} | " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v <= 1e-9 for v in worst.values()), worst
    # every calibration block that is on has entries, in the rows of its own camera only
    S = sr.by_state(cols, Hx, n)
    for c in (0, 1):
        cam = pair.cams[c]
        for first, size in ((cam.ext_id, 6), (cam.int_id, 8)):
            if first < 0:
                continue
            f_own, f_other = (1, 2) if c == 0 else (2, 1)      # a feature seen by this camera only, by the other only
            assert np.abs(S[f_own][first:first + size]).max() > 0 and not S[f_other][first:first + size].any()


# ------------------------------------------------------------------ 3. the update
def _check_update(out, ref, P0, c, n, what):
    assert out["status"] == ref["status"] == 0 and out["n_pool"] == ref["n_pool"], what
    assert np.array_equal(out["ids"], ref["ids"]), (what, out["ids"], ref["ids"])
    assert np.array_equal(out["accepted"], ref["accepted"]) and out["n_rows"] == ref["n_rows"], what
    assert out["n_msckf"] == len(ref["ids"]) and out["n_accepted"] == int(ref["accepted"].sum()) and out["n_slam"] == 0 and out["n_init"] == 0
    dp = np.abs(out["p_FinG"] - ref["p_FinG"]).max() if len(ref["ids"]) else 0.0
    ddx = np.abs(out["dx"] - ref["dx"]).max()
    dP = np.abs(c.cov_download(n) - ref["P"]).max()
    print(f"{what}: pool {out['n_pool']} selected {len(ref['ids'])} accepted {int(ref['accepted'].sum())} rows {ref['n_rows']} | "
          f"p {dp:.1e} dx {ddx:.1e} (|dx| {np.abs(ref['dx']).max():.1e}) P {dP:.1e} (|P| {np.abs(P0).max():.1e})")
    assert dp < 1e-6 and ddx <= 1e-7 * max(1.0, np.abs(ref["dx"]).max()) and dP <= 1e-8 * np.abs(P0).max(), what
    assert sr.db_equal(_db(c), ref["db"]), what


@pytest.mark.parametrize("pairing", list(sr.PAIRINGS))
def test_stereo_update_points(pkg, jo, fo, oracle, pairing):
    model0, model1 = sr.PAIRINGS[pairing]
    sc, pair, tracks, names, opt, P, ref = _update_ref(pkg, jo, fo, oracle, model1, model0)
    n = sc["n_state"]
    c = _stereo_ctx(pkg, pair)
    try:
        _fill(c, tracks)
        assert sr.db_equal(_db(c), tracks)
        c.cov_upload(P)
        out = c.stereo_update_points(pair.views[0], pair.side, n, **opt, **sr.TRI)
        _check_update(out, ref, P, c, n, "first update")
        assert len(ref["ids"]) == opt["max_msckf"] and (ref["accepted"] == 0).any() and ref["accepted"].sum() >= 10
        # ---- one frame later, on the database the first update left behind
        sc2, pair2, new = sr.advance(pkg, sc, pair, fo.undistort, ref["db"])
        assert len(new) >= 5
        _fill(c, new)
        opt2 = dict(opt, t_prev_frame=float(sc["t"][-1]), state_time=float(sc2["t"][-1]))
        ref2 = sr.update_points(jo, oracle, pair2, sr.db_append(ref["db"], new), ref["P"], **opt2)
        assert ref2["n_pool"] >= 5 and len(ref2["ids"]) >= 3
        out2 = c.stereo_update_points(pair2.views[0], pair2.side, n, **opt2, **sr.TRI)
        _check_update(out2, ref2, P, c, n, "second update")
    finally:
        c.close()


# ------------------------------------------------------------------ 4. one camera: the monocular update
def test_one_camera_equals_the_monocular_update(pkg, fo):
    sc = synth.vio_scene(F=60, M=15, noise_px=0.4, seed=9)
    t, K8, n = sc["t"], sc["K8"], sc["n_state"]
    st, _ = synth.scene_views(pkg, sc)
    side = pkg.CameraSide(sc["R_ItoC"], sc["p_IinC"], K8)
    P = synth.spd_cov(n, seed=4) * 1e-4
    mono, ster = pkg.Context(pkg.default_config(W, H)), pkg.Context(pkg.default_config(W, H))
    try:
        ster.stereo_configure(K8, 0)
        for f in range(60):
            a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
            uv = sc["obs_uv"][a:b].astype(np.float32)
            uvn = fo.undistort(K8, uv)
            mono.db_append_measurements(f + 1, sc["obs_time"][a:b], uv, uvn)
            ster.stereo_db_append_measurements(f + 1, 0, sc["obs_time"][a:b], uv, uvn)
        mono.cov_upload(P)
        ster.cov_upload(P)
        kw = dict(t_prev_frame=t[-2], state_time=t[-1], window_full=True, **sr.TRI)
        a = mono.camera_update_points(st, n, 30, 15, **kw)
        b = ster.stereo_update_points(st, side, n, 30, 15, **kw)
        assert a["status"] == b["status"] == 0 and a["n_pool"] == b["n_pool"] and len(a["ids"]) == 30
        assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["accepted"], b["accepted"]) and a["n_rows"] == b["n_rows"]
        assert np.abs(a["p_FinG"] - b["p_FinG"]).max() < 1e-6
        assert np.abs(a["dx"] - b["dx"]).max() <= 1e-7 * max(1.0, np.abs(a["dx"]).max())
        assert np.abs(mono.cov_download(n) - ster.cov_download(n)).max() <= 1e-8 * np.abs(P).max()
        assert set(int(i) for i in mono.db_select(1, 1e18)) == set(int(i) for i in ster.stereo_db_ids())
    finally:
        mono.close()
        ster.close()


def test_one_equidistant_camera_equals_the_monocular_update(pkg):
    """the same with camera 0 equidistant: a stereo context whose tracks have camera-0 observations only gives the update of a monocular
    equidistant context.  (Camera 1 is configured radtan and has no observation: its model must not reach camera 0's rows.)"""
    sc = synth.vio_scene(F=60, M=15, noise_px=0.0, seed=9)
    t, n = sc["t"], sc["n_state"]
    K8 = np.concatenate([sc["K8"][:4], sr.EQUI0_COEFFS])
    st = pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], sc["R_ItoC"], sc["p_IinC"], K8, clone_R_fej=sc["Rf"], clone_p_fej=sc["pf"],
                       intrinsic_state_id=sc["intr_id"], sigma_pix=1.5)
    side = pkg.CameraSide(sc["R_ItoC"], sc["p_IinC"], sc["K8"])
    P = synth.spd_cov(n, seed=4) * 1e-4
    rng = np.random.default_rng(10)
    mono, ster = pkg.Context(pkg.default_config(W, H)), pkg.Context(pkg.default_config(W, H))
    try:
        for c in (mono, ster):
            c.set_camera_model("equidistant")
        ster.stereo_configure(sc["K8"], 0)
        for f in range(60):
            a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
            un = []
            for tm in sc["obs_time"][a:b]:
                R, p = sc["pose_fn"](tm)
                pc = sc["R_ItoC"] @ (R @ (sc["pts"][f] - p)) + sc["p_IinC"]
                un.append(pc[:2] / pc[2])
            uv = (cam_equi.distort(K8, np.array(un)) + rng.normal(0, 0.4, (b - a, 2))).astype(np.float32)
            uvn = cam_equi.undistort(K8, uv)
            mono.db_append_measurements(f + 1, sc["obs_time"][a:b], uv, uvn)
            ster.stereo_db_append_measurements(f + 1, 0, sc["obs_time"][a:b], uv, uvn)
        mono.cov_upload(P)
        ster.cov_upload(P)
        kw = dict(t_prev_frame=t[-2], state_time=t[-1], window_full=True, **sr.TRI)
        a = mono.camera_update_points(st, n, 30, 15, **kw)
        b = ster.stereo_update_points(st, side, n, 30, 15, **kw)
        assert a["status"] == b["status"] == 0 and a["n_pool"] == b["n_pool"] and len(a["ids"]) == 30
        assert a["accepted"].sum() >= 15                                   # (the data are consistent under the equidistant model)
        assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["accepted"], b["accepted"]) and a["n_rows"] == b["n_rows"]
        dp, ddx, dP = np.abs(a["p_FinG"] - b["p_FinG"]).max(), np.abs(a["dx"] - b["dx"]).max(), np.abs(mono.cov_download(n) - ster.cov_download(n)).max()
        print(f"equidistant camera 0 alone: accepted {int(a['accepted'].sum())} of 30 | p {dp:.1e} (1e-6) dx {ddx:.1e} (|dx| {np.abs(a['dx']).max():.1e}) P {dP:.1e} (|P| {np.abs(P).max():.1e})")
        assert dp < 1e-6
        assert ddx <= 1e-7 * max(1.0, np.abs(a["dx"]).max())
        assert dP <= 1e-8 * np.abs(P).max()
        assert set(int(i) for i in mono.db_select(1, 1e18)) == set(int(i) for i in ster.stereo_db_ids())
    finally:
        mono.close()
        ster.close()


# ------------------------------------------------------------------ 5. what is refused
def test_refusals_leave_everything_as_it_was(pkg, jo, fo, oracle):
    sc, pair, tracks, names, opt, P, _ = _update_ref(pkg, jo, fo, oracle, sr.RADTAN)
    n = sc["n_state"]
    k = 98
    cols = synth.col_map(n, k)
    batch = synth.msckf_batch(F=20, M=15, k=k, seed=9)
    c, plain = _stereo_ctx(pkg, pair), pkg.Context(pkg.default_config(W, H))
    try:
        _fill(c, tracks)
        c.cov_upload(P)
        c.feat_batch_upload(*batch, cols)
        st, side = pair.views[0], pair.side
        call = lambda ctx=c, st=st, side=side, **kw: ctx.stereo_update_points(st, side, n, **dict(opt, **kw), **sr.TRI)

        def refused(fn, word):
            with pytest.raises(pkg.PlvError) as e:
                fn()
            assert e.value.code == pkg.PLV_E_BADARG and word in str(e.value), str(e.value)

        refused(lambda: call(max_slam=3), "max_slam")
        cp = synth.cpi_scene(sc)
        refused(lambda: call(cpi=pkg.CpiTable(cp["t"], cp["clone_t"], cp["R"], cp["alpha"], cp["v"], gravity=cp["gravity"])), "use_imu_res")
        with_cov = sr.Pair(pkg, sc, pair.cams, dt_id=pair.dt_id, use_imu_cov=1)
        refused(lambda: call(st=with_cov.views[0]), "use_imu_cov")
        plain.cov_upload(P)
        refused(lambda: call(ctx=plain), "stereo")
        refused(lambda: call(side=None), "camera 1")
        for clash in (dict(extrinsic_state_id=pair.cams[0].ext_id + 3), dict(intrinsic_state_id=pair.cams[0].int_id), dict(extrinsic_state_id=pair.dt_id - 5),
                      dict(extrinsic_state_id=pair.cams[1].int_id + 2, intrinsic_state_id=pair.cams[1].int_id)):
            bad = pkg.CameraSide(pair.cams[1].R, pair.cams[1].p, pair.cams[1].K8, **dict(dict(extrinsic_state_id=pair.cams[1].ext_id, intrinsic_state_id=pair.cams[1].int_id), **clash))
            refused(lambda: call(side=bad), "collides")
        c.decision_trace(True)
        refused(lambda: call(), "decision trace")
        c.decision_trace(False)
        # the low-level calls: a wrong order, a camera above 1
        fl = sr.flatten([tracks[i] for i in sorted(tracks)])
        swapped = dict(fl, cam=(1 - fl["cam"]).astype(np.uint8))
        third = dict(fl, cam=np.where(np.arange(len(fl["cam"])) == 0, 2, fl["cam"]).astype(np.uint8))
        for bad, word in ((swapped, "camera 1 comes first"), (third, "cameras 0 and 1")):
            trk = sr.stereo_tracks(pkg, bad, np.ones((len(tracks), 3)))
            refused(lambda: c.stereo_jacobian_columns(st, side, trk), word)
            refused(lambda: c.triangulate_stereo(st, side, trk), word)
            refused(lambda: c.build_jacobians_stereo(st, side, trk, np.arange(20, dtype=np.int32), 62), word)
            refused(lambda: c.build_jacobians_stereo_resident(st, side, trk, np.arange(20, dtype=np.int32), 62), word)
        # ---- database, covariance and the staged batch are as they were
        assert sr.db_equal(_db(c), tracks)
        assert np.array_equal(c.cov_download(n), P)
        plain.feat_batch_upload(*batch, cols)
        a, b = c.msckf_update_resident(n, 1.0), plain.msckf_update_resident(n, 1.0)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    finally:
        c.close()
        plain.close()


# ------------------------------------------------------------------ 6. nothing to do
def test_empty_database_and_empty_selection(pkg, jo, fo, oracle):
    sc, pair, tracks, names, opt, P, _ = _update_ref(pkg, jo, fo, oracle, sr.RADTAN)
    n = sc["n_state"]
    c = _stereo_ctx(pkg, pair)
    try:
        c.cov_upload(P)
        out = c.stereo_update_points(pair.views[0], pair.side, n, **opt, **sr.TRI)
        assert out["status"] == 0 and out["n_pool"] == out["n_msckf"] == out["n_accepted"] == out["n_rows"] == 0 and not out["dx"].any()
        assert np.array_equal(c.cov_download(n), P)
        # a pool that selects nothing: the biased track, the track with one usable observation, a lost single observation
        some = {fid: tracks[fid] for fid in (names["biased"], names["one usable"])}
        some[900] = {1: (np.array([sc["t"][2]]), np.array([[100.0, 100.0]], np.float32), np.zeros((1, 2), np.float32))}
        _fill(c, some)
        out = c.stereo_update_points(pair.views[0], pair.side, n, **opt, **sr.TRI)
        assert out["status"] == 0 and out["n_pool"] == 3 and out["n_msckf"] == out["n_accepted"] == out["n_rows"] == 0 and not out["dx"].any()
        assert np.array_equal(c.cov_download(n), P)
        assert set(_db(c)) == {names["biased"], names["one usable"]}           # (the single observation is taken and dropped)
    finally:
        c.close()


def test_more_observations_than_the_batch_holds(pkg, jo, fo, oracle):
    """a feature with more than max_obs usable observations over both cameras is not truncated: PLV_E_CAPACITY before any launch, the pool
    back in the database, the covariance as it was"""
    sc, pair, tracks, names, opt, P, _ = _update_ref(pkg, jo, fo, oracle, sr.RADTAN)
    n = sc["n_state"]
    c = _stereo_ctx(pkg, pair)
    try:
        _fill(c, tracks)
        c.cov_upload(P)
        with pytest.raises(pkg.PlvError) as e:
            c.stereo_update_points(pair.views[0], pair.side, n, **dict(opt, max_obs=20), **sr.TRI)
        assert e.value.code == pkg.PLV_E_CAPACITY and "max_obs = 20" in str(e.value)
        assert sr.db_equal(_db(c), tracks) and np.array_equal(c.cov_download(n), P)
    finally:
        c.close()
