"""The restatement of the stereo point update (tests/stereo_update_ref.py) and its test scene, pinned without a device: with one
camera it is the monocular composition of oracle pieces (tests/test_gpu_update_frame.py), and the oracle alone reaches every branch
of the selection the GPU tests (tests/test_gpu_stereo_update.py) then hold the library to."""
import numpy as np
import pytest

import oracle_lib
import stereo_update_ref as sr
import synth


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


@pytest.fixture(scope="module")
def fo():
    return oracle_lib.load_front()


def test_one_camera_is_the_monocular_composition(pkg, oracle, jo, fo):
    """every observation in camera 0, camera 1's side equal to camera 0's: jo.triangulate_batch and the composition of
    test_camera_update_points, decision by decision"""
    sc = synth.vio_scene(F=60, M=15, noise_px=0.4, seed=9)
    t, K8, n = sc["t"], sc["K8"], sc["n_state"]
    st, _ = synth.scene_views(pkg, sc)
    cam = sr.Cam(sc["R_ItoC"], sc["p_IinC"], K8, sr.RADTAN, -1, sc["intr_id"])
    pair = sr.Pair(pkg, sc, [cam, sr.Cam(cam.R, cam.p, K8)])
    rng = np.random.default_rng(0)
    tracks = {}
    for f in range(60):
        a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
        uv = sc["obs_uv"][a:b].astype(np.float32)
        if f == 6:
            uv = uv + rng.normal(0, 9.0, uv.shape).astype(np.float32)
        tracks[f + 1] = (sc["obs_time"][a:b].copy(), uv, fo.undistort(K8, uv))
    tracks[501] = (np.array([t[2]]), np.array([[100.0, 100.0]], dtype=np.float32), np.zeros((1, 2), dtype=np.float32))
    P = synth.spd_cov(n, seed=4) * 1e-4
    MAX, MOBS = 30, 15
    out = sr.update_points(jo, oracle, pair, {fid: {0: o} for fid, o in tracks.items()}, P, MAX, MOBS, t[-2], t[-1])
    # ---- the monocular composition
    pool = [fid for fid, (tt, _, _) in sorted(tracks.items()) if (tt < t[1]).any() or not (tt > t[-2]).any()]
    assert out["n_pool"] == len(pool) and 501 in pool
    pool = [fid for fid in pool if len(tracks[fid][0]) >= 2]
    pool.sort(key=lambda fid: -len(tracks[fid][0]))
    ptr = np.concatenate([[0], np.cumsum([len(tracks[f][0]) for f in pool])]).astype(np.int32)
    tr_all = pkg.Tracks(ptr, np.concatenate([tracks[f][0] for f in pool]), np.concatenate([tracks[f][1] for f in pool]),
                        np.zeros((len(pool), 3)), obs_uvn=np.concatenate([tracks[f][2] for f in pool]))
    p_o, ok_o, err_o = jo.triangulate_batch(st, tr_all, **{k: v for k, v in sr.TRI.items()})
    p_s, ok_s, err_s, _, anchors, _ = sr.triangulate_batch(jo, pair, [{0: tracks[f]} for f in pool])
    assert np.array_equal(ok_s, ok_o) and ok_o.sum() > 30 and set(anchors) == {0}
    good = ok_o > 0
    assert np.abs(p_s[good] - p_o[good]).max() <= 1e-9 * max(1.0, np.abs(p_o).max())
    assert np.abs(err_s[good] - err_o[good]).max() <= 1e-7 * err_o[good].max()
    sel = [q for q in range(len(pool)) if ok_o[q] and err_o[q] < 3.0][:MAX]
    assert len(sel) == MAX and pool.index(7) not in sel
    assert np.array_equal(out["ids"], np.array([pool[q] for q in sel], dtype=np.uint64))
    sptr = np.concatenate([[0], np.cumsum([len(tracks[pool[q]][0]) for q in sel])]).astype(np.int32)
    tr_sel = pkg.Tracks(sptr, np.concatenate([tracks[pool[q]][0] for q in sel]), np.concatenate([tracks[pool[q]][1] for q in sel]), p_o[sel])
    cols = jo.columns(st, tr_sel)
    rows, Hf, Hx, res = jo.build_jacobians(st, tr_sel, cols, 2 * MOBS)
    rc_o, P_o, dx_o, acc_o, nrows_o = oracle.msckf_update(P, rows, Hf, Hx, res, cols, st.c.sigma_pix ** 2, synth.q95_table())
    assert rc_o == out["status"] == 0 and np.array_equal(out["accepted"], acc_o) and out["n_rows"] == nrows_o and acc_o.sum() > 15
    assert np.abs(out["p_FinG"] - p_o[sel]).max() < 1e-6
    assert np.abs(out["dx"] - dx_o).max() <= 1e-7 * max(1.0, np.abs(dx_o).max())
    assert np.abs(out["P"] - P_o).max() <= 1e-8 * np.abs(P).max()
    used = {int(i) for i, a in zip(out["ids"], acc_o) if a}
    assert set(out["db"]) == {fid for fid in tracks if fid not in used and fid != 501}


@pytest.mark.parametrize("pairing", list(sr.PAIRINGS))
def test_scene_reaches_every_branch(pkg, oracle, jo, fo, pairing):
    model0, model1 = sr.PAIRINGS[pairing]
    sc, pair, tracks, names, opt = sr.update_scene(pkg, fo.undistort, model1=model1, model0=model0)
    assert (pair.cams[0].model, pair.cams[1].model) == (model0, model1)
    n = sc["n_state"]
    assert len(sc["t"]) == 15 and 38 <= len(tracks) <= 42
    assert np.linalg.norm(pair.cams[1].p - pair.cams[0].p) == pytest.approx(0.1, abs=0.01) and not np.allclose(pair.cams[1].K8, pair.cams[0].K8)
    P = synth.spd_cov(n, seed=4) * 1e-4
    out = sr.update_points(jo, oracle, pair, tracks, P, **opt)
    tr = out["trace"]
    seen = {fid: (len(ft.get(0, ((),))[0]), len(ft.get(1, ((),))[0])) for fid, ft in tracks.items()}
    # features seen by camera 0 only, by camera 1 only, and by both; in the update
    sel = {int(i) for i in out["ids"]}
    assert any(seen[f][1] == 0 for f in sel) and any(seen[f][0] == 0 for f in sel) and any(min(seen[f]) > 0 for f in sel)
    # the anchor: a tie, a strict majority for each camera — among the triangulated
    tri_ok = [f for f in tr["ok"] if tr["ok"][f]]
    assert any(tr["n_valid"][f][0] == tr["n_valid"][f][1] and tr["anchor"][f] == 1 for f in tri_ok)
    assert any(tr["n_valid"][f][0] > tr["n_valid"][f][1] > 0 and tr["anchor"][f] == 0 for f in tri_ok)
    assert any(tr["n_valid"][f][1] > tr["n_valid"][f][0] > 0 and tr["anchor"][f] == 1 for f in tri_ok)
    # one observation without bounding clones, in camera 1 only: it is back in the database, the feature went on without it
    f = names["late in cam1"]
    assert tr["n_valid"][f] == (15, 15) and seen[f] == (15, 16)
    late = sc["t"][-1] + 0.005
    assert f in sel and out["accepted"][list(out["ids"]).index(f)]
    assert set(out["db"][f]) == {1} and list(out["db"][f][1][0]) == [late]
    # a feature left with fewer than 2 usable observations: everything of it is back
    f = names["one usable"]
    assert sum(tr["n_valid"][f]) == 1 and not tr["ok"][f] and f not in sel and len(out["db"][f][0][0]) == 1 and len(out["db"][f][1][0]) == 15
    # the averaging matters: below 3 px over the cameras, above over the observations
    f = names["camera-averaged"]
    assert tr["ok"][f] and tr["err"][f] < 3.0 < tr["err_obs"][f], (tr["err"][f], tr["err_obs"][f])
    # a biased track fails the consistency test
    f = names["biased"]
    assert tr["ok"][f] and tr["err"][f] >= 3.0 and f not in sel
    # the cap is reached, and candidates behind it return untouched
    assert len(sel) == opt["max_msckf"] and len(tr["order"]) > len(tr["ok"])
    assert out["status"] == 0 and out["accepted"].sum() >= 10 and (out["accepted"] == 0).any()
    f = names["gate"]
    assert f in sel and not out["accepted"][list(out["ids"]).index(f)]
    # still tracked: never left the database
    for f in names["tracked"]:
        assert f not in tr["order"] and sr.db_equal({f: out["db"][f]}, {f: tracks[f]})
    # whatever was accepted is gone, the rest is there
    gone = {int(i) for i, a in zip(out["ids"], out["accepted"]) if a} - {names["late in cam1"]}
    assert not gone & set(out["db"]) and set(tracks) - gone - {names["late in cam1"]} <= set(out["db"])


@pytest.mark.parametrize("pairing", ["equidistant-radtan", "equidistant-equidistant"])
def test_equidistant_camera_0_decides_the_scene(pkg, oracle, jo, fo, pairing):
    """the scenes with camera 0 equidistant still accept and reject — in the triangulation and at the gate — and the same scene with
    camera 0 read as radtan (its eight numbers as fx fy cx cy k1 k2 p1 p2) gives other verdicts: a launch that takes the wrong model
    for camera 0 does not pass the GPU tests' comparison of `ok`, the selection and `accepted`"""
    model0, model1 = sr.PAIRINGS[pairing]
    sc, pair, tracks, names, opt = sr.update_scene(pkg, fo.undistort, model1=model1, model0=model0)
    ids = sorted(tracks)
    feats = [tracks[i] for i in ids]
    p_o, ok_o, err_o, _, _, nv = sr.triangulate_batch(jo, pair, feats)
    assert ok_o.sum() >= 25 and (ok_o == 0).any()
    P = synth.spd_cov(sc["n_state"], seed=4) * 1e-4
    out = sr.update_points(jo, oracle, pair, tracks, P, **opt)
    assert out["status"] == 0 and out["accepted"].sum() >= 10 and (out["accepted"] == 0).any()
    wrong = sr.read_as_radtan(pair)
    p_w, ok_w, err_w, _, _, _ = sr.triangulate_batch(jo, wrong, feats)
    both = (ok_o > 0) & (ok_w > 0) & np.array([n[0] > 0 for n in nv])
    assert both.sum() >= 10
    consistent = lambda ok, err: [bool(o) and e < 3.0 for o, e in zip(ok, err)]
    assert consistent(ok_o, err_o) != consistent(ok_w, err_w)                       # the 3 px test of the selection
    assert np.abs(err_w[both] - err_o[both]).min() > 1e-3                            # every error camera 0 has a part in
    out_w = sr.update_points(jo, oracle, wrong, tracks, P, **opt)
    assert list(out_w["ids"]) != list(out["ids"]) or list(out_w["accepted"]) != list(out["accepted"])
    print(f"{pairing}: triangulated {int(ok_o.sum())} of {len(ids)}, accepted {int(out['accepted'].sum())} of {len(out['ids'])}; camera 0 read as "
          f"radtan: consistent {sum(consistent(ok_w, err_w))} (was {sum(consistent(ok_o, err_o))}), selected {len(out_w['ids'])}, accepted {int(out_w['accepted'].sum())}")


@pytest.mark.parametrize("calib", ["all", "cam0", "cam1", "none"])
def test_stereo_jacobian_columns_on_the_host(pkg, jo, fo, calib):
    """plv_stereo_jacobian_columns is host integer logic: [ext0][int0][dt][ext1][int1], each when estimated, then the clones in
    first-seen order; another observation order, a camera above 1 and a colliding state id are refused"""
    import ctypes as C
    lib = pkg.load_library()
    sc, pair, obs = sr.stereo_scene(pkg, fo.undistort, F=8, calib=calib)
    feats = [obs[1], sr.cut(obs[2], None, ()), sr.cut(obs[3], (), None), obs[0]]
    fl = sr.flatten(feats)

    def columns(fl, side):
        trk = sr.stereo_tracks(pkg, fl, np.zeros((len(feats), 3)))
        cols, k = np.zeros(512, np.int32), C.c_int()
        rc = lib.plv_stereo_jacobian_columns(C.byref(pair.views[0].c), C.byref(side.c), C.byref(trk.c), cols.ctypes.data_as(C.POINTER(C.c_int)), 512,
                                             C.byref(k))
        return rc, cols[:k.value].copy()

    rc, cols = columns(fl, pair.side)
    want = sr.columns(jo, pair, feats)
    assert rc == 0 and np.array_equal(cols, want)
    n0 = sc["n_state"] - 21
    head = {"all": list(range(n0, n0 + 6)) + list(range(15, 23)) + [n0 + 6] + list(range(n0 + 7, n0 + 21)),
            "cam0": list(range(n0, n0 + 6)) + list(range(15, 23)) + [n0 + 6], "cam1": [n0 + 6] + list(range(n0 + 7, n0 + 21)), "none": []}[calib]
    assert list(cols[:len(head)]) == head and len(cols) == len(head) + 6 * 15 and len(set(cols)) == len(cols)
    assert columns(dict(fl, cam=(1 - fl["cam"]).astype(np.uint8)), pair.side)[0] == pkg.PLV_E_BADARG
    assert columns(dict(fl, cam=(fl["cam"] + 1).astype(np.uint8)), pair.side)[0] == pkg.PLV_E_BADARG
    if calib in ("all", "cam0"):
        clash = pkg.CameraSide(pair.cams[1].R, pair.cams[1].p, pair.cams[1].K8, extrinsic_state_id=pair.cams[0].int_id + 4)
        assert columns(fl, clash)[0] == pkg.PLV_E_BADARG and b"collides" in lib.plv_last_error()
