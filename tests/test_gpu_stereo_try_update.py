"""plv_stereo_try_update on the device: the point half with a CPI table (use_imu_res) against tests/stereo_cpi_ref.py — the scene
tests/test_stereo_cpi_ref_cpu.py pins: 752 x 480 observations only, a 15-clone window, max_msckf as in sr.update_scene —, the state
it moves, point_used, and what it refuses.  Tolerances are those of tests/test_gpu_stereo_update.py: p 1e-6, dx 1e-7 x max(1, |dx|),
P 1e-8 x max|P0|; the variables after boxplus take the bound of dx."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import stereo_cpi_ref as scr
import stereo_update_ref as sr
import synth
from vio_sequence import rot_2_quat

pytestmark = pytest.mark.gpu

W, H = 752, 480
_REF = {}


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


@pytest.fixture(scope="module")
def fo():
    return oracle_lib.load_front()


def _ref(pkg, jo, fo, oracle, model1, model0=sr.RADTAN):
    """(scene, pair, tracks, names, options, table records, P, the restatement's first update), once per pairing and left unchanged"""
    if (model0, model1) not in _REF:
        sc, pair, tracks, names, opt, cp = scr.update_scene(pkg, fo.undistort, model1=model1, model0=model0)
        P = synth.spd_cov(sc["n_state"], seed=4) * 1e-4
        _REF[model0, model1] = (sc, pair, tracks, names, opt, cp, P, scr.update_points(jo, oracle, pair, tracks, P, cp, scr.table(pkg, cp), **opt))
    return _REF[model0, model1]


def _stereo_ctx(pkg, pair, tracks=None, P=None):
    c = pkg.Context(pkg.default_config(W, H))
    if pair.cams[0].model == sr.EQUI:
        c.set_camera_model("equidistant")
    c.stereo_configure(pair.cams[1].K8, pair.cams[1].model)
    for fid, ft in (tracks or {}).items():
        for cam, o in ft.items():
            if len(o[0]):
                c.stereo_db_append_measurements(fid, cam, o[0], o[1], o[2])
    if P is not None:
        c.cov_upload(P)
    return c


def _db(c):
    ids = c.stereo_db_ids()
    out = {int(i): {} for i in ids}
    for cam in (0, 1):
        ptr, t, uv, uvn = c.stereo_db_export(ids, cam)
        for q, i in enumerate(ids):
            if ptr[q + 1] > ptr[q]:
                out[int(i)][cam] = (t[ptr[q]:ptr[q + 1]], uv[ptr[q]:ptr[q + 1]], uvn[ptr[q]:ptr[q + 1]])
    return out


class Moving:
    """A pair's state as variables the library moves: a view and a CameraSide of their own arrays, and the BoxPlus whose entries mirror
    into them — clones (JPL quaternion with the view's matrix as output, position), both extrinsics, both intrinsics, the time offset."""

    def __init__(self, pkg, sc, pair):
        own = dict(sc, **{k: np.array(sc[k]) for k in ("t", "R", "p", "Rf", "pf", "ids")})
        cams = [sr.Cam(c.R.copy(), c.p.copy(), c.K8.copy(), c.model, c.ext_id, c.int_id) for c in pair.cams]
        self.pair = sr.Pair(pkg, own, cams, dt=pair.dt, dt_id=pair.dt_id, sigma_pix=pair.sigma, **pair.kw)
        self.st, self.side = self.pair.views[0], self.pair.side
        st = self.st
        N = len(st.t)
        self.q = np.array([rot_2_quat(R.reshape(3, 3)) for R in st.R])
        addr = lambda obj, struct, name: C.addressof(obj) + getattr(struct, name).offset
        ent = []
        for i in range(N):
            ent += [("quat", int(st.ids[i]), self.q[i], st.R[i], None), ("vec", int(st.ids[i]) + 3, st.p[i], None, None)]
        self.qe = np.array([rot_2_quat(c.R) for c in cams])
        self.Re, self.pe, self.K = np.zeros((2, 9)), np.array([c.p for c in cams]), np.array([c.K8 for c in cams])
        self.dt = np.array([pair.dt])
        for c, (obj, struct) in enumerate(((st.c, pkg.PlvStateView), (self.side.c, pkg.PlvCameraSide))):
            if cams[c].ext_id >= 0:
                ent += [("quat", cams[c].ext_id, self.qe[c], self.Re[c], addr(obj, struct, "R_ItoC")),
                        ("vec", cams[c].ext_id + 3, self.pe[c], None, addr(obj, struct, "p_IinC"))]
            if cams[c].int_id >= 0:
                ent.append(("vec", cams[c].int_id, self.K[c], None, addr(obj, struct, "intrinsics")))
        if pair.dt_id >= 0:
            ent.append(("vec", pair.dt_id, self.dt, None, addr(st.c, pkg.PlvStateView, "cam_dt")))
        self.cams, self.dt_id = cams, pair.dt_id
        self.plus = pkg.BoxPlus(ent)

    def values(self):
        """every variable's value, and what the view and the side hold of them (the mirrors)"""
        st, side = self.st, self.side
        return dict(q=self.q.copy(), R=st.R.copy(), p=st.p.copy(), qe=self.qe.copy(), pe=self.pe.copy(), K=self.K.copy(), dt=self.dt.copy(),
                    view_R=np.array(st.c.R_ItoC), view_p=np.array(st.c.p_IinC), view_K=np.array(st.c.intrinsics), view_dt=np.array([st.c.cam_dt]),
                    side_R=np.array(side.c.R_ItoC), side_p=np.array(side.c.p_IinC), side_K=np.array(side.c.intrinsics))

    def expected(self, pkg, before, dx):
        """`before` (values()) moved by dx with the host arithmetic tests/test_state_boxplus.py holds to the reference's types"""
        ids = self.st.ids
        want = {k: v.copy() for k, v in before.items()}
        q = before["q"].copy()
        R = np.zeros((len(ids), 9))
        pkg.jpl_left_update(q, np.array([dx[i:i + 3] for i in ids]), R)
        want["q"], want["R"] = q, R
        want["p"] = before["p"] + np.array([dx[i + 3:i + 6] for i in ids])
        for c, pre in enumerate(("view", "side")):
            cam = self.cams[c]
            if cam.ext_id >= 0:
                qe, Re = before["qe"][c:c + 1].copy(), np.zeros((1, 9))
                pkg.jpl_left_update(qe, dx[cam.ext_id:cam.ext_id + 3].reshape(1, 3), Re)
                want["qe"][c], want[pre + "_R"] = qe[0], Re[0]
                want["pe"][c] = before["pe"][c] + dx[cam.ext_id + 3:cam.ext_id + 6]
                want[pre + "_p"] = want["pe"][c]
            if cam.int_id >= 0:
                want["K"][c] = before["K"][c] + dx[cam.int_id:cam.int_id + 8]
                want[pre + "_K"] = want["K"][c]
        if self.dt_id >= 0:
            want["dt"] = before["dt"] + dx[self.dt_id]
            want["view_dt"] = want["dt"]
        return want


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


def _check_used(c, used, what):
    ids, p, newest = c.point_used_list()
    assert [int(i) for i in ids] == sorted(used), (what, ids, sorted(used))
    for i, fid in enumerate(ids):
        assert np.abs(p[i] - used[int(fid)][0]).max() < 1e-6 and newest[i] == used[int(fid)][1], (what, int(fid))


def _check_state(pkg, mv, before, ref_dx, what):
    got, want = mv.values(), mv.expected(pkg, before, ref_dx)
    tol = 1e-7 * max(1.0, np.abs(ref_dx).max())
    worst = {k: float(np.abs(got[k] - want[k]).max()) for k in want}
    print(f"{what}: variables after boxplus, worst {max(worst.values()):.1e} (tolerance {tol:.1e})")
    assert all(v <= tol for v in worst.values()), (what, worst)
    # the mirrors hold what the variables hold, bit for bit; the intrinsics of both cameras moved
    assert np.array_equal(got["view_R"], mv.Re[0]) and np.array_equal(got["side_R"], mv.Re[1])
    assert np.array_equal(got["view_K"], got["K"][0]) and np.array_equal(got["side_K"], got["K"][1])
    assert np.array_equal(got["view_p"], got["pe"][0]) and np.array_equal(got["side_p"], got["pe"][1]) and got["view_dt"][0] == got["dt"][0]
    assert np.abs(got["K"][0] - before["K"][0]).max() > 0 and np.abs(got["K"][1] - before["K"][1]).max() > 0


@pytest.mark.parametrize("pairing", list(sr.PAIRINGS))
def test_cpi_update_against_restatement(pkg, jo, fo, oracle, pairing):
    """the pairings (camera 0, camera 1); camera 0's model is the context's (tests/test_stereo_cpi_ref_cpu.py: read as radtan, a scene
    with camera 0 equidistant gives another selection or other verdicts)"""
    model0, model1 = sr.PAIRINGS[pairing]
    sc, pair, tracks, names, opt, cp, P, ref = _ref(pkg, jo, fo, oracle, model1, model0)
    n = sc["n_state"]
    c = _stereo_ctx(pkg, pair, tracks, P)
    try:
        assert sr.db_equal(_db(c), tracks)
        mv = Moving(pkg, sc, pair)
        before = mv.values()
        out, lines, _ = c.stereo_try_update(mv.st, mv.side, mv.plus, n, **opt, lines=False, cpi=scr.table(pkg, cp), **sr.TRI)
        assert lines is None
        _check_update(out, ref, P, c, n, "first update")
        _check_used(c, ref["used"], "first update")
        _check_state(pkg, mv, before, ref["dx"], "first update")
        # ---- one frame later, on the database, the covariance and point_used the first update left behind
        sc2, pair2, new = sr.advance(pkg, sc, pair, fo.undistort, ref["db"])
        assert len(new) >= 5
        for fid, ft in new.items():
            for cam, o in ft.items():
                c.stereo_db_append_measurements(fid, cam, o[0], o[1], o[2])
        cp2 = scr.cut_table(synth.cpi_scene(sc2), sc2)
        opt2 = dict(opt, t_prev_frame=float(sc["t"][-1]), state_time=float(sc2["t"][-1]))
        ref2 = scr.update_points(jo, oracle, pair2, sr.db_append(ref["db"], new), ref["P"], cp2, scr.table(pkg, cp2), **opt2)
        assert ref2["n_pool"] >= 5 and len(ref2["ids"]) >= 3 and ref2["unserved"][0] + ref2["unserved"][1] >= 1
        mv2 = Moving(pkg, sc2, pair2)
        before2 = mv2.values()
        out2, _, _ = c.stereo_try_update(mv2.st, mv2.side, mv2.plus, n, **opt2, lines=False, cpi=scr.table(pkg, cp2), **sr.TRI)
        _check_update(out2, ref2, P, c, n, "second update")
        _check_used(c, {**ref["used"], **ref2["used"]}, "second update")       # (no line half: nothing cleans the list)
        _check_state(pkg, mv2, before2, ref2["dx"], "second update")
    finally:
        c.close()


def test_without_table_equals_update_points_plus_boxplus(pkg, jo, fo, oracle):
    sc, pair, tracks, names, opt, cp, P, _ = _ref(pkg, jo, fo, oracle, sr.RADTAN)
    n = sc["n_state"]
    a, b = _stereo_ctx(pkg, pair, tracks, P), _stereo_ctx(pkg, pair, tracks, P)
    try:
        ma, mb = Moving(pkg, sc, pair), Moving(pkg, sc, pair)
        want = a.stereo_update_points(ma.st, ma.side, n, **opt, **sr.TRI)
        ma.plus.apply(want["dx"])
        out, lines, _ = b.stereo_try_update(mb.st, mb.side, mb.plus, n, **opt, lines=False, **sr.TRI)
        assert lines is None and want["n_accepted"] >= 10 and np.abs(want["dx"]).max() > 0
        for k in ("n_pool", "n_msckf", "n_accepted", "n_rows", "n_returned", "status"):
            assert out[k] == want[k], k
        assert np.array_equal(out["ids"], want["ids"]) and np.array_equal(out["accepted"], want["accepted"])
        assert np.array_equal(out["dx"], want["dx"]) and np.array_equal(out["p_FinG"], want["p_FinG"])
        assert np.array_equal(a.cov_download(n), b.cov_download(n))
        da, db = _db(a), _db(b)
        assert set(da) == set(db)
        for fid in da:
            for cam in (0, 1):
                assert (cam in da[fid]) == (cam in db[fid])
                if cam in da[fid]:
                    assert all(np.array_equal(x, y) for x, y in zip(da[fid][cam], db[fid][cam])), (fid, cam)
        va, vb = ma.values(), mb.values()
        for k in va:
            assert np.array_equal(va[k], vb[k]), k
        # plv_stereo_update_points records nothing in point_used, the try_update does
        assert len(a.point_used_list()[0]) == 0 and set(int(i) for i in out["ids"]) <= set(int(i) for i in b.point_used_list()[0])
    finally:
        a.close()
        b.close()


def test_table_adds_no_synchronisation(pkg, jo, fo, oracle):
    """one call with a table that serves every observation, one without, on twins: the same update route, the same number of
    synchronisations, at most two launches more (cpi_pose_kernel in front of the triangulation; the Jacobian launch reads its poses)"""
    sc, pair, tracks, names, opt, _, P, _ = _ref(pkg, jo, fo, oracle, sr.RADTAN)
    n = sc["n_state"]
    cp = synth.cpi_scene(sc)
    assert all(scr.servable(sc["t"], cp, x + pair.dt) for ft in tracks.values() for o in ft.values() for x in o[0])
    a, b = _stereo_ctx(pkg, pair, tracks, P), _stereo_ctx(pkg, pair, tracks, P)
    try:
        ma, mb = Moving(pkg, sc, pair), Moving(pkg, sc, pair)
        tab = scr.table(pkg, cp)
        for c in (a, b):
            c.synchronize()
        c0 = pkg.counters()
        plain, _, _ = a.stereo_try_update(ma.st, ma.side, ma.plus, n, **opt, lines=False, **sr.TRI)
        c1 = pkg.counters()
        with_t, _, _ = b.stereo_try_update(mb.st, mb.side, mb.plus, n, **opt, lines=False, cpi=tab, **sr.TRI)
        c2 = pkg.counters()
        assert plain["n_accepted"] >= 10 and with_t["n_accepted"] >= 10
        assert a.update_compression_mode()[1] == b.update_compression_mode()[1]
        d_plain = {k: c1[k] - c0[k] for k in ("launches", "syncs")}
        d_table = {k: c2[k] - c1[k] for k in ("launches", "syncs")}
        print(f"without a table {d_plain}, with a table {d_table}, route {a.update_compression_mode()[1]}")
        assert d_table["syncs"] == d_plain["syncs"]
        assert d_plain["launches"] < d_table["launches"] <= d_plain["launches"] + 2
    finally:
        a.close()
        b.close()


def test_refusals_leave_everything_as_it_was(pkg, jo, fo, oracle):
    sc, pair, tracks, names, opt, cp, P, _ = _ref(pkg, jo, fo, oracle, sr.RADTAN)
    n = sc["n_state"]
    k = 98
    cols = synth.col_map(n, k)
    batch = synth.msckf_batch(F=20, M=15, k=k, seed=9)
    c, plain = _stereo_ctx(pkg, pair, tracks, P), pkg.Context(pkg.default_config(W, H))
    try:
        c.feat_batch_upload(*batch, cols)
        c.point_used_insert(4242, np.array([1.0, 2.0, 3.0]), sc["t"][-1])
        mv = Moving(pkg, sc, pair)
        before = mv.values()
        tab = scr.table(pkg, cp)

        def call(ctx=c, st=mv.st, side=mv.side, plus=mv.plus, **kw):
            return ctx.stereo_try_update(st, side, plus, n, **dict(opt, **kw), lines=False, cpi=tab, **sr.TRI)

        def refused(fn, word):
            with pytest.raises(pkg.PlvError) as e:
                fn()
            assert e.value.code == pkg.PLV_E_BADARG and word in str(e.value), str(e.value)

        # max_slam is not an argument of the one-call wrapper: through the structure
        io, _ = c._try_update_io(mv.plus, n, opt["max_msckf"], opt["max_obs"], opt["t_prev_frame"], opt["state_time"], lines=False, cpi=tab, **sr.TRI)
        op = C.cast(io.opt_points, C.POINTER(pkg.PlvUpdateOptions)).contents
        op.max_slam = 3
        assert c.lib.plv_stereo_try_update(c.h, C.byref(mv.st.c), C.byref(mv.side.c), C.byref(io)) == pkg.PLV_E_BADARG
        assert b"max_slam" in c.lib.plv_last_error()
        op.max_slam = 0
        with_cov = sr.Pair(pkg, sc, pair.cams, dt_id=pair.dt_id, use_imu_cov=1)
        refused(lambda: call(st=with_cov.views[0]), "use_imu_cov")
        c.decision_trace(True)
        refused(lambda: call(), "decision trace")
        c.decision_trace(False)
        plain.cov_upload(P)
        refused(lambda: call(ctx=plain), "stereo")
        refused(lambda: call(side=None), "camera 1")
        for clash in (dict(extrinsic_state_id=pair.cams[0].ext_id + 3), dict(intrinsic_state_id=pair.cams[0].int_id), dict(extrinsic_state_id=pair.dt_id - 5),
                      dict(extrinsic_state_id=pair.cams[1].int_id + 2, intrinsic_state_id=pair.cams[1].int_id)):
            bad = pkg.CameraSide(pair.cams[1].R, pair.cams[1].p, pair.cams[1].K8, **dict(dict(extrinsic_state_id=pair.cams[1].ext_id, intrinsic_state_id=pair.cams[1].int_id), **clash))
            refused(lambda: call(side=bad), "collides")
        # what plv_state_boxplus refuses of the variables: an index beyond the covariance, an unknown kind
        K = np.zeros(8)
        refused(lambda: call(plus=pkg.BoxPlus([("vec", n - 4, K, None, None)])), "variable")
        odd = pkg.BoxPlus([("vec", 0, K, None, None)])
        odd.vars[0].kind = 7
        refused(lambda: call(plus=odd), "variable")
        # ---- covariance, variables, both databases, point_used and the staged batch are as they were
        after = mv.values()
        for key in before:
            assert np.array_equal(before[key], after[key]), key
        assert sr.db_equal(_db(c), tracks) and c.line_db_size() == 0
        assert np.array_equal(c.cov_download(n), P)
        ids, p, newest = c.point_used_list()
        assert list(ids) == [4242] and np.array_equal(p[0], [1.0, 2.0, 3.0]) and newest[0] == sc["t"][-1]
        plain.feat_batch_upload(*batch, cols)
        a, b = c.msckf_update_resident(n, 1.0), plain.msckf_update_resident(n, 1.0)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    finally:
        c.close()
        plain.close()
