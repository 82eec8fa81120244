"""GPU parity of the landmark passes (plv_camera_update_slam / plv_camera_init_slam) against the oracle, landmark by landmark.

The expected values are the existing oracle bindings chained in Python as the reference's loops chain them (UpdaterCamera.cpp:296-369):
per list entry the system of get_feature_jacobian_full on the CURRENT state (JacOracle.build_jacobians, which honours feat_rep), then
Oracle.slam_update / Oracle.slam_initialize on the host covariance, then the host plv_state_boxplus and the landmarks' value += dx.

The state is the smallest that exercises everything: 6 clones (intr_order + 1 = 4 is the floor), extrinsic, intrinsic and time-offset
calibration on, max_obs = 6, 4 landmarks of which the last closes the covariance (n = 78).

Tolerance: the single-step tolerances of tests/test_gpu_slam.py (1e-9 of max|P|, 1e-8 of max(1e-3, max|dx|) for corrections) times the
number of applied steps — each step's error enters the next linearly at these sizes.  The largest ratio seen is printed."""
import ctypes

import numpy as np
import pytest

import oracle_lib
import synth
import synth_dataset as sd

pytestmark = pytest.mark.gpu

MAX_OBS = 6
LD = 2 * MAX_OBS
CHI2_MULT = 5.0
CAM_DT = 0.003
N_LM = 4
RATIOS = {}     # largest tolerance ratios seen, by check


@pytest.fixture(scope="module")
def own_ctx(pkg):
    """A context of this module's own: the passes hand estimated intrinsics to the context (plv_set_camera_intrinsics)."""
    c = pkg.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


@pytest.fixture(scope="module")
def scene():
    sc = synth.vio_scene(n_clones=6, F=12, M=6, seed=21, noise_px=1.0, dt_clone=0.1, fej_noise=1e-3, depth_scale=0.35)
    return sc


class FilterState:
    """Mean of a small filter in numpy arrays wired as the driver wires them: the state view reads the clone arrays the boxplus call
    writes, and its calibration fields are that call's mirrors."""

    def __init__(self, pkg, sc, rep):
        N = len(sc["t"])
        self.pkg, self.sc, self.rep = pkg, sc, rep
        self.q = np.array([sd.rot_2_quat(R) for R in sc["R"]])
        self.R = np.zeros((N, 9))
        pkg.jpl_left_update(self.q, None, self.R)
        assert np.abs(self.R.reshape(N, 3, 3) - sc["R"]).max() < 1e-12
        self.p = np.array(sc["p"], dtype=np.float64)
        self.Rf, self.pf = np.array(sc["Rf"]).reshape(N, 9).copy(), np.array(sc["pf"]).copy()
        self.qe = sd.rot_2_quat(sc["R_ItoC"])[None].copy()
        self.Re = np.zeros((1, 9))
        pkg.jpl_left_update(self.qe, None, self.Re)
        self.pe, self.K, self.dt = np.array(sc["p_IinC"]), np.array(sc["K8"]), np.array([CAM_DT])
        self.imu_q, self.imu_x = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(12)
        self.n_ext = int(sc["n_state"])
        self.n_base = self.n_ext + 7
        self.sv = pkg.StateView(sc["t"], self.R, self.p, sc["ids"], self.Re.reshape(3, 3), self.pe, self.K, clone_R_fej=self.Rf,
                                clone_p_fej=self.pf, cam_dt=CAM_DT, extrinsic_state_id=self.n_ext, intrinsic_state_id=15,
                                dt_state_id=self.n_ext + 6, sigma_pix=1.0, use_pol_cov=1, intr_ori_cov=1e-6, intr_pos_cov=1e-6, feat_rep=rep)
        assert np.shares_memory(self.sv.R, self.R) and np.shares_memory(self.sv.p, self.p)
        base = ctypes.addressof(self.sv.c)
        m_R, m_p, m_K, m_dt = (base + getattr(pkg.PlvStateView, f).offset for f in ("R_ItoC", "p_IinC", "intrinsics", "cam_dt"))
        ent = [("quat", 0, self.imu_q, None, None), ("vec", 3, self.imu_x, None, None),
               ("quat", self.n_ext, self.qe[0], self.Re[0], m_R), ("vec", self.n_ext + 3, self.pe, None, m_p),
               ("vec", 15, self.K, None, m_K), ("vec", self.n_ext + 6, self.dt, None, m_dt)]
        for i in range(N):
            ent += [("quat", int(sc["ids"][i]), self.q[i], self.R[i], None), ("vec", int(sc["ids"][i]) + 3, self.p[i], None, None)]
        self.plus = pkg.BoxPlus(ent)
        self.lms = pkg.Landmarks(16)

    def add_landmarks(self, xyz, fej_xyz, featids):
        for j, (p, pf, fid) in enumerate(zip(xyz, fej_xyz, featids)):
            self.lms.append(fid, self.n_base + 3 * j, self.rep, self.pkg.landmark_from_xyz(self.rep, p), self.pkg.landmark_from_xyz(self.rep, pf))

    def apply(self, dx):
        self.plus.apply(np.ascontiguousarray(dx))
        for i in range(len(self.lms)):
            e = self.lms[i]
            for q in range(3):
                e.value[q] += dx[e.id + q]

    def arrays(self):
        return dict(q=self.q, p=self.p, R=self.R, qe=self.qe, Re=self.Re, pe=self.pe, K=self.K, dt=self.dt, imu_q=self.imu_q, imu_x=self.imu_x,
                    view_R=np.array(self.sv.c.R_ItoC), view_p=np.array(self.sv.c.p_IinC), view_K=np.array(self.sv.c.intrinsics),
                    view_dt=np.array([self.sv.c.cam_dt]), lm=self.lms.values().copy(), n_lm=np.array([len(self.lms)]),
                    lm_fej=np.array([list(self.lms[i].fej) for i in range(len(self.lms))]).reshape(-1, 3))

    def snapshot(self):
        return {k: np.array(v, copy=True) for k, v in self.arrays().items()}


def _project(sc, R, p, X, cam_dt_shift=None):
    pc = sc["R_ItoC"] @ (R @ (X - p)) + sc["p_IinC"]
    return synth.radtan_distort(sc["K8"], pc[:2] / pc[2])


def _observe(sc, X, times, rng, noise_px=1.0, shift_px=0.0):
    """Observations of point X stamped `times` (image time = stamp + CAM_DT)."""
    uv = []
    for t in times:
        R, p = sc["pose_fn"](t + CAM_DT)
        uv.append(_project(sc, R, p, X) + rng.normal(0, noise_px, 2) + shift_px)
    return np.array(uv, dtype=np.float32).reshape(-1, 2)


def _usable(sc, t):
    return sc["t"][0] - 0.01 <= t + CAM_DT <= sc["t"][-1]


def _tracks(pkg, entries, with_p=False, res=None):
    ptr = np.cumsum([0] + [len(e["t"]) for e in entries]).astype(np.int32)
    t = np.concatenate([e["t"] for e in entries])
    uv = np.concatenate([e["uv"] for e in entries])
    p = np.array([e.get("p", np.zeros(3)) for e in entries])
    kw = dict(res_R=res[0], res_p=res[1]) if res is not None else {}
    return pkg.Tracks(ptr, t, uv, p, **kw), np.array([e["id"] for e in entries], dtype=np.uint64)


def _update_entries(sc, lm_xyz):
    """The update list: 1 observation, 2, a 60 px outlier (gate), max_obs, one observation outside the window (dropped), max_obs + 1
    usable (skipped), an id without a landmark (skipped)."""
    rng = np.random.default_rng(77)
    t = sc["t"]
    inside = lambda n, lo=1: np.sort(rng.choice(np.linspace(t[lo] + 0.004, t[-1] - 0.012, 23), n, replace=False))
    ent = []
    ent.append(dict(id=100, t=np.array([t[3] + 0.02])))
    ent.append(dict(id=101, t=np.array([t[2] - CAM_DT, t[4] + 0.031])))                      # (one exactly at a clone)
    ent.append(dict(id=102, t=inside(MAX_OBS), shift=60.0))
    ent.append(dict(id=103, t=inside(MAX_OBS, 0)))
    ent.append(dict(id=100, t=np.concatenate([[t[0] - 5.0], inside(3)])))
    ent.append(dict(id=101, t=inside(MAX_OBS + 1)))
    ent.append(dict(id=999, t=inside(3)))
    xyz = {100: lm_xyz[0], 101: lm_xyz[1], 102: lm_xyz[2], 103: lm_xyz[3], 999: lm_xyz[0]}
    for e in ent:
        e["uv"] = _observe(sc, xyz[e["id"]], np.clip(e["t"], t[0], None), rng, shift_px=e.get("shift", 0.0))
    return ent


def _system(pkg, jo, fs, t, uv, p, p_fej, res=None):
    """get_feature_jacobian_full for one landmark on fs's current state: rows, Hf, Hx, res, cols."""
    kw = dict(res_R=res[0], res_p=res[1]) if res is not None else {}
    tr = pkg.Tracks([0, len(t)], t, uv, [p], p_FinG_fej=[p_fej], **kw)
    cols = jo.columns(fs.sv, tr)
    rows, Hf, Hx, r = jo.build_jacobians(fs.sv, tr, cols, LD)
    m = int(rows[0])
    return m, Hf[0].T[:m].copy(), Hx[0].T[:m].copy(), r[0][:m].copy(), cols


def _cpi_for(pkg, jo, fs, entries):
    """The poses of every observation from the CPI table, once, on the state at entry: (table, per entry (R, p, ok))."""
    cs = synth.cpi_scene(fs.sc)
    tab = pkg.CpiTable(cs["t"], cs["clone_t"], cs["R"], cs["alpha"], cs["v"], gravity=tuple(cs["gravity"]))
    out = []
    for e in entries:
        R, p, ok = jo.cpi_poses(fs.sv, tab, e["t"] + CAM_DT)
        out.append((R, p, ok.astype(bool)))
    return tab, out


def _oracle_update_chain(pkg, oracle, jo, fs, P, entries, q95, cpi=None):
    """UpdaterCamera::slam_update over the list: verdicts, per-entry dx, the number of applied steps; fs and P end as the reference's."""
    n = P.shape[0]
    verdict, dxs, states = [], [], []
    for j, e in enumerate(entries):
        states.append(fs.snapshot())
        keep = np.array([_usable(fs.sc, x) for x in e["t"]])
        if cpi is not None:
            keep &= cpi[j][2]
        lm = next((fs.lms[i] for i in range(len(fs.lms)) if fs.lms[i].featid == e["id"]), None)
        m = int(keep.sum())
        dxs.append(np.zeros(n))
        if lm is None or m < 1 or m > MAX_OBS:
            verdict.append(0)
            continue
        res = (cpi[j][0][keep], cpi[j][1][keep]) if cpi is not None else None
        r, Hf, Hx, rs, cols = _system(pkg, jo, fs, e["t"][keep], e["uv"][keep], pkg.landmark_xyz(lm.rep, np.array(lm.value)),
                                      pkg.landmark_xyz(lm.rep, np.array(lm.fej)), res)
        assert r == 2 * m
        H = np.hstack([Hx, Hf])
        cols_f = np.concatenate([cols, [lm.id, lm.id + 1, lm.id + 2]]).astype(np.int32)
        rc, P2, acc, dx = oracle.slam_update(P, H, rs, cols_f, q95, chi2_mult=CHI2_MULT)
        if rc != 0:
            verdict.append(3)
        elif not acc:
            verdict.append(2)
        else:
            verdict.append(1)
            P[:] = P2
            fs.apply(dx)
            dxs[-1] = dx
    return np.array(verdict), np.array(dxs), states


def _ratio(name, err, tol):
    r = float(err) / float(tol)
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    print(f"[tolerance ratio] {name}: {r:.3e}")
    return r


def _compare_states(tag, a, b, tol):
    worst = 0.0
    for k in ("q", "p", "qe", "pe", "K", "dt", "lm", "view_R", "view_p", "view_K", "view_dt"):
        if a[k].size:
            worst = max(worst, float(np.abs(a[k] - b[k]).max()))
    assert _ratio(tag, worst, tol) <= 1.0


def _start(pkg, sc, rep, seed=5):
    rng = np.random.default_rng(seed)
    fs_g, fs_o = FilterState(pkg, sc, rep), FilterState(pkg, sc, rep)
    lm_true = sc["pts"][:N_LM]
    est, fej = lm_true + rng.normal(0, 0.01, (N_LM, 3)), lm_true + rng.normal(0, 0.01, (N_LM, 3))
    for fs in (fs_g, fs_o):
        fs.add_landmarks(est, fej, [100, 101, 102, 103])
    n = fs_g.n_base + 3 * N_LM
    assert n == 78 and fs_g.lms[N_LM - 1].id + 3 == n
    P = np.asfortranarray(synth.spd_cov(n, seed=seed + 1))
    return fs_g, fs_o, lm_true, P


@pytest.mark.parametrize("use_cpi", [False, True], ids=["polynomial", "cpi"])
@pytest.mark.parametrize("rep", [0, 1], ids=["GLOBAL_3D", "GLOBAL_FULL_INVERSE_DEPTH"])
def test_update_pass_against_the_oracle_chain(pkg, own_ctx, oracle, jo, scene, rep, use_cpi):
    ctx, sc, q95 = own_ctx, scene, synth.q95_table()
    fs_g, fs_o, lm_true, P0 = _start(pkg, sc, rep)
    entries = _update_entries(sc, lm_true)
    tab, cpi = _cpi_for(pkg, jo, fs_o, entries) if use_cpi else (None, None)
    if use_cpi:   # (one observation inside the window falls between the records of two clones: the table cannot serve it, it is dropped)
        assert sum(int((~c[2]).sum()) for c in cpi) == 2 and not cpi[4][2][0] and not cpi[2][2].all()
    n = P0.shape[0]
    P_o = P0.copy(order="F")
    verdict_o, dx_o, states = _oracle_update_chain(pkg, oracle, jo, fs_o, P_o, entries, q95, cpi)
    assert list(verdict_o) == [1, 1, 2, 1, 1, 0, 0], verdict_o
    steps = int((verdict_o == 1).sum())
    # the landmark after the rejected one is linearised on the unchanged state
    for k in states[2]:
        assert np.array_equal(states[2][k], states[3][k]), k

    ctx.cov_upload(P0)
    tr, ids = _tracks(pkg, entries)
    c0 = pkg.counters()
    out = ctx.camera_update_slam(fs_g.sv, fs_g.plus, fs_g.lms, MAX_OBS, chi2_mult=CHI2_MULT, cpi=tab, tracks=tr, ids=ids, want_dx=n)
    c1 = pkg.counters()
    assert list(out["verdict"]) == list(verdict_o), (out["verdict"], verdict_o)
    assert (out["n_list"], out["n_applied"], out["n_gate"], out["n_not_psd"], out["n_skipped"], out["cov_n"]) == (7, steps, 1, 0, 2, n)
    P_g = ctx.cov_download(n)
    assert _ratio("update: covariance", np.abs(P_g - P_o).max(), 1e-9 * np.abs(P_o).max() * steps) <= 1.0
    applied = 0
    for j in range(len(entries)):
        if verdict_o[j] != 1:
            assert not out["dx_each"][j].any()
            continue
        applied += 1
        tol = 1e-8 * max(1e-3, np.abs(dx_o[j]).max()) * applied
        assert _ratio(f"update: dx of entry {j}", np.abs(out["dx_each"][j] - dx_o[j]).max(), tol) <= 1.0
    _compare_states("update: mean", fs_g.snapshot(), fs_o.snapshot(), 1e-8 * max(1e-3, np.abs(dx_o).max()) * steps)
    assert np.array_equal(fs_g.snapshot()["lm_fej"], fs_o.snapshot()["lm_fej"])
    # (with want_dx the pass still waits once per landmark: the copy of dx is a host copy)
    assert c1["syncs"] - c0["syncs"] <= len(entries) + (2 if use_cpi else 1)


@pytest.mark.parametrize("rep", [0, 1], ids=["GLOBAL_3D", "GLOBAL_FULL_INVERSE_DEPTH"])
def test_update_pass_synchronisations_and_bytes(pkg, own_ctx, jo, scene, rep):
    """At most one host synchronisation per landmark plus a constant per call; with max_obs observations per landmark the bytes
    copied per landmark stay below half of one landmark system, 8 ld (k + 4) bytes.  Both are read as the difference between a list
    and the same list twice, which cancels the per-call part."""
    ctx, sc = own_ctx, scene
    rng = np.random.default_rng(3)
    t = sc["t"]
    used = {}
    for with_cpi in (False, True):
        for reps in (1, 2):
            fs, _, lm_true, P0 = _start(pkg, sc, rep)
            ent = []
            for _ in range(reps):
                for j in range(N_LM):
                    tt = np.sort(rng.choice(np.linspace(t[0] + 0.004, t[-1] - 0.012, 29), MAX_OBS, replace=False))
                    ent.append(dict(id=100 + j, t=tt, uv=_observe(sc, lm_true[j], tt, rng)))
            tab = _cpi_for(pkg, jo, fs, ent)[0] if with_cpi else None
            ctx.cov_upload(P0)
            tr, ids = _tracks(pkg, ent)
            k = max(len(jo.columns(fs.sv, pkg.Tracks([0, MAX_OBS], e["t"], e["uv"], [lm_true[0]]))) for e in ent)
            c0 = pkg.counters()
            out = ctx.camera_update_slam(fs.sv, fs.plus, fs.lms, MAX_OBS, chi2_mult=CHI2_MULT, cpi=tab, tracks=tr, ids=ids)
            c1 = pkg.counters()
            assert out["n_skipped"] == 0 and out["n_applied"] + out["n_gate"] == len(ent)
            used[(with_cpi, reps)] = (c1["syncs"] - c0["syncs"], c1["copy_bytes"] - c0["copy_bytes"], c1["launches"] - c0["launches"],
                                      c1["copies"] - c0["copies"], k)
        (s1, b1, l1, m1, k1), (s2, b2, l2, m2, k2) = used[(with_cpi, 1)], used[(with_cpi, 2)]
        per_lm_syncs, per_lm_bytes = (s2 - s1) / N_LM, (b2 - b1) / N_LM
        print(f"[update pass, cpi={with_cpi}] per landmark: {per_lm_syncs} syncs, {per_lm_bytes} bytes, {(l2 - l1) / N_LM} launches, "
              f"{(m2 - m1) / N_LM} copies; per call: {s1 - N_LM * per_lm_syncs} syncs; k = {k2}, half a system = {4 * LD * (k2 + 4)} bytes")
        assert per_lm_syncs <= 1.0 and s1 <= N_LM + 2
        assert per_lm_bytes < 0.5 * 8 * LD * (min(k1, k2) + 4)


def _init_entries(sc):
    """The initialisation list: a zero residual (chi < 1e-7), 2 observations (4 rows), a 60 px outlier in the updating rows (gate),
    max_obs, 1 observation, an id the state already holds, and one more good candidate that meets the grown state."""
    rng = np.random.default_rng(91)
    t = sc["t"]
    pts = sc["pts"][N_LM:]
    inside = lambda n: np.sort(rng.choice(np.linspace(t[0] + 0.004, t[-1] - 0.012, 23), n, replace=False))
    ent = [dict(id=204, t=t[1:5] - CAM_DT, X=pts[4], exact=True),      # (first: its residual is zero on the state as it starts)
           dict(id=200, t=np.array([t[1] + 0.02, t[5] - 0.03]), X=pts[0]),
           dict(id=201, t=inside(MAX_OBS), X=pts[1], shift_late=60.0),
           dict(id=202, t=inside(MAX_OBS), X=pts[2]),
           dict(id=203, t=inside(1), X=pts[3]),
           dict(id=101, t=inside(4), X=pts[5]),
           dict(id=206, t=inside(3), X=pts[6])]
    for e in ent:
        if e.get("exact"):
            # the candidate's position reprojected without noise at the state's own clone poses: every residual is zero up to rounding
            e["p"] = e["X"].copy()
            e["uv"] = np.array([_project(sc, sc["R"][i], sc["p"][i], e["X"]) for i in range(1, 5)], dtype=np.float64)
            continue
        e["uv"] = _observe(sc, e["X"], e["t"], rng)
        if "shift_late" in e:
            e["uv"][3:] += e["shift_late"]
        e["p"] = e["X"] + rng.normal(0, 0.02, 3)
    return ent


def _oracle_init_chain(pkg, oracle, jo, fs, P, entries, q95, slam_ids):
    verdict, dxs, sizes = [], [], []
    for e in entries:
        n = P.shape[0]
        keep = np.array([_usable(fs.sc, x) for x in e["t"]])
        m = int(keep.sum())
        dxs.append(None)
        sizes.append(n)
        if e["id"] in slam_ids or any(fs.lms[i].featid == e["id"] for i in range(len(fs.lms))) or m < 2 or m > MAX_OBS:
            verdict.append(0)
            continue
        r, Hf, Hx, rs, cols = _system(pkg, jo, fs, e["t"][keep], e["uv"][keep], e["p"], e["p"])
        assert r == 2 * m >= 4
        ok, P2, dxi, dx = oracle.slam_initialize(P, Hf, Hx, rs, cols, q95, chi2_mult=CHI2_MULT)
        if not ok:
            verdict.append(2)
            continue
        verdict.append(1)
        P = np.asfortranarray(P2)
        v = pkg.landmark_from_xyz(fs.rep, e["p"])
        fs.lms.append(e["id"], n, fs.rep, v + dxi, v)
        fs.apply(dx)
        dxs[-1] = (dxi, dx)
    return np.array(verdict), dxs, sizes, P


@pytest.mark.parametrize("rep", [0, 1], ids=["GLOBAL_3D", "GLOBAL_FULL_INVERSE_DEPTH"])
def test_init_pass_against_the_oracle_chain(pkg, own_ctx, oracle, jo, scene, rep):
    ctx, sc, q95 = own_ctx, scene, synth.q95_table()
    fs_g, fs_o, _, P0 = _start(pkg, sc, rep)
    entries = _init_entries(sc)
    n0 = P0.shape[0]
    slam_ids = [100, 101, 102, 103]
    verdict_o, dx_o, sizes, P_o = _oracle_init_chain(pkg, oracle, jo, fs_o, P0.copy(order="F"), entries, q95, slam_ids)
    assert list(verdict_o) == [2, 1, 2, 1, 0, 0, 1], verdict_o
    steps = int((verdict_o == 1).sum())
    assert P_o.shape[0] == n0 + 3 * steps and sizes[-1] == n0 + 6       # the last candidate met the twice-grown state

    ctx.cov_upload(P0)
    tr, ids = _tracks(pkg, entries)
    c0 = pkg.counters()
    out = ctx.camera_init_slam(fs_g.sv, fs_g.plus, fs_g.lms, MAX_OBS, chi2_mult=CHI2_MULT, slam_ids=slam_ids, tracks=tr, ids=ids, want_dx=n0)
    c1 = pkg.counters()
    assert list(out["verdict"]) == list(verdict_o), (out["verdict"], verdict_o)
    assert out["cov_n"] == n0 + 3 * steps and len(fs_g.lms) == N_LM + steps and out["n_applied"] == steps
    assert [fs_g.lms[i].featid for i in range(N_LM, N_LM + steps)] == [200, 202, 206]
    assert [fs_g.lms[i].id for i in range(N_LM, N_LM + steps)] == [n0, n0 + 3, n0 + 6]
    P_g = ctx.cov_download(n0 + 3 * steps)
    assert _ratio("init: covariance", np.abs(P_g - P_o).max(), 1e-9 * np.abs(P_o).max() * steps) <= 1.0
    applied, dmax = 0, 1e-3
    for j, d in enumerate(dx_o):
        row = out["dx_each"][j]
        if d is None:
            assert not row.any()
            continue
        applied += 1
        dxi, dx = d
        dmax = max(dmax, np.abs(dx).max(), np.abs(dxi).max())
        assert _ratio(f"init: dx_init of candidate {j}", np.abs(row[:3] - dxi).max(), 1e-9 * max(1.0, np.abs(dxi).max()) * applied) <= 1.0
        assert _ratio(f"init: dx of candidate {j}", np.abs(row[3:3 + len(dx)] - dx).max(), 1e-8 * max(1e-3, np.abs(dx).max()) * applied) <= 1.0
    _compare_states("init: mean", fs_g.snapshot(), fs_o.snapshot(), 1e-8 * dmax * steps)
    assert np.abs(fs_g.snapshot()["lm_fej"] - fs_o.snapshot()["lm_fej"]).max() == 0.0
    # at most two host synchronisations per candidate plus a constant
    assert c1["syncs"] - c0["syncs"] <= 2 * len(entries) + 1
    print(f"[init pass] {c1['syncs'] - c0['syncs']} syncs, {c1['launches'] - c0['launches']} launches, {c1['copy_bytes'] - c0['copy_bytes']} bytes "
          f"for {len(entries)} candidates ({steps} initialised)")


@pytest.mark.parametrize("rep", [0, 1], ids=["GLOBAL_3D", "GLOBAL_FULL_INVERSE_DEPTH"])
def test_rejected_candidates_leave_the_covariance_bit_equal(pkg, own_ctx, scene, rep):
    ctx, sc = own_ctx, scene
    fs, _, _, P0 = _start(pkg, sc, rep)
    entries = [e for e in _init_entries(sc) if e["id"] in (201, 203, 204, 101)]
    before = fs.snapshot()
    ctx.cov_upload(P0)
    tr, ids = _tracks(pkg, entries)
    out = ctx.camera_init_slam(fs.sv, fs.plus, fs.lms, MAX_OBS, chi2_mult=CHI2_MULT, slam_ids=[101], tracks=tr, ids=ids)
    assert list(out["verdict"]) == [2, 2, 0, 0] and out["cov_n"] == P0.shape[0] and len(fs.lms) == N_LM
    assert np.array_equal(ctx.cov_download(P0.shape[0]), P0)
    after = fs.snapshot()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # ... and an update list in which nothing passes leaves everything as it was, too
    lm_true = sc["pts"][:N_LM]
    upd = [e for e in _update_entries(sc, lm_true) if e["id"] == 999]
    tt = np.linspace(sc["t"][1] + 0.004, sc["t"][-1] - 0.012, MAX_OBS)
    # (600 px: far beyond any gate on the state as it starts, whatever the representation's covariance)
    upd.insert(0, dict(id=102, t=tt, uv=_observe(sc, lm_true[2], tt, np.random.default_rng(8), shift_px=600.0)))
    tr, ids = _tracks(pkg, upd)
    out = ctx.camera_update_slam(fs.sv, fs.plus, fs.lms, MAX_OBS, chi2_mult=CHI2_MULT, tracks=tr, ids=ids, want_dx=P0.shape[0])
    assert list(out["verdict"]) == [2, 0] and not out["dx_each"].any()
    assert np.array_equal(ctx.cov_download(P0.shape[0]), P0)
    after = fs.snapshot()
    assert all(np.array_equal(before[k], after[k]) for k in before)


def test_refused_arguments_change_nothing(pkg, own_ctx, scene):
    ctx, sc = own_ctx, scene
    lib, C = ctx.lib, ctypes
    fs, _, lm_true, P0 = _start(pkg, sc, 1)
    n = P0.shape[0]
    ctx.cov_upload(P0)
    upd = _update_entries(sc, lm_true)[:2]
    ini = _init_entries(sc)[1:2]
    before = fs.snapshot()
    opt = pkg.PlvUpdateOptions(0, MAX_OBS, CHI2_MULT, pkg.PlvTriOptions(0, 0, 0, 0, 0), 0.0, 0.0, 0, 0, 0, None, 0, None)
    res, verdict = pkg.PlvSlamResult(), np.zeros(8, dtype=np.uint8)
    vp = lambda a: C.cast(a, C.c_void_p)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))

    def update(st=fs.sv, o=opt, n_var=fs.plus.n, vars_=fs.plus.vars, n_lm=None, lms=fs.lms.a, r=res, ids="own", v=verdict):
        tr, own_ids = _tracks(pkg, upd)
        return lib.plv_camera_update_slam(ctx.h, C.byref(st.c) if st is not None else None, C.byref(o) if o is not None else None, n_var,
                                          vp(vars_) if vars_ is not None else None, len(fs.lms) if n_lm is None else n_lm,
                                          vp(lms) if lms is not None else None, C.byref(tr.c), C.byref(r) if r is not None else None,
                                          u64(own_ids) if ids == "own" else None, u8(v) if v is not None else None, None)

    def init(cap=16, n_lm=None, lms=fs.lms.a, r=res, v=verdict, vars_=fs.plus.vars):
        tr, own_ids = _tracks(pkg, ini)
        nl = C.c_int(len(fs.lms))
        return lib.plv_camera_init_slam(ctx.h, C.byref(fs.sv.c), C.byref(opt), fs.plus.n, vp(vars_) if vars_ is not None else None,
                                        C.byref(nl) if n_lm is None else None, cap, vp(lms) if lms is not None else None, C.byref(tr.c),
                                        C.byref(r) if r is not None else None, u64(own_ids), u8(v) if v is not None else None, None)

    def unchanged():
        after = fs.snapshot()
        return np.array_equal(ctx.cov_download(n), P0) and all(np.array_equal(before[k], after[k]) for k in before)

    bad = pkg.PLV_E_BADARG
    # null pointers
    for call in (lambda: update(st=None), lambda: update(o=None), lambda: update(vars_=None), lambda: update(lms=None), lambda: update(r=None),
                 lambda: update(ids=None), lambda: update(v=None), lambda: init(n_lm="null"), lambda: init(lms=None), lambda: init(r=None),
                 lambda: init(v=None), lambda: init(vars_=None)):
        assert call() == bad
        assert unchanged()
    # an unknown representation, a landmark beyond the covariance
    for field, value in (("rep", 3), ("id", n - 2), ("id", -1)):
        keep = getattr(fs.lms[1], field)
        setattr(fs.lms.a[1], field, value)
        assert update() == bad and init() == bad
        setattr(fs.lms.a[1], field, keep)
        assert unchanged()
    # a variable beyond the covariance
    keep = fs.plus.vars[3].id
    fs.plus.vars[3].id = n - 1
    assert update() == bad and init() == bad
    fs.plus.vars[3].id = keep
    assert unchanged()
    # no room for the candidates
    assert init(cap=len(fs.lms)) == bad and unchanged()
    # ... and the same calls with nothing wrong are taken
    assert update() == 0 and list(verdict[:2]) == [1, 1]
    assert init() == 0 and verdict[0] == 1


def test_record_tolerance_ratios():
    """(last in the file) the largest tolerance ratios the parity tests above saw, for profiles/slam_pass.json"""
    for k in sorted(RATIOS):
        print(f"[largest ratio] {k}: {RATIOS[k]:.3e}")
    assert all(v <= 1.0 for v in RATIOS.values())
