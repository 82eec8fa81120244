"""Restatement of the stereo point update (plv_triangulate_stereo, plv_build_jacobians_stereo, plv_stereo_update_points), composed of
oracle pieces that exist: what CamHelper::get_features / feature_triangulation / moving_consistency / get_feature_jacobian_full and
UpdaterCamera::msckf_update do when Feature::timestamps holds two cameras.

Order.  A feature's observations are visited camera 1 first (oldest to newest), then camera 0 — the iteration order of the
reference's std::unordered_map that got key 0, then key 1 (include/plviwo.h, "Order and anchor").
Anchor.  The last observation of the camera with strictly more usable observations, camera 1 on a tie.  jo.triangulate
(orc_triangulate) anchors on the LAST entry of the list it is handed, so the list is rotated by whole camera blocks: the anchor
camera's block comes last — [camera 0, camera 1] when camera 1 anchors, [camera 1, camera 0] when camera 0 does.  The sums over the
observations then run in that order; the library stages the same order for its kernel.
Jacobians.  jo.build_jacobians once per camera on that camera's observations with that camera's view; the blocks are stacked camera 1
then camera 0 and scattered into the joint columns by state index.  The oracle has no fisheye model: an equidistant camera's rows
are formed from the oracle's rows for the same camera without distortion (dz/dzn = diag(fx, fy) there) and tests/cam_equi.py — the
identity tests/test_gpu_equidistant.py holds the monocular path to; it needs isotropic noise (use_pol_cov off).
Consistency error.  The pixel residual of every usable observation (CamBase::distort_d's float round trip), averaged per camera and
then over the cameras that have observations."""
import numpy as np

import cam_equi
import synth

RADTAN, EQUI = 0, 1
MILD_EQUI = np.array([458.654, 457.296, 367.215, 248.375, -0.013, 0.002, -0.0005, 0.0001])
EQUI0_COEFFS = np.array([-0.35, 0.12, -0.03, 0.004])  # camera 0 when equidistant: STRONG of test_gpu_equidistant.py on the scene's fx fy cx cy
TRI = dict(max_cond=1e7, max_dist=100.0, max_baseline=1e3, min_dist=0.1)


class Cam:
    def __init__(self, R_ItoC, p_IinC, K8, model=RADTAN, ext_id=-1, int_id=-1):
        self.R, self.p, self.K8, self.model, self.ext_id, self.int_id = np.asarray(R_ItoC, float), np.asarray(p_IinC, float), np.asarray(K8, float), model, ext_id, int_id


class Pair:
    """The two cameras on one window: views[c] is the plv_state_view of camera c (shared time offset)."""

    def __init__(self, pkg, sc, cams, dt=0.0, dt_id=-1, sigma_pix=1.5, **kw):
        self.pkg, self.sc, self.cams, self.dt, self.dt_id, self.sigma, self.kw = pkg, sc, cams, dt, dt_id, sigma_pix, kw
        self.views = [self.view(c.K8, c) for c in cams]
        self.side = pkg.CameraSide(cams[1].R, cams[1].p, cams[1].K8, cams[1].model, cams[1].ext_id, cams[1].int_id)

    def view(self, K8, c):
        sc = self.sc
        return self.pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], c.R, c.p, K8, clone_R_fej=sc["Rf"], clone_p_fej=sc["pf"], cam_dt=self.dt,
                                  extrinsic_state_id=c.ext_id, intrinsic_state_id=c.int_id, dt_state_id=self.dt_id, sigma_pix=self.sigma, **self.kw)


def distort_px(K8, model, un):
    """CamBase::distort_d: normalised (double) -> pixel, through float both ways; the radtan expressions in the kernels' order"""
    if model == EQUI:
        return cam_equi.distort(K8, np.asarray(un, float).reshape(1, 2))[0].astype(np.float64)
    K = [float(v) for v in K8]
    x, y = float(np.float32(un[0])), float(np.float32(un[1]))
    r = float(np.sqrt(x * x + y * y))
    r_2 = r * r
    r_4 = r_2 * r_2
    x1 = x * (1 + K[4] * r_2 + K[5] * r_4) + 2 * K[6] * x * y + K[7] * (r_2 + 2 * x * x)
    y1 = y * (1 + K[4] * r_2 + K[5] * r_4) + K[6] * (r_2 + 2 * y * y) + 2 * K[7] * x * y
    return np.array([float(np.float32(K[0] * x1 + K[2])), float(np.float32(K[1] * y1 + K[3]))])


def flatten(feats):
    """feats: list of {cam: (t, uv, uvn[, res_R, res_p])} -> obs_ptr, t, uv, uvn, cam, res_R, res_p in the reference's order"""
    ptr, t, uv, uvn, cam, rR, rp = [0], [], [], [], [], [], []
    for ft in feats:
        for c in (1, 0):
            if c not in ft or len(ft[c][0]) == 0:
                continue
            o = ft[c]
            t += list(o[0]); uv += list(np.asarray(o[1], np.float32).reshape(-1, 2)); uvn += list(np.asarray(o[2], np.float32).reshape(-1, 2))
            cam += [c] * len(o[0])
            if len(o) > 3:
                rR += list(np.asarray(o[3]).reshape(-1, 9)); rp += list(np.asarray(o[4]).reshape(-1, 3))
        ptr.append(len(t))
    f32 = lambda a: np.array(a, np.float32).reshape(-1, 2)
    return dict(ptr=np.array(ptr, np.int32), t=np.array(t, float), uv=f32(uv), uvn=f32(uvn), cam=np.array(cam, np.uint8),
                res_R=np.array(rR).reshape(-1, 9) if rR else None, res_p=np.array(rp).reshape(-1, 3) if rp else None)


def stereo_tracks(pkg, fl, p):
    return pkg.StereoTracks(fl["ptr"], fl["t"], fl["uv"], fl["cam"], p, obs_uvn=fl["uvn"], res_R=fl["res_R"], res_p=fl["res_p"])


def imu_pose(jo, pair, t, res=None):
    """(R_GtoI, p_IinG) of an observation at time t, None without bounding clones"""
    it = jo.interpolate(pair.views[0], t + pair.dt, fej=False)
    if it is None:
        return None
    return (np.asarray(res[0]).reshape(3, 3), np.asarray(res[1])) if res is not None else (it[0], it[1])


def cam_pose(cam, R_GtoI, p_IinG):
    R_GtoC = cam.R @ R_GtoI
    return R_GtoC, p_IinG - R_GtoC.T @ cam.p


def usable(jo, pair, ft):
    """per camera the indices of the observations with bounding clones"""
    return {c: [i for i in range(len(ft[c][0])) if imu_pose(jo, pair, ft[c][0][i]) is not None] if c in ft else [] for c in (0, 1)}


def triangulate(jo, pair, ft, tri=TRI):
    """one feature: (ok, p_FinG, camera-averaged error, per-observation mean error, anchor camera, usable counts)"""
    use = usable(jo, pair, ft)
    n0, n1 = len(use[0]), len(use[1])
    anchor = 0 if n0 > n1 else 1
    Rc, pc, uvn, meta = [], [], [], []
    for c in ((0, 1) if anchor == 1 else (1, 0)):
        for i in use[c]:
            o = ft[c]
            R, p = imu_pose(jo, pair, o[0][i], (o[3][i], o[4][i]) if len(o) > 3 else None)
            Rg, pg = cam_pose(pair.cams[c], R, p)
            Rc.append(Rg); pc.append(pg); uvn.append(o[2][i]); meta.append((c, np.asarray(o[1][i], np.float32)))
    if n0 + n1 < 2:
        return False, np.zeros(3), 0.0, 0.0, anchor, (n0, n1)
    ok, p = jo.triangulate(np.array(Rc), np.array(pc), np.array(uvn, np.float32), min_dist=tri["min_dist"], max_dist=tri["max_dist"],
                           max_cond=tri["max_cond"], max_baseline=tri["max_baseline"])
    if not ok:
        return False, np.zeros(3), 0.0, 0.0, anchor, (n0, n1)
    e = {0: [], 1: []}
    for (c, uv), Rg, pg in zip(meta, Rc, pc):
        pC = Rg @ (p - pg)
        d = distort_px(pair.cams[c].K8, pair.cams[c].model, pC[:2] / pC[2])
        r0, r1 = float(uv[0]) - d[0], float(uv[1]) - d[1]
        e[c].append(np.sqrt(r0 * r0 + r1 * r1))
    per_cam = []
    for c in (1, 0):
        if e[c]:
            s = 0.0
            for v in e[c]:
                s += v
            per_cam.append(s / len(e[c]))
    avg = 0.0
    for v in per_cam:
        avg += v
    return True, p, avg / len(per_cam), float(np.mean(e[0] + e[1])), anchor, (n0, n1)


def triangulate_batch(jo, pair, feats, tri=TRI):
    out = [triangulate(jo, pair, ft, tri) for ft in feats]
    return (np.array([o[1] for o in out]), np.array([o[0] for o in out], np.uint8), np.array([o[2] for o in out]), np.array([o[3] for o in out]),
            [o[4] for o in out], [o[5] for o in out])


def columns(jo, pair, feats):
    """joint column order: [ext0][int0][dt][ext1][int1] (each when estimated), then the clones in first-seen order over the batch"""
    fl = flatten(feats)
    tr = pair.pkg.Tracks(fl["ptr"], fl["t"], fl["uv"], np.zeros((len(feats), 3)))
    c0 = list(jo.columns(pair.views[0], tr))
    head = (6 if pair.cams[0].ext_id >= 0 else 0) + (8 if pair.cams[0].int_id >= 0 else 0) + (1 if pair.dt_id >= 0 else 0)
    extra = []
    if pair.cams[1].ext_id >= 0:
        extra += list(range(pair.cams[1].ext_id, pair.cams[1].ext_id + 6))
    if pair.cams[1].int_id >= 0:
        extra += list(range(pair.cams[1].int_id, pair.cams[1].int_id + 8))
    return np.array(c0[:head] + extra + c0[head:], np.int32)


def _camera_rows(jo, pair, c, feats, p, ld):
    """(rows [F], cols, Hf, Hx, res) of camera c's observations of every feature, from the oracle with camera c's view"""
    cam = pair.cams[c]
    one = [{c: ft[c]} if c in ft else {} for ft in feats]
    fl = flatten(one)
    F = len(feats)
    if len(fl["t"]) == 0:
        return np.zeros(F, np.int32), np.zeros(0, np.int32), np.zeros((F, 3, ld)), np.zeros((F, 0, ld)), np.zeros((F, ld))
    K0 = np.concatenate([cam.K8[:4], np.zeros(4)])
    view = pair.views[c] if cam.model == RADTAN else pair.view(K0, cam)
    tr = pair.pkg.Tracks(fl["ptr"], fl["t"], fl["uv"], p, res_R=fl["res_R"], res_p=fl["res_p"])
    cols = jo.columns(view, tr)
    rows, Hf, Hx, res = jo.build_jacobians(view, tr, cols, ld)
    if cam.model == RADTAN:
        return rows, cols, Hf, Hx, res
    assert not pair.kw.get("use_pol_cov", 0), "the equidistant restatement needs isotropic noise"
    intr = [j for j, s in enumerate(cols) if cam.int_id >= 0 and cam.int_id <= s < cam.int_id + 8]
    other = [j for j in range(len(cols)) if j not in intr]
    S = np.diag([1 / cam.K8[0], 1 / cam.K8[1]])
    for f, ft in enumerate(one):
        k = 0
        for i in range(len(ft[c][0]) if c in ft else 0):
            o = ft[c]
            pose = imu_pose(jo, pair, o[0][i], (o[3][i], o[4][i]) if len(o) > 3 else None)
            if pose is None:
                continue
            Rg, pg = cam_pose(cam, *pose)
            pC = Rg @ (p[f] - pg)
            un = pC[:2] / pC[2]
            dzn, dzeta = cam_equi.distort_jacobian(cam.K8, un.reshape(1, 2))
            A = dzn[0] @ S
            r = slice(2 * k, 2 * k + 2)
            Hf[f][:, r] = (A @ Hf[f][:, r].T).T
            blk = Hx[f][:, r].T.copy()
            new = np.zeros_like(blk)
            new[:, other] = A @ blk[:, other]
            if intr:
                new[:, intr] = dzeta[0] / pair.sigma
            Hx[f][:, r] = new.T
            d = cam_equi.distort(cam.K8, un.reshape(1, 2))[0].astype(np.float64)
            res[f][r] = (np.asarray(o[1][i], np.float32).astype(np.float64) - d) / pair.sigma
            k += 1
        assert 2 * k == rows[f]
    return rows, cols, Hf, Hx, res


def build_jacobians(jo, pair, feats, p, cols, ld):
    """the joint systems in the layout of plv_build_jacobians: rows [F], Hf [F][3][ld], Hx [F][k][ld], res [F][ld]"""
    F, k = len(feats), len(cols)
    at = {int(s): j for j, s in enumerate(cols)}
    rows, Hf, Hx, res = np.zeros(F, np.int32), np.zeros((F, 3, ld)), np.zeros((F, k, ld)), np.zeros((F, ld))
    per = {c: _camera_rows(jo, pair, c, feats, np.asarray(p, float).reshape(-1, 3), ld) for c in (1, 0)}
    for f in range(F):
        base = 0
        for c in (1, 0):
            r_c, cols_c, Hf_c, Hx_c, res_c = per[c]
            m = int(r_c[f])
            keep = min(m, max(0, ld - base))          # (rows past ld are not written, as by the kernel)
            Hf[f][:, base:base + keep] = Hf_c[f][:, :keep]
            res[f][base:base + keep] = res_c[f][:keep]
            for j, s in enumerate(cols_c):
                Hx[f][at[int(s)], base:base + keep] = Hx_c[f][j, :keep]
            base += m
        rows[f] = base
    return rows, Hf, Hx, res


def by_state(cols, Hx, n):
    """Hx [F][k][ld] scattered to state indices [F][n][ld]: the comparison that does not depend on the column order"""
    out = np.zeros((Hx.shape[0], n, Hx.shape[2]))
    out[:, np.asarray(cols, int), :] = Hx
    return out


def update_points(jo, oracle, pair, tracks, P, max_msckf, max_obs, t_prev_frame, state_time, window_full=True, tri=TRI, dt_exp=0.01):
    """tracks: {id: {cam: (t, uv, uvn)}}.  Returns the decisions, dx, P and the database afterwards ({id: {cam: (t, uv, uvn)}})."""
    t = pair.sc["t"]
    dt, t_oldest, t_oldest2 = pair.dt, t[0], t[1]
    db = {fid: {c: tuple(np.array(a) for a in ft[c]) for c in ft if len(ft[c][0])} for fid, ft in tracks.items()}
    unused = {}

    def back(fid, c, o, idx):
        if len(idx) == 0:
            return
        u = unused.setdefault(fid, {}).setdefault(c, [np.zeros(0), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)])
        for q in range(3):
            u[q] = np.concatenate([u[q], np.asarray(o[q])[idx]])

    times = lambda ft: np.concatenate([ft[c][0] for c in ft])
    pool = [fid for fid in sorted(db) if (times(db[fid]) < t_oldest2 - dt).any() or not (times(db[fid]) > t_prev_frame - dt).any()]
    n_pool = len(pool)
    cand = {}
    for fid in pool:
        ft = db.pop(fid)
        kept = {}
        for c in ft:
            tm = ft[c][0] + dt
            new, old = tm > state_time + dt_exp, tm < t_oldest - dt_exp
            back(fid, c, ft[c], np.flatnonzero(new))
            m = ~(new | old)
            if m.any():
                kept[c] = tuple(a[m] for a in ft[c])
        if sum(len(kept[c][0]) for c in kept) >= 2:
            cand[fid] = kept
    order = sorted(cand, key=lambda fid: (-sum(len(cand[fid][c][0]) for c in cand[fid]), fid))
    feats = [cand[fid] for fid in order]
    trace = dict(order=order, n_valid={}, ok={}, err={}, err_obs={}, anchor={})
    sel, p_sel = [], []
    for fid, ft in zip(order, feats):
        whole = lambda: [back(fid, c, ft[c], np.arange(len(ft[c][0]))) for c in ft]
        if len(sel) >= max_msckf:
            whole()
            continue
        ok, p, err, err_obs, anchor, (n0, n1) = triangulate(jo, pair, ft, tri)
        trace["n_valid"][fid], trace["ok"][fid], trace["err"][fid], trace["err_obs"][fid], trace["anchor"][fid] = (n0, n1), ok, err, err_obs, anchor
        if n0 + n1 < 2 or not ok or not err < 3.0:
            whole()
            continue
        assert n0 + n1 <= max_obs
        sel.append(fid)
        p_sel.append(p)
    out = dict(n_pool=n_pool, ids=np.array(sel, np.uint64), trace=trace, p_FinG=np.array(p_sel).reshape(-1, 3), dx=np.zeros(len(P)), P=P.copy(),
               accepted=np.zeros(0, np.uint8), n_rows=0, status=0)
    if sel:
        chosen = []
        for fid in sel:
            use = usable(jo, pair, cand[fid])
            for c in cand[fid]:
                back(fid, c, cand[fid][c], np.array([i for i in range(len(cand[fid][c][0])) if i not in use[c]], int))
            chosen.append({c: tuple(a[use[c]] for a in cand[fid][c]) for c in cand[fid] if use[c]})
        cols = columns(jo, pair, chosen)
        rows, Hf, Hx, res = build_jacobians(jo, pair, chosen, out["p_FinG"], cols, 2 * max_obs)
        rc, P_o, dx_o, acc, nrows = oracle.msckf_update(P, rows, Hf, Hx, res, cols, pair.sigma ** 2, synth.q95_table())
        out.update(status=rc, P=P_o, dx=dx_o, accepted=acc, n_rows=nrows, cols=cols)
        for fid, ft, a in zip(sel, chosen, acc):
            if not a:
                for c in ft:
                    back(fid, c, ft[c], np.arange(len(ft[c][0])))
    for fid, u in unused.items():
        for c, o in u.items():
            old = db.setdefault(fid, {}).get(c)
            db[fid][c] = tuple(o) if old is None else tuple(np.concatenate([old[q], o[q]]) for q in range(3))
    if window_full:
        for fid in list(db):
            for c in list(db[fid]):
                m = ~(db[fid][c][0] < t_oldest)
                db[fid][c] = tuple(a[m] for a in db[fid][c])
                if not m.any():
                    del db[fid][c]
            if not db[fid]:
                del db[fid]
    out["db"] = db
    return out


# ------------------------------------------------------------------ the test scene
def _small_rot(w):
    return synth._exp_so3(np.array(w, float))


def stereo_scene(pkg, undistort, model1=RADTAN, calib="all", dt=0.0, seed=31, F=40, noise_px=0.4, scene_kw=None, model0=RADTAN, **kw):
    """synth.vio_scene (15 clones, F features) seen by a pair: camera 1 has a 0.1 m baseline, a slightly rotated R_ItoC and its own
    intrinsics (radtan, or equidistant).  Camera 0 is the scene's camera; with model0 equidistant it keeps the scene's fx fy cx cy,
    carries EQUI0_COEFFS and its observations are rendered through cam_equi.distort, as camera 1's are.  State layout: IMU 15 | int0 8 | clones | ext0 6 | dt 1 | ext1 6 | int1 8.
    calib: "all", "cam0" (camera 1's blocks off), "cam1" (camera 0's off), "none"; returns (sc, pair, obs) with
    obs[f] = {cam: (t, uv, uvn)} holding every clone-time observation of feature f in both cameras (noise_px each)."""
    sc = synth.vio_scene(F=F, M=15, noise_px=noise_px, seed=seed, **(scene_kw or {}))
    n0 = sc["n_state"]
    sc["n_state"] = n0 + 21
    on0, on1 = calib in ("all", "cam0"), calib in ("all", "cam1")
    K1 = MILD_EQUI.copy() if model1 == EQUI else sc["K8"] * np.array([1.01, 0.99, 1.02, 0.97, 0.9, 1.1, -1.0, 0.8])
    K0 = np.concatenate([sc["K8"][:4], EQUI0_COEFFS]) if model0 == EQUI else sc["K8"]
    cams = [Cam(sc["R_ItoC"], sc["p_IinC"], K0, model0, n0 if on0 else -1, sc["intr_id"] if on0 else -1),
            Cam(_small_rot([0.004, 0.012, -0.006]) @ sc["R_ItoC"], sc["p_IinC"] + np.array([-0.1, 0.002, 0.001]), K1, model1,
                n0 + 7 if on1 else -1, n0 + 13 if on1 else -1)]
    pair = Pair(pkg, sc, cams, dt=dt, dt_id=n0 + 6 if calib != "none" else -1, **kw)
    rng = np.random.default_rng(seed + 1)
    rng0 = np.random.default_rng(seed + 2)  # (camera 0's pixel noise when it is rendered here: camera 1's draws stay what they were)
    obs = []
    for f in range(F):
        a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
        tt = sc["obs_time"][a:b].copy()
        if model0 == EQUI:
            un0 = []
            for tm in tt:
                R, p = sc["pose_fn"](tm)
                pc = cams[0].R @ (R @ (sc["pts"][f] - p)) + cams[0].p
                un0.append(pc[:2] / pc[2])
            uv0 = (cam_equi.distort(K0, np.array(un0)) + rng0.normal(0, noise_px, (len(tt), 2))).astype(np.float32)
            ft = {0: (tt - dt, uv0, cam_equi.undistort(K0, uv0))}
        else:
            ft = {0: (tt - dt, sc["obs_uv"][a:b].astype(np.float32), undistort(sc["K8"], sc["obs_uv"][a:b].astype(np.float32)))}
        uv1 = []
        for tm in tt:
            R, p = sc["pose_fn"](tm)
            pc = cams[1].R @ (R @ (sc["pts"][f] - p)) + cams[1].p
            un = pc[:2] / pc[2]
            d = cam_equi.distort(K1, un.reshape(1, 2))[0] if model1 == EQUI else synth.radtan_distort(K1, un)
            uv1.append(d + rng.normal(0, noise_px, 2))
        uv1 = np.array(uv1, np.float32)
        ft[1] = (tt - dt, uv1, cam_equi.undistort(K1, uv1) if model1 == EQUI else undistort(K1, uv1))
        obs.append(ft)
    return sc, pair, obs


def cut(ft, keep0=None, keep1=None):
    """a feature with the observations keep0 / keep1 (index arrays or slices; None: all, (): none) of its two cameras"""
    out = {}
    for c, keep in ((0, keep0), (1, keep1)):
        if keep is None:
            out[c] = ft[c]
        elif not isinstance(keep, slice) and len(keep) == 0:
            continue
        else:
            out[c] = tuple(a[keep].copy() for a in ft[c])
    return out


def with_noise(ft, undistort, pair, sig0, sig1, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for c, s in ((0, sig0), (1, sig1)):
        if c not in ft:
            continue
        uv = (ft[c][1] + rng.normal(0, s, ft[c][1].shape)).astype(np.float32) if s else ft[c][1]
        cam = pair.cams[c]
        out[c] = (ft[c][0], uv, cam_equi.undistort(cam.K8, uv) if cam.model == EQUI else undistort(cam.K8, uv))
    return out


PAIRINGS = {"radtan-radtan": (RADTAN, RADTAN), "radtan-equidistant": (RADTAN, EQUI), "equidistant-radtan": (EQUI, RADTAN),
            "equidistant-equidistant": (EQUI, EQUI)}  # (model0, model1) by the names the tests give their cases


def read_as_radtan(pair):
    """the pair with camera 0 read as radtan on the same eight numbers (what a launch that took the wrong model for it computes)"""
    c0 = pair.cams[0]
    return Pair(pair.pkg, pair.sc, [Cam(c0.R, c0.p, c0.K8, RADTAN, c0.ext_id, c0.int_id), pair.cams[1]], dt=pair.dt, dt_id=pair.dt_id,
                sigma_pix=pair.sigma, **pair.kw)


def update_scene(pkg, undistort, model1=RADTAN, **kw):
    """The database of the update tests: {id: {cam: (t, uv, uvn)}} reaching every branch of the selection (see
    tests/test_stereo_update_ref_cpu.py, which asserts them), with the pair and the options of the call.  model0 (stereo_scene):
    camera 0's model."""
    sc, pair, obs = stereo_scene(pkg, undistort, model1=model1, **kw)
    t = sc["t"]
    full = [f for f in range(len(obs)) if len(obs[f][0][0]) == 15]
    short = [f for f in range(len(obs)) if len(obs[f][0][0]) < 14]
    assert len(full) >= 28 and len(short) >= 2
    tracks = {}
    it = iter(full)
    nxt = lambda: next(it)
    names = {}
    for _ in range(3):
        f = nxt(); tracks[f + 1] = cut(obs[f], None, ()); names.setdefault("cam0 only", []).append(f + 1)
    for _ in range(3):
        f = nxt(); tracks[f + 1] = cut(obs[f], (), None); names.setdefault("cam1 only", []).append(f + 1)
    for _ in range(3):
        f = nxt(); tracks[f + 1] = cut(obs[f], None, slice(4, 15)); names.setdefault("majority 0", []).append(f + 1)
    for _ in range(3):
        f = nxt(); tracks[f + 1] = cut(obs[f], slice(0, 10), None); names.setdefault("majority 1", []).append(f + 1)
    # one observation without bounding clones (behind the newest clone, inside the extrapolation allowance) in camera 1 only
    f = nxt()
    ft = obs[f]
    late = tuple(np.concatenate([a, a[-1:]]) for a in ft[1])
    late[0][-1] = t[-1] + 0.005 - pair.dt
    tracks[f + 1] = {0: ft[0], 1: late}
    names["late in cam1"] = f + 1
    # ... and a feature that such an observation leaves with a single usable one
    f = nxt()
    one = cut(obs[f], slice(0, 1), None)            # (sixteen observations: it is reached before the cap)
    one[1][0][:] = t[-1] + 0.0005 * (1 + np.arange(15)) - pair.dt
    tracks[f + 1] = one
    names["one usable"] = f + 1
    # camera 0: 15 poor observations, camera 1: 3 good ones — the mean over the cameras passes where the mean over the observations fails
    f = nxt()
    tracks[f + 1] = with_noise(cut(obs[f], None, slice(0, 15, 7)), undistort, pair, 3.3, 0.0, 5)
    names["camera-averaged"] = f + 1
    # a biased track: triangulates, fails the 3 px test in both cameras
    f = nxt()
    tracks[f + 1] = with_noise(obs[f], undistort, pair, 9.0, 9.0, 6)
    names["biased"] = f + 1
    # a noisy track that passes the 3 px test and meets the gate
    f = nxt()
    tracks[f + 1] = with_noise(obs[f], undistort, pair, 2.0, 2.0, 7)
    names["gate"] = f + 1
    # the rest: six full tracks, then short ones that sort behind the one-camera tracks (so that the cap falls among those)
    for q, f in enumerate(it):
        tracks[f + 1] = obs[f] if q < 6 else cut(obs[f], slice(8, 15), slice(8, 15))
    # still tracked, nothing old: never leaves the database
    for f in short:
        tracks[f + 1] = cut(obs[f], slice(-3, None), slice(-3, None))
    names["tracked"] = [f + 1 for f in short]
    opt = dict(max_msckf=20, max_obs=31, t_prev_frame=float(t[-2]), state_time=float(t[-1]), window_full=True)
    return sc, pair, tracks, names, opt


def db_equal(a, b):
    """two databases {id: {cam: (t, uv, uvn)}} hold the same observations per camera (in any order within a camera)"""
    if set(a) != set(b):
        return False
    for fid in a:
        for c in (0, 1):
            x, y = a[fid].get(c), b[fid].get(c)
            nx, ny = (0 if x is None else len(x[0])), (0 if y is None else len(y[0]))
            if nx != ny:
                return False
            if nx:
                ix, iy = np.argsort(x[0], kind="stable"), np.argsort(y[0], kind="stable")
                if not all(np.array_equal(np.asarray(x[q])[ix], np.asarray(y[q])[iy]) for q in range(3)):
                    return False
    return True


def with_res_poses(sc, feats, seed=2, noise=1e-3):
    """the features with an IMU pose for the residual at every observation (plv_tracks::res_R / res_p): the true pose, perturbed"""
    rng = np.random.default_rng(seed)
    out = []
    for ft in feats:
        g = {}
        for c in ft:
            R = np.array([(synth._exp_so3(rng.normal(0, noise, 3)) @ sc["pose_fn"](tm)[0]).ravel() for tm in ft[c][0]])
            p = np.array([sc["pose_fn"](tm)[1] + rng.normal(0, noise, 3) for tm in ft[c][0]])
            g[c] = (ft[c][0], ft[c][1], ft[c][2], R, p)
        out.append(g)
    return out


def long_feature(sc, pair, undistort, point, n1, n0, seed=3, noise_px=0.3):
    """one landmark observed n1 times by camera 1 and n0 times by camera 0, at distinct times inside the window"""
    rng = np.random.default_rng(seed)
    t = sc["t"]
    ft = {}
    for c, n in ((1, n1), (0, n0)):
        cam = pair.cams[c]
        tt = np.linspace(t[0] + 0.003, t[-1] - 0.003, n) + (0.0007 if c else 0.0) - pair.dt
        uv = []
        for tm in tt:
            R, p = sc["pose_fn"](tm + pair.dt)
            pc = cam.R @ (R @ (point - p)) + cam.p
            un = pc[:2] / pc[2]
            d = cam_equi.distort(cam.K8, un.reshape(1, 2))[0] if cam.model == EQUI else synth.radtan_distort(cam.K8, un)
            uv.append(d + rng.normal(0, noise_px, 2))
        uv = np.array(uv, np.float32)
        ft[c] = (tt, uv, cam_equi.undistort(cam.K8, uv) if cam.model == EQUI else undistort(cam.K8, uv))
    return ft


def advance(pkg, sc, pair, undistort, db, noise_px=0.4, seed=8):
    """one frame later: the window moves by one clone; every feature of db observed at the newest clone is observed again, in the
    cameras that saw it.  Returns (sc2, pair2, {id: {cam: (t, uv, uvn)}} of the new frame's observations)."""
    rng = np.random.default_rng(seed)
    t = sc["t"]
    sc2 = dict(sc)
    sc2["t"] = np.concatenate([t[1:], [t[-1] + (t[-1] - t[-2])]])
    poses = [sc["pose_fn"](ti) for ti in sc2["t"]]
    sc2["R"] = np.array([R for R, _ in poses]); sc2["p"] = np.array([p for _, p in poses])
    sc2["Rf"], sc2["pf"] = sc2["R"].copy(), sc2["p"].copy()
    pair2 = Pair(pkg, sc2, pair.cams, dt=pair.dt, dt_id=pair.dt_id, sigma_pix=pair.sigma, **pair.kw)
    tn = sc2["t"][-1]
    R, p = poses[-1]
    new = {}
    for fid, ft in db.items():
        for c in ft:
            if len(ft[c][0]) and (ft[c][0] + pair.dt == t[-1]).any():
                cam = pair.cams[c]
                pc = cam.R @ (R @ (sc["pts"][fid - 1] - p)) + cam.p
                un = pc[:2] / pc[2]
                d = cam_equi.distort(cam.K8, un.reshape(1, 2))[0] if cam.model == EQUI else synth.radtan_distort(cam.K8, un)
                uv = np.array([d + rng.normal(0, noise_px, 2)], np.float32)
                new.setdefault(fid, {})[c] = (np.array([tn - pair.dt]), uv, cam_equi.undistort(cam.K8, uv) if cam.model == EQUI else undistort(cam.K8, uv))
    return sc2, pair2, new


def db_append(db, new):
    out = {fid: dict(ft) for fid, ft in db.items()}
    for fid, ft in new.items():
        for c, o in ft.items():
            old = out.setdefault(fid, {}).get(c)
            out[fid][c] = tuple(np.asarray(a) for a in o) if old is None else tuple(np.concatenate([old[q], o[q]]) for q in range(3))
    return out
