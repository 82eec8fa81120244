"""A CPU stand-in for the stereo driver: oracle_context.PyMirrorContext with the calls pl-viwo_amd/system.py makes for a stereo pair.
tracker_feed_stereo is stereo_ref.StereoRef (TrackKLT::feed_stereo restated on the oracle's primitives), stereo_try_update is
stereo_cpi_ref.update_points (the point half over both cameras, with the CPI table under use_imu_res, and the point_used fill)
followed by the mirror's own line half on camera 0: the lines are fed from camera 0's equalised image and camera 0's points, the pool
is formed and triangulated before the point dx is applied, the line update runs on the updated state.  Test infrastructure.
Under use_imu_res the line half takes the CPI table as the library's does (plv_update_options::cpi): an observation the table
cannot serve leaves its line for the database behind the sort, the lines are triangulated on the table's poses formed on the state of
camera_get_line_features, the rows on those formed on the updated state (tests/test_gpu_imu_res_route.py holds the library's line
update to this composition)."""
import numpy as np

import stereo_cpi_ref as scr
import stereo_ref
import stereo_update_ref as sr
from oracle_context import PyMirrorContext


class _Pair:
    """what stereo_update_ref reads of a sr.Pair, built from the driver's state view and camera side"""

    def __init__(self, pkg, st, right):
        m = int(st.c.n_clones)
        c0, c1 = st.c, right.c
        self.pkg, self.sc = pkg, dict(t=np.array(st.t[:m], dtype=np.float64))
        self.dt, self.dt_id, self.sigma = float(c0.cam_dt), int(c0.dt_state_id), float(c0.sigma_pix)
        self.kw = dict(use_pol_cov=int(c0.use_pol_cov))
        arr = lambda a, shape: np.array(a, dtype=np.float64).reshape(shape)
        self.cams = [sr.Cam(arr(c0.R_ItoC, (3, 3)), arr(c0.p_IinC, 3), arr(c0.intrinsics, 8), sr.RADTAN, int(c0.extrinsic_state_id), int(c0.intrinsic_state_id)),
                     sr.Cam(arr(c1.R_ItoC, (3, 3)), arr(c1.p_IinC, 3), arr(c1.intrinsics, 8), int(c1.model), int(c1.extrinsic_state_id), int(c1.intrinsic_state_id))]
        view = lambda cam: pkg.StateView(st.t[:m], st.R[:m], st.p[:m], st.ids[:m], cam.R, cam.p, cam.K8, clone_R_fej=st.Rf[:m], clone_p_fej=st.pf[:m],
                                         cam_dt=self.dt, extrinsic_state_id=cam.ext_id, intrinsic_state_id=cam.int_id, dt_state_id=self.dt_id,
                                         sigma_pix=self.sigma, use_pol_cov=int(c0.use_pol_cov), intr_ori_cov=float(c0.intr_ori_cov),
                                         intr_pos_cov=float(c0.intr_pos_cov), feat_rep=int(c0.feat_rep), dt_exp=float(c0.dt_exp),
                                         intr_err_mlt=float(c0.intr_err_mlt))
        self.views = [view(self.cams[0]), view(self.cams[1])]


class StereoMirrorContext(PyMirrorContext):
    CAMERA_MODELS = ("radtan",)      # (the oracle's front end undistorts with the radtan model only)

    def __init__(self, cfg):
        PyMirrorContext.__init__(self, cfg)
        self.sref = None

    # ---- the stereo tracker
    def stereo_configure(self, K8_right, model_right=0):
        assert int(model_right) == 0
        c = self.cfg
        self.sref = stereo_ref.StereoRef(stereo_ref.Settings(c.num_features, c.grid_x, c.grid_y, c.min_px_dist, c.fast_threshold), self.K8, K8_right)

    def set_camera_intrinsics(self, K8):
        PyMirrorContext.set_camera_intrinsics(self, K8)
        if self.sref is not None:
            self.sref.K8 = (self.K8.copy(), self.sref.K8[1])

    def stereo_set_intrinsics(self, cam, K8):
        if cam == 0:
            return self.set_camera_intrinsics(K8)
        self.sref.K8 = (self.sref.K8[0], np.array(K8, dtype=np.float64))

    def tracker_feed_stereo(self, t, left, right, encoding="mono8", mask_left=None, mask_right=None):
        if encoding != "mono8":      # (the library converts on the device; its host yardstick is the dataset reader's)
            assert encoding == "bayer_rggb8", encoding
            import importlib
            kaist = importlib.import_module(self.pkg.__name__ + ".kaist")
            left, right = kaist.bayer_rg_to_grey(left), kaist.bayer_rg_to_grey(right)
        self.sref.feed(t, left, right, mask_left, mask_right)
        # what the line half reads: camera 0's equalised image and camera 0's points (TrackLSD::feed_monocular on image 0)
        self.pts, self.ids, self.prev = self.sref.pts[0], self.sref.ids[0], (self.sref.prev[0][0], None)

    def stereo_last(self, cam):
        return self.sref.pts[cam].copy(), self.sref.ids[cam].copy()

    def stereo_db_cleanup_measurements(self, t):
        for fid in list(self.sref.db):
            kept = tuple([o for o in obs if not o[0] < t] for obs in self.sref.db[fid])
            if kept[0] or kept[1]:
                self.sref.db[fid] = kept
            else:
                del self.sref.db[fid]

    def _tracks(self):
        out = {}
        for fid, obs in self.sref.db.items():
            ft = {}
            for cam in (0, 1):
                if obs[cam]:
                    a = np.array(obs[cam], dtype=np.float64)
                    ft[cam] = (a[:, 0].copy(), np.array([o[1:3] for o in obs[cam]], np.float32), np.array([o[3:5] for o in obs[cam]], np.float32))
            if ft:
                out[fid] = ft
        return out

    # ---- UpdaterCamera::try_update for the pair
    def stereo_try_update(self, st, right, plus, n, max_msckf, max_obs, t_prev_frame, state_time, window_full=True, chi2_mult=1.0, min_dist=0.1,
                          max_dist=60.0, max_cond=1e4, max_baseline=40.0, refine=True, init_min_meas=10, lines=True, cap=512, cpi=None):
        assert chi2_mult == 1.0 and refine
        pair = _Pair(self.pkg, st, right)
        cp = dict(t=cpi.t, clone_t=cpi.clone_t) if cpi is not None else None
        ref = scr.update_points(self.jo, self.o, pair, self._tracks(), self.P, cp, cpi, max_msckf, max_obs, t_prev_frame, state_time, bool(window_full),
                                tri=dict(max_cond=max_cond, max_dist=max_dist, max_baseline=max_baseline, min_dist=min_dist), dt_exp=float(st.c.dt_exp))
        self.sref.db = {fid: tuple([(float(o[0][i]), o[1][i][0], o[1][i][1], o[2][i][0], o[2][i][1]) for i in range(len(o[0]))] if o is not None else []
                                   for o in (ft.get(0), ft.get(1))) for fid, ft in ref["db"].items()}
        self.mir.used.update(ref["used"])
        acc = np.array(ref["accepted"], dtype=np.uint8)
        if ref["status"] == 0:
            self.P = np.array(ref["P"], order="F")
        out = dict(dx=ref["dx"], n_pool=ref["n_pool"], n_msckf=len(ref["ids"]), n_accepted=int(acc.sum()), n_rows=int(ref["n_rows"]), status=int(ref["status"]),
                   ids=ref["ids"], accepted=acc, p_FinG=ref["p_FinG"], n_slam=0, n_init=0)
        kw = dict(t_prev_frame=t_prev_frame, state_time=state_time, window_full=window_full, chi2_mult=chi2_mult)
        if lines:      # the pool is formed and triangulated on the state before the point dx is applied (UpdaterCamera.cpp:148-152)
            self.camera_get_line_features(st, n, max_obs, cpi=cpi, **kw)

        def apply(r):
            if r["status"] != 0 or r["n_accepted"] < 1 or plus is None:
                return
            plus.apply(np.ascontiguousarray(r["dx"], dtype=np.float64))
            if st.c.intrinsic_state_id >= 0:
                self.set_camera_intrinsics(np.array(st.c.intrinsics))
            if right.c.intrinsic_state_id >= 0:
                self.stereo_set_intrinsics(1, np.array(right.c.intrinsics))

        apply(out)
        if not lines:
            return out, None, 0
        n_db = self.line_db_size()
        lo = self.camera_update_lines(st, n, max_obs, cap=cap, cpi=cpi, **kw)
        apply(lo)
        return out, lo, n_db

    # ---- the mirror's line half with a CPI table: PyMirrorContext's two methods, the table's hand-back and poses added
    def camera_get_line_features(self, st, n, max_obs, t_prev_frame, state_time, window_full=True, chi2_mult=1.0, cpi=None):
        if cpi is None:
            return PyMirrorContext.camera_get_line_features(self, st, n, max_obs, t_prev_frame, state_time, window_full, chi2_mult)
        pkg, mir = self.pkg, self.mir
        ct = [float(x) for x in st.t]
        dt = float(st.c.cam_dt)
        t_oldest, t_oldest2 = ct[0], ct[1]
        unused = {}

        def give(lid, e, i):
            u = unused.get(lid)
            if u is None:
                u = unused[lid] = dict(t=[], uv=[], uvn=[], points=list(e["points"]), D=e["D"])
            u["t"].append(e["t"][i]), u["uv"].append(e["uv"][i]), u["uvn"].append(e["uvn"][i])

        take = sorted(k for k, e in self.ldb.items() if any(t < t_oldest2 - dt for t in e["t"]) or not any(t > t_prev_frame - dt for t in e["t"]))
        pool = [(k, self.ldb.pop(k)) for k in take]
        kept = []
        for lid, e in pool:
            keep = []
            for i, t in enumerate(e["t"]):
                tm = t + dt
                if tm > state_time + 0.01:
                    give(lid, e, i)
                elif tm < t_oldest - 0.01:
                    continue
                else:
                    keep.append(i)
            if len(keep) >= 2:
                kept.append((lid, dict(t=[e["t"][i] for i in keep], uv=[e["uv"][i] for i in keep], uvn=[e["uvn"][i] for i in keep],
                                       points=e["points"], D=e["D"])))
        kept.sort(key=lambda x: -len(x[1]["t"]))     # stable
        # get_imu_poses with the table (cpi_attach behind the sort): what it cannot serve goes back; a line left with fewer than two
        # observations cannot be triangulated and goes back whole (the update's `valid < 2`)
        cp, ct_arr = dict(t=cpi.t, clone_t=cpi.clone_t), np.array(ct)
        served = []
        for lid, e in kept:
            ok = [scr.servable(ct_arr, cp, t + dt) for t in e["t"]]
            for i in range(len(e["t"])):
                if not ok[i]:
                    give(lid, e, i)
            e = dict(e, t=[x for x, o in zip(e["t"], ok) if o], uv=[x for x, o in zip(e["uv"], ok) if o], uvn=[x for x, o in zip(e["uvn"], ok) if o])
            if len(e["t"]) < 2:
                for i in range(len(e["t"])):
                    give(lid, e, i)
                continue
            served.append((lid, e))
        kept = served
        lg, ok = np.zeros((0, 6)), np.zeros(0, dtype=np.uint8)
        if kept:
            ptr = np.concatenate([[0], np.cumsum([len(e["t"]) for _, e in kept])]).astype(np.int32)
            anchor, has = np.zeros((len(kept), 3)), np.zeros(len(kept), dtype=np.uint8)
            for l, (lid, e) in enumerate(kept):
                for pid in e["points"]:               # the first triangulated point of the line (REF LineHelper.cpp:233-247)
                    if pid in mir.used:
                        anchor[l], has[l] = mir.used[pid][0], 1
                        break
            tt = np.concatenate([e["t"] for _, e in kept])
            R, p, okp = self.jo.cpi_poses(st, cpi, tt + dt)
            assert okp.all()
            lt_all = pkg.LineTracks(ptr, tt, np.concatenate([e["uv"] for _, e in kept]), seg_uvn=np.concatenate([e["uvn"] for _, e in kept]),
                                    D=[e["D"] for _, e in kept], anchor_pt=anchor, has_pt=has, res_R=R, res_p=p)
            lg, ok = self.jo.triangulate_lines(st, lt_all)
        self._prep = dict(n_pool=len(pool), kept=kept, unused=unused, give=give, lg=lg, ok=ok)

    def camera_update_lines(self, st, n, max_obs, t_prev_frame, state_time, window_full=True, chi2_mult=1.0, cap=512, cpi=None):
        if cpi is None:
            return PyMirrorContext.camera_update_lines(self, st, n, max_obs, t_prev_frame, state_time, window_full, chi2_mult, cap)
        assert getattr(self, "_prep", None) is not None
        prep, self._prep = self._prep, None
        pkg, mir = self.pkg, self.mir
        ct = [float(x) for x in st.t]
        dt = float(st.c.cam_dt)
        t_oldest = ct[0]
        bounding = lambda t: mir._bounding(ct, t + dt)
        kept, unused, give, lg, ok = prep["kept"], prep["unused"], prep["give"], prep["lg"], prep["ok"]
        out = dict(dx=np.zeros(n), n_pool=prep["n_pool"], n_lines=0, n_accepted=0, n_rows=0, status=0, ids=[], accepted=[])
        if kept:
            sel, t_first = [], {}
            for l, (lid, e) in enumerate(kept):
                valid = sum(bounding(t) for t in e["t"])
                if not ok[l] or valid < 2 or len(sel) >= cap:
                    for i in range(len(e["t"])):
                        give(lid, e, i)
                    continue
                if valid > max_obs:
                    t_first[l] = valid - max_obs
                sel.append(l)
            if sel:
                tt, uv, counts = [], [], []
                for l in sel:
                    lid, e = kept[l]
                    c = seen = 0
                    for i, t in enumerate(e["t"]):
                        if not bounding(t):
                            give(lid, e, i)
                            continue
                        seen += 1
                        if seen <= t_first.get(l, 0):
                            continue
                        tt.append(t), uv.append(e["uv"][i])
                        c += 1
                    counts.append(c)
                sptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
                R, p, okp = self.jo.cpi_poses(st, cpi, np.array(tt) + dt)      # (on the updated state: the rows' poses)
                assert okp.all()
                lt = pkg.LineTracks(sptr, np.array(tt), np.array(uv, dtype=np.float32), line_FinG=lg[sel], res_R=R, res_p=p)
                cols = self.jo.line_columns(st, lt)
                rows, Hf, Hx, res = self.jo.build_line_jacobians(st, lt, cols, 2 * max_obs)
                rc, P2, dx, acc, nrows = self.o.msckf_update(self.P, rows, Hf, Hx, res, cols, st.c.sigma_pix ** 2, self.q95, chi2_mult=chi2_mult,
                                                             res_norm_gate=0.0)
                out.update(n_lines=len(sel), ids=[kept[l][0] for l in sel], accepted=list(acc), n_rows=int(nrows), status=int(rc),
                           line_FinG=lg[sel])
                if rc == 0:
                    self.P = np.array(P2, order="F")
                    out["dx"] = dx
                out["n_accepted"] = int(np.sum(acc))
                for l, a in zip(sel, acc):
                    if not a:
                        lid, e = kept[l]
                        for i, t in enumerate(e["t"]):
                            if bounding(t):
                                give(lid, e, i)
        for lid, u in unused.items():
            d = self.ldb.get(lid)
            if d is None:
                d = self.ldb[lid] = dict(t=[], uv=[], uvn=[], points=list(u["points"]), D=u["D"])
            d["t"].extend(u["t"]), d["uv"].extend(u["uv"]), d["uvn"].extend(u["uvn"])
        if window_full:
            for lid in list(self.ldb):
                e = self.ldb[lid]
                keep = [i for i, t in enumerate(e["t"]) if not t < t_oldest]
                if not keep:
                    del self.ldb[lid]
                elif len(keep) != len(e["t"]):
                    for key in ("t", "uv", "uvn"):
                        e[key] = [e[key][i] for i in keep]
            for pid in [pid for pid, (_, newest) in mir.used.items() if newest < t_oldest]:   # point_used->cleanup_measurements
                del mir.used[pid]
        return out
