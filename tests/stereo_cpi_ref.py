"""The point half of plv_stereo_try_update restated: stereo_update_ref.update_points with use_imu_res (a CPI table) and the
point_used fill, composed of the same oracle pieces.

Served or not.  Whether the table serves an observation's time + dt is decided from times alone (REF State.cpp:273-355; the rule is
spelled out at cpi_servable in csrc/camera_tracks.hpp): a record stored at exactly that time whose clone is in the window; else two
neighbouring records of one clone that has not left the window; and that clone with a record of its own.  test_stereo_cpi_ref_cpu.py
holds `servable` to the `ok` of the oracle's pose function.
Poses.  The served observations get the oracle's CPI pose (orc_cpi_poses, tests/test_oracle_cpi.py) as res_R / res_p; from there on it
is stereo_update_ref's triangulation, Jacobians and update.  The pair shares one time offset: a left and a right observation of one
frame ask for one time and share one pose (`pose_of`).
Unserved observations leave the feature for its own camera's track in the database, as observations without bounding clones do (REF
CamHelper.cpp:356-365) — for every feature of the pool, as the library does (the reference does it feature by feature until the cap
ends its loop; a feature it never reaches goes back whole either way: the same database).
point_used.  Every feature the loop triangulates before the cap, consistent or not, is copied to point_used (REF CamHelper.cpp:
648-699): id -> (p_FinG, newest observation time)."""
import numpy as np

import stereo_update_ref as sr
import synth


def servable(clone_t, cp, tq):
    """cpi_servable from times alone: clone_t the window's clone times, cp the table (t ascending, clone_t per record)"""
    t, ct = cp["t"], cp["clone_t"]
    n = len(t)
    e = np.flatnonzero(t == tq)
    if len(e) and (clone_t == ct[e[0]]).any():
        c = ct[e[0]]
    else:
        if n == 0 or tq < t[0] or tq > t[-1]:
            return False
        i0 = 0 if tq == t[0] else int(np.searchsorted(t, tq, side="left")) - 1
        i1 = n - 1 if tq == t[-1] else int(np.searchsorted(t, tq, side="right"))
        if ct[i0] != ct[i1] or ct[i0] < clone_t[0]:
            return False
        c = ct[i0]
    return bool((clone_t == c).any() and (t == c).any())


def cut_table(cp, sc, n_oldest=1):
    """synth.cpi_scene's table without the records integrated from the n_oldest oldest clones: their times are not served"""
    keep = cp["clone_t"] > sc["t"][n_oldest - 1]
    return dict(cp, t=cp["t"][keep], clone_t=cp["clone_t"][keep], R=cp["R"][keep], alpha=cp["alpha"][keep], v=cp["v"][keep])


def table(pkg, cp):
    return pkg.CpiTable(cp["t"], cp["clone_t"], cp["R"], cp["alpha"], cp["v"], gravity=cp["gravity"])


def update_scene(pkg, undistort, model1=sr.RADTAN, model0=sr.RADTAN):
    """sr.update_scene with one more track and the cut CPI table of its window.  The added track ("two then one") has camera 0's
    observations at the two oldest clones and camera 1's fifteen behind the newest clone (no bounding clones; the table serves
    them): seventeen observations, so the loop reaches it before the cap, two of them usable — and one once the table does not serve
    the oldest frame."""
    sc, pair, tracks, names, opt = sr.update_scene(pkg, undistort, model1=model1, model0=model0)
    _, _, obs = sr.stereo_scene(pkg, undistort, model1=model1, model0=model0)        # (seeded: the observations update_scene cut its tracks from)
    f = names["one usable"] - 1
    fid = max(tracks) + 100
    tracks = dict(tracks)
    tracks[fid] = {0: tuple(a[:2].copy() for a in obs[f][0]), 1: tuple(a.copy() for a in tracks[names["one usable"]][1])}
    names = dict(names, **{"two then one": fid})
    cp = cut_table(synth.cpi_scene(sc), sc)
    return sc, pair, tracks, names, opt, cp


def update_points(jo, oracle, pair, tracks, P, cp, tab, max_msckf, max_obs, t_prev_frame, state_time, window_full=True, tri=sr.TRI, dt_exp=0.01):
    """sr.update_points with the table: returns its dict plus `used` ({id: (p_FinG, newest)}), `unserved` ({cam: count} over the features
    the loop examined), `below_two` (ids with two usable observations before the table's hand-back and fewer after), `times` (the
    distinct served times) and `pose_of` ({id: {cam: index into times per kept observation}}) with `kept_t`, those observations' times.
    cp = None: no table — every observation is served and keeps its polynomial pose (sr.update_points plus the point_used fill)."""
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
    # ---- get_imu_poses with the table: unserved observations go back per camera, the others carry the oracle's CPI pose
    served_times, pose_of, kept_t, n_unserved_of = [], {}, {}, {}
    for fid in order:
        ft, kept = cand[fid], {}
        before = sum(len(v) for v in sr.usable(jo, pair, ft).values())
        n_unserved_of[fid] = {0: 0, 1: 0}
        for c in (1, 0):
            if c not in ft:
                continue
            if cp is None:
                kept[c] = ft[c]
                continue
            ok = np.array([servable(t, cp, tq) for tq in ft[c][0] + dt])
            n_unserved_of[fid][c] = int((~ok).sum())
            back(fid, c, ft[c], np.flatnonzero(~ok))
            if not ok.any():
                continue
            tq = ft[c][0][ok] + dt
            R, p, ok_o = jo.cpi_poses(pair.views[0], tab, tq)
            assert ok_o.all(), "the oracle's pose function refuses a time the restated rule serves"
            kept[c] = tuple(a[ok] for a in ft[c]) + (R, p)
            for x in tq:
                if x not in served_times:
                    served_times.append(x)
            pose_of.setdefault(fid, {})[c] = [served_times.index(x) for x in tq]
            kept_t.setdefault(fid, {})[c] = kept[c][0]
        cand[fid] = kept
        after = sum(len(v) for v in sr.usable(jo, pair, kept).values())
        n_unserved_of[fid]["below_two"] = before >= 2 > after
    feats = [cand[fid] for fid in order]
    trace = dict(order=order, n_valid={}, ok={}, err={}, err_obs={}, anchor={})
    sel, p_sel, used, examined = [], [], {}, []
    for fid, ft in zip(order, feats):
        whole = lambda: [back(fid, c, ft[c], np.arange(len(ft[c][0]))) for c in ft]
        if len(sel) >= max_msckf:
            whole()
            continue
        examined.append(fid)
        ok, p, err, err_obs, anchor, (n0, n1) = sr.triangulate(jo, pair, ft, tri) if ft else (False, np.zeros(3), 0.0, 0.0, 1, (0, 0))
        trace["n_valid"][fid], trace["ok"][fid], trace["err"][fid], trace["err_obs"][fid], trace["anchor"][fid] = (n0, n1), ok, err, err_obs, anchor
        if n0 + n1 >= 2 and ok:
            used[fid] = (p.copy(), max(float(ft[c][0][-1]) for c in ft))
        if n0 + n1 < 2 or not ok or not err < 3.0:
            whole()
            continue
        assert n0 + n1 <= max_obs
        sel.append(fid)
        p_sel.append(p)
    out = dict(n_pool=n_pool, ids=np.array(sel, np.uint64), trace=trace, p_FinG=np.array(p_sel).reshape(-1, 3), dx=np.zeros(len(P)), P=P.copy(),
               accepted=np.zeros(0, np.uint8), n_rows=0, status=0, used=used, times=np.array(served_times), pose_of=pose_of, kept_t=kept_t,
               unserved={c: sum(n_unserved_of[fid][c] for fid in examined) for c in (0, 1)},
               below_two=[fid for fid in examined if n_unserved_of[fid]["below_two"]])
    if sel:
        chosen = []
        for fid in sel:
            use = sr.usable(jo, pair, cand[fid])
            for c in cand[fid]:
                back(fid, c, cand[fid][c], np.array([i for i in range(len(cand[fid][c][0])) if i not in use[c]], int))
            chosen.append({c: tuple(a[use[c]] for a in cand[fid][c]) for c in cand[fid] if use[c]})
        cols = sr.columns(jo, pair, chosen)
        rows, Hf, Hx, res = sr.build_jacobians(jo, pair, chosen, out["p_FinG"], cols, 2 * max_obs)
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
