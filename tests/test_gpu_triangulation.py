"""Point and line triangulation on the device (triangulate_feature and line_triangulate_one, csrc/jacobian_kernels.hip) held to the CPU
oracle on the case matrix of tests/triangulation_cases.py, which tests/test_triangulation_cases_cpu.py proves on the oracle's trace:
every track length around the lane stride and the four-candidate threshold, invalid observations at every position, every gate
rejecting next to a neighbour that passes, every exit of the refinement the search reached and failed-step streaks of every length
on both paths of the refinement; for lines every branch, an invalid first observation and the 8 degree test on both sides.

triangulate_feature runs in three settings, and every batch a setting can express runs through it:
  triangulate   triangulate_kernel behind plv_triangulate, on global arrays
  fused         wave 0 of jacobian_nullspace_kernel inside camera_update_points while the pool fits max_msckf (LDS copies, o0 = 0)
  capped        triangulate_kernel launched inside camera_update_points when the pool exceeds max_msckf (the selection stops at the cap)
The one-call settings run with the decision trace on and are held to the compiled CPU frame on the same databases, column by column
(N_OBS, TRI_OK, REPROJ, COND, DEPTH, REF_DEPTH, BASELINE): the NaN pattern equal, the values by value.

Which launch ran is read from the context's profile.  The one-call routes return positions for the features their selection took
(triangulated, mean reprojection error below 3 px, inside the cap): a track that carries an 80 px outlier (the longest streaks) is
held there by its verdict and its four decision values (condition number, both depths, baseline ratio), and by position through
plv_triangulate.

Asserted per feature, rejected ones included: `ok` equal, rejected outputs zero, positions / reprojection errors / decision values /
lines to the larger of the bound the existing tests hold (1e-9 x max(1, largest entry); rtol 1e-7; 1e-8) and ten times the batch's
spread under 2^-52 noise on its camera poses (triangulation_cases.point_spread).  The three settings agree with each other at least as
closely.  Measured worst differences and what a set of one-line mutations of the two device functions does to this file:
profiles/HISTORY.md."""
import numpy as np
import pytest

import fused_cases as fc
import oracle_lib as ol
import synth
import triangulation_cases as tc

pytestmark = pytest.mark.gpu

MAX_OBS = 20          # the one-call batches hold tracks of up to 20 valid observations: the fused launch takes them whole
COLS = (0, 1, 2, 4, 5, 6, 7)   # N_OBS, TRI_OK, REPROJ, COND, DEPTH, REF_DEPTH, BASELINE of Context.DECISION_VALUES
POINT_BATCHES = tc.point_batches()
LINE_BATCHES = tc.line_batches()


@pytest.fixture(scope="module")
def jo(pkg):
    return ol.load_jac(pkg)


@pytest.fixture(scope="module")
def sc():
    return tc.scene()


_REF = {}


def _reference(pkg, jo, sc, bt):
    """(built batch, oracle result, tolerances) of a point batch, computed once and left unchanged"""
    if bt.name not in _REF:
        b = tc.build(pkg, bt, ol.load_front().undistort, sc)
        r = tc.oracle_points(jo, b)
        for a in r.values():
            a.setflags(write=False)
        _REF[bt.name] = (b, r, tc.point_tolerances(r, tc.POINT_SPREAD[bt.name]))     # (the spread stored with the case: the CPU test holds it to the oracle)
    return _REF[bt.name]


def _close(a, o, rel, what):
    """NaN pattern equal; |a - o| <= rel x |o| elsewhere.  Returns the largest relative difference."""
    a, o = np.asarray(a, dtype=np.float64), np.asarray(o, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(o)), (what, a, o)
    fin = ~np.isnan(o)
    if not fin.any():
        return 0.0
    inf = np.isinf(o[fin])
    assert np.array_equal(a[fin][inf], o[fin][inf]), (what, a, o)
    d = np.abs(a[fin][~inf] - o[fin][~inf]) / np.maximum(np.abs(o[fin][~inf]), 1e-300)
    worst = float(d.max()) if d.size else 0.0
    assert worst <= rel, (what, worst, rel, a, o)
    return worst


def _check_points(name, got, r, tol, what):
    """(p, ok, err) of a route against the oracle's: returns the worst differences (position, reprojection error)"""
    p, ok, err = got
    assert np.array_equal(ok, r["ok"]), (name, what, np.nonzero(ok != r["ok"])[0])
    bad = r["ok"] == 0
    assert not p[bad].any() and not err[bad].any(), (name, what)          # rejected outputs are zero, as the kernel writes them
    good = ~bad
    if not good.any():
        return 0.0, 0.0
    dp = float(np.abs(p[good] - r["p"][good]).max())
    assert dp <= tol["p"], (name, what, dp, tol["p"], int(np.abs(p - r["p"]).max(axis=1).argmax()))
    return dp, _close(err[good], r["err"][good], tol["err"], (name, what, "reprojection error"))


# the launches of the two one-call settings, by the names the library's own profile gives them
LAUNCHES = {"fused": ({"tri_jacobian_nullspace_kernel"}, {"triangulate_kernel", "jacobian_nullspace_kernel"}),
            "capped": ({"triangulate_kernel", "jacobian_nullspace_kernel"}, {"tri_jacobian_nullspace_kernel"})}


def _one_call(pkg, b, r, tracks, max_msckf, route):
    """camera_update_points with the decision trace on and the compiled CPU frame on the same databases.  Every track is in the pool
    (no measurement is newer than t_prev_frame).  The context's profile says which launches ran: the setting under test, not the
    other one."""
    sc_, opt = b["sc"], b["batch"].opt
    n = sc_["n_state"]
    P = synth.spd_cov(n, seed=4) * 1e-4
    t_last = float(sc_["t"][-1])
    args = (b["st"], n, max_msckf, MAX_OBS)
    kw = dict(t_prev_frame=t_last + 1.0, state_time=t_last, window_full=True, **opt)
    c = pkg.Context(pkg.default_config(752, 480))
    try:
        c.decision_trace(True)
        fc.fill_databases(c, "points", tracks, {}, device=True)
        c.cov_upload(P)
        c.prof_enable(True)
        out = c.camera_update_points(*args, **kw)
        c.prof_enable(False)
        ran = set(name for name, (count, _) in c.prof_table().items() if count > 0)
        ids, vals = c.last_point_decisions()
    finally:
        c.close()
    must, must_not = LAUNCHES[route]
    assert must <= ran and not (must_not & ran), (b["batch"].name, route, sorted(ran))
    fr = ol.FrameOracle(pkg, pkg.default_config(752, 480), fc.q95_table())
    fr.set_intrinsics(sc_["K8"])
    fc.fill_databases(fr, "points", tracks, {}, device=False)
    Po = np.array(P, dtype=np.float64, order="F")
    ref = fr.update_points(Po, b["st"], max_msckf, MAX_OBS, kw["t_prev_frame"], kw["state_time"], True, 1.0, opt["min_dist"], opt["max_dist"], opt["max_cond"],
                           opt["max_baseline"], opt["refine"])
    ids_o, vals_o = fr.last_point_decisions()
    fr.close()
    return out, dict(zip((int(i) for i in ids), vals)), ref, dict(zip((int(i) for i in ids_o), vals_o))


@pytest.mark.parametrize("bt", POINT_BATCHES, ids=lambda bt: bt.name)
def test_point_routes_against_the_oracle(pkg, ctx, jo, sc, bt):
    b, r, tol = _reference(pkg, jo, sc, bt)
    F = len(bt.tracks)
    # ---- plv_triangulate
    p, ok, err = ctx.triangulate(b["st"], b["tr"], **bt.opt)
    worst = {"triangulate": _check_points(bt.name, (p, ok, err), r, tol, "triangulate")}
    line = f"{bt.name:24s} {F:2d} features, {int(r['ok'].sum()):2d} accepted | tolerance p {tol['p']:.1e} err {tol['err']:.1e} values {tol['vals']:.1e} | triangulate: p {worst['triangulate'][0]:.1e} err {worst['triangulate'][1]:.1e}"
    # ---- the one-call routes
    routes = {}
    tr = b["tr"]
    tracks = {f + 1: (tr.t[tr.ptr[f]:tr.ptr[f + 1]].copy(), tr.uv[tr.ptr[f]:tr.ptr[f + 1]].copy(), tr.uvn[tr.ptr[f]:tr.ptr[f + 1]].copy()) for f in range(F)}
    for route in ("fused", "capped"):
        if route not in bt.routes:
            continue
        cap = 40 if route == "fused" else max(1, F // 2)
        assert (F <= cap) == (route == "fused")
        out, dev, ref, orc = _one_call(pkg, b, r, tracks, cap, route)
        assert out["status"] == ref["status"] == 0 and out["n_pool"] == ref["n_pool"] and out["n_truncated"] == ref["n_truncated"] == 0
        assert np.array_equal(out["ids"], ref["ids"]) and set(dev) == set(orc)
        if route == "capped" and (r["ok"] > 0).sum() >= cap + 2:
            assert out["n_msckf"] <= cap
        pool = sorted(orc)
        assert len(pool) == sum(1 for k in bt.tracks if k.M >= 2)                  # (a track of one measurement never reaches the pool)
        wv = 0.0
        for i in pool:
            f = i - 1
            a, o = dev[i], orc[i]
            assert a[0] == o[0] and a[1] == o[1] == r["ok"][f], (bt.name, route, bt.tracks[f].name, a, o)
            _close(a[2], o[2], tol["err"], (bt.name, route, bt.tracks[f].name, "reprojection error"))
            wv = max(wv, _close(a[[4, 5, 6, 7]], o[[4, 5, 6, 7]], tol["vals"], (bt.name, route, bt.tracks[f].name, "condition number, depths, baseline ratio")))
            _close(o[[4, 5, 6, 7]], r["vals"][f], 0.0, "the frame oracle's values are the batch oracle's")
        sel = [int(i) - 1 for i in ref["ids"]]
        dp = float(np.abs(out["p_FinG"] - r["p"][sel]).max()) if sel else 0.0
        assert dp <= tol["p"], (bt.name, route, dp, tol["p"])
        assert np.array_equal(ref["p_FinG"], r["p"][sel])
        routes[route] = (out, dev, sel)
        worst[route] = (dp, wv)
        line += f" | {route}: p {dp:.1e} values {wv:.1e}"
    # ---- the three settings agree with each other at least as closely as each does with the oracle
    for route, (out, dev, sel) in routes.items():
        if sel:
            assert np.abs(out["p_FinG"] - p[sel]).max() <= tol["p"], (bt.name, route, "against triangulate")
        for i, a in dev.items():
            if a[1]:
                _close(a[2], err[i - 1], tol["err"], (bt.name, route, "reprojection error against triangulate"))
    if len(routes) == 2:
        (o1, d1, s1), (o2, d2, s2) = routes["fused"], routes["capped"]
        for i in d1:
            _close(d1[i][list(COLS)], d2[i][list(COLS)], max(tol["vals"], tol["err"]), (bt.name, "fused against capped", i))
    print(line)


_LREF = {}


@pytest.mark.parametrize("bt", LINE_BATCHES, ids=lambda bt: bt.name)
def test_line_triangulation_against_the_oracle(pkg, ctx, jo, sc, bt):
    if bt.name not in _LREF:
        b = tc.build_lines(pkg, bt, sc)
        r = tc.oracle_lines(jo, b)
        _LREF[bt.name] = (b, r, tc.line_tolerance(r, tc.LINE_SPREAD[bt.name]))
    b, r, tol = _LREF[bt.name]
    out, ok = ctx.triangulate_lines(b["st"], b["lt"])
    assert np.array_equal(ok, r["ok"]), [k.name for k, a, o in zip(bt.lines, ok, r["ok"]) if a != o]
    assert not out[r["ok"] == 0].any()
    assert np.isfinite(out).all()
    d = np.abs(out - r["lines"]).max(axis=1)
    assert d.max() <= tol, (bt.name, bt.lines[int(d.argmax())].name, d.max(), tol)
    print(f"lines {bt.name:10s} {len(bt.lines):2d} lines, {int(ok.sum()):2d} triangulated | tolerance {tol:.1e} | worst {d.max():.1e} ({bt.lines[int(d.argmax())].name})")


def test_anchor_walk_of_the_one_call_line_route(pkg, jo, sc):
    """camera_update_points, camera_get_line_features, camera_update_lines on the databases of triangulation_cases.anchor_walk against
    the compiled CPU frame: a classified line's anchor is its first point that the point update triangulated in this call, its second
    because the first failed, an old anchor (in front of a point triangulated now too), or none (plane pairs).  The lines by value: an
    anchored line is (anchor x direction, direction), so a wrong anchor moves it by metres; the bound is the larger of 1e-9 x max(1,
    largest entry) and ten times the lines' spread on the compiled CPU frame under 2^-52 noise on the camera poses (the anchors'
    own movement included: triangulation_cases.anchor_walk_spread, stored as LINE_SPREAD["anchor-walk"])."""
    w = tc.anchor_walk(pkg, ol.load_front().undistort, sc)
    pts_o, dec_o, lns_o = tc.anchor_walk_oracle(pkg, w, fc.q95_table())
    r = tc.oracle_points(jo, w["b"])
    tol = tc.point_tolerances(r, tc.WALK_POINT_SPREAD)
    st, n, opt = w["b"]["st"], w["n"], tc.WALK_OPT
    t_last = float(w["sc"]["t"][-1])
    c = pkg.Context(pkg.default_config(752, 480))
    try:
        c.decision_trace(True)
        fc.fill_databases(c, "points", w["tracks"], {}, device=True)
        fc.fill_databases(c, "lines", w["ltracks"], w["used"], device=True)
        c.cov_upload(w["P"])
        pts = c.camera_update_points(st, n, 40, MAX_OBS, t_prev_frame=t_last + 1.0, state_time=t_last, window_full=True, **opt)
        c.camera_get_line_features(st)
        lns = c.camera_update_lines(st, n, MAX_OBS, t_prev_frame=t_last + 1.0, state_time=t_last, window_full=True)
    finally:
        c.close()
    assert pts["status"] == lns["status"] == 0 and np.array_equal(pts["ids"], pts_o["ids"])
    assert np.abs(pts["p_FinG"] - pts_o["p_FinG"]).max() <= tol["p"]
    assert lns["n_pool"] == lns_o["n_pool"] and np.array_equal(lns["ids"], lns_o["ids"]) and len(lns["ids"]) == len(tc.WALK_LINES)
    bound = max(1e-9 * max(1.0, np.abs(lns_o["line_FinG"]).max()), 10 * tc.LINE_SPREAD["anchor-walk"])
    d = np.abs(lns["line_FinG"] - lns_o["line_FinG"]).max(axis=1)
    assert d.max() <= bound, (int(lns["ids"][int(d.argmax())]), d.max(), bound)
    print(f"anchor walk: {len(lns['ids'])} lines | bound {bound:.1e} | worst {d.max():.1e} (line {int(lns['ids'][int(d.argmax())])})")
