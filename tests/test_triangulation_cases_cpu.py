"""CPU test of the triangulation case matrix (tests/triangulation_cases.py): with the oracle's trace (orc_set_tri_trace /
orc_set_line_trace) every case reaches the stage, the Levenberg-Marquardt exit and the failed-step streak it names, every value of every
axis occurs, and the conditions hold that make a comparison of the device with the oracle meaningful: every gate value at least 1e-6
(relative) from its threshold, and no trace record or verdict changed by relative noise of 2^-52 on the camera poses.  What the outputs
move by under that noise is the batch's spread, which the device tests take their tolerance from.

The two exits no physical track reached.  The refinement also ends when lam reaches 1e10 (13 failed steps in a row) and when the
damped 3 x 3 solve meets a zero pivot.  Searched on the oracle with the trace on:
  * 378 000 tracks of this module's geometry, M in {2, 3, 8, 15, 16, 17, 24} x depth {5, 40, 140} m x noise {0, 0.3, 1} px x one
    outlier of {0, 15, 80} px x 2000 seeds, and 96 750 more at M in {3, 8, 15, 16, 17, 24, 40} (250 seeds per condition; seeds up to
    2999 for M = 16, 17, 24 with an 80 px outlier at 40 and 140 m): neither exit.  The longest streak in front of an accepted step
    is 14 (one track, whose trace the 2^-52 noise changes: not kept; the cases stop at 13).  A step
    fails only when its cost is strictly larger than the last accepted one, and a step too small to move a float residual leaves the
    cost equal, which counts as accepted: a streak ends where lam has shrunk the step below the float resolution of the residuals.
    Five accepted steps occurred for M = 2 and 3 only (12 + 2 tracks).
  * 20 000 + 4 800 sets of camera poses no camera ever had (arbitrary 3 x 3 matrices; matrices with a zero row; positions and uvn
    from 1e-3 to 1e3), handed in per observation through res_R / res_p: a zero row makes h3 == 0, and then either the first cost is
    NaN and all 13 steps fail (lam cap; the feature ends NaN behind the loop), or the Hessian has a zero pivot and the first damped
    solve fails (the linear solution stands and is accepted).  Arbitrary matrices take five steps at every M.
These are the batch "lm-exits-raw-poses": both exits on both paths of the refinement (M <= 16 and M >= 17), the branches themselves, not
imitations of them."""
import numpy as np
import pytest

import oracle_lib as ol
import triangulation_cases as tc


@pytest.fixture(scope="module")
def jo(pkg):
    return ol.load_jac(pkg)


@pytest.fixture(scope="module")
def points(pkg, jo):
    """[(built batch, oracle result, stable, spread)] of every point batch, computed once"""
    fo, sc, out = ol.load_front(), tc.scene(), []
    for bt in tc.point_batches():
        b = tc.build(pkg, bt, fo.undistort, sc)
        r = tc.oracle_points(jo, b)
        out.append((b, r) + tc.point_spread(pkg, jo, b, r))
    return out


@pytest.fixture(scope="module")
def lines(pkg, jo):
    sc, out = tc.scene(), []
    for bt in tc.line_batches():
        b = tc.build_lines(pkg, bt, sc)
        r = tc.oracle_lines(jo, b)
        out.append((b, r) + tc.line_spread(pkg, jo, b, r))
    return out


def _accepting_streaks(rec):
    return [n for n, acc in ol.streaks(rec) if acc]


def test_point_cases_reach_what_they_name(points):
    for b, r, stable, s in points:
        bt = b["batch"]
        assert 0 < len(bt.tracks) <= 40, bt.name
        print(f"== {bt.name}: stable {stable}, spread p {s['p']:.1e} values {s['vals']:.1e} reprojection {s['err']:.1e}, "
              f"smallest gate margin {tc.point_margins(b, r).min():.1e}")
        for f, (k, rec) in enumerate(zip(bt.tracks, r["trace"])):
            stage, exit_ = ol.TRI_STAGES[rec[1]], ol.LM_EXITS[rec[2]]
            print(f"   {k.name:30s} valid {rec[0]:3d}  {stage:22s} exit {exit_:14s} passes {rec[3]:2d} accepted {rec[4]}  streaks {ol.streaks(rec)}")
            assert rec[0] == b["n_valid"][f], (bt.name, k.name)
            assert bool(r["ok"][f]) == (stage == "accepted")
            assert stage == k.expect["stage"], (bt.name, k.name, stage)
            if "exit" in k.expect:
                assert exit_ == k.expect["exit"], (bt.name, k.name, exit_)
            if "streak" in k.expect:
                assert k.expect["streak"] in _accepting_streaks(rec), (bt.name, k.name, ol.streaks(rec))
            if "linear_inside" in k.expect:       # the linear depth passed the range the refined one left
                assert bt.opt["min_dist"] <= r["vals"][f][1] <= bt.opt["max_dist"]
            if not bt.opt["refine"]:
                assert exit_ == "none" and rec[3] == 0
            if r["ok"][f]:
                assert np.isfinite(r["p"][f]).all() and np.isfinite(r["err"][f]) and np.isfinite(r["vals"][f][:2]).all()
            else:
                assert not r["p"][f].any() and r["err"][f] == 0


def test_point_axes_are_covered(points):
    by_name = {b["batch"].name: (b, r) for b, r, _, _ in points}
    traces = np.concatenate([r["trace"] for _, r, _, _ in points])
    # track length: every count, and in front of the refinement (stage accepted) where there are two or more
    assert set(tc.LENGTHS) <= set(int(n) for n in traces[:, 0])
    ok_n = set(int(rec[0]) for rec in traces if ol.TRI_STAGES[rec[1]] == "accepted")
    assert set(n for n in tc.LENGTHS if n >= 2) <= ok_n
    # every rejection fails a feature next to one that passes, in one batch (one option set)
    for stage, names in (("condition number", ("gate-cond-1e4", "gate-cond-1e7")), ("linear depth low", ("gate-depth",)), ("linear depth high", ("gate-depth",)),
                         ("refined depth high", ("gate-depth",)), ("refined depth low", ("gate-refined-low",)), ("baseline ratio", ("gate-baseline",)),
                         ("too few observations", ("lengths-long", "lengths-short", "invalid-far", "invalid-past"))):
        for name in names:
            stages = [ol.TRI_STAGES[rec[1]] for rec in by_name[name][1]["trace"]]
            assert stage in stages and "accepted" in stages, (stage, name)
    b, r = by_name["gate-depth"]
    inside = [b["batch"].opt["min_dist"] <= v[1] <= b["batch"].opt["max_dist"] for v, rec in zip(r["vals"], r["trace"]) if ol.TRI_STAGES[rec[1]] == "refined depth high"]
    assert inside and all(inside)
    assert not by_name["refine-off"][0]["batch"].opt["refine"]
    # exits of the refinement, on both paths (four candidates: up to 16 observations; one at a time: 17 and more)
    for lo, hi in ((2, 16), (17, 10 ** 6)):
        recs = [rec for rec in traces if lo <= rec[0] <= hi]
        assert {"small decrease", "small step", "five runs", "lam cap", "solve failed"} <= set(ol.LM_EXITS[rec[2]] for rec in recs), (lo, hi)
        st = set(n for rec in recs for n in _accepting_streaks(rec))
        assert set(range(1, 9)) <= st and max(st) >= 9, (lo, hi, sorted(st))
    # ... and the streaks a case was chosen for are where they were put
    for name, lo, hi in (("streaks-four-candidates", 2, 16), ("streaks-serial", 17, tc.N_CLONES)):
        b, r = by_name[name]
        assert all(lo <= n <= hi for n in r["trace"][:, 0])
        st = set(k.expect["streak"] for k in b["batch"].tracks)
        assert set(range(1, 9)) <= st and max(st) >= 9
    # the four-candidate pass: a streak of s failed steps is accepted by lane group s % 4 of pass s // 4 + 1 after the linearisation
    spec = set(n for rec in by_name["streaks-four-candidates"][1]["trace"] for n in _accepting_streaks(rec)) | {0}
    assert {(n // 4, n % 4) for n in spec} >= {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0)}
    # invalid observations: first, last, inner, all but one, a block across a multiple of 64
    bad = [k.bad for k in by_name["invalid-far"][0]["batch"].tracks]
    M = [k.M for k in by_name["invalid-far"][0]["batch"].tracks]
    assert any(b_ == (0,) for b_ in bad) and any(b_ == (m - 1,) for b_, m in zip(bad, M)) and any(len(b_) == m - 1 for b_, m in zip(bad, M))
    assert any(len(b_) == 1 and 0 < b_[0] < m - 1 for b_, m in zip(bad, M)) and any(len(b_) > 1 and b_[0] < 64 <= b_[-1] for b_ in bad)
    # window: the three offsets and cam_dt
    assert {0.0, 0.013, -0.004} <= set(getattr(k, "offset", 0.0) for b, _, _, _ in points for k in b["batch"].tracks)
    assert any(b["batch"].cam_dt != 0 for b, _, _, _ in points)
    # every route gets everything it can express: lengths on both sides of the four-candidate threshold, every gate stage next to an
    # accepted neighbour, the refinement switched off, every exit a physical track reaches and every streak length on both paths of the
    # refinement.  Only tracks of more than 20 observations (the one-call batch rows) and poses handed in per observation (the one-call
    # routes take none) are left to plv_triangulate alone.
    for b, _, _, _ in points:
        long_or_raw = [isinstance(k, tc.Raw) or k.M > tc.N_CLONES or k.bad_t == "far" for k in b["batch"].tracks]
        assert ("fused" in b["batch"].routes) == ("capped" in b["batch"].routes) == (not any(long_or_raw)), b["batch"].name
        assert "triangulate" in b["batch"].routes
    for route in ("triangulate", "fused", "capped"):
        mine = [(b, r) for b, r, _, _ in points if route in b["batch"].routes]
        recs = np.concatenate([r["trace"] for _, r in mine])
        assert {0, 1, 2, 3, 7, 8, 9, 15, 16, 17} <= set(int(x) for x in recs[:, 0]), route
        for stage in ol.TRI_STAGES:
            if stage in ("linear solve failed", "NaN"):          # (a singular linear system / a NaN: the raw-pose batch has the NaN)
                continue
            assert any(stage in [ol.TRI_STAGES[rec[1]] for rec in r["trace"]] and (r["ok"] > 0).any() for _, r in mine), (route, stage)
        assert any(not b["batch"].opt["refine"] and (r["ok"] > 0).any() and (r["ok"] == 0).any() for b, r in mine), route
        for lo, hi in ((2, 16), (17, tc.N_CLONES)):
            sub = [rec for rec in recs if lo <= rec[0] <= hi]
            assert {"small decrease", "small step"} <= set(ol.LM_EXITS[rec[2]] for rec in sub), (route, lo)
            st = set(n for rec in sub for n in _accepting_streaks(rec))
            assert set(range(1, 9)) <= st and max(st) >= 9, (route, lo, sorted(st))
        assert "five runs" in set(ol.LM_EXITS[rec[2]] for rec in recs), route


def test_point_margins_and_stability(points):
    for b, r, stable, s in points:
        m = tc.point_margins(b, r)
        assert (m >= 1e-6).all(), (b["batch"].name, [b["batch"].tracks[f].name for f in np.nonzero(m < 1e-6)[0]])
        assert stable, b["batch"].name
        assert s["p"] < 1e-6 and s["vals"] < 1e-5, (b["batch"].name, s)      # (a case the rounding of its input moves by more says nothing)
        stored = tc.POINT_SPREAD[b["batch"].name]                             # the spread stored with the case is the measured one
        for key in ("p", "vals", "err"):
            assert s[key] <= stored[key] <= 1.1 * s[key], (b["batch"].name, key, s[key], stored[key])
    assert set(tc.POINT_SPREAD) == set(b["batch"].name for b, _, _, _ in points)


def test_line_cases_reach_what_they_name(lines):
    for b, r, stable, s in lines:
        bt = b["batch"]
        print(f"== lines {bt.name}: stable {stable}, spread {s:.1e}, smallest |cos| margin {tc.line_margins(r).min():.1e}")
        for l, (k, rec) in enumerate(zip(bt.lines, r["trace"])):
            cosv = rec[5:][~np.isnan(rec[5:])]
            print(f"   {k.name:30s} valid {int(rec[0]):3d} first {int(rec[1]):2d}  {ol.LINE_BRANCHES[int(rec[2])]:12s} pairs tried {int(rec[3]):3d} used {int(rec[4]):3d}")
            assert rec[0] == k.M - len(k.bad) and ol.LINE_BRANCHES[int(rec[2])] == k.expect["branch"], (bt.name, k.name)
            assert rec[1] == k.expect.get("first", rec[1]) and rec[4] == k.expect.get("used", rec[4]), (bt.name, k.name)
            assert len(cosv) == rec[3] == (rec[0] - 1 if k.expect["branch"] == "plane pairs" else 0)
            assert rec[4] == (cosv < 0.99).sum()
            if k.expect.get("mix"):
                assert 0 < rec[4] < rec[3]
            assert bool(r["ok"][l]) == (k.expect["branch"] == "anchored" or rec[4] > 0)
            assert np.isfinite(r["lines"][l]).all() and (r["ok"][l] or not r["lines"][l].any())
        assert (tc.line_margins(r) >= 1e-6).all() and stable, bt.name
        assert s <= tc.LINE_SPREAD[bt.name] <= 1.1 * s, (bt.name, s)


def test_line_axes_are_covered(lines):
    ks = [(k, rec) for b, r, _, _ in lines for k, rec in zip(b["batch"].lines, r["trace"])]
    n = set(int(rec[0]) for _, rec in ks)
    assert {0, 1, 2, 3} <= n and max(n) >= 65
    for branch in ("anchored", "plane pairs"):
        assert any(rec[1] > 0 and k.expect["branch"] == branch for k, rec in ks)            # a first observation that is invalid
        assert any(rec[0] >= 65 and k.expect["branch"] == branch for k, rec in ks)
    assert {1, 2, 3} <= set(k.D for k, _ in ks if k.expect["branch"] == "anchored")
    assert any(k.D > 0 and not k.has_pt and k.expect["branch"] == "plane pairs" for k, _ in ks)
    assert any(k.D == 0 and k.has_pt and k.expect["branch"] == "plane pairs" for k, _ in ks)
    assert any(rec[3] >= 2 and rec[4] == 0 for _, rec in ks) and any(rec[3] >= 2 and rec[4] == 1 for _, rec in ks)
    assert any(rec[3] > 64 and 0 < rec[4] < rec[3] for _, rec in ks)


def test_trace_off_leaves_the_oracle_unchanged(pkg, jo, points, lines):
    """with no buffer set the oracle returns what it returns with the trace on, bit for bit, on every batch (NaN where it is NaN)"""
    for b, r, _, _ in points:
        p, ok, err = jo.triangulate_batch(b["st"], b["tr"], **b["batch"].opt)
        assert np.array_equal(p, r["p"], equal_nan=True) and np.array_equal(ok, r["ok"]) and np.array_equal(err, r["err"], equal_nan=True), b["batch"].name
    for b, r, _, _ in lines:
        out, ok = jo.triangulate_lines(b["st"], b["lt"])
        assert np.array_equal(out, r["lines"]) and np.array_equal(ok, r["ok"]), b["batch"].name


def test_anchor_walk_takes_what_it_names(pkg, jo):
    """the one-call line route's anchors on the compiled CPU frame: the first point triangulated now, the second because the first
    failed, an old anchor (also in front of a point triangulated now: the order of the line's points decides), none at all; a point
    triangulated now replaces its old entry"""
    import fused_cases as fc
    w = tc.anchor_walk(pkg, ol.load_front().undistort)
    pts, dec, lns = tc.anchor_walk_oracle(pkg, w, fc.q95_table())
    r = tc.oracle_points(jo, w["b"])
    now = {i: r["p"][f] for f, i in enumerate(w["ids"]) if r["ok"][f]}
    assert set(now) == {101, 103} and dec[102][1] == 0 and lns["status"] == 0
    assert sorted(int(i) for i in lns["ids"]) == sorted(tc.WALK_LINES)            # every line is triangulated, one way or the other
    kinds = set()
    for i, l in zip(lns["ids"], lns["line_FinG"]):
        pids, D, (kind, pid) = tc.WALK_LINES[int(i)]
        kinds.add((kind, pids.index(pid) if kind else -1))
        cands = dict(now=now, old=tc.WALK_OLD)
        for k2, table in cands.items():
            for p2, a in table.items():
                same = np.abs(l[:3] - np.cross(a, l[3:])).max() < 1e-12
                assert same == ((k2, p2) == (kind, pid)), (int(i), k2, p2)
        print(f"   line {int(i)} points {pids} D {D}: anchor {kind} {pid if kind else ''}")
    assert {("now", 0), ("now", 1), ("now", 2), ("old", 0), ("old", 1), (None, -1)} <= kinds
    stable, ps = tc.point_spread(pkg, jo, w["b"], r)
    assert stable and all(ps[k] <= tc.WALK_POINT_SPREAD[k] <= 1.1 * ps[k] for k in ps), ps
    stable, s = tc.anchor_walk_spread(pkg, w, fc.q95_table(), lns)
    assert stable and s <= tc.LINE_SPREAD["anchor-walk"] <= 1.1 * s, s
