"""GPU parity of the two-view RANSAC gate (ransac_hyp_kernel, ransac_select_kernel) with the CPU oracle, hypothesis by hypothesis, on
the case matrix of tests/ransac_cases.py (tests/test_ransac_cases_cpu.py proves on the oracle alone that every case reaches what it
names), and of plv_undistort at its block edges and on a lens that takes cv::undistortPoints' fallback.

Both sides run the same operation sequence (subset draw, full-pivot elimination, cubic from + - * / sqrt, normalisation, inlier count),
so everything is compared for equality: models by their bits, which also tells -0.0 from 0.0 (the only trace a double root with R == 0
leaves of the order of its two roots)."""
import numpy as np
import pytest

import oracle_lib
import ransac_cases
import synth

pytestmark = pytest.mark.gpu

CASES = ransac_cases.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def fo():
    return oracle_lib.load_front()


@pytest.fixture(scope="module")
def contexts(pkg):
    """one context per (confidence, iteration cap): both are read from the configuration when the context is made"""
    made = {}

    def get(conf=0.999, max_iters=1000):
        if (conf, max_iters) not in made:
            cfg = pkg.default_config(320, 240)
            cfg.ransac_conf, cfg.ransac_max_iters = conf, max_iters
            made[conf, max_iters] = pkg.Context(cfg)
        return made[conf, max_iters]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def ref_hyp(fo):
    """the oracle's hypotheses of every case, computed once"""
    return {c["name"]: fo.ransac_hypotheses(c["m1"], c["m2"], c["thr"], c["seed"], ransac_cases.nhyp(c)) for c in CASES}


def _compact(F, valid):
    """the library's three models in root order + validity bits -> run7point's compacted list"""
    out, nm = np.zeros_like(F), np.zeros(len(F), dtype=np.int32)
    for k in range(3):
        sel = np.flatnonzero((valid >> k) & 1)
        out[sel, nm[sel]] = F[sel, k]
        nm[sel] += 1
    return out, nm


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hypotheses_match_oracle(contexts, ref_hyp, case):
    """plv_ransac_hypotheses against orc_ransac_hypotheses: which models exist, their nine numbers, their inlier counts"""
    nh = ransac_cases.nhyp(case)
    rF, rnm, rcnt = ref_hyp[case["name"]]
    F, valid, cnt = contexts().ransac_hypotheses(case["m1"], case["m2"], case["thr"], case["seed"], nh)
    assert ((valid >= 0) & (valid < 8)).all()
    F, nm = _compact(F, valid)
    assert np.array_equal(nm, rnm), np.flatnonzero(nm != rnm)[:10]
    if not np.array_equal(F, rF):
        bad = np.flatnonzero((F != rF).reshape(nh, -1).any(axis=1))
        pytest.fail(f"{len(bad)} hypotheses differ (first {bad[:5]}), largest |difference| {np.nanmax(np.abs(F - rF))}")
    assert np.array_equal(F.view(np.int64), rF.view(np.int64)), "models equal by value, not by their bits (signed zeros)"
    assert np.array_equal(cnt, rcnt), np.flatnonzero((cnt != rcnt).any(axis=1))[:10]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gate_matches_oracle(contexts, fo, case):
    """plv_ransac_fundamental against orc_ransac_fundamental: mask, inliers, iterations used"""
    a, ag, ai = fo.ransac(case["m1"], case["m2"], case["thr"], case["conf"], case["max_iters"], case["seed"])
    b, bg, bi = contexts(case["conf"], case["max_iters"]).ransac(case["m1"], case["m2"], case["thr"], seed=case["seed"])
    assert (bg, bi) == (ag, ai)
    assert np.array_equal(a, b), int((a != b).sum())
    assert (ag, ai) == (case["inliers"] if case["inliers"] is not None else ag, case["iters"])


def test_hypotheses_rejects_bad_arguments(pkg, contexts):
    c = contexts()
    m = np.zeros((8, 2), np.float32)
    for n, nh in ((6, 10), (8, 0), (8, 4097)):
        with pytest.raises(pkg.PlvError):
            c.ransac_hypotheses(m[:n], m[:n], 0.01, 0, nh)
    F, valid, cnt = c.ransac_hypotheses(m, m, 0.01, 0, 4096)       # the largest batch: all points equal, no subset, no model
    assert not valid.any() and (cnt == -1).all()


def test_perform_matching_600_points(pkg, fo):
    """600 tracked points on a rendered pair: the inlier count's tail loop (n > 512), mask = klt & inlier and the copy the selection
    kernel makes for the host, in one call"""
    w, h = 752, 480
    canvas = synth.texture_canvas(w, h, seed=42)
    f0, f1 = synth.render_frame(canvas, w, h), synth.render_frame(canvas, w, h, tx=4.2, ty=-3.1, rot_deg=0.3, scale=1.002)
    c = pkg.Context(pkg.default_config(w, h))
    c.feed_image(f0)
    c.feed_image(f1)
    K = np.array(list(c.cfg.intrinsics))
    pts = synth.grid_points(w, h, 600, seed=5, border=16)
    assert len(pts) == 600
    pts[:3] = [[w + 30.0, 50.0], [-30.0, -30.0], [2.5, 3.5]]          # lost by the flow: klt = 0 whatever the epipolar error
    rc, a1, am, an0, an1 = fo.perform_matching(fo.pyramid(fo.equalize_hist(f0)), fo.pyramid(fo.equalize_hist(f1)), pts, pts, K)
    b1, bm, bn0, bn1, its = c.perform_matching(pts, pts)
    assert rc == 0
    assert np.array_equal(a1, b1) and np.array_equal(an0, bn0) and np.array_equal(an1, bn1)
    assert np.array_equal(am, bm), int((am != bm).sum())
    assert 512 < int(bm.sum()) < 600 and not bm[:2].any()
    c.close()


# fx fy cx cy k1 k2 p1 p2
LENSES = {
    "default": None,
    "tangential": (458.654, 457.296, 367.215, 248.375, 0.0, 0.0, 1.5e-3, -2.5e-3),
    "wide": (200.0, 200.0, 376.0, 240.0, -0.4, 0.02, 0.0, 0.0),
}


@pytest.mark.parametrize("lens", list(LENSES))
def test_undistort_bit_exact_at_block_edges(pkg, fo, lens):
    """plv_undistort against the oracle at n around the 64-thread block and at 1000, points out to 50 px beyond the image.  The wide
    lens' 1 + k1 r^2 + k2 r^4 is negative for a normalised radius between about 1.7 and 4.1: cv::undistortPoints gives such a point back
    as it came, and the image corners (radius 2.2) are among them."""
    w, h = 752, 480
    cfg = pkg.default_config(w, h)
    if LENSES[lens] is not None:
        for i, v in enumerate(LENSES[lens]):
            cfg.intrinsics[i] = v
    c = pkg.Context(cfg)
    K = np.array(list(cfg.intrinsics))
    rng = np.random.default_rng(3)
    uv = np.column_stack([rng.uniform(-50, w + 50, 1000), rng.uniform(-50, h + 50, 1000)]).astype(np.float32)
    uv[:4] = [[-50, -50], [w + 50, h + 50], [K[2], K[3]], [0, h]]
    ref = fo.undistort(K, uv)
    plain = np.column_stack([(uv[:, 0].astype(np.float64) - K[2]) * (1.0 / K[0]),
                             (uv[:, 1].astype(np.float64) - K[3]) * (1.0 / K[1])]).astype(np.float32)
    fell_back = (ref == plain).all(axis=1) & (np.hypot(plain[:, 0], plain[:, 1]) > 1e-3)
    if lens == "wide":
        r = np.hypot(plain[:, 0].astype(np.float64), plain[:, 1])
        assert fell_back[(r > 1.75) & (r < 4.0)].all() and not fell_back[r < 0.5].any()
        assert 50 < fell_back.sum() < 950
    else:
        assert not fell_back.any()
    for n in (1, 63, 64, 65, 1000):
        got = c.undistort(uv[:n])
        assert np.array_equal(got.view(np.int32), ref[:n].view(np.int32)), (n, np.flatnonzero((got != ref[:n]).any(axis=1))[:10])
    c.close()
