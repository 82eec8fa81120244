"""The case matrix of the two-view RANSAC gate (ransac_hyp_kernel / ransac_select_kernel, K7).

Every case is a dict: `m1`, `m2` (float32 [n][2], normalised coordinates), `thr`, `seed`, `conf`, `max_iters`, and what the case is
there for: `reach` (slots of the oracle's trace that must count at least once; oracle_lib.RANSAC_TRACE names them), `never` (slots that
must stay at zero), `trace` (slots with an exact value), `iters` (the adaptive loop's iteration count) and `inliers`.  The numbers were
found by running the CPU oracle and are written here as literals; tests/test_ransac_cases_cpu.py proves on the oracle alone that every
case still does what it says, tests/test_gpu_ransac.py holds the device to the oracle on all of them.  Nothing here needs a GPU or the
oracle.

Branches no case reaches (searched for, see SEARCHED below): the `xr` clamp of the three-root branch and the non-finite model.
"""
import numpy as np

THR = 2.0 / 458.654          # 2 px at the default focal length
PX = 1.0 / 458.0


def two_view(n, seed, outliers, noise_px=0.3, rot=0.05, trans=(0.3, 0.05, 0.1), planar=False):
    """n correspondences of a scene 4 .. 12 m in front of two cameras, 0.3 px of noise, `outliers` of them moved by up to 0.2"""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(4, 12, n)])
    if planar:
        X[:, 2] = 8.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    th = rot
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    X2 = X @ R.T + np.array(trans)
    m1, m2 = X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]
    m1 = m1 + rng.normal(0, noise_px / 458, m1.shape)
    m2 = m2 + rng.normal(0, noise_px / 458, m2.shape)
    bad = rng.choice(n, outliers, replace=False)
    m2[bad] += rng.uniform(-0.2, 0.2, (outliers, 2))
    return m1.astype(np.float32), m2.astype(np.float32)


def grid_7x5():
    """35 points on a 7 x 5 grid of multiples of 1/8: every row, column and diagonal is a collinear triple"""
    gx, gy = np.meshgrid(np.arange(7) - 3.0, np.arange(5) - 2.0)
    return (np.column_stack([gx.ravel(), gy.ravel()]) / 8.0).astype(np.float32)


def _noisy(m, px, seed):
    return (m.astype(np.float64) + np.random.default_rng(seed).normal(0, px * PX, m.shape)).astype(np.float32)


def _ulp_up(m, share, seed):
    """`share` of the coordinates one float32 step up: the smallest difference two images can have"""
    m = m.copy()
    sel = np.random.default_rng(seed).random(m.shape) < share
    m[sel] = np.nextafter(m[sel], np.float32(10))
    return m


def _case(name, m1, m2, thr=THR, seed=0, conf=0.999, max_iters=1000, **expect):
    m1, m2 = np.ascontiguousarray(m1, dtype=np.float32), np.ascontiguousarray(m2, dtype=np.float32)
    assert m1.shape == m2.shape and m1.shape[1] == 2
    c = dict(name=name, m1=m1, m2=m2, thr=float(thr), seed=int(seed), conf=float(conf), max_iters=int(max_iters), reach=(), never=(),
             trace={}, iters=None, inliers=None)
    assert set(expect) <= {"reach", "never", "trace", "iters", "inliers"}, expect
    c.update(expect)
    return c


# ---------------------------------------------------------------------------------------------- sizes
# (n, inliers, iterations): 25 % outliers (two of them below n = 12).  n = 8, 9 draw duplicates all the time; n <= 512 is counted on the
# eight points a lane holds in registers, 513 sends lane 0 into the tail loop, 1100 every lane for more than one round.
SIZE_NS = (7, 8, 9, 10, 12, 63, 64, 65, 511, 512, 513, 600, 1100)
SIZES = {7: (7, 1), 8: (8, 2), 9: (8, 12), 10: (9, 11), 12: (10, 21), 63: (42, 115), 64: (49, 41), 65: (50, 44), 511: (388, 104),
         512: (346, 104), 513: (385, 49), 600: (419, 82), 1100: (794, 64)}


def _size_cases():
    out = []
    for n in SIZE_NS:
        inl, it = SIZES.get(n, (None, None))
        out.append(_case(f"size-{n}", *two_view(n, 100 + n, max(2, round(0.25 * n))), inliers=inl, iters=it))
    return out


# ---------------------------------------------------------------------------------------------- stops of the adaptive loop
# (n, outliers, data seed) -> iterations used at conf 0.999 and a cap of 1000: one hypothesis; inside the first pass of 64; exactly at,
# one behind, one before the pass borders; the cap.
STOPS = {1: (40, 0, 7), 11: (40, 0, 0), 64: (100, 20, 24), 65: (100, 30, 13), 127: (250, 75, 29), 128: (64, 19, 33), 129: (100, 30, 35),
         1000: (40, 20, 1)}


def _stop_cases():
    return [_case(f"stop-{it}", *two_view(n, s, o), iters=it) for it, (n, o, s) in STOPS.items()]


# (n, outliers, data seed) -> (inliers, iterations): two models of the winning hypothesis reach the same count with different inliers.
# The loop keeps the first of them (`good > best`, not `>=`).
SLOT_TIES = {(10, 3, 20): (8, 29), (11, 2, 10): (9, 25), (14, 3, 50): (11, 34)}


def _tie_cases():
    return [_case(f"slot-tie-{n}", *two_view(n, s, o), inliers=inl, iters=it) for (n, o, s), (inl, it) in SLOT_TIES.items()]


# one 40 %-outlier set under other caps and confidences: (setting) -> (inliers, iterations)
SET40 = (100, 40, 7)
CAPS = {1: (21, 1), 2: (21, 2), 63: (47, 63), 64: (47, 64), 65: (47, 65), 128: (49, 128), 129: (49, 129), 2000: (57, 350)}
CONFS = {0.0: (21, 1), 0.5: (49, 102), 0.99: (57, 288), 0.999999: (59, 548), 1.0: (59, 1000)}


def _setting_cases():
    n, o, s = SET40
    m1, m2 = two_view(n, s, o)
    out = [_case(f"cap-{k}", m1, m2, max_iters=k, inliers=inl, iters=it) for k, (inl, it) in CAPS.items()]
    out += [_case(f"conf-{k}", m1, m2, conf=k, inliers=inl, iters=it) for k, (inl, it) in CONFS.items()]
    return out


# ---------------------------------------------------------------------------------------------- nothing found, everything found
def _extreme_cases():
    rng = np.random.default_rng(11)
    a, b = rng.uniform(-0.6, 0.6, (100, 2)), rng.uniform(-0.6, 0.6, (100, 2))
    clean = two_view(100, 12, 0, noise_px=0.0)
    return [
        _case("unrelated-100", a, b, **EXTREME.get("unrelated-100", {})),
        # nine unrelated points: a hypothesis explains its own seven and no more.  Seven is the least the loop accepts.
        _case("unrelated-9", a[:9], b[:9], **EXTREME.get("unrelated-9", {})),
        _case("outliers-90", *two_view(100, 13, 90), **EXTREME.get("outliers-90", {})),
        _case("thr-0", *two_view(100, 14, 25), thr=0.0, **EXTREME.get("thr-0", {})),
        # a threshold below the sample's own rounding error: counts of 1 .. 6 occur, and none of them may become a mask
        _case("thr-tiny", *two_view(100, 14, 25), thr=1e-17, **EXTREME.get("thr-tiny", {})),
        # the same at a threshold that lets exactly the sample through: a best of seven is a mask of seven
        _case("thr-1e-16", *two_view(100, 14, 25), thr=1e-16, **EXTREME.get("thr-1e-16", {})),
        _case("thr-10-noiseless", *clean, thr=10.0, **EXTREME.get("thr-10-noiseless", {})),
    ]


EXTREME = {
    "unrelated-100": dict(inliers=10, iters=1000),
    "unrelated-9": dict(inliers=7, iters=37),
    "outliers-90": dict(inliers=14, iters=1000),
    "thr-0": dict(inliers=0, iters=1000),
    "thr-tiny": dict(inliers=0, iters=1000),
    "thr-1e-16": dict(inliers=7, iters=1000),
    "thr-10-noiseless": dict(inliers=100, iters=1, reach=("three",), trace=dict(hypotheses=1)),
}


# ---------------------------------------------------------------------------------------------- degenerate geometry
def _degenerate_cases():
    m1 = two_view(250, 21, 0)[0]
    g = grid_7x5()
    rot = two_view(250, 22, 0, noise_px=0.0, trans=(0, 0, 0))
    rotn = two_view(250, 22, 60, noise_px=0.3, trans=(0, 0, 0))
    rng = np.random.default_rng(23)
    line1 = np.column_stack([rng.uniform(-0.5, 0.5, 60), np.full(60, 0.25)])
    line2 = rng.uniform(-0.5, 0.5, (60, 2))
    th, s = 0.3, 1.1
    sim = s * g.astype(np.float64) @ np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T + np.array([0.05, -0.02])
    ten = two_view(10, 24, 0)
    D = DEGENERATE
    return [
        _case("identical", m1, m1.copy(), **D.get("identical", {})),
        _case("grid-shift", g, g + np.float32([0.125, 0.0]), **D.get("grid-shift", {})),
        # one coordinate in fifty a float step off: most samples still fail the rank test, some pass it with a last pivot between
        # 1e-14 and 1e-10, the first that passes takes every point
        _case("identical-ulp", m1, _ulp_up(m1, 0.02, 2), **D.get("identical-ulp", {})),
        _case("identical-noise-1e-4", m1, _noisy(m1, 1e-4, 25), **D.get("identical-noise-1e-4", {})),
        _case("identical-noise-0.05", m1, _noisy(m1, 0.05, 26), **D.get("identical-noise-0.05", {})),
        _case("rotation", *rot, **D.get("rotation", {})),
        _case("rotation-noise", *rotn, **D.get("rotation-noise", {})),
        _case("planar", *two_view(250, 27, 60, planar=True), **D.get("planar", {})),
        _case("one-line", line1, line2, **D.get("one-line", {})),
        _case("grid-similarity", g, sim, **D.get("grid-similarity", {})),
        _case("ten-repeated", np.tile(ten[0], (20, 1)), np.tile(ten[1], (20, 1)), **D.get("ten-repeated", {})),
    ]


# identical images and a pure shift on a grid: the constraint matrix has rank 6, every hypothesis fails the rank test at elimination
# step 6, no track survives.  (What the reference does there too; recorded, not endorsed.)
DEGENERATE = {
    "identical": dict(inliers=0, iters=1000, trace=dict(rank_fail=1000, rank_step=6, retry=0, no_subset=0)),
    "grid-shift": dict(inliers=0, iters=1000, reach=("retry",), trace=dict(rank_fail=1000, rank_step=6, no_subset=0)),
    "identical-ulp": dict(inliers=250, iters=8, reach=("rank_fail", "three", "f8_zero"), trace=dict(rank_fail=7, rank_step=6)),
    "identical-noise-1e-4": dict(inliers=250, iters=1, trace=dict(rank_fail=0, hypotheses=1)),
    "identical-noise-0.05": dict(inliers=250, iters=1, trace=dict(rank_fail=0, hypotheses=1)),
    "rotation": dict(inliers=250, iters=1, trace=dict(rank_fail=0, hypotheses=1)),
    "rotation-noise": dict(inliers=195, iters=36),
    "planar": dict(inliers=192, iters=40),
    "one-line": dict(inliers=0, iters=1000, trace=dict(retry=16000, no_subset=1000, rank_fail=0)),
    "grid-similarity": dict(inliers=35, iters=1, reach=("three",), trace=dict(retry=3, no_subset=0)),
    "ten-repeated": dict(inliers=200, iters=3, reach=("retry", "no_subset")),
}


# ---------------------------------------------------------------------------------------------- bad rows
def nan_rows():
    m1, m2 = two_view(100, 31, 20)
    m2 = m2.copy()
    m2[::9] = np.nan
    return m1, m2


def _nan_cases():
    return [_case("nan-rows", *nan_rows(), **NAN_ROWS)]


# every ninth row of m2 is NaN: the pivot scan never picks a NaN, a sample with a bad row fails the rank test (at step 5: the row's
# three finite entries are used up), the rest of the loop goes on
NAN_ROWS = dict(inliers=66, iters=123, reach=("rank_fail", "three", "one"), trace=dict(rank_fail=82, rank_step=5))

# ---------------------------------------------------------------------------------------------- crafted seven-point samples
# n == 7: the sample is rows 0 .. 6, one hypothesis.  Found by random search over dyadic coordinates (multiples of 1/4 in [-2, 2], m2 a
# copy, mirror or transpose of m1 with one to four rows moved): (branch, m1, m2).
CRAFTED = [
    ("c1_zero", [1.75, -1.25, 2.0, -0.5, -1.0, -1.5, 0.5, 2.0, 2.0, -1.5, -1.5, -1.0, -0.25, 0.5],
     [-1.25, 1.75, -0.5, 2.0, -1.5, -1.0, 2.0, 0.5, -1.5, 2.0, -1.0, -1.5, 0.0, 2.0]),
    ("c1_zero", [-2.0, -1.5, -1.5, 1.0, 2.0, 2.0, -0.5, 2.0, 0.0, 2.0, -0.5, 1.0, -0.5, -0.5],
     [-2.0, -1.5, -1.5, 1.0, 2.0, 2.0, -0.5, 2.0, 0.0, 2.0, -0.5, 1.0, -1.5, -0.5]),
    ("c1_zero", [0.75, 0.5, 1.25, -1.75, -0.75, -0.5, 0.5, 1.0, 0.0, -1.0, 1.75, -1.25, -1.75, -0.75],
     [-0.75, 0.5, -1.25, -1.75, 0.75, -0.5, -0.5, 1.0, 1.25, -0.25, -1.75, -1.25, 1.75, -0.75]),
    ("c1_zero", [-1.5, -1.75, -0.75, 0.0, -1.0, 0.5, 1.25, 1.25, 1.5, 1.75, 1.0, -2.0, 1.0, 0.0],
     [-1.75, -1.5, 0.0, -0.75, 0.5, -1.0, 0.25, -1.75, 1.75, 1.5, -2.0, 1.0, 0.0, 1.0]),
    ("c1_zero", [0.5, -1.5, 0.5, 0.5, -1.5, 2.0, 1.5, -2.0, 0.5, -2.0, 1.0, 1.0, 1.0, 1.5],
     [0.5, -1.5, 0.5, 0.5, -1.5, 2.0, 1.5, -2.0, 0.5, -2.0, 1.0, 1.0, -0.5, -1.0]),
    ("linear", [-0.5, 1.0, -2.0, -1.0, 2.0, 0.0, 1.5, -1.0, 1.0, 1.0, 0.5, -2.0, 0.0, -0.5],
     [1.0, -0.5, -1.0, -2.0, 0.0, 2.0, -1.0, 1.5, -1.5, -1.0, -2.0, 0.5, -0.5, 0.0]),
    ("linear", [0.0, 1.5, 1.5, 2.0, -1.5, -1.0, -0.5, -0.5, -2.0, 2.0, 0.0, 2.0, -2.0, -1.0],
     [0.0, 1.5, 1.5, 2.0, -1.5, -1.0, -0.5, -0.5, 0.0, 1.0, 0.0, 2.0, -2.0, -1.0]),
    ("linear", [2.0, -1.25, -1.25, 2.0, 0.75, -1.0, -2.0, 1.5, 0.25, -2.0, 0.75, 0.0, 0.5, 1.25],
     [0.75, 1.0, 2.0, -1.25, -1.0, 0.75, 1.5, -2.0, -2.0, 0.25, 0.0, 0.75, 1.25, 0.5]),
    ("linear", [2.0, -2.0, 1.5, 0.0, 1.0, -1.5, 1.5, 2.0, 1.5, -1.5, 1.0, -1.0, -0.5, -1.0],
     [2.0, -2.0, 1.5, 0.0, 1.0, -1.5, 1.5, 2.0, 1.5, -1.5, 1.0, -1.0, 0.0, 0.0]),
    ("linear", [2.0, -2.0, -1.0, -1.5, -0.5, 1.0, -1.0, -1.0, -1.0, -1.0, 0.0, -1.0, 1.0, -2.0],
     [2.0, -2.0, -1.0, -1.5, -0.5, 1.0, -1.0, -1.0, -2.0, 0.5, 0.0, -1.0, 1.0, -2.0]),
    ("quad_neg", [-1.0, -2.0, -0.5, 1.0, -1.5, -1.0, -1.0, 2.0, 0.5, 1.5, 0.0, -1.5, 0.0, 2.0],
     [-2.0, -1.0, 1.0, -0.5, -1.0, -1.5, 2.0, -1.0, -1.5, 1.0, -1.5, 0.0, 2.0, 0.5]),
    ("quad_neg", [0.0, -1.25, -0.5, 1.75, -2.0, -1.0, -0.5, -0.75, 0.75, -2.0, 1.25, 0.5, 0.0, 0.25],
     [0.0, -1.25, -0.5, 1.75, -2.0, -1.0, -0.5, -0.75, 2.0, -1.25, 1.25, 0.5, 0.0, 0.25]),
    ("quad_neg", [0.5, 0.25, 1.0, 1.0, 1.5, 0.0, 2.0, 0.5, 0.0, -0.25, 0.0, 0.25, 1.5, 2.0],
     [-1.5, -0.75, 1.0, 1.0, 1.5, 0.0, 2.0, 0.5, 0.0, -0.25, 0.0, 0.25, 1.5, 2.0]),
    ("quad", [1.25, 1.0, -0.5, 1.75, -1.75, -0.75, 1.5, 1.5, 2.0, 2.0, -0.25, -1.0, -0.75, -0.25],
     [1.5, 0.5, 1.75, -0.5, -0.75, -1.75, 1.5, 1.5, 2.0, 2.0, -1.0, -0.25, -0.25, -0.75]),
    ("quad", [2.0, -0.5, 0.5, 2.0, -0.5, -2.0, -2.0, 2.0, 0.0, -2.0, 1.5, -1.5, 0.5, 0.5],
     [1.0, 2.0, 0.5, 2.0, -0.5, -2.0, -2.0, 2.0, 0.0, -2.0, 1.5, -1.5, 0.5, 0.5]),
    ("quad", [-0.25, -2.0, 1.5, 0.0, 1.25, -1.75, -1.5, 1.5, 1.75, -1.75, 1.75, 0.25, -0.5, -0.75],
     [-2.0, -0.25, 0.0, 1.5, -1.75, 1.25, -1.75, 1.5, -1.75, 1.75, 0.25, 1.75, -0.75, -0.5]),
    ("quad", [2.0, 1.75, 0.25, 0.75, -2.0, -2.0, 0.0, 0.5, -0.25, -0.75, -2.0, 2.0, 2.0, 1.25],
     [2.0, 1.75, 0.25, 0.75, -2.0, -2.0, 0.0, 0.5, -0.25, -0.75, -1.75, -0.75, 2.0, 1.25]),
    ("quad", [2.0, 1.5, 0.5, -0.5, -1.0, 0.0, 1.0, -1.0, 1.0, 0.0, -1.0, -1.5, 0.5, -1.0],
     [2.0, 1.5, 0.5, -0.5, -1.0, 0.0, 1.0, -1.0, 1.0, 0.0, -1.0, -1.5, -1.0, 0.5]),
    ("quad", [-1.5, 2.0, -1.0, 0.5, 1.5, 2.0, 0.0, 2.0, 1.0, 2.0, -1.5, -1.5, -2.0, -1.0],
     [1.0, 0.5, 1.0, 0.5, -1.5, 2.0, -0.0, 2.0, 1.0, 0.5, 0.5, -2.0, 2.0, 0.0]),
    ("double", [1.75, 1.5, 0.0, -0.75, -0.25, 1.75, -1.75, -1.5, 1.75, 1.75, -2.0, 0.5, -1.0, 1.25],
     [1.75, -1.25, 0.0, -0.75, -0.25, 1.75, -1.75, -1.5, 1.75, 1.75, -2.0, 0.5, -1.0, 1.25]),
    ("double", [0.25, -1.0, -0.75, 2.0, -1.0, -0.75, -2.0, 0.5, 0.25, 0.5, -0.75, 1.0, -0.25, 1.75],
     [-1.0, 0.25, 2.0, -0.75, 2.0, -1.25, 0.5, -2.0, 0.5, 0.25, 1.0, -0.75, 1.75, -0.25]),
    ("double", [-1.0, 0.5, 0.0, 0.5, -2.0, 0.5, 1.5, 0.0, -2.0, -0.5, -0.5, 0.0, 2.0, 1.0],
     [0.5, -1.0, 0.5, 0.0, 0.5, -2.0, 0.0, 1.5, -0.5, 1.5, 0.0, -0.5, 1.0, 2.0]),
    ("double", [2.0, 0.0, -1.5, 1.0, -2.0, 0.5, 2.0, 0.0, 2.0, 0.0, -0.5, -1.5, 0.5, 1.0],
     [1.9999998807907104, 2.5008036530493882e-08, -1.5, 1.0000001192092896, -2.0, 0.5, -0.5000000596046448, 0.49999985098838806, 2.000000238418579, -1.7658378226315108e-07, 7.258137912913298e-08, -1.5000001192092896, 0.49999991059303284, 1.0]),
    ("double", [1.0, 1.5, -2.0, 1.5, 1.0, 1.0, 1.0, -2.0, 0.0, 1.0, -1.0, -1.5, -0.5, 1.5],
     [-1.0, 1.5, -1.0, 0.0, -1.0, 1.0, -1.0, -2.0, -0.0, 1.0, -1.0, 1.5, 0.5, 1.5]),
    ("double", [-1.5, -0.5, 0.0, -0.25, 1.25, 0.25, 0.5, 1.25, -0.5, 2.0, -1.5, 0.75, -1.75, -1.5],
     [1.5, -0.5, -0.0, -0.25, 0.5, 1.0, -0.5, 1.25, 0.5, 2.0, 1.5, 0.75, 1.75, -1.5]),
    ("f8_zero", [1.25, -0.5, 0.0, 0.0, -0.25, 0.0, 2.0, -1.0, 1.75, -1.25, -1.75, -0.75, -1.0, 0.5],
     [1.25, -0.5, 0.0, 0.0, -0.25, 0.0, 2.0, -1.0, 1.75, -1.25, -1.75, -0.75, 1.25, 0.25]),
    ("f8_zero", [0.25, 1.75, -0.75, -1.75, -0.25, 0.5, -1.25, 2.0, 0.0, 0.0, 0.25, 0.25, -0.25, 0.25],
     [-2.0, -2.0, 0.75, -1.75, 1.75, -2.0, -1.5, 0.5, -0.0, 0.0, -0.25, 0.25, -2.0, -1.0]),
    ("f8_zero", [-1.0, 0.25, 0.5, -1.25, -1.25, 0.25, -0.5, 0.0, -1.25, -0.25, -1.0, 0.25, 0.5, 0.0],
     [0.5, -1.0, -0.5, -1.25, 1.25, 0.25, 0.5, 0.0, -0.25, 0.0, 1.0, 0.25, -0.5, 0.0]),
    ("f8_zero", [0.25, -0.75, -0.25, -1.0, 0.25, 1.5, 0.5, -0.25, 0.75, -1.5, 1.5, -0.5, -1.5, -0.75],
     [0.25, -0.75, 1.25, 0.75, 1.5, -1.5, 0.5, -0.25, 0.75, -1.5, 1.5, -0.5, -1.5, -0.75]),
    ("f8_zero", [1.25, 1.0, -0.5, 1.75, -1.75, -0.75, 1.5, 1.5, 2.0, 2.0, -0.25, -1.0, -0.75, -0.25],
     [1.5, 0.5, 1.75, -0.5, -0.75, -1.75, 1.5, 1.5, 2.0, 2.0, -1.0, -0.25, -0.25, -0.75]),
    ("f8_zero", [0.0, -1.5, 0.0, 0.5, 2.0, 1.5, 1.5, 0.5, 1.5, 2.0, -2.0, 0.0, -2.0, 1.0],
     [0.0, -1.5, 0.0, 0.5, 2.0, 1.5, 1.5, 0.5, 1.5, 2.0, -2.0, 0.0, -1.5, 1.5]),
    ("f8_zero", [2.0, -0.5, -0.5, -0.25, -1.75, 1.0, -0.25, -0.25, 1.5, 1.25, -0.25, 0.0, 0.5, -0.5],
     [-2.0, -0.5, 0.5, -0.25, 1.75, 1.0, 0.25, -0.25, -0.75, 1.5, 0.25, 0.0, -0.5, -0.5]),
    # d == 0 with R == 0 and a1 == 0: the two roots are -0.0 and +0.0 in this order, which only the models' bits can tell
    ("double", [1.5, -2.0, 1.0, 1.0, 1.5, 1.5, -0.5, 1.0, -1.5, -1.5, 0.5, -2.0, 0.0, 0.0],
     [-2.0, 1.5, 1.0, 1.0, -1.0, -1.0, 1.0, -0.5, -1.5, -1.5, -2.0, 0.5, 0.0, 0.0]),
    ("double", [1.0, 0.25, -2.0, -0.25, -1.5, 0.0, 0.25, -0.75, 1.75, 1.75, 0.25, -1.75, 1.0, 2.0],
     [-1.0, 0.25, 2.0, -0.25, 1.5, 0.5, -0.25, -0.75, -1.75, 1.75, -0.25, -1.75, -1.0, 2.0]),
    ("double", [1.5, 2.0, -0.5, -1.5, 0.5, 2.0, 1.0, 0.0, 2.0, 0.5, -1.5, 0.5, -2.0, 1.0],
     [1.5, 2.0, -0.5, -1.5, 0.5, 2.0, 1.0, 0.0, -0.5, -0.5, -1.5, 0.5, -2.0, 1.0]),
]
SEARCHED = ("1.7 million such draws (one in seven of the first 300 000 with m2 perturbed by 1e-7) and the 1000 hypotheses of every case "
            "above: the xr clamp and the non-finite model were never reached")


def _crafted_cases():
    out = []
    for k, (branch, a, b) in enumerate(CRAFTED):
        out.append(_case(f"crafted-{branch}-{k}", np.float32(a).reshape(7, 2), np.float32(b).reshape(7, 2), reach=(branch,), iters=1))
    return out


def nhyp(case):
    """hypotheses to compare one by one: the case's cap, at most 1000; the one there is for n == 7"""
    return 1 if len(case["m1"]) == 7 else min(case["max_iters"], 1000)


_all = None


def cases():
    global _all
    if _all is None:
        _all = (_size_cases() + _stop_cases() + _tie_cases() + _setting_cases() + _extreme_cases() + _degenerate_cases() + _nan_cases() +
                _crafted_cases())
        names = [c["name"] for c in _all]
        assert len(set(names)) == len(names)
    return _all
