"""The case matrix of point and line triangulation (test infrastructure; tests/test_triangulation_cases_cpu.py proves on the oracle's
trace that the cases reach what they name, tests/test_gpu_triangulation.py runs them on the device).

triangulate_feature and line_triangulate_one (csrc/jacobian_kernels.hip) decide which MSCKF points and lines enter the filter.  The
point batches below walk the inputs on which that code decides something, one option set per batch:

  track length   0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130 valid observations: the lanes stride by 64, the ballot compaction runs
                 over several bases, and up to 16 the refinement takes the four-candidate pass
  invalid obs    times the window does not serve at the first, the last (the anchor is then not the track's last observation), an
                 inner position, all but one, and a block that spans a multiple of 64
  gates          condition number (1e4 and 1e7), linear depth below / above the range, refined depth outside after a linear depth
                 inside, baseline ratio; refinement off.  Every rejection has a neighbour in its batch that passes
  LM exits       small decrease, step below 1e-6, five accepted steps; lam >= 1e10 and a failed solve inside the loop (camera poses no
                 camera ever had, handed in per observation: Raw)
  streaks        failed steps in front of an accepted one, 1 .. 8 and >= 9, for M <= 16 (lane groups 0 .. 3 of the first and second
                 four-candidate pass and the third pass) and for M >= 17 (one candidate at a time)
  window         observations 0, +13 ms, -4 ms off the clone times; cam_dt in the state view

A track is `Trk`: where its landmark lies in the newest camera, how many observations it has, how they are disturbed and when they
were taken.  The streak / exit tracks were found by a seeded search over such tracks on the oracle with its trace on (what was searched:
the docstring of tests/test_triangulation_cases_cpu.py); the module keeps what the search found (FOUND, RAW_TRACKS), the CPU test holds
every one of them to what it names.

The line batches do the same for line_triangulate_one: valid observations 0, 1, 2, 3, 65+; a first observation that is invalid in
both branches; the anchored branch for D = 1, 2, 3; D > 0 without an anchor and D = 0 with one (both plane pairs); every pair under
the 8 degree test, exactly one passing, a mix."""
from collections import namedtuple

import numpy as np

import synth

N_CLONES = 20
DT_CLONE = 0.05
WIDE = dict(min_dist=0.1, max_dist=500.0, max_cond=1e12, max_baseline=1e6, refine=True)   # no gate decides

# where: "clones" = the last M clone times (+ offset on all but the newest), "spread" = M times evenly over the window (between the clones),
# bad: positions (within the track) of observations whose time the window does not serve, bad_t: "past" = 4 ms past the newest clone
# (kept by the pool of the one-call routes, refused by the interpolation), "far" = 5 s before the window
Trk = namedtuple("Trk", "name M depth noise outlier seed where offset bad bad_t expect")


def trk(name, M, depth=8.0, noise=0.3, outlier=0.0, seed=0, where=None, offset=0.0, bad=(), bad_t="past", **expect):
    return Trk(name, M, depth, noise, outlier, seed, where or ("clones" if M <= N_CLONES else "spread"), offset, tuple(bad), bad_t, expect)


Batch = namedtuple("Batch", "name opt tracks cam_dt routes")

# Camera poses handed in per observation (res_R / res_p on the tracks, identity extrinsics) that no camera ever had: the only inputs on
# which the refinement ends at lam >= 1e10 or on a failed 3 x 3 solve.  kind "zero-row": every camera matrix has a zero row (h3 == 0:
# the cost of every step is NaN or inf), "any": arbitrary 3 x 3 matrices.
Raw = namedtuple("Raw", "name kind M seed expect")
NO_GATE = dict(min_dist=-1e300, max_dist=1e300, max_cond=1e300, max_baseline=1e300, refine=True)


def raw(name, kind, M, seed, **expect):
    return Raw(name, kind, M, seed, expect)


def raw_arrays(k):
    """(R_GtoC [M][9], p_CinG [M][3], uvn [M][2]) of a Raw track"""
    rng = np.random.default_rng(30000 + 7919 * k.seed + 31 * k.M)
    if k.kind == "zero-row":
        R = rng.normal(0, 1, (k.M, 3, 3))
        R[:, rng.integers(0, 3)] = 0
        pc = rng.normal(0, 1, (k.M, 3))
    else:
        R = rng.normal(0, 1, (k.M, 3, 3))
        pc = rng.normal(0, 10.0 ** rng.integers(-3, 4), (k.M, 3))
    uvn = rng.normal(0, 10.0 ** rng.integers(-3, 3), (k.M, 2)).astype(np.float32)
    return R.reshape(k.M, 9), pc, uvn


def scene():
    """the window every batch uses: 20 clones 50 ms apart on synth.vio_scene's arc"""
    return synth.vio_scene(n_clones=N_CLONES, F=1, M=3, seed=3, dt_clone=DT_CLONE)


def _track_arrays(sc, k, cam_dt):
    """(times as stamped, uv) of one Trk: the landmark sits at `depth` in front of the newest camera, inside the image"""
    rng = np.random.default_rng(10000 + 7919 * k.seed + 31 * k.M)
    t = sc["t"]
    n = k.M
    if k.where == "clones":
        idx = np.arange(N_CLONES - n, N_CLONES)
        times = t[idx] + np.where(idx < N_CLONES - 1, k.offset, 0.0)
    else:
        times = np.linspace(t[0] + 0.002, t[-1], n)
    R_l, p_l = sc["pose_fn"](t[-1])
    xn = np.array([rng.uniform(-0.35, 0.35), rng.uniform(-0.25, 0.25)])
    pc = np.array([xn[0], xn[1], 1.0]) * k.depth
    pG = R_l.T @ (sc["R_ItoC"].T @ (pc - sc["p_IinC"])) + p_l
    uv = np.zeros((n, 2))
    for i, tm in enumerate(times):
        R, p = sc["pose_fn"](tm)
        q = sc["R_ItoC"] @ (R @ (pG - p)) + sc["p_IinC"]
        uv[i] = synth.radtan_distort(sc["K8"], q[:2] / q[2]) + rng.normal(0, k.noise, 2)
    if k.outlier:
        j = int(rng.integers(0, n))
        ang = rng.uniform(0, 2 * np.pi)
        uv[j] += k.outlier * np.array([np.cos(ang), np.sin(ang)])
    times = times.copy()
    for j in k.bad:
        times[j] = t[-1] + 0.004 if k.bad_t == "past" else t[0] - 5.0
    return times - cam_dt, uv


def build(pkg, batch, undistort, sc=None):
    """The batch as the C-ABI takes it: dict(batch, sc, st, tr, n_valid [F]); undistort = FrontOracle.undistort"""
    sc = sc or scene()
    if batch.tracks and isinstance(batch.tracks[0], Raw):
        parts = [raw_arrays(k) for k in batch.tracks]
        ptr = np.concatenate([[0], np.cumsum([k.M for k in batch.tracks])]).astype(np.int32)
        uvn = np.concatenate([x[2] for x in parts])
        uv = (uvn * sc["K8"][:2] + sc["K8"][2:4]).astype(np.float32)
        st = pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], np.eye(3), np.zeros(3), sc["K8"], intrinsic_state_id=15)
        tr = pkg.Tracks(ptr, np.concatenate([sc["t"][N_CLONES - k.M:] for k in batch.tracks]), uv, np.zeros((len(parts), 3)), obs_uvn=uvn,
                        res_R=np.concatenate([x[0] for x in parts]), res_p=np.concatenate([x[1] for x in parts]))
        return dict(batch=batch, sc=sc, st=st, tr=tr, n_valid=np.array([k.M for k in batch.tracks]))
    T, UV = [], []
    for k in batch.tracks:
        a, b = _track_arrays(sc, k, batch.cam_dt)
        T.append(a), UV.append(b)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in T])]).astype(np.int32)
    t_all, uv_all = np.concatenate(T), np.concatenate(UV).astype(np.float32)
    uvn = undistort(sc["K8"], uv_all)
    st = pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], sc["R_ItoC"], sc["p_IinC"], sc["K8"], intrinsic_state_id=15, cam_dt=batch.cam_dt)
    tr = pkg.Tracks(ptr, t_all, uv_all, np.zeros((len(T), 3)), obs_uvn=uvn)
    n_valid = np.array([k.M - len(k.bad) for k in batch.tracks])
    return dict(batch=batch, sc=sc, st=st, tr=tr, n_valid=n_valid)


def perturbed_state(pkg, sc, rep, cam_dt=0.0):
    """the scene's state view with relative noise of 2^-52 on its camera poses (clone rotations and positions), seeded by `rep`"""
    rng = np.random.default_rng(500 + rep)
    eps = 2.0 ** -52
    R = sc["R"] * (1 + eps * rng.choice([-1.0, 0.0, 1.0], sc["R"].shape))
    p = sc["p"] * (1 + eps * rng.choice([-1.0, 0.0, 1.0], sc["p"].shape))
    return pkg.StateView(sc["t"], R, p, sc["ids"], sc["R_ItoC"], sc["p_IinC"], sc["K8"], intrinsic_state_id=15, cam_dt=cam_dt)


# ------------------------------------------------------------------ point batches
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130)


def _length_tracks(bad_t="far", lengths=LENGTHS):
    out = []
    for n in lengths:
        if n == 0:
            out.append(trk("valid-0", 3, bad=(0, 1, 2), bad_t=bad_t, stage="too few observations"))
        elif n == 1:
            out.append(trk("valid-1", 3, bad=(0, 2), bad_t=bad_t, stage="too few observations"))
        else:
            out.append(trk(f"valid-{n}", n, seed=n, stage="accepted"))
            out.append(trk(f"valid-{n}-far", n, depth=25.0, seed=100 + n, stage="accepted"))
    return out


def _invalid_tracks(bad_t, longs):
    """invalid observations at every position: (M, bad positions)"""
    spec = [("first", 9, (0,)), ("last", 9, (8,)), ("inner", 9, (4,)), ("first-last", 16, (0, 15)), ("inner-two", 17, (3, 9)),
            ("all-but-one", 6, (0, 1, 2, 4, 5)), ("all-but-two", 6, (0, 2, 3, 5)), ("last-three", 18, (15, 16, 17)), ("17-to-16", 17, (5,))]
    if longs:
        spec += [("block-60-70", 130, tuple(range(60, 70))), ("block-0-64", 130, tuple(range(0, 64))), ("block-120-130", 130, tuple(range(120, 130))),
                 ("65-last", 65, (64,)), ("65-first", 65, (0,)), ("80-to-16", 80, tuple(range(8, 72)))]
    return [trk(f"invalid-{name}", M, seed=40 + i, bad=bad, bad_t=bad_t, stage="too few observations" if M - len(bad) < 2 else "accepted")
            for i, (name, M, bad) in enumerate(spec)]


def _gate_tracks():
    cond4 = [trk("cond-pass-5m", 12, depth=5.0, seed=1, stage="accepted"), trk("cond-fail-60m", 12, depth=60.0, seed=2, stage="condition number"),
             trk("cond-pass-3m", 16, depth=3.0, seed=3, stage="accepted"), trk("cond-fail-120m", 18, depth=120.0, seed=4, stage="condition number"),
             trk("cond-fail-200m", 5, depth=200.0, noise=0.1, seed=5, stage="condition number")]
    cond7 = [trk("cond-pass-60m", 12, depth=60.0, noise=0.1, seed=2, stage="accepted"), trk("cond-pass-5m", 12, depth=5.0, seed=1, stage="accepted"),
             trk("cond-fail-short-300m", 3, depth=300.0, noise=0.05, seed=6, stage="condition number"),
             trk("cond-fail-two-400m", 2, depth=400.0, noise=0.05, seed=7, stage="condition number")]
    depth = [trk("depth-pass-8m", 12, depth=8.0, seed=1, stage="accepted"), trk("depth-low-2m", 12, depth=2.0, seed=2, stage="linear depth low"),
             trk("depth-high-40m", 12, depth=40.0, noise=0.1, seed=3, stage="linear depth high"), trk("depth-pass-15m", 17, depth=15.0, seed=4, stage="accepted"),
             trk("depth-low-3m", 18, depth=3.0, seed=5, stage="linear depth low")]
    base = [trk("base-pass-8m", 12, depth=8.0, seed=1, stage="accepted"), trk("base-fail-45m", 19, depth=45.0, noise=0.05, seed=2, stage="baseline ratio"),
            trk("base-fail-short", 4, depth=12.0, noise=0.05, seed=3, stage="baseline ratio"), trk("base-pass-5m", 17, depth=5.0, seed=4, stage="accepted")]
    return cond4, cond7, depth, base


# Found by a seeded search on the oracle with its trace on (what was searched: the docstring of tests/test_triangulation_cases_cpu.py;
# seeds 0 .. 2999): (M, depth, noise, outlier, seed) -> what the refinement does.  `streak` is the length of the failed-step streak in
# front of an accepted step that the track was chosen for.  Kept are tracks whose trace 2^-52 noise on the poses does not change.
FOUND = {
    "exit": [
        (3, 5.0, 1.0, 0.0, 193, {'stage': 'accepted', 'exit': 'five runs'}), (3, 5.0, 1.0, 0.0, 222, {'stage': 'accepted', 'exit': 'five runs'}),
        (2, 5.0, 0.3, 0.0, 225, {'stage': 'accepted', 'exit': 'five runs'}), (2, 40.0, 0.3, 0.0, 112, {'stage': 'accepted', 'exit': 'five runs'}),
        (2, 5.0, 0.0, 0.0, 5, {'stage': 'accepted', 'exit': 'small step'}), (2, 5.0, 0.0, 0.0, 0, {'stage': 'accepted', 'exit': 'small decrease'}),
        (17, 5.0, 0.0, 0.0, 2, {'stage': 'accepted', 'exit': 'small step'}), (17, 5.0, 0.0, 0.0, 0, {'stage': 'accepted', 'exit': 'small decrease'}),
    ],
    "streak-spec": [
        (16, 5.0, 0.3, 0.0, 34, {'stage': 'accepted', 'streak': 1}), (15, 5.0, 0.3, 0.0, 45, {'stage': 'accepted', 'streak': 1}),
        (3, 5.0, 0.3, 0.0, 46, {'stage': 'accepted', 'streak': 1}), (16, 5.0, 0.3, 0.0, 24, {'stage': 'accepted', 'streak': 2}),
        (15, 5.0, 0.3, 0.0, 1, {'stage': 'accepted', 'streak': 2}), (3, 5.0, 0.3, 0.0, 0, {'stage': 'accepted', 'streak': 2}),
        (16, 5.0, 0.3, 0.0, 3, {'stage': 'accepted', 'streak': 3}), (15, 5.0, 0.3, 0.0, 15, {'stage': 'accepted', 'streak': 3}),
        (3, 5.0, 0.3, 0.0, 26, {'stage': 'accepted', 'streak': 3}), (16, 5.0, 0.3, 0.0, 0, {'stage': 'accepted', 'streak': 4}),
        (15, 5.0, 0.3, 0.0, 3, {'stage': 'accepted', 'streak': 4}), (3, 5.0, 0.3, 0.0, 13, {'stage': 'accepted', 'streak': 4}),
        (16, 5.0, 0.3, 0.0, 1, {'stage': 'accepted', 'streak': 5}), (8, 5.0, 0.3, 0.0, 2, {'stage': 'accepted', 'streak': 5}),
        (16, 5.0, 0.3, 0.0, 27, {'stage': 'accepted', 'streak': 6}), (8, 5.0, 0.3, 0.0, 0, {'stage': 'accepted', 'streak': 6}),
        (16, 5.0, 0.3, 0.0, 46, {'stage': 'accepted', 'streak': 7}), (8, 5.0, 0.3, 0.0, 8, {'stage': 'accepted', 'streak': 7}),
        (16, 5.0, 0.3, 0.0, 158, {'stage': 'accepted', 'streak': 8}), (8, 5.0, 0.3, 0.0, 13, {'stage': 'accepted', 'streak': 8}),
        (16, 5.0, 0.3, 80.0, 112, {'stage': 'accepted', 'streak': 9}), (8, 5.0, 0.3, 80.0, 2, {'stage': 'accepted', 'streak': 9}),
        (16, 40.0, 0.3, 80.0, 36, {'stage': 'accepted', 'streak': 10}), (16, 40.0, 0.3, 80.0, 380, {'stage': 'accepted', 'streak': 11}),
        (16, 140.0, 0.3, 80.0, 184, {'stage': 'accepted', 'streak': 12}), (16, 40.0, 1.0, 80.0, 2816, {'stage': 'accepted', 'streak': 13}),
    ],
    "streak-serial": [
        (17, 5.0, 0.3, 0.0, 18, {'stage': 'accepted', 'streak': 1}), (24, 5.0, 0.3, 0.0, 62, {'stage': 'accepted', 'streak': 1}),
        (17, 5.0, 0.3, 0.0, 1, {'stage': 'accepted', 'streak': 2}), (24, 5.0, 0.3, 0.0, 2, {'stage': 'accepted', 'streak': 2}),
        (17, 5.0, 0.3, 0.0, 27, {'stage': 'accepted', 'streak': 3}), (24, 5.0, 0.3, 0.0, 1, {'stage': 'accepted', 'streak': 3}),
        (17, 5.0, 0.3, 0.0, 4, {'stage': 'accepted', 'streak': 4}), (24, 5.0, 0.3, 0.0, 7, {'stage': 'accepted', 'streak': 4}),
        (17, 5.0, 0.3, 0.0, 3, {'stage': 'accepted', 'streak': 5}), (24, 5.0, 0.3, 0.0, 3, {'stage': 'accepted', 'streak': 5}),
        (17, 5.0, 0.3, 0.0, 24, {'stage': 'accepted', 'streak': 6}), (24, 5.0, 0.3, 0.0, 0, {'stage': 'accepted', 'streak': 6}),
        (17, 5.0, 0.3, 0.0, 0, {'stage': 'accepted', 'streak': 7}), (24, 5.0, 0.3, 0.0, 43, {'stage': 'accepted', 'streak': 7}),
        (17, 5.0, 0.3, 0.0, 22, {'stage': 'accepted', 'streak': 8}), (24, 5.0, 0.3, 0.0, 37, {'stage': 'accepted', 'streak': 8}),
        (17, 5.0, 0.3, 80.0, 232, {'stage': 'accepted', 'streak': 9}), (40, 5.0, 0.3, 80.0, 123, {'stage': 'accepted', 'streak': 9}),
        (24, 40.0, 0.3, 80.0, 107, {'stage': 'accepted', 'streak': 10}), (24, 140.0, 0.3, 80.0, 231, {'stage': 'accepted', 'streak': 11}),
        (17, 40.0, 1.0, 80.0, 1519, {'stage': 'accepted', 'streak': 12}), (17, 140.0, 1.0, 80.0, 61, {'stage': 'accepted', 'streak': 13}),
        (17, 40.0, 0.3, 0.0, 38, {'stage': 'accepted', 'streak': 10}), (17, 40.0, 0.3, 80.0, 31, {'stage': 'accepted', 'streak': 10}),
        (17, 40.0, 1.0, 80.0, 43, {'stage': 'accepted', 'streak': 11}),
    ],
    "refined-depth": [
        (17, 19.8, 1.0, 0.0, 8, {'stage': 'refined depth high', 'linear_inside': True}),
        (8, 19.9, 0.3, 0.0, 1, {'stage': 'refined depth high', 'linear_inside': True}),
        (12, 19.9, 0.3, 0.0, 3, {'stage': 'refined depth high', 'linear_inside': True}),
    ],
    "refined-low": [
        (2, 40.0, 0.3, 0.0, 580, {'stage': 'refined depth low', 'linear_inside': True}),
        (17, 40.0, 0.0, 80.0, 59, {'stage': 'refined depth low', 'linear_inside': True}),
        (17, 40.0, 0.0, 80.0, 549, {'stage': 'refined depth low', 'linear_inside': True}),
    ],
}


def found_tracks(kind):
    return [trk(f"{kind}-{i}", M, depth=d, noise=nz, outlier=o, seed=s, **ex) for i, (M, d, nz, o, s, ex) in enumerate(FOUND.get(kind, []))]


# Found by the same kind of search over raw_arrays() (seeds 0 .. 399 per kind and length): the exits no physical track reached.  A zero
# row makes h3 == 0: either the first cost is NaN and every step "fails" until lam reaches 1e10 (the feature then ends NaN), or the
# Hessian's pivot is zero and the first damped solve fails (the linear solution stands).  Arbitrary matrices take five steps, on both
# paths of the refinement (the physical five-step tracks have 2 or 3 observations).
RAW_TRACKS = [raw(f"lam-cap-{M}", "zero-row", M, s, stage="NaN", exit="lam cap") for M, s in ((2, 0), (3, 0), (8, 2), (16, 2), (17, 2), (20, 1))] + \
             [raw(f"solve-failed-{M}", "zero-row", M, s, stage="accepted", exit="solve failed") for M, s in ((2, 1), (3, 3), (8, 0), (16, 0), (17, 0), (20, 0))] + \
             [raw(f"five-runs-{M}", "any", M, s, stage="accepted", exit="five runs") for M, s in ((8, 1), (16, 0), (17, 0), (20, 0))]


def point_batches():
    cond4, cond7, depth, base = _gate_tracks()
    ALL, TRI = ("triangulate", "fused", "capped"), ("triangulate",)
    b = [
        Batch("lengths-long", WIDE, _length_tracks("far", [n for n in LENGTHS if n <= 1 or n > 17]), 0.0, TRI),
        Batch("lengths-short", WIDE, _length_tracks("past", [n for n in LENGTHS if n <= 17]), 0.0, ALL),
        Batch("invalid-far", WIDE, _invalid_tracks("far", True), 0.0, TRI),
        Batch("invalid-past", WIDE, _invalid_tracks("past", False), 0.0, ALL),
        Batch("gate-cond-1e4", dict(WIDE, max_cond=1e4), cond4, 0.0, ALL),
        Batch("gate-cond-1e7", dict(WIDE, max_cond=1e7), cond7, 0.0, ALL),
        Batch("gate-depth", dict(WIDE, min_dist=4.0, max_dist=20.0), depth + found_tracks("refined-depth"), 0.0, ALL),
        Batch("gate-depth-long", dict(WIDE, min_dist=4.0, max_dist=20.0),
              [trk("depth-low-3m-40", 40, depth=3.0, seed=5, stage="linear depth low"), trk("depth-pass-8m-65", 65, seed=6, stage="accepted"),
               trk("depth-high-40m-64", 64, depth=40.0, noise=0.1, seed=7, stage="linear depth high")], 0.0, TRI),
        Batch("gate-baseline", dict(WIDE, max_baseline=40.0), base, 0.0, ALL),
        Batch("gate-refined-low", WIDE, found_tracks("refined-low") + [trk("low-pass-40m", 17, depth=40.0, noise=0.1, seed=9, stage="accepted")], 0.0, ALL),
        Batch("refine-off", dict(WIDE, refine=False, max_dist=30.0, max_cond=1e7),
              [trk("r0-pass", 12, seed=1, stage="accepted"), trk("r0-two", 2, depth=4.0, seed=2, stage="accepted"), trk("r0-high", 12, depth=50.0, noise=0.05, seed=3, stage="linear depth high"),
               trk("r0-16", 16, seed=4, stage="accepted"), trk("r0-17", 17, seed=5, stage="accepted")], 0.0, ALL),
        Batch("refine-off-long", dict(WIDE, refine=False, max_dist=30.0, max_cond=1e7),
              [trk("r0-65", 65, seed=4, stage="accepted"), trk("r0-130-high", 130, depth=50.0, noise=0.05, seed=6, stage="linear depth high")], 0.0, TRI),
        Batch("lm-exits", WIDE, found_tracks("exit"), 0.0, ALL),
        Batch("lm-exits-raw-poses", NO_GATE, RAW_TRACKS, 0.0, TRI),
        Batch("streaks-four-candidates", WIDE, found_tracks("streak-spec"), 0.0, ALL),
        Batch("streaks-serial", WIDE, [k for k in found_tracks("streak-serial") if k.M <= N_CLONES], 0.0, ALL),
        Batch("streaks-serial-long", WIDE, [k for k in found_tracks("streak-serial") if k.M > N_CLONES], 0.0, TRI),
    ]
    for name, off, cam_dt in (("window-0ms", 0.0, 0.0), ("window-13ms", 0.013, 0.0), ("window-m4ms", -0.004, 0.0), ("window-13ms-camdt", 0.013, 0.013)):
        tracks = [trk(f"w-{M}", M, depth=d, seed=M, offset=off, stage="accepted") for M, d in ((20, 8.0), (19, 20.0), (17, 5.0), (16, 12.0), (11, 8.0), (4, 6.0), (2, 4.0))]
        b.append(Batch(name, WIDE, tracks, cam_dt, ALL))
    return b


# ------------------------------------------------------------------ line batches
# depth: of the line's midpoint in the newest camera.  The window's baseline is 0.95 m across the line (the arc moves along x, the lines
# stand along y): the planes through the line from two cameras b metres apart meet at atan(b / depth), so at 3 m the later pairs pass the
# 8 degree test and the earlier ones do not, at 30 m none does, and at 6.6 m only the pair with the window's two ends does.
Ln = namedtuple("Ln", "name M depth seed D has_pt bad bad_t where expect")


def ln(name, M, depth=3.0, seed=0, D=0, has_pt=False, bad=(), bad_t="past", where=None, **expect):
    return Ln(name, M, depth, seed, D, has_pt, tuple(bad), bad_t, where or ("clones" if M <= N_CLONES else "spread"), expect)


LineBatch = namedtuple("LineBatch", "name lines")


def _line_arrays(sc, k):
    rng = np.random.default_rng(20000 + 7919 * k.seed + 31 * k.M)
    t = sc["t"]
    times = t[N_CLONES - k.M:].copy() if k.where == "clones" else np.linspace(t[0] + 0.002, t[-1], k.M)
    R_l, p_l = sc["pose_fn"](t[-1])
    to_G = lambda pc: R_l.T @ (sc["R_ItoC"].T @ (pc - sc["p_IinC"])) + p_l
    mid = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), 1.0]) * k.depth
    d = np.array([rng.uniform(-0.1, 0.1), 1.0, rng.uniform(-0.1, 0.1)])
    d /= np.linalg.norm(d)
    half = 0.12 * k.depth
    aG, bG = to_G(mid - half * d), to_G(mid + half * d)
    K8 = sc["K8"]
    uvn, uv = np.zeros((k.M, 4)), np.zeros((k.M, 4))
    for i, tm in enumerate(times):
        R, p = sc["pose_fn"](tm)
        for e, (P3, other) in enumerate(((aG, bG), (bG, aG))):
            P3 = P3 + 0.1 * rng.uniform(-1, 1) * (other - P3)          # the visible end points slide along the line from view to view
            q = sc["R_ItoC"] @ (R @ (P3 - p)) + sc["p_IinC"]
            xn = q[:2] / q[2] + rng.normal(0, 0.3 / K8[0], 2)
            uvn[i, 2 * e:2 * e + 2] = xn
            uv[i, 2 * e:2 * e + 2] = K8[0] * xn[0] + K8[2], K8[1] * xn[1] + K8[3]
    for j in k.bad:
        times[j] = t[-1] + 0.004 if k.bad_t == "past" else t[0] - 5.0
    anchor = aG + rng.uniform(0.2, 0.8) * (bG - aG) + rng.normal(0, 0.01, 3)
    return times, uv, uvn, anchor


def build_lines(pkg, batch, sc=None):
    """dict(batch, sc, st, lt) of a LineBatch"""
    sc = sc or scene()
    parts = [_line_arrays(sc, k) for k in batch.lines]
    ptr = np.concatenate([[0], np.cumsum([len(x[0]) for x in parts])]).astype(np.int32)
    st = pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], sc["R_ItoC"], sc["p_IinC"], sc["K8"], intrinsic_state_id=15)
    lt = pkg.LineTracks(ptr, np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts]), seg_uvn=np.concatenate([x[2] for x in parts]),
                        D=[k.D for k in batch.lines], anchor_pt=np.array([x[3] for x in parts]), has_pt=[1 if k.has_pt else 0 for k in batch.lines])
    return dict(batch=batch, sc=sc, st=st, lt=lt)


def line_batches():
    counts = [ln("valid-0", 3, bad=(0, 1, 2), bad_t="far", branch="too few"), ln("valid-1", 3, bad=(0, 2), branch="too few"),
              ln("valid-1-anchored", 4, D=2, has_pt=True, bad=(0, 1, 3), branch="too few"),
              ln("valid-2", 2, depth=0.25, seed=1, branch="plane pairs", used=1), ln("valid-2-of-20", 20, seed=2, bad=tuple(range(1, 19)), branch="plane pairs", used=1),
              ln("valid-3", 20, seed=3, bad=tuple(range(1, 18)), bad_t="far", branch="plane pairs"), ln("valid-20", 20, seed=4, branch="plane pairs"),
              ln("valid-65", 65, seed=5, branch="plane pairs"), ln("valid-130", 130, seed=6, branch="plane pairs"),
              ln("valid-66-of-70", 70, seed=7, bad=(0, 1, 64, 65), bad_t="far", branch="plane pairs", first=2),
              ln("valid-65-anchored", 65, seed=8, D=3, has_pt=True, branch="anchored"), ln("valid-2-anchored", 2, seed=9, D=1, has_pt=True, branch="anchored")]
    branches = [ln("first-invalid-pairs", 20, seed=11, bad=(0,), branch="plane pairs", first=1),
                ln("first-three-invalid-pairs", 20, seed=12, bad=(0, 1, 2), bad_t="far", branch="plane pairs", first=3),
                ln("first-invalid-anchored", 12, seed=13, D=2, has_pt=True, bad=(0,), branch="anchored", first=1),
                ln("first-five-invalid-anchored", 20, seed=14, D=1, has_pt=True, bad=(0, 1, 2, 3, 4), bad_t="far", branch="anchored", first=5),
                ln("anchored-D1", 15, seed=15, D=1, has_pt=True, branch="anchored"), ln("anchored-D2", 15, seed=16, D=2, has_pt=True, branch="anchored"),
                ln("anchored-D3", 15, seed=17, D=3, has_pt=True, branch="anchored"),
                ln("D2-no-anchor", 20, seed=18, D=2, has_pt=False, branch="plane pairs"), ln("D0-with-anchor", 20, seed=19, D=0, has_pt=True, branch="plane pairs"),
                ln("last-invalid-pairs", 20, seed=20, bad=(19,), branch="plane pairs"), ln("inner-invalid-pairs", 20, seed=21, bad=(7, 8, 15), bad_t="far", branch="plane pairs")]
    angle = [ln("all-under-30m", 20, depth=30.0, seed=31, branch="plane pairs", used=0), ln("all-under-60m-long", 65, depth=60.0, seed=32, branch="plane pairs", used=0),
             ln("one-passes", 20, depth=6.4, seed=31, branch="plane pairs", used=1), ln("mix-3m", 20, depth=3.0, seed=34, branch="plane pairs", mix=True),
             ln("mix-4m-long", 130, depth=4.0, seed=35, branch="plane pairs", mix=True), ln("near-most-pass", 6, depth=0.25, seed=36, branch="plane pairs"),
             ln("all-under-anchored", 20, depth=30.0, seed=37, D=1, has_pt=True, branch="anchored")]
    return [LineBatch("counts", counts), LineBatch("branches", branches), LineBatch("angle", angle)]


# ------------------------------------------------------------------ the oracle's answers, their margins and their spread
def perturbed_tracks(pkg, b, rep):
    """a batch's tracks with the same noise on the camera poses they carry themselves (Raw tracks)"""
    tr = b["tr"]
    rng = np.random.default_rng(500 + rep)
    eps = 2.0 ** -52
    return pkg.Tracks(tr.ptr, tr.t, tr.uv, tr.pf, obs_uvn=tr.uvn, res_R=tr.rR * (1 + eps * rng.choice([-1.0, 0.0, 1.0], tr.rR.shape)),
                      res_p=tr.rp * (1 + eps * rng.choice([-1.0, 0.0, 1.0], tr.rp.shape)))


def oracle_points(jo, b, st=None, tr=None):
    """dict(p, ok, err, vals [F][4], trace) of the batch on the oracle with its trace on"""
    p, ok, err, vals, trace = jo.triangulate_batch_traced(st or b["st"], tr or b["tr"], **b["batch"].opt)
    return dict(p=p, ok=ok, err=err, vals=vals, trace=trace)


def oracle_lines(jo, b, st=None):
    out, ok, trace = jo.triangulate_lines_traced(st or b["st"], b["lt"])
    return dict(lines=out, ok=ok, trace=trace)


def point_margins(b, r):
    """per feature the smallest distance of a gate value from its threshold, relative to the threshold (inf: no value was tested)"""
    o = b["batch"].opt
    m = np.full(len(r["ok"]), np.inf)
    for f, (cond, d_lin, d_ref, base) in enumerate(r["vals"]):
        for v, thr in ((cond, o["max_cond"]), (d_lin, o["min_dist"]), (d_lin, o["max_dist"]), (d_ref, o["min_dist"]), (d_ref, o["max_dist"]), (base, o["max_baseline"])):
            if not np.isnan(v):
                m[f] = min(m[f], abs(v - thr) / abs(thr))
    return m


def line_margins(r):
    """per line the smallest relative distance of a tested |cos| from 0.99"""
    c = r["trace"][:, 5:]
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(c), np.inf, np.abs(c - 0.99) / 0.99).min(axis=1)


def _rel_move(a, b):
    fin = ~np.isnan(a)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(a[fin]), 1e-300)))


def point_spread(pkg, jo, b, r=None, reps=3):
    """(stable, spread): the batch rerun `reps` times on camera poses disturbed by 2^-52 relative.  stable: no trace record and no
    verdict changed.  spread = dict(p: largest absolute move of a position, vals: largest relative move of a decision value (condition
    number, depths, baseline ratio), err: largest relative move of a reprojection error)."""
    r = r or oracle_points(jo, b)
    stable, s = True, dict(p=0.0, vals=0.0, err=0.0)
    for rep in range(reps):
        q = oracle_points(jo, b, tr=perturbed_tracks(pkg, b, rep)) if b["tr"].rR is not None else oracle_points(jo, b, perturbed_state(pkg, b["sc"], rep, b["batch"].cam_dt))
        stable = stable and np.array_equal(q["trace"], r["trace"]) and np.array_equal(q["ok"], r["ok"]) and np.array_equal(np.isnan(q["vals"]), np.isnan(r["vals"]))
        s["p"] = max(s["p"], float(np.abs(q["p"] - r["p"]).max()))
        s["vals"] = max(s["vals"], _rel_move(r["vals"], q["vals"]))
        s["err"] = max(s["err"], _rel_move(np.where(r["ok"] > 0, r["err"], np.nan), q["err"]))
    return stable, s


def line_spread(pkg, jo, b, r=None, reps=3):
    """(stable, spread) of a line batch: the same perturbation; the trace's counts must not change (its |cos| values move with the
    poses), spread = largest absolute move of one of a line's six numbers"""
    r = r or oracle_lines(jo, b)
    stable, s = True, 0.0
    for rep in range(reps):
        q = oracle_lines(jo, b, perturbed_state(pkg, b["sc"], rep))
        stable = stable and np.array_equal(q["trace"][:, :5], r["trace"][:, :5]) and np.array_equal(q["ok"], r["ok"])
        stable = stable and np.array_equal(q["trace"][:, 5:] >= 0.99, r["trace"][:, 5:] >= 0.99)
        s = max(s, float(np.abs(q["lines"] - r["lines"]).max()))
    return stable, s


def point_tolerances(r, s):
    """The bounds of the device comparison: the larger of what the existing tests hold (1e-9 x max(1, largest entry) for positions,
    rtol 1e-7 for the reprojection error, 1e-8 relative for the recorded decision values: test_one_call_update_by_value) and ten times
    the batch's spread."""
    return dict(p=max(1e-9 * max(1.0, float(np.abs(r["p"]).max())), 10 * s["p"]), err=max(1e-7, 10 * s["err"]), vals=max(1e-8, 10 * s["vals"]))


def line_tolerance(r, s):
    return max(1e-9 * max(1.0, float(np.abs(r["lines"]).max())), 10 * s)


# ------------------------------------------------------------------ the anchor walk of the one-call line route
# A classified line (D > 0) takes as its anchor the first of its points that point_used holds, and point_used holds what the point update
# of this frame triangulated (whether or not the gate took it) next to what earlier frames left.  Point ids: 101 and 103 triangulate now,
# 102 fails now (linear depth above the range), 104 is an old anchor without a track, 105 is nowhere; 101 also has an old entry, which
# this frame's triangulation replaces.
WALK_OPT = dict(WIDE, min_dist=4.0, max_dist=20.0)
WALK_POINTS = {101: trk("now-8m", 12, depth=8.0, seed=1), 102: trk("fails-40m", 12, depth=40.0, noise=0.1, seed=3), 103: trk("now-15m", 17, depth=15.0, seed=4)}
WALK_OLD = {104: np.array([1.5, -0.7, 9.0]), 101: np.array([-2.0, 0.4, 6.0])}
# line id -> (points of the line in order, D, where the anchor comes from: ("now" | "old" | None, point id))
WALK_LINES = {11: ((101, 103), 1, ("now", 101)), 12: ((102, 103), 2, ("now", 103)), 13: ((102, 104), 3, ("old", 104)), 14: ((102, 105), 2, (None, 0)),
              15: ((104, 101), 1, ("old", 104)), 16: ((105, 102, 101), 3, ("now", 101)), 17: ((), 1, (None, 0)), 18: ((103,), 2, ("now", 103))}


def anchor_walk(pkg, undistort, sc=None):
    """dict(b, tracks, ltracks, used, n, P): the databases of the anchor walk (fused_cases.fill_databases takes them)"""
    sc = sc or scene()
    ids = sorted(WALK_POINTS)
    b = build(pkg, Batch("anchor-walk", WALK_OPT, [WALK_POINTS[i] for i in ids], 0.0, ()), undistort, sc)
    tr = b["tr"]
    tracks = {i: (tr.t[tr.ptr[f]:tr.ptr[f + 1]].copy(), tr.uv[tr.ptr[f]:tr.ptr[f + 1]].copy(), tr.uvn[tr.ptr[f]:tr.ptr[f + 1]].copy()) for f, i in enumerate(ids)}
    ltracks = {}
    for q, (lid, (pids, D, _)) in enumerate(sorted(WALK_LINES.items())):
        times, uv, uvn, _ = _line_arrays(sc, ln("walk", 15 - q % 3, depth=3.0, seed=50 + q))
        ltracks[lid] = (times, uv.astype(np.float32), uvn.astype(np.float32), D, list(pids))
    used = {i: (p, float(sc["t"][-3])) for i, p in WALK_OLD.items()}
    n = sc["n_state"]
    return dict(b=b, sc=sc, ids=ids, tracks=tracks, ltracks=ltracks, used=used, n=n, P=synth.spd_cov(n, seed=4) * 1e-4)


def anchor_walk_oracle(pkg, w, q95, st=None):
    """the compiled CPU frame on the walk's databases: (point update, its decisions by id, line update)"""
    import fused_cases as fc
    import oracle_lib
    sc, opt = w["sc"], WALK_OPT
    t_last = float(sc["t"][-1])
    fr = oracle_lib.FrameOracle(pkg, pkg.default_config(752, 480), q95)
    fr.set_intrinsics(sc["K8"])
    fc.fill_databases(fr, "points", w["tracks"], {}, device=False)
    fc.fill_databases(fr, "lines", w["ltracks"], w["used"], device=False)
    P = np.array(w["P"], dtype=np.float64, order="F")
    st = st or w["b"]["st"]
    pts = fr.update_points(P, st, 40, 20, t_last + 1.0, t_last, True, 1.0, opt["min_dist"], opt["max_dist"], opt["max_cond"], opt["max_baseline"], True)
    ids, vals = fr.last_point_decisions()
    fr.get_line_features(st, 20, t_last + 1.0, t_last)
    lns = fr.update_lines(P, st, 20, t_last + 1.0, t_last)
    fr.close()
    return pts, dict(zip((int(i) for i in ids), vals)), lns


def anchor_walk_spread(pkg, w, q95, lns=None, reps=3):
    """(stable, spread) of the walk's lines on the compiled CPU frame under the same perturbation of the camera poses: stable = the
    same lines in the same order, spread = the largest absolute move of one of a line's six numbers"""
    lns = lns or anchor_walk_oracle(pkg, w, q95)[2]
    stable, s = True, 0.0
    for rep in range(reps):
        q = anchor_walk_oracle(pkg, w, q95, perturbed_state(pkg, w["sc"], rep))[2]
        stable = stable and np.array_equal(q["ids"], lns["ids"])
        if stable:
            s = max(s, float(np.abs(q["line_FinG"] - lns["line_FinG"]).max()))
    return stable, s


# ------------------------------------------------------------------ the spread, stored with the cases
# What point_spread / line_spread / anchor_walk_spread measure on the oracle (the largest move of a batch's outputs under 2^-52 noise on
# its camera poses, three seeded repetitions), rounded up to two digits.  tests/test_triangulation_cases_cpu.py holds the stored values
# to the measured ones; the device tests take their tolerance from the stored ones.  The reprojection error does not move at all: it
# is a mean of distances between float pixel coordinates.
POINT_SPREAD = {
    "lengths-long": dict(p=5.4e-12, vals=2.7e-12, err=0.0),
    "lengths-short": dict(p=9.1e-11, vals=1.4e-10, err=0.0),
    "invalid-far": dict(p=9.5e-13, vals=1.1e-12, err=0.0),
    "invalid-past": dict(p=9.5e-13, vals=1.1e-12, err=0.0),
    "gate-cond-1e4": dict(p=4.1e-14, vals=3e-10, err=0.0),
    "gate-cond-1e7": dict(p=2.4e-10, vals=1.4e-08, err=0.0),
    "gate-depth": dict(p=2.3e-12, vals=5.1e-12, err=0.0),
    "gate-depth-long": dict(p=3.1e-13, vals=2.6e-12, err=0.0),
    "gate-baseline": dict(p=2.2e-13, vals=1.3e-11, err=0.0),
    "gate-refined-low": dict(p=3e-11, vals=7e-07, err=0.0),
    "refine-off": dict(p=6.9e-13, vals=5.6e-12, err=0.0),
    "refine-off-long": dict(p=7.2e-15, vals=4.7e-12, err=0.0),
    "lm-exits": dict(p=2.5e-10, vals=8.3e-11, err=0.0),
    "lm-exits-raw-poses": dict(p=1.1e-09, vals=3.9e-11, err=0.0),
    "streaks-four-candidates": dict(p=1.7e-10, vals=4.6e-12, err=0.0),
    "streaks-serial": dict(p=2.5e-10, vals=2.4e-12, err=0.0),
    "streaks-serial-long": dict(p=1.9e-11, vals=5.2e-13, err=0.0),
    "window-0ms": dict(p=3.4e-12, vals=5.3e-12, err=0.0),
    "window-13ms": dict(p=3.5e-12, vals=5.6e-12, err=0.0),
    "window-m4ms": dict(p=1.9e-12, vals=3.5e-12, err=0.0),
    "window-13ms-camdt": dict(p=3.5e-12, vals=5.6e-12, err=0.0),
}
LINE_SPREAD = {"counts": 1.6e-15, "branches": 8.9e-16, "angle": 7.2e-15, "anchor-walk": 2.3e-12}
WALK_POINT_SPREAD = dict(p=2.3e-12, vals=5.1e-12, err=0.0)     # the three point tracks of the anchor walk
