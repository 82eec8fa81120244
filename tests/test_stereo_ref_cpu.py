"""CPU tests of tests/stereo_ref.py, the restatement test_gpu_stereo_tracker.py holds the stereo tracker to:
  * its grid extraction, run as a monocular detection, is DetectOracle.perform_detection (points, order, ids);
  * the shapes the GPU test uses exercise the right camera's `is_stereo` exception (the counts were checked with the oracle when
    the streams were drawn);
  * over the GPU test's streams the restatement itself reaches every branch that test is about."""
import numpy as np
import pytest

import oracle_lib
import stereo_ref
import synth


def _equalised(w, h, tx=0.0):
    canvas = synth.texture_canvas(w, h, seed=42)
    return oracle_lib.load_front().equalize_hist(synth.render_frame(canvas, w, h, tx=tx))


SHAPES = {"320x240": (320, 240, stereo_ref.Settings(60, 5, 4, 10)), "256x192": (256, 192, stereo_ref.Settings(40, 4, 3, 8))}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_restated_extraction_is_perform_detection(shape, tracked, masked):
    w, h, cfg = SHAPES[shape]
    img = _equalised(w, h)
    do = oracle_lib.load_detect()
    mask = None
    if masked:
        mask = np.zeros((h, w), np.uint8)
        mask[h // 3:h // 2, :] = 255          # a band that covers whole rows (cells whose sample point is masked are skipped)
        mask[: h // 4, w // 2:w // 2 + 9] = 200  # > 127, not 255: points and corners are masked, the cell is not
    pts, ids, currid = np.zeros((0, 2), np.float32), np.zeros(0, np.uint64), 0
    if tracked:  # every third point of a first detection, moved a little, two of them into one min_px_dist cell
        p, i, currid = do.perform_detection(img, None, pts, ids, 0, cfg.num_features, cfg.grid_x, cfg.grid_y, cfg.min_px_dist, cfg.fast_threshold)
        pts, ids = p[::3] + np.float32([1.25, -0.5]), i[::3]
        pts = np.vstack([pts, pts[:1] + np.float32(0.5)]).astype(np.float32)
        ids = np.concatenate([ids, [np.uint64(currid + 1)]]).astype(np.uint64)
        currid += 1
    want = do.perform_detection(img, mask, pts, ids, currid, cfg.num_features, cfg.grid_x, cfg.grid_y, cfg.min_px_dist, cfg.fast_threshold)
    got = stereo_ref.Detection(cfg).monocular(img, mask, pts, ids, currid)
    assert len(want[1]) > len(ids)  # (the top-up ran)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])
    assert got[2] == want[2]


@pytest.mark.parametrize("shape,disparity,corners,tracked,collisions", [("320x240", 6.0, 78, 78, 5), ("256x192", 4.0, 47, 46, 2)])
def test_shapes_exercise_the_exception(shape, disparity, corners, tracked, collisions):
    """a first detection on the left image tracked into the right one: how many of the right points share a min_px_dist cell"""
    w, h, cfg = SHAPES[shape]
    fo, do = oracle_lib.load_front(), oracle_lib.load_detect()
    eq_l, eq_r = _equalised(w, h), _equalised(w, h, tx=disparity)
    p, _, _ = do.perform_detection(eq_l, None, np.zeros((0, 2), np.float32), np.zeros(0, np.uint64), 0, cfg.num_features, cfg.grid_x, cfg.grid_y,
                                   cfg.min_px_dist, cfg.fast_threshold)
    p1, st, _ = fo.lk_track(fo.pyramid(eq_l), fo.pyramid(eq_r), p, p)
    assert (len(p), int(st.sum())) == (corners, tracked)
    assert abs(float(np.median((p1 - p)[st.astype(bool), 0])) - disparity) < 0.01  # (the tracked points sit at the rendered offset)
    cells = {}
    for k in np.flatnonzero(st):
        c = (int(p1[k, 0] / np.float32(cfg.min_px_dist)), int(p1[k, 1] / np.float32(cfg.min_px_dist)))
        cells[c] = cells.get(c, 0) + 1
    assert sum(v - 1 for v in cells.values()) == collisions


def _band_reaches_every_branch(after, ref):
    later = ref.frames[1:]  # (the first pair is detected on, not tracked)
    assert any("left top-up" in e for e in later)
    assert any("right top-up" in e for e in later)
    assert any(e == {"no top-up"} for e in later)
    for kind in ("stereo tracks", "left-only tracks", "right-only tracks", "new stereo features", "new left-only features",
                 "new right-only features", "right points kept by the is_stereo exception", "right corners under mask_right"):
        assert ref.stats[kind] > 0, (kind, dict(ref.stats))
    # the three kinds as the lists hold them at the end of a frame
    both = [len(set(a[1].tolist()) & set(a[3].tolist())) for a in after]
    assert max(both) > 0
    assert any(len(set(a[1].tolist()) - set(a[3].tolist())) > 0 for a in after)
    assert any(len(set(a[3].tolist()) - set(a[1].tolist())) > 0 for a in after)
    # ... and in the database: features with observations in both cameras, in the left one alone, in the right one alone
    kinds = {(bool(l), bool(r)) for l, r in ref.db.values()}
    assert kinds == {(True, True), (True, False), (False, True)}


def test_band_stream_reaches_every_branch():
    _, after, ref = stereo_ref.reference_run("band")
    _band_reaches_every_branch(after, ref)


def _two_cameras_are_separated(s, ref):
    """the run differs from the one in which camera 1 is read with camera 0's intrinsics and model"""
    assert not np.array_equal(ref.K8[0], ref.K8[1])
    same = stereo_ref.StereoRef(s.cfg, ref.K8[0], ref.K8[0], models=(ref.models[0], ref.models[0]))
    stereo_ref.run_stream(s, same)
    obs = lambda r: sorted((fid, o) for fid, (_, right_obs) in r.db.items() for o in right_obs)
    assert obs(same) != obs(ref)
    assert ref.stats["stereo tracks"] > 0 and ref.stats["right-only tracks"] > 0


def test_two_camera_stream_separates_the_cameras():
    """with the right camera's own intrinsics the restatement's result differs from the one with the left camera's for both (so
    the GPU test does tell which intrinsics camera 1 was undistorted and gated with)"""
    s, after, ref = stereo_ref.reference_run("two cameras")
    assert not np.array_equal(s.K_left, s.K_right)
    _two_cameras_are_separated(s, ref)


def test_cut_stream_resets_and_detects_again():
    _, after, ref = stereo_ref.reference_run("cut")
    e = ref.frames
    assert "fewer than 10 points" in e[3] and "reset" not in e[3]
    assert len(after[3][1]) == 0 and len(after[3][3]) == 0
    assert "detection on the current pair" in e[4] and len(after[4][1]) >= 10
    assert "reset" in e[6] and len(after[6][1]) == 0 and len(after[6][3]) == 0
    assert "detection on the current pair" in e[7] and len(after[7][1]) >= 10 and len(after[7][3]) >= 10


# ---- the model pairings (camera 0, camera 1): RR, RE, ER, EE of stereo_ref.PAIRINGS
def _same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


@pytest.mark.parametrize("name", ["band", "two cameras", "cut"])
def test_composed_matching_is_perform_matching(name):
    """(a) StereoRef.match (LK, the camera's undistortion, RANSAC, status & inlier) under RR is FrontOracle.perform_matching bit for
    bit: the lists after every pair and the database, normalised coordinates included"""
    s, after, ref = stereo_ref.reference_run(name)
    whole = stereo_ref.StereoRef(s.cfg, s.K_left, s.K_right)
    whole.match = whole.match_oracle
    assert _same_lists(stereo_ref.run_stream(s, whole), after)
    assert whole.db == ref.db and len(ref.db) > 0
    assert whole.stats == ref.stats


@pytest.mark.parametrize("name,pairing,coeffs", stereo_ref.PAIRING_RUNS)
def test_pairing_runs_reach_what_their_streams_are_for(name, pairing, coeffs):
    """(b) the events and stats of the RR stream, (c) every matching hands RANSAC at least 10 points and keeps at least 10,
    (d) in some frame RANSAC rejects some points and keeps others"""
    s, after, ref = stereo_ref.reference_run(name, pairing, coeffs)
    assert ref.models == stereo_ref.PAIRINGS[pairing]
    if name == "band":
        _band_reaches_every_branch(after, ref)
    else:
        _two_cameras_are_separated(s, ref)
    tracked = range(1, len(ref.frames))
    assert sorted((f, cam) for f, cam, _, _, _ in ref.matchings) == [(f, cam) for f in tracked for cam in (0, 1)]
    print(f"{name} {pairing} {coeffs}: smallest (handed, inliers, kept) =", min(m[2:] for m in ref.matchings), "smallest kept",
          min(m[4] for m in ref.matchings))
    assert all(n >= 10 and kept >= 10 for _, _, n, _, kept in ref.matchings), ref.matchings
    assert any(0 < inl < n for _, _, n, inl, _ in ref.matchings), ref.matchings
    if name == "two cameras" and coeffs == "strong" and ref.models[1] == "equidistant":
        # camera 1 (f = 150, the wider view) under the strong set: RANSAC decides on fisheye coordinates in a quiet frame too
        assert any(f == 1 and cam == 1 and 10 <= inl < n for f, cam, n, inl, _ in ref.matchings), ref.matchings


@pytest.mark.parametrize("name,pairing,coeffs", stereo_ref.PAIRING_RUNS)
def test_pairing_runs_have_no_rounding_ties(name, pairing, coeffs):
    """(e) the device's undistortion is held to 1 ulp of cam_equi.undistort, not to its bits: the run decides nothing on a last
    bit, so with every normalised coordinate moved by a seeded -1 / 0 / +1 ulp the lists after every pair are the same"""
    s, after, ref = stereo_ref.reference_run(name, pairing, coeffs)
    for seed in (1, 2, 3):
        moved = stereo_ref.StereoRef(s.cfg, ref.K8[0], ref.K8[1], models=ref.models, jitter=np.random.default_rng(seed))
        assert _same_lists(stereo_ref.run_stream(s, moved), after), seed
        assert moved.stats == ref.stats
        un = lambda r: np.array([o[3:5] for l, rr in r.db.values() for o in l + rr], dtype=np.float32)
        assert not np.array_equal(un(moved), un(ref))  # (the coordinates did move)


def test_pairings_give_different_tracks():
    """(f) RR, RE, ER and EE on one stream end on different id lists and count different tracks: a feed that swaps or ignores a
    camera's model gives another pairing's run, not its own"""
    runs = {p: stereo_ref.reference_run("two cameras", p, None if p == "RR" else "strong") for p in stereo_ref.PAIRINGS}
    final = {p: (r[1][-1][1].tolist(), r[1][-1][3].tolist()) for p, r in runs.items()}
    counts = {p: tuple(r[2].stats[k] for k in ("stereo tracks", "left-only tracks", "right-only tracks")) for p, r in runs.items()}
    print(counts)
    names = sorted(runs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert final[a] != final[b], (a, b)
            assert counts[a] != counts[b], (a, b)


def test_intrinsics_change_between_pairs_shows():
    """the run test_gpu_stereo_tracker.py holds plv_stereo_set_intrinsics to: K8 of one equidistant camera replaced before pair 3
    gives other lists than the unchanged run, and keeps the conditions (c) and (e)"""
    s, plain, ref = stereo_ref.reference_run("two cameras", "EE", "strong")
    for cam in (0, 1):
        K_new = stereo_ref.changed_intrinsics(ref.K8[cam])
        s2, after, changed = stereo_ref.changed_run(cam)
        assert _same_lists(after[:stereo_ref.CHANGE_AT], plain[:stereo_ref.CHANGE_AT])
        assert not _same_lists(after, plain)
        assert all(n >= 10 and kept >= 10 for _, _, n, _, kept in changed.matchings), changed.matchings
        assert np.array_equal(changed.K8[cam], K_new) and np.array_equal(changed.K8[1 - cam], ref.K8[1 - cam])
        moved = stereo_ref.StereoRef(s.cfg, ref.K8[0], ref.K8[1], models=ref.models, jitter=np.random.default_rng(4))
        assert _same_lists(stereo_ref.run_stream(s, moved, {stereo_ref.CHANGE_AT: (cam, K_new)}), after)
