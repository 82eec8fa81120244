"""GPU tests of the line tracker on a stereo context: with two images the reference tracks lines on image 0 by feed_monocular
(TrackLSD::feed_new_camera, TrackLSD.cpp:54-57), so on a context fed through plv_tracker_feed_stereo the line code reads camera 0's
equalised image, camera 0's last points and the context's own intrinsics.  Lines depend on the image and on the points handed in
and on nothing else: a monocular context fed the left images and handed the same points is the reference, bit for bit.

The pairs are the first three of stereo_ref's "two cameras" stream (320 x 240, the stream test_gpu_stereo_tracker.py feeds).  Its
texture has no drawn edges: at the shipped thresholds (segments of 20 half-resolution pixels, 40 px kept) the oracle's detector finds
5 - 6 segments per frame, at 10 / 20 px about 90 — the thresholds this test sets, so that lines own points and match over frames."""
import numpy as np
import pytest

import stereo_ref

pytestmark = pytest.mark.gpu

N_PAIRS = 3


@pytest.fixture(scope="module")
def stream():
    s = {x.name: x for x in stereo_ref.streams()}["two cameras"]
    frames = []
    for f, fr in enumerate(s.frames()):
        if f == N_PAIRS:
            break
        frames.append(fr)
    return s, frames


def _context(pkg, s, stereo):
    cfg = pkg.default_config(s.w, s.h)
    cfg.num_features, cfg.grid_x, cfg.grid_y = s.cfg.num_features, s.cfg.grid_x, s.cfg.grid_y
    cfg.min_px_dist, cfg.fast_threshold = s.cfg.min_px_dist, s.cfg.fast_threshold
    cfg.line_length_threshold, cfg.line_min_length_px = 10, 20.0
    for i, v in enumerate(s.K_left):
        cfg.intrinsics[i] = float(v)
    ctx = pkg.Context(cfg)
    if stereo:
        ctx.stereo_configure(s.K_right, 0)
    return ctx


def _line_state(ctx):
    lines, ids = ctx.line_tracker_last()
    rel_ptr, rel_id = ctx.line_tracker_last_points()
    return lines, ids, rel_ptr, rel_id, ctx.line_db_size()


def _assert_same(got, want, where):
    for k, (g, w) in enumerate(zip(got, want)):
        name = ("lines", "line ids", "rel_ptr", "rel_id", "line_db_size")[k]
        assert np.array_equal(g, w), (where, name)


@pytest.mark.parametrize("walk", [0, 2])
def test_lines_of_a_stereo_context_are_camera_0s(pkg, stream, walk):
    """stereo context + the points handed in == monocular context on the left images + the same points; and plv_line_tracker_feed
    on a stereo twin == plv_line_tracker_feed_points with plv_stereo_last(0).  walk = 2: the component-parallel device walk."""
    s, frames = stream
    st, twin, mono = _context(pkg, s, True), _context(pkg, s, True), _context(pkg, s, False)
    try:
        vps = st.vanishing_points(np.eye(3), s.K_left)
        for c in (st, twin, mono):
            c.line_walk_mode(walk)
        n_lines = []
        for f, (t, left, right, _, _) in enumerate(frames):
            st.tracker_feed_stereo(t, left, right)
            twin.tracker_feed_stereo(t, left, right)
            mono.tracker_feed(t, left)
            pts, ids = st.stereo_last(0)
            assert len(ids) >= 10
            st.line_tracker_feed_points(t, vps, pts, ids)
            mono.line_tracker_feed_points(t, vps, pts, ids)
            twin.line_tracker_feed(t, vps)
            assert st.line_walk_info()["mode"] == walk and twin.line_walk_info()["mode"] == walk
            want = _line_state(mono)
            _assert_same(_line_state(st), want, ("points handed in", walk, f))
            _assert_same(_line_state(twin), want, ("the context's own points", walk, f))
            n_lines.append(len(want[1]))
            # the cached detection of the frame is camera 0's image too
            assert np.array_equal(st.detect_lines(0), mono.detect_lines(0)), f
        # the comparison is of something: every frame has lines that own points, and they reach the track store
        assert min(n_lines) > 0, n_lines
        assert mono.line_db_size() > 0
        # neither tracker has borrowed the other's state
        assert st.db_size() == 0 and len(st.tracker_last()[1]) == 0
        assert mono.stereo_db_size() == 0
    finally:
        for c in (st, twin, mono):
            c.close()


def test_line_feed_before_the_first_pair_is_refused(pkg, stream):
    s, frames = stream
    ctx = _context(pkg, s, True)
    try:
        vps = ctx.vanishing_points(np.eye(3), s.K_left)
        with pytest.raises(pkg.PlvError) as e:
            ctx.line_tracker_feed(frames[0][0], vps)
        assert e.value.code == pkg.PLV_E_BADARG and "no image has been fed" in str(e.value)
        assert ctx.line_db_size() == 0 and len(ctx.line_tracker_last()[1]) == 0
        # the refusal left nothing behind: the first pair then gives lines on camera 0's image
        t, left, right, _, _ = frames[0]
        ctx.tracker_feed_stereo(t, left, right)
        ctx.line_tracker_feed(t, vps)
        assert len(ctx.detect_lines(0)) > 0
    finally:
        ctx.close()
