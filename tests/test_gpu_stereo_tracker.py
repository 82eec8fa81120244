"""GPU tests of the stereo point tracker (plv_stereo_* / plv_tracker_feed_stereo) against tests/stereo_ref.py, the restatement of
TrackKLT::feed_stereo / perform_detection_stereo on the CPU oracle's primitives: the last points and ids of both cameras frame after
frame, and the per-camera database at the end, bit for bit.  The streams (stereo_ref.streams, 320 x 240 and 256 x 192, 6 - 8 pairs)
are the ones test_stereo_ref_cpu.py shows to reach every branch."""
import ctypes as C

import numpy as np
import pytest

import stereo_ref
import synth

pytestmark = pytest.mark.gpu


def _context(pkg, s, configure=True):
    cfg = pkg.default_config(s.w, s.h)
    cfg.num_features, cfg.grid_x, cfg.grid_y = s.cfg.num_features, s.cfg.grid_x, s.cfg.grid_y
    cfg.min_px_dist, cfg.fast_threshold = s.cfg.min_px_dist, s.cfg.fast_threshold
    for i, v in enumerate(s.K_left):
        cfg.intrinsics[i] = float(v)
    ctx = pkg.Context(cfg)
    if configure:
        ctx.stereo_configure(s.K_right, 0)
    return ctx


def _state(ctx):
    return ctx.stereo_last(0) + ctx.stereo_last(1)


def _assert_state(ctx, want, where):
    got = _state(ctx)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (where, ("left points", "left ids", "right points", "right ids")[k], len(g), len(w))


def _assert_database(ctx, ref):
    ids = np.array(sorted(ref.db), dtype=np.uint64)
    assert np.array_equal(ctx.stereo_db_ids(), ids)
    assert ctx.stereo_db_size() == len(ids)
    for cam in (0, 1):
        ptr, t, uv, uvn = ctx.stereo_db_export(ids, cam)
        for k, fid in enumerate(ids):
            obs = ref.db[int(fid)][cam]
            a, b = ptr[k], ptr[k + 1]
            assert b - a == len(obs), (cam, int(fid))
            assert np.array_equal(t[a:b], np.array([o[0] for o in obs], dtype=np.float64)), (cam, int(fid))
            assert np.array_equal(uv[a:b], np.array([o[1:3] for o in obs], dtype=np.float32).reshape(-1, 2)), (cam, int(fid))
            assert np.array_equal(uvn[a:b], np.array([o[3:5] for o in obs], dtype=np.float32).reshape(-1, 2)), (cam, int(fid))


@pytest.mark.parametrize("name", ["band", "two cameras", "cut"])
def test_stream_matches_restatement(pkg, name):
    """band: mask_left all zero and a band in mask_right; two cameras: the right camera's own intrinsics (its undistortion and its
    RANSAC threshold are camera 1's: with camera 0's the restatement gives another result, test_stereo_ref_cpu.py); cut: fewer than
    10 surviving points, then none — the "both masks empty" reset — each followed by a detection on the next pair."""
    s, after, ref = stereo_ref.reference_run(name)
    ctx = _context(pkg, s)
    try:
        for f, (t, left, right, ml, mr) in enumerate(s.frames()):
            ctx.tracker_feed_stereo(t, left, right, mask_left=ml, mask_right=mr)
            _assert_state(ctx, after[f], (name, f))
        _assert_database(ctx, ref)
        # the database calls: what FeatureDatabase::cleanup_measurements and a removal leave
        t_cut = 10.0 + 0.05 * 2
        ctx.stereo_db_cleanup_measurements(t_cut)
        left_over = sorted(fid for fid, (l, r) in ref.db.items() if any(o[0] >= t_cut for o in l + r))
        assert np.array_equal(ctx.stereo_db_ids(), np.array(left_over, dtype=np.uint64))
        if left_over:
            ptr, t, _, _ = ctx.stereo_db_export(np.array(left_over[:1], dtype=np.uint64), 0)
            assert np.all(t >= t_cut)
            ctx.stereo_db_remove(left_over[:1])
            assert ctx.stereo_db_size() == len(left_over) - 1
    finally:
        ctx.close()


def test_bayer_pair_is_the_converted_grey_pair(pkg):
    s, _, _ = stereo_ref.reference_run("two cameras")
    a, b = _context(pkg, s), _context(pkg, s)
    try:
        for f, (t, left, right, _, _) in enumerate(s.frames()):
            if f == 4:
                break
            # (the rendered frames read as RGGB mosaics: any bytes are a mosaic)
            grey_l, grey_r = a.image_convert(left, "bayer_rggb8"), a.image_convert(right, "bayer_rggb8")
            a.tracker_feed_stereo(t, left, right, encoding="bayer_rggb8")
            b.tracker_feed_stereo(t, grey_l, grey_r)
            want = _state(b)
            assert len(want[1]) >= 10 and len(want[3]) >= 10
            _assert_state(a, want, f)
        ids = b.stereo_db_ids()
        assert len(ids) > 0 and np.array_equal(a.stereo_db_ids(), ids)
        for cam in (0, 1):
            for x, y in zip(a.stereo_db_export(ids, cam), b.stereo_db_export(ids, cam)):
                assert np.array_equal(x, y)
    finally:
        a.close()
        b.close()


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_refused_arguments_leave_everything_as_it_was(pkg):
    s, after, _ = stereo_ref.reference_run("band")
    frames = list(s.frames())
    ctx = _context(pkg, s)
    lib, h, bad = ctx.lib, ctx.h, pkg.PLV_E_BADARG
    try:
        for f in range(2):
            t, left, right, ml, mr = frames[f]
            ctx.tracker_feed_stereo(t, left, right, mask_left=ml, mask_right=mr)
        before, size = _state(ctx), ctx.stereo_db_size()
        t, left, right, ml, mr = frames[2]
        w = s.w
        n, pts, ids = C.c_int(), np.zeros((4096, 2), np.float32), np.zeros(4096, np.uint64)
        ptr = np.zeros(2, np.int32)
        K = np.ascontiguousarray(s.K_right)
        refusals = {
            "null left image": lambda: lib.plv_tracker_feed_stereo(h, t, None, w, _u8(right), w, 0, None, None),
            "null right image": lambda: lib.plv_tracker_feed_stereo(h, t, _u8(left), w, None, w, 0, None, None),
            "bad encoding": lambda: lib.plv_tracker_feed_stereo(h, t, _u8(left), w, _u8(right), w, 99, None, None),
            "negative encoding": lambda: lib.plv_tracker_feed_stereo(h, t, _u8(left), w, _u8(right), w, -1, None, None),
            "left stride below the width": lambda: lib.plv_tracker_feed_stereo(h, t, _u8(left), w - 1, _u8(right), w, 0, None, None),
            "right stride below the width": lambda: lib.plv_tracker_feed_stereo(h, t, _u8(left), w, _u8(right), w - 1, 0, None, None),
            "stride below width x 3 bytes": lambda: lib.plv_tracker_feed_stereo(h, t, _u8(left), 3 * w - 1, _u8(right), 3 * w, pkg.ENCODINGS["bgr8"], None, None),
            "last of camera 2": lambda: lib.plv_stereo_last(h, 2, pts.ctypes.data_as(C.POINTER(C.c_float)), ids.ctypes.data_as(C.POINTER(C.c_uint64)), 4096, C.byref(n)),
            "last of camera -1": lambda: lib.plv_stereo_last(h, -1, pts.ctypes.data_as(C.POINTER(C.c_float)), ids.ctypes.data_as(C.POINTER(C.c_uint64)), 4096, C.byref(n)),
            "intrinsics of camera 2": lambda: lib.plv_stereo_set_intrinsics(h, 2, K.ctypes.data_as(C.POINTER(C.c_double))),
            "export of camera 2": lambda: lib.plv_stereo_db_export_tracks(h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), 1, 2, ptr.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, 0),
        }
        for what, call in refusals.items():
            assert call() == bad, what
            assert lib.plv_last_error(), what
            _assert_state(ctx, before, what)
            assert ctx.stereo_db_size() == size, what
        # the monocular feeds on a context the stereo tracker has taken
        mono = {
            "tracker_feed": lambda: ctx.tracker_feed(t, left),
            "tracker_feed_encoded": lambda: ctx.tracker_feed_encoded(t, left, "mono8"),
            "tracker_feed_staged": lambda: ctx.tracker_feed_staged(t, 0),
            "tracker_feed_downsampled": lambda: ctx.tracker_feed_downsampled(t, np.zeros((2 * s.h, 2 * s.w), np.uint8)),
            "camera_frame": lambda: ctx.camera_frame(synth.scene_views(pkg, synth.vio_scene(n_clones=5, F=4, M=3))[0], t, img=left),
        }
        for what, call in mono.items():
            with pytest.raises(pkg.PlvError) as e:
                call()
            assert e.value.code == bad, what
            assert "stereo" in str(e.value), what
            _assert_state(ctx, before, what)
            assert ctx.stereo_db_size() == size and ctx.db_size() == 0, what
        # ... and the next pair gives what it gives without any of this
        ctx.tracker_feed_stereo(t, left, right, mask_left=ml, mask_right=mr)
        _assert_state(ctx, after[2], "the pair after the refusals")
    finally:
        ctx.close()


def test_stereo_feed_needs_configure_and_a_context_of_its_own(pkg):
    s, after, _ = stereo_ref.reference_run("band")
    t, left, right, ml, mr = next(iter(s.frames()))
    ctx = _context(pkg, s, configure=False)
    try:
        with pytest.raises(pkg.PlvError) as e:
            ctx.tracker_feed_stereo(t, left, right)
        assert e.value.code == pkg.PLV_E_BADARG and "plv_stereo_configure" in str(e.value)
        assert ctx.stereo_db_size() == 0
        ctx.stereo_configure(s.K_right, 0)  # (the refusal left nothing behind: the stream starts as on a fresh context)
        ctx.tracker_feed_stereo(t, left, right, mask_left=ml, mask_right=mr)
        _assert_state(ctx, after[0], "first pair after the refusal")
    finally:
        ctx.close()
    # a context the monocular tracker has taken refuses the pair, and goes on tracking one camera
    ctx = _context(pkg, s)
    try:
        ctx.tracker_feed(t, left)
        pts, ids = ctx.tracker_last()
        assert len(ids) >= 10
        with pytest.raises(pkg.PlvError) as e:
            ctx.tracker_feed_stereo(t + 0.05, left, right)
        assert e.value.code == pkg.PLV_E_BADARG and "monocular" in str(e.value)
        got = ctx.tracker_last()
        assert np.array_equal(got[0], pts) and np.array_equal(got[1], ids)
        assert len(ctx.stereo_last(0)[1]) == 0 and ctx.stereo_db_size() == 0
        ctx.tracker_feed(t + 0.05, left)
        assert ctx.db_size() > 0
    finally:
        ctx.close()
