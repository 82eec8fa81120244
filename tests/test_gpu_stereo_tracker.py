"""GPU tests of the stereo point tracker (plv_stereo_* / plv_tracker_feed_stereo) against tests/stereo_ref.py, the restatement of
TrackKLT::feed_stereo / perform_detection_stereo on the CPU oracle's primitives: the last points and ids of both cameras frame after
frame, and the per-camera database at the end, bit for bit.  The streams (stereo_ref.streams, 320 x 240 and 256 x 192, 6 - 8 pairs)
are the ones test_stereo_ref_cpu.py shows to reach every branch."""
import ctypes as C

import numpy as np
import pytest

import cam_equi
import stereo_ref
import synth

pytestmark = pytest.mark.gpu


def _context(pkg, s, configure=True, K8=None, models=("radtan", "radtan"), model_first=True):
    """a context for stream s; K8, models: per camera (default: the stream's own intrinsics, both radtan).  Camera 0's model is the
    context's (plv_set_camera_model), camera 1's comes with plv_stereo_configure; model_first: the order of the two calls."""
    cfg = pkg.default_config(s.w, s.h)
    cfg.num_features, cfg.grid_x, cfg.grid_y = s.cfg.num_features, s.cfg.grid_x, s.cfg.grid_y
    cfg.min_px_dist, cfg.fast_threshold = s.cfg.min_px_dist, s.cfg.fast_threshold
    for i, v in enumerate(s.K_left):
        cfg.intrinsics[i] = float(v)
    ctx = pkg.Context(cfg)
    if K8 is None:
        K8 = (s.K_left, s.K_right)
    else:
        ctx.set_camera_intrinsics(K8[0])
    if model_first and models[0] != "radtan":
        ctx.set_camera_model(models[0])
    if configure:
        ctx.stereo_configure(K8[1], stereo_ref.MODELS.index(models[1]))
    if not model_first:
        ctx.set_camera_model(models[0])
    return ctx


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _state(ctx):
    return ctx.stereo_last(0) + ctx.stereo_last(1)


def _assert_state(ctx, want, where):
    got = _state(ctx)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (where, ("left points", "left ids", "right points", "right ids")[k], len(g), len(w))


def _assert_database(ctx, ref, K8_at=None):
    """ids, stamps and uv bit for bit; uvn bit for bit for a radtan camera, within 1 ulp of cam_equi.undistort (on the intrinsics
    the camera had at the observation's time, K8_at(cam, t), by default the restatement's) for an equidistant one.  Returns the
    largest uvn difference in ulp per camera."""
    ids = np.array(sorted(ref.db), dtype=np.uint64)
    assert np.array_equal(ctx.stereo_db_ids(), ids)
    assert ctx.stereo_db_size() == len(ids)
    worst = [0, 0]
    for cam in (0, 1):
        ptr, t, uv, uvn = ctx.stereo_db_export(ids, cam)
        if ref.models[cam] == "equidistant":  # (the rule test_gpu_equidistant.py::test_tracker_obs_uvn_follow_the_model holds the monocular feed to)
            assert len(uv) > 0
            want = np.zeros_like(uvn)
            for k in range(len(t)):
                want[k] = cam_equi.undistort(ref.K8[cam] if K8_at is None else K8_at(cam, t[k]), uv[k:k + 1])[0]
            worst[cam] = int(_ulps(uvn, want).max())
            assert worst[cam] <= 1, (cam, worst[cam])
        for k, fid in enumerate(ids):
            obs = ref.db[int(fid)][cam]
            a, b = ptr[k], ptr[k + 1]
            assert b - a == len(obs), (cam, int(fid))
            assert np.array_equal(t[a:b], np.array([o[0] for o in obs], dtype=np.float64)), (cam, int(fid))
            assert np.array_equal(uv[a:b], np.array([o[1:3] for o in obs], dtype=np.float32).reshape(-1, 2)), (cam, int(fid))
            if ref.models[cam] == "radtan":
                assert np.array_equal(uvn[a:b], np.array([o[3:5] for o in obs], dtype=np.float32).reshape(-1, 2)), (cam, int(fid))
    return worst


RUNS = [(n, "RR", None) for n in ("band", "two cameras", "cut")] + stereo_ref.PAIRING_RUNS
RUN_IDS = [n if p == "RR" else f"{n}-{p}-{c}" for n, p, c in RUNS]
PAIRING_IDS = RUN_IDS[3:]


@pytest.mark.parametrize("name,pairing,coeffs", RUNS, ids=RUN_IDS)
def test_stream_matches_restatement(pkg, name, pairing, coeffs):
    """band: mask_left all zero and a band in mask_right; two cameras: the right camera's own intrinsics (its undistortion and its
    RANSAC threshold are camera 1's: with camera 0's the restatement gives another result, test_stereo_ref_cpu.py); cut: fewer than
    10 surviving points, then none — the "both masks empty" reset — each followed by a detection on the next pair.
    The pairings (camera 0, camera 1) RE, ER, EE: an equidistant camera carries a coefficient set of test_gpu_equidistant.py on
    the stream's fx fy cx cy.  test_stereo_ref_cpu.py shows that in these runs both cameras' RANSAC decides on at least 10 points in
    every pair, that no decision hangs on a last bit of a normalised coordinate, and that the four pairings end on different lists."""
    s, after, ref = stereo_ref.reference_run(name, pairing, coeffs)
    ctx = _context(pkg, s) if pairing == "RR" else _context(pkg, s, K8=ref.K8, models=ref.models)
    try:
        for f, (t, left, right, ml, mr) in enumerate(s.frames()):
            ctx.tracker_feed_stereo(t, left, right, mask_left=ml, mask_right=mr)
            _assert_state(ctx, after[f], (name, pairing, f))
        worst = _assert_database(ctx, ref)
        print(f"{name} {pairing} {coeffs}: lists of {len(after)} pairs and {len(ref.db)} features' stamps and uv bit-equal; uvn "
              + ", ".join(f"camera {c} ({ref.models[c]}) " + ("bit-equal" if ref.models[c] == "radtan" else f"within {worst[c]} ulp of cam_equi (tolerance 1)")
                          for c in (0, 1)))
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


def _feed_all(ctx, s, after, where, before_frame=None):
    for f, (t, left, right, ml, mr) in enumerate(s.frames()):
        if f >= len(after):
            break
        if before_frame:
            before_frame(f)
        ctx.tracker_feed_stereo(t, left, right, mask_left=ml, mask_right=mr)
        _assert_state(ctx, after[f], (where, f))


@pytest.mark.parametrize("name,pairing,coeffs", stereo_ref.PAIRING_RUNS, ids=PAIRING_IDS)
def test_restatement_on_the_device_undistortion_gives_the_same_lists(pkg, name, pairing, coeffs):
    """the restatement run again with plv_undistort of a helper context per camera in place of cam_equi.undistort / the oracle's:
    the device's normalised coordinates (within 1 ulp) decide everything as the restatement's do.  Should
    test_stream_matches_restatement ever fail, this tells a rounding tie (this fails too) from a fault (this passes)."""
    s, after, ref = stereo_ref.reference_run(name, pairing, coeffs)
    helpers = []
    try:
        for cam in (0, 1):
            h = pkg.Context(pkg.default_config(s.w, s.h))
            helpers.append(h)
            h.set_camera_intrinsics(ref.K8[cam])
            h.set_camera_model(ref.models[cam])
        calls = []

        def device_undistort(cam, uv):
            calls.append(cam)
            return helpers[cam].undistort(uv)

        dev = stereo_ref.StereoRef(s.cfg, ref.K8[0], ref.K8[1], models=ref.models, undistort=device_undistort)
        got = stereo_ref.run_stream(s, dev)
    finally:
        for h in helpers:
            h.close()
    assert calls.count(0) >= 2 * (len(after) - 1) and calls.count(1) >= 2 * (len(after) - 1)
    for f, (a, b) in enumerate(zip(got, after)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (name, pairing, f)
    un = lambda r, cam: np.array([o[3:5] for fid in sorted(r.db) for o in r.db[fid][cam]], dtype=np.float32).reshape(-1, 2)
    for cam in (0, 1):
        d = _ulps(un(dev, cam), un(ref, cam))
        print(f"{name} {pairing} {coeffs} camera {cam} ({ref.models[cam]}): {int((d > 0).sum())} of {d.size} coordinates differ, max {int(d.max())} ulp (tolerance {0 if ref.models[cam] == 'radtan' else 1})")
        assert d.max() <= (0 if ref.models[cam] == "radtan" else 1)


def test_order_of_model_and_configure_does_not_matter(pkg):
    """plv_set_camera_model before or after plv_stereo_configure on a fresh context: camera 0 is equidistant, camera 1 radtan either
    way (ER: the pairing in which a configure that took the context's model for camera 1, or reset it, would show)"""
    s, after, ref = stereo_ref.reference_run("two cameras", "ER", "strong")
    for model_first in (True, False):
        ctx = _context(pkg, s, K8=ref.K8, models=ref.models, model_first=model_first)
        try:
            _feed_all(ctx, s, after[:3], f"model first: {model_first}")
            _assert_database(ctx, _Upto(ref, after[:3], s))
        finally:
            ctx.close()


class _Upto:
    """the restatement's database cut to the first pairs of a run"""

    def __init__(self, ref, after, s):
        t_end = [t for t, *_ in s.frames()][len(after) - 1]
        self.models, self.K8 = ref.models, ref.K8
        self.db = {}
        for fid, (l, r) in ref.db.items():
            l, r = [o for o in l if o[0] <= t_end], [o for o in r if o[0] <= t_end]
            if l or r:
                self.db[fid] = (l, r)


@pytest.mark.parametrize("cam", [0, 1])
def test_set_intrinsics_between_pairs_reaches_the_next_pair(pkg, cam):
    """plv_stereo_set_intrinsics(cam, K) between two pairs, both cameras equidistant: from the next pair on that camera's uvn and
    RANSAC threshold are the new K's, the other camera's stay (the restatement run whose K8[cam] changes at that pair; it differs
    from the unchanged run and is free of rounding ties, test_stereo_ref_cpu.py)"""
    s, after, ref = stereo_ref.changed_run(cam)
    _, _, plain = stereo_ref.reference_run("two cameras", "EE", "strong")
    K_old, K_new = plain.K8, stereo_ref.changed_intrinsics(plain.K8[cam])
    stamps = [t for t, *_ in s.frames()]
    ctx = _context(pkg, s, K8=K_old, models=ref.models)
    try:
        _feed_all(ctx, s, after, f"camera {cam}", lambda f: ctx.stereo_set_intrinsics(cam, K_new) if f == stereo_ref.CHANGE_AT else None)
        worst = _assert_database(ctx, ref, lambda c, t: K_new if c == cam and t >= stamps[stereo_ref.CHANGE_AT] else K_old[c])
        print(f"K8 of camera {cam} changed before pair {stereo_ref.CHANGE_AT}: lists bit-equal, uvn within {worst} ulp of cam_equi (tolerance 1)")
    finally:
        ctx.close()


def test_configure_with_an_unknown_model_leaves_the_pair(pkg):
    s, after, ref = stereo_ref.reference_run("two cameras", "RE", "strong")
    ctx = _context(pkg, s, K8=ref.K8, models=ref.models)
    try:
        _feed_all(ctx, s, after[:2], "before the refusal")
        with pytest.raises(pkg.PlvError) as e:
            ctx.stereo_configure(s.K_left, 2)  # (other intrinsics too: neither they nor the model are taken)
        assert e.value.code == pkg.PLV_E_BADARG and "model" in str(e.value)
        for f, (t, left, right, ml, mr) in enumerate(s.frames()):
            if f in (2, 3):
                ctx.tracker_feed_stereo(t, left, right, mask_left=ml, mask_right=mr)
                _assert_state(ctx, after[f], ("after the refusal", f))
        _assert_database(ctx, _Upto(ref, after[:4], s))
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
