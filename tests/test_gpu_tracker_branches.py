"""GPU tests of the monocular tracker feed (plv_tracker_feed and its siblings, tracker_api.hip) against tests/mono_ref.py, the
restatement of TrackKLT::feed_monocular on the CPU oracle's primitives, over the streams test_mono_ref_cpu.py shows to reach every
branch: masks that change, frames that lose every track, the fewer-than-10 frame and the n == 0 reset, each followed by a detection on
the next image.  Everything is compared bit for bit (the front end is bit-reproducible by design): the last points and ids and the
stored mask after every frame, the whole database at the end.  The same streams under the three detect-ahead modes, through the
staged / encoded / downsampled routes, under the three histogram methods and with the line prefetch on; the database calls at their
edges; CLAHE at tile sizes other than the front-end test's 94 x 60."""
import ctypes as C
import functools

import numpy as np
import pytest

import mono_ref
import oracle_lib
import synth
import track_image_ref as R

pytestmark = pytest.mark.gpu

MASK_LAYER = R.MASK


def _context(pkg, s, method=mono_ref.HISTOGRAM, **more):
    cfg = pkg.default_config(s.w, s.h)
    cfg.num_features, cfg.grid_x, cfg.grid_y = s.cfg.num_features, s.cfg.grid_x, s.cfg.grid_y
    cfg.min_px_dist, cfg.fast_threshold, cfg.histogram_method = s.cfg.min_px_dist, s.cfg.fast_threshold, method
    for i, v in enumerate(s.K):
        cfg.intrinsics[i] = float(v)
    for k, v in more.items():
        setattr(cfg, k, v)
    return pkg.Context(cfg)


def _assert_lists(ctx, want, where):
    pts, ids = ctx.tracker_last()
    assert np.array_equal(ids, want[1]), (where, "ids", len(ids), len(want[1]))
    assert pts.dtype == want[0].dtype and np.array_equal(pts, want[0]), (where, "points")


def _assert_stored_mask(ctx, mask, where):
    """the mask the tracker holds as its last one, read back through the track image's mask layer (its set pixels tint the current
    image; none stored: the plain image)"""
    grey = ctx.pyramid_level(0, 0)
    assert np.array_equal(ctx.track_image(MASK_LAYER), R.render(grey, R.prims_array([]), mask)), (where, "stored mask")


def _run(ctx, s, after, feed=None, between=None, masks=True):
    feed = feed or (lambda t, img, mask: ctx.tracker_feed(t, img, mask))
    for f, (t, img, mask) in enumerate(s.frames()):
        feed(t, img, mask)
        _assert_lists(ctx, after[f], (s.name, f))
        if masks:
            _assert_stored_mask(ctx, after[f][2], (s.name, f))
        if between:
            between(f)


@pytest.mark.parametrize("name", mono_ref.STREAMS)
def test_stream_matches_restatement(pkg, name):
    """band: a mask on every frame, one band of 128 and one of 127 (`> 127`), jumps that carry points out of the image; cut: fewer than
    10 points, then every track lost under an all-255 mask, each followed by a detection on the next image; strip: the n == 0 reset
    behind the top-up; regain: the detection after a loss under a mask"""
    s, after, ref = mono_ref.reference_run(name)
    ctx = _context(pkg, s)
    try:
        _run(ctx, s, after)
        mono_ref.assert_database(ctx, ref.db)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", mono_ref.STREAMS)
def test_detection_modes_give_the_same_lists(pkg, name, mode):
    """mode 1 starts the next frame's top-up at the end of every feed that kept a point (plv_perform_detection_ahead, with the frame's
    mask); the feeds that end with empty lists start none and the next feed detects on its own image"""
    s, after, ref = mono_ref.reference_run(name)
    ctx = _context(pkg, s)
    try:
        ctx.tracker_detect_ahead(mode)
        _run(ctx, s, after, masks=False)
        mono_ref.assert_database(ctx, ref.db)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["band", "cut"])
def test_a_detection_between_two_feeds_does_not_reach_the_next_feed(pkg, name):
    """mode 1: a detection of the caller's on the current image, with points of its own, meets the job the feed started ahead; that
    job is not the caller's and must not answer it, and the next feed (whose job is gone) still tops up as the restatement does"""
    s, after, ref = mono_ref.reference_run(name)
    do = oracle_lib.load_detect()
    ctx = _context(pkg, s)
    other = np.float32([[40.5, 50.25], [120.0, 90.0], [15.0, 15.0]])
    other_ids = np.uint64([900001, 900002, 900003])

    def between(f):
        if f % 2 == 0:
            eq = ctx.pyramid_level(0, 0)
            got = ctx.perform_detection(0, other, other_ids, 950000)
            want = do.perform_detection(eq, None, other, other_ids, 950000, s.cfg.num_features, s.cfg.grid_x, s.cfg.grid_y, s.cfg.min_px_dist,
                                        s.cfg.fast_threshold)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and got[2] == want[2], f

    try:
        ctx.tracker_detect_ahead(1)
        _run(ctx, s, after, between=between, masks=False)
        mono_ref.assert_database(ctx, ref.db)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _band_with_images_fed_past_the_tracker():
    """band with another image fed past the tracker (plv_feed_image) behind frames 4 and 5: (stream, the extra image per frame, lists
    after every frame, the restatement)"""
    s = mono_ref.stream("band")
    canvas = synth.texture_canvas(s.w, s.h, seed=42)
    extra = {f: synth.render_frame(canvas, s.w, s.h, tx=s.offsets[f][0] + 1.0, ty=s.offsets[f][1]) for f in (4, 5)}
    ref = mono_ref.OracleTracker(s.cfg, s.K)
    after = []
    for f, (t, img, mask) in enumerate(s.frames()):
        ref.feed(t, img, mask)
        after.append((ref.pts.copy(), ref.ids.copy(), ref.mask_last))
        if f in extra:
            ref.feed_image(extra[f])
    return s, extra, after, ref


def test_a_stale_job_is_not_taken_by_the_feeds_own_top_up(pkg):
    """mode 1: the feed of frame f starts the next top-up ahead on image f; an image fed past the tracker then becomes the last image,
    so the next feed's own top-up (PLV_PYR_LAST, the very points and mask the job was started with) meets a job that is one image
    old: it must detect in place, on the image that is the last one now.  The extra images are frame 4 and 5 shifted by a pixel, and
    the top-ups behind them add corners (their positions are that image's): a feed that took the stale job gives other points."""
    s, extra, after, ref = _band_with_images_fed_past_the_tracker()
    assert "top-up adds" in ref.frames[5] and "top-up adds" in ref.frames[6]
    plain = mono_ref.reference_run("band")[1]
    assert not np.array_equal(after[5][0], plain[5][0]) and not np.array_equal(after[6][0], plain[6][0])
    ctx = _context(pkg, s)
    try:
        ctx.tracker_detect_ahead(1)
        _run(ctx, s, after, between=lambda f: ctx.feed_image(extra[f]) if f in extra else None, masks=False)
        mono_ref.assert_database(ctx, ref.db)
    finally:
        ctx.close()


@pytest.mark.parametrize("route", ["staged", "encoded"])
def test_routes_give_the_same_lists(pkg, route):
    """band, its mask and its lost tracks through plv_image_stage + plv_tracker_feed_staged and through plv_tracker_feed_encoded"""
    s, after, ref = mono_ref.reference_run("band")
    ctx = _context(pkg, s)

    def staged(t, img, mask):
        slot = int(round((t - 10.0) / 0.05)) % 8
        ctx.image_stage(slot, img)
        ctx.tracker_feed_staged(t, slot, mask)

    try:
        _run(ctx, s, after, feed=staged if route == "staged" else (lambda t, img, mask: ctx.tracker_feed_encoded(t, img, "mono8", mask)))
        mono_ref.assert_database(ctx, ref.db)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _halved_band():
    """band rendered at 640 x 480 with its offsets and its mask doubled, halved by the oracle: (stream at 320 x 240, the full-size
    frames, the restatement over the halved ones)"""
    s = mono_ref.stream("band")
    fo = oracle_lib.load_front()
    canvas = synth.texture_canvas(2 * s.w, 2 * s.h, seed=42)
    big = [(t, synth.render_frame(canvas, 2 * s.w, 2 * s.h, tx=2 * tx, ty=2 * ty), np.repeat(np.repeat(mask, 2, axis=0), 2, axis=1))
           for (t, _, mask), (tx, ty) in zip(s.frames(), s.offsets)]
    ref = mono_ref.OracleTracker(s.cfg, s.K)
    after = []
    for t, img, mask in big:
        ref.feed(t, fo.downsample(img), fo.downsample(mask))
        after.append((ref.pts.copy(), ref.ids.copy(), ref.mask_last))
    return s, big, after, ref


def test_downsampled_route_with_a_mask_and_lost_tracks(pkg):
    s, big, after, ref = _halved_band()
    fo = oracle_lib.load_front()
    assert ref.stats["dropped on the current mask"] > 0 and ref.stats["dropped as out of image"] > 0 and ref.stats["top-up adds"] > 0
    a, b = _context(pkg, s), _context(pkg, s)
    try:
        for f, (t, img, mask) in enumerate(big):
            a.tracker_feed_downsampled(t, img, mask)
            b.tracker_feed(t, fo.downsample(img), fo.downsample(mask))
            _assert_lists(a, after[f], ("downsampled", f))
            _assert_lists(b, after[f], ("halved by the oracle", f))
            _assert_stored_mask(a, after[f][2], ("downsampled", f))
        mono_ref.assert_database(a, ref.db)
        mono_ref.assert_database(b, ref.db)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("method", [mono_ref.NONE, mono_ref.HISTOGRAM, mono_ref.CLAHE], ids=["none", "histogram", "clahe"])
def test_histogram_methods(pkg, method):
    s, after, ref = mono_ref.reference_run("band", method)
    assert min(len(a[1]) for a in after) >= 1 and max(len(a[1]) for a in after) >= 30
    ctx = _context(pkg, s, method)
    try:
        _run(ctx, s, after)
        mono_ref.assert_database(ctx, ref.db)
    finally:
        ctx.close()


def _line_state(ctx):
    lines, ids = ctx.line_tracker_last()
    rel_ptr, rel_id = ctx.line_tracker_last_points()
    return lines, ids, rel_ptr, rel_id


# how the line detector's pixel work gets onto the stream of a feed with plv_line_prefetch_mode on:
#   "hook": the shipped equal Canny thresholds — the image feed launches it between histogram and pyramid (plv_ctx::edges_hook,
#           plv_line_edges_early), tracker_feed_fed finds edges_hook_fired and launches nothing itself, whichever exit it then takes;
#   "feed": thresholds with hysteresis — the hook declines (line_api.hip: canny_th1 != canny_th2), and tracker_feed_fed's own
#           launch_prefetch() runs on the exit the frame takes: the detection on the current image, the n == 0 reset, the matching.
PREFETCH = {"hook": dict(canny_th1=50, canny_th2=50), "feed": dict(canny_th1=30, canny_th2=90)}


@pytest.mark.parametrize("how", sorted(PREFETCH))
@pytest.mark.parametrize("name", ["cut", "strip"])
def test_line_prefetch_on_every_exit(pkg, name, how):
    """The line feed of every frame, the frames that end with empty lists included, gives the lines, ids and line database of a
    context without prefetch, and the point lists stay the restatement's.  That the work was launched inside the tracker feed, on
    every frame and so on each of the three exits (cut: detection on the current image in frames 0, 4 and 6, matching in the others;
    strip: the n == 0 reset in frame 3), shows in the library's launch counter: the tracker feed of the prefetching context issues
    more launches than the other context's, its line feed fewer (the edge kernel is not launched twice).  A launch that is missing
    shows there; one on the wrong image or in the wrong order shows in the bytes.
    With the shipped line settings these small frames have hardly a line; with chains from 5 and segments from 12 px on (a setting
    test_gpu_line_settings.py holds to the oracle) the oracle keeps 43 lines with points on them over cut and 46 over strip under
    the shipped thresholds, none on the frames whose lists are empty."""
    s, after, ref = mono_ref.reference_run(name)
    exits = {"cut": {3: "fewer than 10 points", 4: "detection after a loss, without a mask", 5: "everything lost"},
             "strip": {3: "n == 0 reset", 4: "detection after a loss, without a mask"}}[name]
    for f, what in exits.items():
        assert what in ref.frames[f], (f, what)
    a, b = (_context(pkg, s, line_length_threshold=5, line_min_length_px=12.0, **PREFETCH[how]) for _ in range(2))
    try:
        a.line_prefetch_mode(True)
        vps = a.vanishing_points(np.eye(3), s.K)
        n_lines = 0
        for f, (t, img, mask) in enumerate(s.frames()):
            launches = {}
            for c in (a, b):
                n0 = pkg.counters()["launches"]
                c.tracker_feed(t, img, mask)
                n1 = pkg.counters()["launches"]
                c.line_tracker_feed(t, vps)
                launches[c] = (n1 - n0, pkg.counters()["launches"] - n1)
                _assert_lists(c, after[f], (name, f))
            assert launches[a][0] > launches[b][0] and launches[a][1] < launches[b][1], (name, how, f, launches[a], launches[b])
            for x, y, what in zip(_line_state(a), _line_state(b), ("lines", "line ids", "rel_ptr", "rel_id")):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, f, what)
            n_lines += len(a.line_tracker_last()[1])
        assert n_lines >= 20  # (there were lines to compare)
        ids = b.line_db_ids()
        assert np.array_equal(a.line_db_ids(), ids) and a.line_db_size() == b.line_db_size() == len(ids)
        ea, eb = a.line_db_export(ids), b.line_db_export(ids)
        for k in eb:
            assert ea[k].dtype == eb[k].dtype and ea[k].tobytes() == eb[k].tobytes(), (name, k)
        mono_ref.assert_database(a, ref.db)
        mono_ref.assert_database(b, ref.db)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------- the database calls
@pytest.fixture(scope="module")
def band_db(pkg):
    """a context that has run `band` (tracks that ended at the jumps, tracks the top-ups of frames 5 and 6 began)"""
    s, after, ref = mono_ref.reference_run("band")
    ctx = _context(pkg, s)
    for t, img, mask in s.frames():
        ctx.tracker_feed(t, img, mask)
    yield ctx, s, ref
    ctx.close()


def test_db_select_at_below_and_above_an_observation_time(band_db):
    ctx, s, ref = band_db
    T = s.times()
    told = {0: set(), 1: set()}
    for tq in (T[4], T[5], T[6]):
        for t in (np.nextafter(tq, 0.0), tq, np.nextafter(tq, np.inf)):
            for mode in (0, 1):
                want = mono_ref.db_select(ref.db, mode, t)
                assert np.array_equal(ctx.db_select(mode, t), want), (mode, t)
                told[mode].add(want.tobytes())
    # (the stamp itself and its two neighbours do not all give one answer: `>=` and `<` at the stamp are what is looked at)
    first_seen = {obs[0][0] for obs in ref.db.values()}
    last_seen = {obs[-1][0] for obs in ref.db.values()}
    assert {T[5], T[6]} <= first_seen and {T[4], T[5]} <= last_seen
    assert len(told[0]) >= 4 and len(told[1]) >= 3
    assert np.array_equal(ctx.db_select(1, np.inf), np.array(sorted(ref.db), dtype=np.uint64)) and len(ctx.db_select(0, -np.inf)) == 0


def test_db_export_of_absent_ids_and_one_short(pkg, band_db):
    ctx, s, ref = band_db
    present = np.array(sorted(ref.db), dtype=np.uint64)
    absent = np.uint64([int(present[-1]) + 1, 10 ** 12])
    ptr, t, uv, uvn = ctx.db_export(absent)
    assert ptr.tolist() == [0, 0, 0] and len(t) == len(uv) == len(uvn) == 0
    mixed = np.concatenate([absent[:1], present[:3], absent[1:], present[3:5]])
    for g, w in zip(ctx.db_export(mixed), mono_ref.db_export(ref.db, mixed)):
        assert np.array_equal(g, w)
    # one observation short: PLV_E_CAPACITY, and nothing written behind the capacity (nor anything of the track that does not fit)
    want = mono_ref.db_export(ref.db, present)
    total = int(want[0][-1])
    cap = total - 1
    ptr = np.full(len(present) + 1, -7, dtype=np.int32)
    t, uv, uvn = np.full(total + 8, -7.0), np.full((total + 8, 2), -7.0, np.float32), np.full((total + 8, 2), -7.0, np.float32)
    u64p, ip, dp, fp = C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)
    rc = ctx.lib.plv_db_export_tracks(ctx.h, present.ctypes.data_as(u64p), len(present), ptr.ctypes.data_as(ip), t.ctypes.data_as(dp),
                                      uv.ctypes.data_as(fp), uvn.ctypes.data_as(fp), cap)
    assert rc == pkg.PLV_E_CAPACITY
    fits = int(want[0][-2])  # (every track but the last fits)
    assert np.array_equal(ptr[:-1], want[0][:-1]) and ptr[-1] == -7
    assert np.array_equal(t[:fits], want[1][:fits]) and np.array_equal(uv[:fits], want[2][:fits]) and np.array_equal(uvn[:fits], want[3][:fits])
    assert (t[fits:] == -7.0).all() and (uv[fits:] == -7.0).all() and (uvn[fits:] == -7.0).all()


def test_db_disparity_is_the_restatements(band_db):
    ctx, s, ref = band_db
    T = s.times()
    for a, b in ((1, 2), (2, 3), (1, 3), (3, 4), (6, 7), (7, 6)):
        want = mono_ref.db_disparity(ref.db, T[a], T[b])
        assert want[2] >= 10
        assert ctx.db_disparity(T[a], T[b]) == want, (a, b)
    # fewer than two common tracks: nothing was observed at the first frame's stamp, nothing between two stamps
    for t0, t1 in ((T[0], T[1]), (T[1], np.nextafter(T[2], 0.0)), (T[1], T[1] + 100.0)):
        assert mono_ref.db_disparity(ref.db, t0, t1) == (-1.0, -1.0, 0)
        assert ctx.db_disparity(t0, t1) == (-1.0, -1.0, 0)


def test_db_cleanup_and_removal_exactly(pkg):
    """cleanup_measurements at observation times (the observation at that very time stays) and just above one (it goes), then
    removal of present, absent and repeated ids"""
    s, after, ref = mono_ref.reference_run("band")
    ctx = _context(pkg, s)
    try:
        for t, img, mask in s.frames():
            ctx.tracker_feed(t, img, mask)
        T = s.times()
        db = mono_ref.db_copy(ref.db)
        for t in (T[3], T[4], np.nextafter(T[5], np.inf)):
            before = len(db)
            ctx.db_cleanup_measurements(t)
            mono_ref.db_cleanup_measurements(db, t)
            mono_ref.assert_database(ctx, db)
            assert 0 < len(db) < before, t  # (tracks went with their last observation, others stayed)
            # tracks last seen at the cut's own time are still there, with that one observation.  This pins the library's `< t`
            # (mono_ref.db_cleanup_measurements); Feature::clean_older_measurements of the reference drops `<= t`.  Whoever aligns
            # the library and the compiled oracle with the reference changes the restatement, and this assertion to its opposite.
            if t == T[4]:
                assert any(len(obs) == 1 and obs[0][0] == T[4] for obs in db.values())
        have = sorted(db)
        gone = [have[0], have[2], 10 ** 12, have[0], have[-1], have[-1] + 1]
        ctx.db_remove(np.uint64(gone))
        mono_ref.db_remove(db, gone)
        assert ctx.db_size() == len(have) - 3
        mono_ref.assert_database(ctx, db)
        ctx.db_remove(np.uint64(gone))  # (all of them absent now)
        ctx.db_remove(np.zeros(0, np.uint64))
        # the disparity's boundary: two tracks seen at both stamps give a result, one alone gives (-1, -1, 0)
        both = [fid for fid in sorted(db) if {T[6], T[7]} <= {o[0] for o in db[fid]}]
        assert len(both) >= 3
        for left in (2, 1):
            ctx.db_remove(np.uint64(both[left:]))
            mono_ref.db_remove(db, both[left:])
            want = mono_ref.db_disparity(db, T[6], T[7])
            assert want[2] == (2 if left == 2 else 0) and (left == 2 or want == (-1.0, -1.0, 0))
            assert ctx.db_disparity(T[6], T[7]) == want, left
        mono_ref.assert_database(ctx, db)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- CLAHE off the 94 x 60 tile
@pytest.mark.parametrize("w,h", sorted(mono_ref.CLAHE_SIZES))
def test_clahe_at_other_tile_sizes(pkg, w, h):
    """feed_image under PLV_HIST_CLAHE against FrontOracle.clahe and the oracle's pyramid of it, level 0 and level 2 (40 x 40, the
    size whose clip is the floor of 1, has two levels: its level 1), for the images test_mono_ref_cpu.py counts the redistribution
    cases of"""
    fo = oracle_lib.load_front()
    cfg = pkg.default_config(w, h)
    cfg.histogram_method = mono_ref.CLAHE
    ctx = pkg.Context(cfg)
    try:
        for kind in mono_ref.CLAHE_IMAGES:
            img = mono_ref.clahe_image(w, h, kind)
            ctx.feed_image(img)
            eq = fo.clahe(img)
            pyr = fo.pyramid(eq)
            assert ctx.pyramid_levels(0) == pyr.levels == (2 if (w, h) == (40, 40) else pyr.levels) and pyr.levels >= 2
            top = min(2, pyr.levels - 1)
            assert np.array_equal(ctx.pyramid_level(0, 0), eq), (kind, "level 0", int((ctx.pyramid_level(0, 0) != eq).sum()))
            assert np.array_equal(ctx.pyramid_level(0, top), pyr.level(top)[0]), (kind, "level", top)
    finally:
        ctx.close()


def test_clahe_refuses_a_size_its_tiles_do_not_divide(pkg):
    cfg = pkg.default_config(100, 100)
    cfg.histogram_method = mono_ref.CLAHE
    ctx = pkg.Context(cfg)
    try:
        img = mono_ref.clahe_image(320, 240, "noise")[:100, :100]
        with pytest.raises(pkg.PlvError) as e:
            ctx.feed_image(img)
        assert e.value.code == pkg.PLV_E_BADARG and "100x100" in str(e.value)
        assert ctx.pyramid_levels(0) == 0
        with pytest.raises(pkg.PlvError):
            ctx.pyramid_level(0, 0)
        with pytest.raises(pkg.PlvError) as e:
            ctx.tracker_feed(1.0, img)
        assert e.value.code == pkg.PLV_E_BADARG and "100x100" in str(e.value)
        assert ctx.pyramid_levels(0) == 0 and len(ctx.tracker_last()[1]) == 0 and ctx.db_size() == 0
    finally:
        ctx.close()
