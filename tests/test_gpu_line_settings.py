"""The line detector off its shipped settings, on the GPU, held to the oracle on the case matrix of tests/line_setting_cases.py: canny_kernel
and canny_hyst_kernel (hysteresis, the two cleared corners behind it), the host stage, fld_walk_kernel / fld_fit_kernel (walk mode 1),
the component-parallel kernels (walk mode 2) with buffers, dropped components and chord windows sized by line_length_threshold, the
ahead-of-time detection, the tracker feed with prefetch, and the settings the detector refuses — through plv_detect_lines,
plv_line_detect_launch / _finish, plv_tracker_feed + plv_line_tracker_feed, plv_line_chains and plv_line_walk_info.

Contracts (none of them new): walk mode 0 (the host stage) gives the oracle's detect_lines bit for bit, as test_detect_lines_parity holds
it at the shipped settings; walk modes 1 and 2 give the restated chains exactly (points and order) and the oracle's segments in number
and order within SEG_TOL = 2e-3 px (float rounding of the device fit's atan2 / cos / sin), as test_gpu_line_walk_parallel.py holds them.

The settings of a context are fixed when it is created, so "shipped, hysteresis, shipped again" runs on two contexts of the same image
interleaved; inside one context the paths are switched by the walk mode and the ahead-of-time launch.

Found by these tests: canny_kernel cleared FastLineDetector's two corners itself, in front of canny_hyst_kernel; with hysteresis a strong
pixel inside a cleared corner then promoted nothing.  Measured on the MI355X on corner_tl / corner_br at 30 / 320 with that order: no
chain and no segment in any walk mode, where the oracle keeps 228 / 230 edge pixels, two chains (115 + 113 / 116 + 114 points) and two
segments.  The corners are now cleared by canny_hyst_kernel behind its flood when it runs, and the device returns the oracle's two
segments bit for bit; the equal-thresholds path launches and stores what it did (test_shipped_path_launches_and_copies_nothing_more).
Everything else of the matrix agreed with the oracle at the first run.

Five one-line, value-only mutations (none moves an address), each built into a library of its own on a scratch copy and run once on the
MI355X against this module and against the three line modules the suite had before (test_gpu_linefront.py,
test_gpu_line_walk_parallel.py, test_gpu_frontend.py):

  mutation                                                                 caught here by (first of N failing tests)                     before
  line_kernels.hip  canny_kernel clears the corners with hysteresis too    test_case_in_every_walk_mode[corner_tl-canny30_320] (5)       no
  line_kernels.hip  min_px = 21 in launch_line_labels / _walk_components   test_case_in_every_walk_mode[walk_bar_and_stub-len5] (8)      no
  line_kernels.hip  canny_kernel m > high -> m >= high                     test_case_in_every_walk_mode[faint_band-canny30_48] (1)       no
  line_kernels.hip  launch_line_edges without the swap of low and high     test_case_in_every_walk_mode[fading_bars-canny90_30] (2)      no
  line_api.hip      final filter thr2 = 40 * 40 instead of the setting     test_case_in_every_walk_mode[fading_bars-combined] (25)       no

(m >= high passed the matrix as first written: wherever a bar has a corner the corner's gradient is above the threshold and promotes the
flanks.  faint_band, a band from border to border whose gradient is exactly the high threshold, was added for it.)
"""
import numpy as np
import pytest
from scipy import ndimage

import line_setting_cases as lc
import oracle_lib
import synth
import test_gpu_linefront as linefront
from test_gpu_line_walk_parallel import SEG_TOL, assert_same_chains, detect_in_mode

pytestmark = pytest.mark.gpu

_EIGHT = np.ones((3, 3), dtype=int)


@pytest.fixture(scope="module")
def lo():
    return oracle_lib.load_line()


def _ctx(pkg, image_name, setting):
    """a context of the case's settings with the case's image fed; level 0 is the image as drawn (histogram_method 0)"""
    ctx = pkg.Context(lc.config(pkg, image_name, setting))
    img = lc.image(image_name)
    ctx.feed_image(img)
    assert np.array_equal(ctx.pyramid_level(0, 0), img)
    return ctx


def _equal_thresholds(setting):
    return lc.SETTINGS[setting]["c1"] == lc.SETTINGS[setting]["c2"]


def _assert_segments_close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if len(ref):
        err = float(np.abs(got - ref).max())
        print(what, "segments", len(ref), "max |device - oracle|", err)
        assert err < SEG_TOL, (what, err)


# ------------------------------------------------------------------------------------------------ the matrix, every route
@pytest.mark.parametrize("image_name,setting", lc.CASES, ids=lc.CASE_IDS)
def test_case_in_every_walk_mode(pkg, lo, image_name, setting):
    ref = lc.reference(lo, image_name, setting)
    what = f"{image_name}-{setting}"
    ctx = _ctx(pkg, image_name, setting)
    try:
        # mode 0, the host stage: the oracle's segments bit for bit
        got = ctx.detect_lines(0)
        print(what, "mode 0:", len(got), "segments, oracle", len(ref["segs"]), "| reference edges", int(ref["edges"].sum()), "chains", len(ref["chains"]))
        assert got.shape == ref["segs"].shape and np.array_equal(got, ref["segs"]), (what, got.shape, ref["segs"].shape)
        assert ctx.line_walk_info()["mode"] == 0
        # mode 1: one wave walks, one lane per chain fits
        s1, c1, i1 = detect_in_mode(ctx, 1)
        print(what, "mode 1:", i1)
        assert i1["mode"] == 1 and i1["fell_back"] == 0 and i1["n_chains"] == len(ref["chains"]), (what, i1, len(ref["chains"]))
        assert_same_chains(c1, ref["chains"], what + ": mode 1")
        _assert_segments_close(s1, ref["segs"], what + ": mode 1")
        # mode 2: by components with equal thresholds; with hysteresis it hands over to mode 1's kernels and says so
        s2, c2, i2 = detect_in_mode(ctx, 2)
        print(what, "mode 2:", i2)
        if _equal_thresholds(setting):
            assert i2["mode"] == 2 and i2["fell_back"] == 0, (what, i2)
            sizes = np.bincount(ndimage.label(ref["edges"], structure=_EIGHT)[0].ravel())[1:]
            assert i2["n_components"] == int((sizes >= lc.SETTINGS[setting]["length"] + 1).sum()), (what, i2, sizes)
            assert i2["longest_component"] == (int(sizes.max()) if i2["n_components"] else 0), (what, i2)
        else:
            assert i2["mode"] == 1 and i2["fell_back"] == 1 and i2["n_components"] == 0, (what, i2)
        assert i2["n_chains"] == len(ref["chains"]), (what, i2, len(ref["chains"]))
        assert_same_chains(c2, ref["chains"], what + ": mode 2")
        assert s2.shape == s1.shape and np.array_equal(s2, s1), (what, s2.shape, s1.shape)
        # ... and the host stage again behind the device modes
        again = ctx.detect_lines(0)
        assert again.shape == got.shape and np.array_equal(again, got), what
    finally:
        ctx.close()


def test_swapped_thresholds_are_the_same_detection(pkg, lo):
    a, b = _ctx(pkg, "fading_bars", "canny90_30"), _ctx(pkg, "fading_bars", "canny30_90")
    try:
        for mode in (0, 1):
            a.line_walk_mode(mode), b.line_walk_mode(mode)
            sa, sb = a.detect_lines(0), b.detect_lines(0)
            assert len(sa) > 0 and sa.shape == sb.shape and np.array_equal(sa, sb), mode
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------------------------------------ the corners
@pytest.mark.parametrize("name", list(lc.CORNERS))
def test_corners_are_cleared_behind_the_hysteresis(pkg, lo, name):
    """strong only inside a cleared corner: the oracle promotes the weak diagonal from there and clears the corner afterwards"""
    ref = lc.reference(lo, name, "canny30_320")
    assert len(ref["segs"]) >= 1 and len(ref["chains"]) >= 1
    ctx = _ctx(pkg, name, "canny30_320")
    try:
        got = ctx.detect_lines(0)
        s1, c1, i1 = detect_in_mode(ctx, 1)
        print(name, "device: segments", got.tolist(), "chains", [len(c) for c in c1], "| oracle: segments", ref["segs"].tolist(), "chains", [len(c) for c in ref["chains"]])
        assert got.shape == ref["segs"].shape and np.array_equal(got, ref["segs"]), (got.shape, ref["segs"].shape)
        assert_same_chains(c1, ref["chains"], name)
        rows, cols = lc.CORNERS[name]
        h, w = ref["edges"].shape
        inside = np.zeros((h, w), dtype=bool)
        inside[rows, cols] = True
        assert not any(inside[p[1], p[0]] for c in c1 for p in c), "a chain point inside a cleared corner"
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the shipped path stays what it was
def test_shipped_path_launches_and_copies_nothing_more(pkg, lo):
    """equal thresholds, host stage: ONE launch (the edge kernel stores its maps where the host reads them) and no copy, synchronous or
    ahead of time (there with the four label kernels); with hysteresis the flood kernel and the two copies of the maps appear"""
    def run(setting, ahead):
        ctx = _ctx(pkg, "fading_bars", setting)
        try:
            ctx.detect_lines(0)                 # (buffers, streams and events exist from here on)
            ctx.synchronize()
            ctx.prof_enable(True)
            ctx.prof_reset()
            c0 = pkg.counters()
            if ahead:
                ctx.line_detect_launch(0)
            segs = ctx.detect_lines(0)
            c1 = pkg.counters()
            ctx.prof_enable(False)
            table = {k: n for k, (n, _) in ctx.prof_table().items() if n}
            assert np.array_equal(segs, lc.reference(lo, "fading_bars", setting)["segs"])
            return table, c1["launches"] - c0["launches"], c1["copies"] - c0["copies"]
        finally:
            ctx.close()
    labels = ("ccl_boundary_kernel", "ccl_roots_kernel", "ccl_assign_kernel", "ccl_flatten_kernel")
    got = [run("shipped", False), run("canny120_120", False), run("shipped", True)[1:], run("canny30_90", False), run("canny30_90", True)[1:]]
    print(got)
    assert got == [({"half_canny_kernel": 1}, 1, 0), ({"half_canny_kernel": 1}, 1, 0), (1 + len(labels), 0),
                   ({"half_canny_kernel": 1, "canny_hyst_kernel": 1}, 2, 2), (2, 2)], got


# ------------------------------------------------------------------------------------------------ ahead of time
@pytest.mark.parametrize("image_name,setting", [("fading_bars", "canny20_200"), ("tex333", "canny30_90"), ("tex333", "len5"), ("tex98", "len5_min12"),
                                                ("corner_br", "canny30_320")])
def test_detection_ahead_of_time_gives_the_same_bytes(pkg, lo, image_name, setting):
    """plv_line_detect_launch / _finish off the shipped settings: with hysteresis the route copies its maps instead of receiving them
    from the kernel and labels nothing; with a short length threshold the label kernels drop components by another min_px"""
    ref = lc.reference(lo, image_name, setting)["segs"]
    ctx = _ctx(pkg, image_name, setting)
    try:
        ctx.feed_image(lc.image(image_name))           # (a second time: there is a previous image, PLV_PYR_LAST)
        sync = ctx.detect_lines(0)
        assert len(ref) > 0 and sync.shape == ref.shape and np.array_equal(sync, ref)
        ctx.line_detect_launch(0)
        ctx.line_detect_finish(0)
        a = ctx.detect_lines(0)
        ctx.line_detect_launch(0)                      # launch without finish: the next detection joins it
        b = ctx.detect_lines(0)
        ctx.line_detect_launch(1)                      # asked for the other image: a detection of image 0 starts from scratch
        c = ctx.detect_lines(0)
        for got in (a, b, c):
            assert got.shape == sync.shape and got.tobytes() == sync.tobytes()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ through the tracker
@pytest.mark.parametrize("setting", ["canny30_90", "combined"])
def test_tracker_feed_with_prefetch(pkg, lo, setting):
    """test_line_tracker_stream's three frames and its oracle composition, the context and lo.detect_lines on the case's settings, the
    frame's lines detected ahead by the point tracker's feed (with hysteresis: launched behind the pyramid, maps copied)"""
    W, H = linefront.W, linefront.H
    canvas = synth.texture_canvas(W, H, seed=11, blobs=200, lines=120)
    frames = [synth.render_frame(canvas, W, H, tx=3.0 * i, ty=-2.0 * i, rot_deg=0.2 * i) for i in range(3)]
    s = lc.SETTINGS[setting]
    cfg = pkg.default_config(W, H)
    cfg.line_length_threshold, cfg.line_distance_threshold = s["length"], s["dist"]
    cfg.canny_th1, cfg.canny_th2, cfg.line_min_length_px = s["c1"], s["c2"], s["min_len"]
    linefront._line_tracker_stream(pkg, lo, frames, W, H, cfg=cfg, detect_args=lc.oracle_args(setting), prefetch=True)


# ------------------------------------------------------------------------------------------------ order
def test_nothing_of_the_other_path_stays_behind(pkg, lo):
    """shipped, hysteresis, shipped again on the same image (two contexts: a context's settings are fixed at its creation), every round
    through the host stage, the ahead-of-time launch and walk mode 2: the third result is the first bit for bit, and each context gives
    the oracle's result for its own settings; then two other images through both, interleaved"""
    names = ("fading_bars", "walk_t_and_cross", "corner_tl")
    a, b = _ctx(pkg, names[0], "shipped"), _ctx(pkg, names[0], "canny20_200")
    try:
        def rounds(ctx):
            host = ctx.detect_lines(0)
            ctx.line_detect_launch(0)
            ahead = ctx.detect_lines(0)
            dev, chains, info = detect_in_mode(ctx, 2)
            return host, ahead, dev, chains
        first, other, third = rounds(a), rounds(b), rounds(a)
        for x, y in zip(first[:3], third[:3]):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        assert_same_chains(third[3], first[3], "shipped again")
        assert np.array_equal(first[0], lc.reference(lo, names[0], "shipped")["segs"]) and np.array_equal(first[1], first[0])
        assert np.array_equal(other[0], lc.reference(lo, names[0], "canny20_200")["segs"]) and np.array_equal(other[1], other[0])
        assert not np.array_equal(first[0], other[0])
        assert_same_chains(other[3], lc.reference(lo, names[0], "canny20_200")["chains"], "hysteresis between")
        for name in names[1:] + names[:1]:
            for ctx, setting in ((a, "shipped"), (b, "canny20_200"), (a, "shipped")):
                ctx.feed_image(lc.image(name))
                got = ctx.detect_lines(0)
                ref = lo.detect_lines(lc.image(name), *lc.oracle_args(setting))
                assert got.shape == ref.shape and np.array_equal(got, ref), (name, setting)
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------------------------------------ refusals
BAD = [("canny_aperture", 5), ("canny_aperture", 0), ("line_length_threshold", 0), ("line_length_threshold", -3), ("line_distance_threshold", 0.0),
       ("line_distance_threshold", -1.0), ("line_distance_threshold", float("nan")), ("line_distance_threshold", float("inf")),
       ("line_min_length_px", -1.0), ("line_min_length_px", float("nan")), ("line_min_length_px", float("inf")), ("canny_th1", -1), ("canny_th2", -50)]


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_settings_the_detector_cannot_honour_are_refused(pkg, lo, field, value):
    """PLV_E_BADARG and a message that names the field, from plv_detect_lines (every walk mode), the ahead-of-time launch and finish and
    the tracker feeds, with and without prefetch; no kernel is launched by the refused call, and the context goes on feeding images and
    tracking points"""
    img = lc.image("walk_bars")
    h, w = img.shape
    cfg = pkg.default_config(w, h)
    cfg.histogram_method = 0
    setattr(cfg, field, value)
    vps = lo.vanishing_points(np.eye(3), np.array(list(cfg.intrinsics)))
    ctx = pkg.Context(cfg)

    def refused(call, *args):
        ctx.synchronize()
        before = pkg.counters()["launches"]
        with pytest.raises(pkg.PlvError) as e:
            call(*args)
        assert e.value.code == pkg.PLV_E_BADARG and field in str(e.value), (call.__name__, str(e.value))
        assert pkg.counters()["launches"] == before, call.__name__
    try:
        ctx.feed_image(img)
        for mode in (0, 1, 2):
            ctx.line_walk_mode(mode)
            refused(ctx.detect_lines, 0)
        ctx.line_walk_mode(0)
        refused(ctx.line_detect_launch, 0)
        refused(ctx.line_detect_finish, 0)
        pts, ids = synth.grid_points(w, h, 50, seed=2), np.arange(1, 51, dtype=np.uint64)
        refused(ctx.line_tracker_feed_points, 1.0, vps, pts, ids)
        for prefetch in (False, True):
            ctx.line_prefetch_mode(prefetch)
            ctx.tracker_feed(2.0 + prefetch, img)          # the point tracker's feed goes through (ahead-of-time launch refused inside, silently)
            refused(ctx.line_tracker_feed, 2.0 + prefetch, vps)
        ctx.line_prefetch_mode(False)
        assert len(ctx.line_tracker_last()[1]) == 0 and ctx.line_db_size() == 0
        # the context is usable: images, the pyramid and the point tracker
        ctx.feed_image(lc.image("walk_disc"))
        assert np.array_equal(ctx.pyramid_level(0, 0), lc.image("walk_disc"))
        ctx.tracker_feed(4.0, img)
        pts_last, ids_last = ctx.tracker_last()
        assert len(pts_last) == len(ids_last)
    finally:
        ctx.close()
    # ... and the same image on a context with the shipped settings is detected as ever
    good = _ctx(pkg, "walk_bars", "shipped")
    try:
        assert np.array_equal(good.detect_lines(0), lc.reference(lo, "walk_bars", "shipped")["segs"])
    finally:
        good.close()
