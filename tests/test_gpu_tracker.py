"""GPU test of the tracker frame logic (TrackKLT::feed_monocular mirror) + feature database over a
synthetic 752x480 stream, against the same frame logic composed from the CPU oracle pieces."""
import numpy as np
import pytest

import mono_ref
import oracle_lib
import synth
from mono_ref import OracleTracker

pytestmark = pytest.mark.gpu


def test_tracker_stream_matches_oracle(pkg):
    w, h = 752, 480
    canvas = synth.texture_canvas(w, h, seed=42)
    rng = np.random.default_rng(5)
    cfg = pkg.default_config(w, h)
    ctx = pkg.Context(cfg)
    ot = OracleTracker(cfg, np.array(list(cfg.intrinsics)))
    tx = ty = rot = 0.0
    for f in range(7):
        img = synth.render_frame(canvas, w, h, tx=tx, ty=ty, rot_deg=rot, scale=1.0 + 0.002 * f)
        t = 10.0 + 0.05 * f
        ctx.tracker_feed(t, img)
        ot.feed(t, img)
        pts, ids = ctx.tracker_last()
        # the whole front-end is bit-reproducible (integer image work, exact LK sums, ordered sub-pixel sums, deterministic RANSAC):
        # identical id lists and positions frame after frame
        assert np.array_equal(ids, ot.ids), (f, len(ids), len(ot.ids))
        assert np.array_equal(pts, np.asarray(ot.pts, dtype=np.float32).reshape(-1, 2)), f
        assert len(ids) >= 150
        tx += rng.uniform(-6, 6)
        ty += rng.uniform(-6, 6)
        rot += rng.uniform(-0.5, 0.5)
    # database: the restatement's ids, and every observation of every track
    assert ctx.db_size() >= 200
    mono_ref.assert_database(ctx, ot.db)
    # selection helpers, at the stamp of a frame (an observation time of the tracks seen in it)
    newest = 10.0 + 0.05 * 6
    lost = ctx.db_select(0, newest)  # not seen in the newest frame
    assert all(int(i) not in {int(j) for j in ids} for i in lost)
    assert np.array_equal(lost, mono_ref.db_select(ot.db, 0, newest))
    old = ctx.db_select(1, 10.0 + 0.05 * 2)
    assert len(old) > 0 and np.array_equal(old, mono_ref.db_select(ot.db, 1, 10.0 + 0.05 * 2))
    db = mono_ref.db_copy(ot.db)
    ctx.db_cleanup_measurements(10.0 + 0.05 * 3)
    mono_ref.db_cleanup_measurements(db, 10.0 + 0.05 * 3)
    ptr2, tt2, _, _ = ctx.db_export(old[:10])
    assert (tt2 >= 10.0 + 0.05 * 3).all()
    assert len(db) < len(ot.db)  # (tracks that ended before the cut went with their observations)
    mono_ref.assert_database(ctx, db)
    n0 = ctx.db_size()
    ctx.db_remove(old[:5])
    mono_ref.db_remove(db, old[:5])
    assert ctx.db_size() == len(db) <= n0
    mono_ref.assert_database(ctx, db)
    ctx.close()


def test_downsampled_feed_matches_oracle(pkg):
    """OptionsCamera::downsample: pyrDown(Size(cols / 2.0, rows / 2.0)) of image and mask, then the usual path
    (REF: UpdaterCamera.cpp:85-98).  Odd source sizes halve downwards."""
    fo = oracle_lib.load_front()
    sw, sh = 1505, 961  # -> 752 x 480
    canvas = synth.texture_canvas(sw, sh, seed=3, blobs=500)
    cfg = pkg.default_config(sw // 2, sh // 2)
    ctx = pkg.Context(cfg)
    img0 = synth.render_frame(canvas, sw, sh)
    small = ctx.downsample(img0)
    assert small.shape == (480, 752) and np.array_equal(small, fo.downsample(img0))
    assert np.array_equal(ctx.downsample(img0[:100, :64]), fo.downsample(img0[:100, :64]))  # a single 16x16 tile column
    # the fed pyramid is the pyramid of the equalised halved image
    ctx.feed_image_downsampled(img0)
    ref = fo.pyramid(fo.equalize_hist(fo.downsample(img0)))
    for l in range(ref.levels):
        assert np.array_equal(ctx.pyramid_level(0, l), ref.level(l)[0]), l
    # tracker stream on the halved images == tracker stream fed the oracle's halved images; the mask is halved too
    ot = OracleTracker(cfg, np.array(list(cfg.intrinsics)))
    ctx2 = pkg.Context(cfg)
    mask = np.zeros((sh, sw), np.uint8)
    mask[:, : sw // 4] = 255
    small_mask = fo.downsample(mask)
    for f in range(3):
        img = synth.render_frame(canvas, sw, sh, tx=3.0 * f, ty=-2.0 * f)
        ctx.tracker_feed_downsampled(20.0 + 0.1 * f, img, mask)
        ctx2.tracker_feed(20.0 + 0.1 * f, fo.downsample(img), small_mask)
    p1, i1 = ctx.tracker_last()
    p2, i2 = ctx2.tracker_last()
    assert len(i1) > 100 and np.array_equal(i1, i2) and np.array_equal(p1, p2)
    assert (small_mask[p1[:, 1].astype(int), p1[:, 0].astype(int)] <= 127).all()
    ctx.close()
    ctx2.close()


def test_kaist_sized_tracker(pkg):
    """The shipped KAIST camera settings (n_pts 1500, 15x15 grid, FAST 20, min_px_dist 10; config_camera.yaml) on a 1280x720 stream."""
    w, h = 1280, 720
    canvas = synth.texture_canvas(w, h, seed=12, blobs=3000)
    cfg = pkg.default_config(w, h)
    cfg.num_features, cfg.grid_x, cfg.grid_y, cfg.min_px_dist, cfg.fast_threshold = 1500, 15, 15, 10, 20
    ctx = pkg.Context(cfg)
    ot = OracleTracker(cfg, np.array(list(cfg.intrinsics)))
    for f in range(3):
        img = synth.render_frame(canvas, w, h, tx=4.0 * f, ty=-3.0 * f, rot_deg=0.2 * f)
        ctx.tracker_feed(30.0 + 0.05 * f, img)
        ot.feed(30.0 + 0.05 * f, img)
    pts, ids = ctx.tracker_last()
    assert len(ids) > 900
    assert np.array_equal(ids, ot.ids)
    assert np.array_equal(pts, np.asarray(ot.pts, dtype=np.float32).reshape(-1, 2))
    ctx.close()
