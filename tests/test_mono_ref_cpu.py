"""CPU tests of tests/mono_ref.py, the restatement test_gpu_tracker.py and test_gpu_tracker_branches.py hold the monocular tracker to:
  * over the GPU tests' streams the restatement reaches every branch of feed_monocular those tests are about;
  * each mistake a mirror of feed_monocular could make (mono_ref.VARIANTS) changes what at least one stream leaves behind;
  * it equals the compiled frame (oracle/frame_oracle.cpp, written independently) frame by frame;
  * its database calls answer as documented on a hand-made database;
  * the CLAHE images of the GPU test reach every way the clipped excess is redistributed."""
from collections import Counter

import numpy as np
import pytest

import mono_ref
import oracle_lib
import synth


def test_streams_reach_every_branch():
    total = sum((mono_ref.reference_run(name)[2].stats for name in mono_ref.STREAMS), Counter())
    for branch in mono_ref.BRANCHES:
        assert total[branch] > 0, (branch, dict(total))
    assert set(total) <= set(mono_ref.BRANCHES)


def test_streams_are_the_ones_drawn():
    """the counts the streams were drawn with (a stream that changes shows here first)"""
    _, after, ref = mono_ref.reference_run("band")
    assert [len(a[1]) for a in after] == [72, 62, 62, 59, 40, 12, 62, 52]
    assert (ref.stats["dropped as out of image"], ref.stats["dropped on the current mask"], ref.stats["dropped as unmatched"]) == (18, 10, 34)
    assert (ref.stats["top-up adds"], ref.stats["top-up adds nothing"], ref.stats["top-up prunes"]) == (2, 5, 6)
    _, after, ref = mono_ref.reference_run("cut")
    e = ref.frames
    assert [len(a[1]) for a in after][:7] == [47, 43, 3, 0, 47, 0, 47]
    assert "fewer than 10 points" in e[3] and "everything lost" in e[3] and "n == 0 reset" not in e[3]
    assert "detection after a loss, without a mask" in e[4] and "everything lost" in e[5] and "detection after a loss, without a mask" in e[6]
    _, after, ref = mono_ref.reference_run("strip")
    e = ref.frames
    assert [len(a[1]) for a in after][:4] == [78, 69, 4, 0] and (after[2][0][:, 0] < 10).all()
    assert "n == 0 reset" in e[3] and "top-up prunes" in e[3] and "detection after a loss, without a mask" in e[4] and len(after[4][1]) >= 10
    _, after, ref = mono_ref.reference_run("regain")
    e = ref.frames
    assert "everything lost" in e[1] and "detection after a loss, with a mask" in e[2] and len(after[2][1]) >= 10 and len(after[3][1]) >= 10
    m = after[2][2]
    assert (m[after[2][0][:, 1].astype(int), after[2][0][:, 0].astype(int)] <= 127).all()


def _left_behind(name, variant):
    _, after, ref = mono_ref.reference_run(name, mono_ref.HISTOGRAM, variant)
    return after, ref.db


def _same_lists(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _same_masks(a, b):
    return all((x[2] is None and y[2] is None) or (x[2] is not None and y[2] is not None and np.array_equal(x[2], y[2])) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", [v for v in mono_ref.VARIANTS if v != "mask not stored on the early exits"])
def test_streams_see_each_variant(variant):
    seen = []
    for name in mono_ref.STREAMS:
        want, want_db = _left_behind(name, None)
        got, got_db = _left_behind(name, variant)
        if not _same_lists(got, want) or got_db != want_db:
            seen.append(name)
    assert seen, variant


def test_a_mask_not_stored_on_an_early_exit_shows_in_the_stored_mask_alone():
    """After the n == 0 reset and after a frame with fewer than 10 points both lists are empty, so the next feed detects with its own
    mask (:110-114) and stores it (:119): nothing ever reads the mask those exits stored, and no stream can show a mirror that skips
    the store through points, ids or database.  What the tracker holds as its last mask does show it (the GPU tests read it back
    through the track image's mask layer after every frame)."""
    seen = []
    for name in mono_ref.STREAMS:
        want, want_db = _left_behind(name, None)
        got, got_db = _left_behind(name, "mask not stored on the early exits")
        assert _same_lists(got, want) and got_db == want_db
        if not _same_masks(got, want):
            seen.append(name)
    assert "cut" in seen and "strip" in seen  # (the fewer-than-10 frame, the n == 0 reset)


def _frame_config(pkg, s, method):
    cfg = pkg.default_config(s.w, s.h)
    cfg.num_features, cfg.grid_x, cfg.grid_y = s.cfg.num_features, s.cfg.grid_x, s.cfg.grid_y
    cfg.min_px_dist, cfg.fast_threshold, cfg.histogram_method = s.cfg.min_px_dist, s.cfg.fast_threshold, method
    for i, v in enumerate(s.K):
        cfg.intrinsics[i] = float(v)
    return cfg


@pytest.mark.parametrize("name,method", [(n, mono_ref.HISTOGRAM) for n in mono_ref.STREAMS] + [("band", mono_ref.NONE)])
def test_restatement_equals_the_compiled_frame(pkg, name, method):
    """FrameOracle.tracker_feed knows HISTOGRAM and NONE (it has no CLAHE)"""
    s, after, ref = mono_ref.reference_run(name, method)
    frame = oracle_lib.FrameOracle(pkg, _frame_config(pkg, s, method), synth.q95_table(64))
    try:
        for f, (t, img, mask) in enumerate(s.frames()):
            frame.tracker_feed(t, img, mask)
            pts, ids = frame.tracker_last()
            assert np.array_equal(ids, after[f][1]), (f, len(ids), len(after[f][1]))
            assert np.array_equal(pts, after[f][0]), f
        ids, counts = frame.db_ids()
        assert [int(i) for i in ids] == sorted(ref.db)
        for fid, n in zip(ids, counts):
            t, uv, uvn = frame.db_track(fid)
            ptr, rt, ruv, ruvn = mono_ref.db_export(ref.db, [fid])
            assert n == ptr[1] and np.array_equal(t, rt) and np.array_equal(uv, ruv) and np.array_equal(uvn, ruvn), int(fid)
        # cleanup_measurements at an observation time: the observation at that time stays in both
        t_cut = s.times()[len(s.offsets) // 2]
        frame.db_cleanup_measurements(t_cut)
        db = mono_ref.db_copy(ref.db)
        mono_ref.db_cleanup_measurements(db, t_cut)
        ids, counts = frame.db_ids()
        assert [int(i) for i in ids] == sorted(db) and [int(c) for c in counts] == [len(db[k]) for k in sorted(db)]
    finally:
        frame.close()


def test_database_calls_on_a_hand_made_database():
    o = lambda t, u, v: (t, np.float32(u), np.float32(v), np.float32(u / 100), np.float32(v / 100))
    db = {7: [o(1.0, 10, 10), o(2.0, 13, 14)], 3: [o(2.0, 5, 5), o(3.0, 5, 6)], 9: [o(1.0, 0, 0), o(2.0, 0.5, 0), o(3.0, 1, 0)], 4: [o(3.0, 1, 1)]}
    # mode 0: no observation at or after t; mode 1: an observation before t
    assert mono_ref.db_select(db, 0, 3.0).tolist() == [7]
    assert mono_ref.db_select(db, 0, np.nextafter(2.0, 0.0)).tolist() == [] and mono_ref.db_select(db, 0, np.nextafter(2.0, 9.0)).tolist() == [7]
    assert mono_ref.db_select(db, 1, 2.0).tolist() == [7, 9] and mono_ref.db_select(db, 1, np.nextafter(2.0, 9.0)).tolist() == [3, 7, 9]
    assert mono_ref.db_select(db, 1, 1.0).tolist() == []
    assert mono_ref.db_disparity(db, 1.0, 2.0) == (2.75, float(np.sqrt(((5.0 - 2.75) ** 2 + (0.5 - 2.75) ** 2) / 1.0)), 2)
    assert mono_ref.db_disparity(db, 1.0, 3.0) == (-1.0, -1.0, 0) and mono_ref.db_disparity(db, 2.0, 2.5) == (-1.0, -1.0, 0)
    ptr, t, uv, uvn = mono_ref.db_export(db, [3, 99, 4])
    assert ptr.tolist() == [0, 2, 2, 3] and t.tolist() == [2.0, 3.0, 3.0] and uv.dtype == np.float32 and uv.tolist() == [[5, 5], [5, 6], [1, 1]]
    c = mono_ref.db_copy(db)
    mono_ref.db_cleanup_measurements(c, 3.0)
    assert sorted(c) == [3, 4, 9] and [len(c[k]) for k in (3, 4, 9)] == [1, 1, 1] and len(db[9]) == 3
    mono_ref.db_cleanup_measurements(c, np.nextafter(3.0, 9.0))
    assert c == {}
    c = mono_ref.db_copy(db)
    mono_ref.db_remove(c, [7, 7, 99])
    assert sorted(c) == [3, 4, 9]


def test_clahe_images_reach_every_redistribution():
    """what clahe_lut_kernel's clip and redistribution meet over the images test_gpu_tracker_branches.py feeds: tiles with nothing
    left over the batches, tiles whose residual goes to bins more than one apart, tiles whose residual is more than half the bins
    (stride 1, not every bin gets one), and a size whose clip is the floor of 1"""
    seen = set()
    for (w, h), clip in mono_ref.CLAHE_SIZES.items():
        for kind in mono_ref.CLAHE_IMAGES:
            got_clip, tiles = mono_ref.clahe_tile_residuals(mono_ref.clahe_image(w, h, kind))
            assert got_clip == clip, (w, h)
            if 10.0 * (w // 8) * (h // 8) / 256 < 1.0:
                assert clip == 1
                seen.add("clip is the floor")
            for clipped, residual, stride in tiles:
                if residual == 0:
                    seen.add("residual 0")
                elif stride > 1:
                    seen.add("residual with stride > 1")
                else:
                    assert residual > 128
                    seen.add("residual > 128")
    assert {"residual 0", "residual with stride > 1", "residual > 128", "clip is the floor"} <= seen, seen
