"""Host images with padded rows through every feed that copies them into a pinned block (one row copy, pack_rows of
pl-viwo_amd/csrc/match_block.hpp, behind plv_tracker_feed, plv_tracker_feed_encoded and plv_tracker_feed_stereo): three frames fed to
two contexts, from packed buffers and from buffers with stride = row + 5 whose padding holds other bytes — points, ids and database
exports equal bit for bit.  256 x 192, the smallest size of the stereo tests (96 x 64 has three pyramid levels at the default window,
their streams four), and tests/stereo_ref.py's plane without masks: the restatement tracks 43 points per camera there, so LK and RANSAC
run (asserted: at least 10 points after every matched frame)."""
import ctypes as C

import numpy as np
import pytest

import stereo_ref

pytestmark = pytest.mark.gpu

W, H, PAD = 256, 192, 5


@pytest.fixture(scope="module")
def stream():
    offs = [(0, 0, 0, 0), (1, 1, 0, 0), (2, 1, 0, 0)]
    K = stereo_ref.intrinsics(W, H, 190.0)
    s = stereo_ref.Stream("strided", W, H, stereo_ref.Settings(40, 4, 3, 8), 4.0, offs, K, K)
    return s, [(t, left, right) for t, left, right, _, _ in s.frames()]


def _context(pkg, s, stereo):
    cfg = pkg.default_config(s.w, s.h)
    cfg.num_features, cfg.grid_x, cfg.grid_y = s.cfg.num_features, s.cfg.grid_x, s.cfg.grid_y
    cfg.min_px_dist, cfg.fast_threshold = s.cfg.min_px_dist, s.cfg.fast_threshold
    for i, v in enumerate(s.K_left):
        cfg.intrinsics[i] = float(v)
    ctx = pkg.Context(cfg)
    if stereo:
        ctx.stereo_configure(s.K_right, 0)
    return ctx


def _padded(img):
    """the same image (H x W or H x W x bpp) as a view of a buffer whose rows are PAD bytes longer, the padding filled with 0xAA"""
    rows = img.reshape(img.shape[0], -1)
    buf = np.full((rows.shape[0], rows.shape[1] + PAD), 0xAA, np.uint8)
    buf[:, :rows.shape[1]] = rows
    if img.ndim == 2:
        view = buf[:, :rows.shape[1]]
    else:
        view = np.lib.stride_tricks.as_strided(buf, shape=img.shape, strides=(buf.strides[0], img.shape[2], 1))
    assert view.strides[0] == rows.shape[1] + PAD and np.array_equal(view, img)
    return view


def _colour(img):
    """a 3-byte image whose channels differ, with the grey image's texture"""
    return np.ascontiguousarray(np.stack([img, 255 - img, np.roll(img, 1, axis=1)], axis=-1))


def _feed_mono(ctx, t, img):
    # (Context.tracker_feed packs its image: the stride goes to the library itself)
    ctx._chk(ctx.lib.plv_tracker_feed(ctx.h, float(t), img.ctypes.data_as(C.POINTER(C.c_uint8)), int(img.strides[0]), None))


@pytest.mark.parametrize("route", ["plv_tracker_feed", "plv_tracker_feed_encoded bgr8"])
def test_monocular_feed_of_padded_rows_equals_the_packed_feed(pkg, stream, route):
    s, frames = stream
    a, b = _context(pkg, s, False), _context(pkg, s, False)
    try:
        seen = set()
        for f, (t, left, _) in enumerate(frames):
            if route == "plv_tracker_feed":
                _feed_mono(a, t, np.ascontiguousarray(left))
                _feed_mono(b, t, _padded(left))
            else:
                a.tracker_feed_encoded(t, _colour(left), "bgr8")
                b.tracker_feed_encoded(t, _padded(_colour(left)), "bgr8")
            (pa, ia), (pb, ib) = a.tracker_last(), b.tracker_last()
            print(route, "frame", f, "points", len(ia), len(ib))
            assert len(ia) >= 10, (route, f)
            assert np.array_equal(pa, pb) and np.array_equal(ia, ib), (route, f)
            seen.update(int(i) for i in ia)
        assert a.db_size() == b.db_size() > 0
        ids = np.array(sorted(seen), dtype=np.uint64)
        ea, eb = a.db_export(ids), b.db_export(ids)
        assert ea[0][-1] >= 10
        for x, y in zip(ea, eb):
            assert np.array_equal(x, y), route
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("encoding", ["mono8", "bayer_rggb8"])
def test_stereo_feed_of_padded_rows_equals_the_packed_feed(pkg, stream, encoding):
    s, frames = stream
    a, b = _context(pkg, s, True), _context(pkg, s, True)
    try:
        for f, (t, left, right) in enumerate(frames):  # (as a Bayer pair the rendered bytes read as mosaics: any bytes are a mosaic)
            a.tracker_feed_stereo(t, np.ascontiguousarray(left), np.ascontiguousarray(right), encoding=encoding)
            b.tracker_feed_stereo(t, _padded(left), _padded(right), encoding=encoding)
            for cam in (0, 1):
                (pa, ia), (pb, ib) = a.stereo_last(cam), b.stereo_last(cam)
                print(encoding, "frame", f, "camera", cam, "points", len(ia), len(ib))
                assert len(ia) >= 10, (encoding, f, cam)
                assert np.array_equal(pa, pb) and np.array_equal(ia, ib), (encoding, f, cam)
        ids = a.stereo_db_ids()
        assert len(ids) >= 10 and np.array_equal(b.stereo_db_ids(), ids)
        for cam in (0, 1):
            ea, eb = a.stereo_db_export(ids, cam), b.stereo_db_export(ids, cam)
            assert ea[0][-1] >= 10
            for x, y in zip(ea, eb):
                assert np.array_equal(x, y), (encoding, cam)
    finally:
        a.close()
        b.close()
