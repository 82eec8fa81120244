"""The track image on the device (include/plviwo.h "track image") against tests/track_image_ref.py, byte for byte: the rasteriser through
plv_draw_primitives, the layers through plv_track_image_primitives / plv_track_image on real tracker state, that the call reads and
never writes, and the replay tool's --track-images."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import synth_dataset as sd
import track_image_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 752, 480
ALL = R.HISTORY | R.ACTIVE | R.LINES | R.MASK
_u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None


# ---------------------------------------------------------------------------------------------- inputs
def _random_prims(rng, w, h, n):
    """n primitives of every kind around and inside a w x h image"""
    out = []
    cx = lambda: int(rng.integers(-20, w + 20))
    cy = lambda: int(rng.integers(-20, h + 20))
    for i in range(n):
        rgb = tuple(int(v) for v in rng.integers(0, 256, 3))
        k = i % 5
        if k == 0:
            out.append(R.disc(cx(), cy(), int(rng.integers(0, 7)), rgb))
        elif k == 1:
            out.append(R.prim(R.RING, cx(), cy(), a=49, b=81, rgb=rgb))
        elif k == 2:
            out.append(R.prim(R.BOX, cx(), cy(), cx(), cy(), rgb=rgb))
        elif k == 3:
            x, y = cx(), cy()
            out.append(R.prim(R.SEG, x, y, x + int(rng.integers(-60, 61)), y + int(rng.integers(-60, 61)), a=int(rng.integers(1, 3)), rgb=rgb))
        else:
            out.append(R.prim(R.SEG, cx(), cy(), cx(), cy(), a=int(rng.integers(1, 3)), rgb=rgb))
    return R.prims_array(out)


def _padded(rng, a, pad):
    """a view of `a` whose rows lie pad elements further apart, with noise in between"""
    wide = rng.integers(0, 256, (a.shape[0], a.shape[1] + pad) + a.shape[2:], dtype=np.uint8)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]]


def _draw_strided(ctx, rng, grey, prims, mask):
    """plv_draw_primitives with every image a slice of a wider array: returns the picture, checks the bytes between the rows"""
    h, w = grey.shape
    big = np.full((h, w + 5, 3), 0xA5, dtype=np.uint8)
    out = ctx.draw_primitives(_padded(rng, grey, 13), prims, None if mask is None else _padded(rng, mask, 3), out=big[:, :w])
    assert out.strides[0] == 3 * (w + 5) and np.all(big[:, w:] == 0xA5)
    return out


# ---------------------------------------------------------------------------------------------- 1. the rasteriser
@pytest.mark.parametrize("size", [(1, 1), (3, 3), (67, 35), (753, 481), (752, 480)])
def test_random_lists_equal_the_reference(ctx, size):
    w, h = size
    rng = np.random.default_rng(1000 + w)
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mask = (rng.integers(0, 4, (h, w)) == 0).astype(np.uint8) * rng.integers(1, 256, (h, w), dtype=np.uint8)
    prims = _random_prims(rng, w, h, 400)
    for m in (None, mask):
        want = R.render(grey, prims, m)
        got = ctx.draw_primitives(grey, prims, m)                                 # packed rows
        assert np.array_equal(got, want), (size, m is not None, "packed", int((got != want).sum()))
        got = _draw_strided(ctx, rng, grey, prims, m)
        assert np.array_equal(got, want), (size, m is not None, "strided", int((got != want).sum()))
    if w >= 67:
        assert not np.array_equal(R.render(grey, prims), R.render(grey, prims[::-1]))   # (the lists overlap: order matters)


def test_primitives_across_tile_borders(ctx):
    """tiles are 64 x 8: primitives that lie on two, four and more of them, and on the partial tiles at the right and bottom edges"""
    w, h = 200, 50
    grey = np.full((h, w), 90, dtype=np.uint8)
    items = [R.disc(64, 16, 5, (1, 2, 3)), R.disc(128, 32, 6, (4, 5, 6)), R.prim(R.RING, 64, 32, a=49, b=81, rgb=(7, 8, 9)),
             R.prim(R.SEG, 60, 10, 70, 12, a=2, rgb=(10, 20, 30)), R.prim(R.SEG, 63, 0, 64, 49, a=2, rgb=(40, 50, 60)),
             R.prim(R.SEG, 0, 15, 199, 16, a=2, rgb=(70, 80, 90)), R.prim(R.SEG, 120, 47, 199, 3, a=1, rgb=(11, 12, 13)),
             R.prim(R.BOX, 63, 15, 128, 32, rgb=(100, 110, 120)), R.prim(R.BOX, 191, 47, 199, 49, rgb=(130, 140, 150)),
             R.prim(R.BOX, 0, 0, 199, 49, rgb=(160, 170, 180)), R.disc(199, 49, 3, (190, 200, 210)), R.disc(192, 48, 2, (220, 230, 240))]
    for prims in ([p] for p in items):                        # each alone, so that nothing hides another's error
        prims = R.prims_array(prims)
        got, want = ctx.draw_primitives(grey, prims), R.render(grey, prims)
        assert np.array_equal(got, want), (prims, int((got != want).sum()))
    prims = R.prims_array(items)
    assert np.array_equal(ctx.draw_primitives(grey, prims), R.render(grey, prims))


def test_primitives_outside_the_image(ctx):
    w, h = 100, 60
    rng = np.random.default_rng(5)
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    far = 1 << 20
    items = [R.disc(-3, -2, 6, (1, 2, 3)), R.disc(-30, 10, 6, (1, 2, 3)), R.disc(103, 61, 6, (4, 5, 6)), R.prim(R.RING, -5, 30, a=49, b=81, rgb=(7, 8, 9)),
             R.prim(R.BOX, -10, -10, 20, 20, rgb=(10, 11, 12)), R.prim(R.BOX, -10, -10, 120, 80, rgb=(13, 14, 15)),
             R.prim(R.BOX, 50, -far, far, 30, rgb=(16, 17, 18)), R.prim(R.BOX, -far, -far, far, far, rgb=(19, 20, 21)),
             R.prim(R.SEG, -far, 7, far, 45, a=2, rgb=(22, 23, 24)), R.prim(R.SEG, 30, far, 70, -far, a=2, rgb=(25, 26, 27)),
             R.prim(R.SEG, far, far, far - 5, far - 9, a=1, rgb=(28, 29, 30)), R.prim(R.SEG, -far, -far, far, far, a=1, rgb=(31, 32, 33)),
             R.prim(R.SEG, far - 1, -far, -far, far - 3, a=2, rgb=(34, 35, 36)), R.disc(far, -far, 2, (37, 38, 39)),
             R.prim(R.SEG, 40, 40, 40, 40, a=1, rgb=(40, 41, 42)), R.prim(R.SEG, 99, 59, 99, 59, a=2, rgb=(43, 44, 45)),
             R.prim(R.SEG, -1, 5, -1, 5, a=2, rgb=(46, 47, 48)), R.prim(R.SEG, 5, -1, 5, -1, a=2, rgb=(49, 50, 51)),
             R.prim(R.SEG, -40, 20, 10, 25, a=2, rgb=(52, 53, 54)), R.prim(R.SEG, 90, 50, 140, 90, a=2, rgb=(55, 56, 57))]
    for p in items:
        prims = R.prims_array([p])
        got, want = ctx.draw_primitives(grey, prims), R.render(grey, prims)
        assert np.array_equal(got, want), (p, int((got != want).sum()))
    prims = R.prims_array(items)
    assert np.array_equal(ctx.draw_primitives(grey, prims), R.render(grey, prims))
    # wholly outside: the grey image comes back
    prims = R.prims_array([items[1], items[13], items[10]])
    assert np.array_equal(ctx.draw_primitives(grey, prims), np.repeat(grey[:, :, None], 3, axis=2))


def test_segments_in_all_octants_both_ways(ctx):
    w = h = 81
    grey = np.zeros((h, w), dtype=np.uint8)
    ends = [(sx * a, sy * b) for a, b in ((30, 11), (11, 30), (30, 30), (30, 0), (0, 30), (29, 10), (7, 2)) for sx in (1, -1) for sy in (1, -1)]
    for dx, dy in ends:
        for thick in (1, 2):
            for x0, y0, x1, y1 in ((40, 40, 40 + dx, 40 + dy), (40 + dx, 40 + dy, 40, 40)):
                prims = R.prims_array([R.prim(R.SEG, x0, y0, x1, y1, a=thick, rgb=(255, 128, 1))])
                got, want = ctx.draw_primitives(grey, prims), R.render(grey, prims)
                assert np.array_equal(got, want), ((x0, y0, x1, y1, thick), int((got != want).sum()))


def test_twenty_thousand_primitives_over_one_tile(ctx):
    """the list of one tile exceeds what its workgroup holds in LDS many times over: rounds, never truncation, and the order across the
    rounds — a box over the whole image painted before the crowd and one painted after it"""
    w, h = 200, 100
    rng = np.random.default_rng(20000)
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    n = 20000
    crowd = np.zeros(n, dtype=R.PRIM_DTYPE)
    crowd["kind"] = R.RING
    crowd["x0"], crowd["y0"] = rng.integers(81, 128, n), rng.integers(17, 23, n)  # (inside the tile 64 .. 127 x 16 .. 23; its columns 64 .. 79 stay free)
    crowd["b"] = rng.integers(0, 2, n)                                # single pixels and discs of radius 1
    crowd["rgb"] = rng.integers(0, 256, (n, 3))
    first = R.prims_array([R.prim(R.BOX, 0, 0, w - 1, h - 1, rgb=(255, 0, 0)), R.prim(R.SEG, 0, 20, w - 1, 20, a=2, rgb=(9, 9, 9))])
    last = R.prims_array([R.prim(R.BOX, 1, 1, w - 2, h - 2, rgb=(0, 255, 0)), R.prim(R.SEG, 0, 20, w - 1, 28, a=1, rgb=(0, 0, 255))])
    prims = np.concatenate([first, crowd, last])
    want = R.render(grey, prims)
    got = ctx.draw_primitives(grey, prims)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(ctx.draw_primitives(grey, prims), got)                  # the same bytes again
    # (the early segment stands where the crowd left room and is hidden under it: both orders are really exercised)
    assert (want[20, 64:80] == 9).all() and not (want[20, 81:128] == 9).all(axis=1).any()
    # a disc over the whole tile at the very end: every pixel of the tile is final after the first round
    prims2 = np.concatenate([prims, R.prims_array([R.disc(96, 20, 40, (1, 2, 3))])])
    assert np.array_equal(ctx.draw_primitives(grey, prims2), R.render(grey, prims2))
    # ... and at the very beginning: it shows only where nothing of the 20 000 landed
    prims3 = np.concatenate([R.prims_array([R.disc(96, 20, 40, (1, 2, 3))]), prims])
    assert np.array_equal(ctx.draw_primitives(grey, prims3), R.render(grey, prims3))


def test_empty_list_and_mask(ctx):
    rng = np.random.default_rng(3)
    for w, h in ((1, 1), (70, 17), (752, 480)):
        grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
        none = np.zeros(0, dtype=R.PRIM_DTYPE)
        got = ctx.draw_primitives(grey, none)
        assert np.array_equal(got, np.repeat(grey[:, :, None], 3, axis=2))
        mask = rng.integers(0, 2, (h, w), dtype=np.uint8) * 255
        got = ctx.draw_primitives(grey, none, mask)
        assert np.array_equal(got, R.render(grey, none, mask))
        assert np.array_equal(got[:, :, :2], np.repeat(grey[:, :, None], 2, axis=2))


def test_largest_case_twice_gives_the_same_bytes(ctx):
    w, h = 753, 481
    rng = np.random.default_rng(77)
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mask = (rng.integers(0, 3, (h, w)) == 0).astype(np.uint8)
    prims = _random_prims(rng, w, h, 3000)
    a = ctx.draw_primitives(grey, prims, mask)
    b = ctx.draw_primitives(grey, prims, mask)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a, R.render(grey, prims, mask))


def test_bad_arguments_leave_the_output_alone(pkg, ctx):
    w, h = 40, 30
    grey = np.full((h, w), 7, dtype=np.uint8)
    mask = np.zeros((h, w), dtype=np.uint8)
    good = R.prims_array([R.disc(5, 5, 2, (1, 2, 3)), R.prim(R.BOX, 1, 1, 9, 9, rgb=(4, 5, 6))])
    pp = lambda a: a.ctypes.data_as(C.POINTER(pkg.PlvDrawPrim))

    def call(grey_=grey, stride=w, prims=good, n=None, mask_=None, mstride=0, rgb_stride=3 * w, null_out=False, ww=w, hh=h):
        out = np.full((h, 3 * w), 0x5A, dtype=np.uint8)
        rc = ctx.lib.plv_draw_primitives(ctx.h, _u8(grey_), stride, ww, hh, pp(prims) if prims is not None else None, len(prims) if n is None else n,
                                         _u8(mask_), mstride, None if null_out else _u8(out), rgb_stride)
        return rc, out

    rc, out = call()
    assert rc == pkg.PLV_OK and np.array_equal(out.reshape(h, w, 3), R.render(grey, good))
    bad_kind, neg_kind, far = good.copy(), good.copy(), good.copy()
    bad_kind["kind"][1], neg_kind["kind"][0], far["x1"][1] = 3, -1, (1 << 24) + 1
    cases = dict(unknown_kind=dict(prims=bad_kind), negative_kind=dict(prims=neg_kind), far_coordinate=dict(prims=far), null_grey=dict(grey_=None),
                 null_list=dict(prims=None, n=2), negative_n=dict(n=-1), short_stride=dict(stride=w - 1), short_rgb_stride=dict(rgb_stride=3 * w - 1),
                 short_mask_stride=dict(mask_=mask, mstride=w - 1), zero_width=dict(ww=0), zero_height=dict(hh=0))
    for name, kw in cases.items():
        rc, out = call(**kw)
        assert rc == pkg.PLV_E_BADARG, name
        assert np.all(out == 0x5A), name
    assert call(null_out=True)[0] == pkg.PLV_E_BADARG
    rc, out = call()                                             # the context still works
    assert rc == pkg.PLV_OK and np.array_equal(out.reshape(h, w, 3), R.render(grey, good))


# ---------------------------------------------------------------------------------------------- 2. the track image on tracker state
@pytest.fixture(scope="module")
def frames():
    """12 rendered frames of the street drive (tests/synth_dataset.py), 752 x 480, grey"""
    return sd.render_frames(0.05 + np.arange(12) * 0.1, style="street", workers=min(8, os.cpu_count() or 1))


def _bonnet(w, h):
    """a mask as a car's bonnet would need: the bottom rows and a corner"""
    m = np.zeros((h, w), dtype=np.uint8)
    m[h - h // 8:, :] = 255
    m[:h // 6, :w // 5] = 1
    return m


def _drive(pkg, images, mask):
    h, w = images[0].shape
    cfg = pkg.default_config(w, h)
    c = pkg.Context(cfg)
    vps = c.vanishing_points(np.eye(3), np.array(list(cfg.intrinsics)))
    for i, img in enumerate(images):
        c.tracker_feed(10.0 + 0.1 * i, img, mask)
        c.line_tracker_feed(10.0 + 0.1 * i, vps)
    return c


def _state(c):
    """what the layers are built from, through the exports the issue names"""
    pts, ids = c.tracker_last()
    ptr, _, uv, _ = c.db_export(ids)
    tracks = {int(fid): uv[ptr[k]:ptr[k + 1]] for k, fid in enumerate(ids) if ptr[k + 1] > ptr[k]}
    lines, lids = c.line_tracker_last()
    rel_ptr, rel_id = c.line_tracker_last_points()
    return dict(pts=pts, ids=ids, tracks=tracks, lines=lines, line_ids=lids, rel_ptr=rel_ptr, rel_id=rel_id, line_db_ids=c.line_db_ids())


@pytest.fixture(scope="module")
def full(pkg, frames):
    mask = _bonnet(W, H)
    c = _drive(pkg, frames, mask)
    yield c, _state(c), mask
    c.close()


@pytest.fixture(scope="module")
def small(pkg, frames):
    """the same drive at 376 x 240: min(W, H) < 400, the reference's is_small"""
    imgs = [np.ascontiguousarray(f[::2, ::2]) for f in frames]
    mask = _bonnet(W // 2, H // 2)
    c = _drive(pkg, imgs, mask)
    yield c, _state(c), mask
    c.close()


def _subsets(s):
    """a highlighted and a flagged subset of the last ids that overlap, plus ids that no track has"""
    ids = s["ids"]
    return [int(v) for v in ids[::3]] + [10 ** 9], [int(v) for v in ids[1::4]] + [int(ids[0]), 10 ** 9 + 1]


def _expect_list(c, s, layers, **kw):
    return R.track_image_list(c.cfg.width, c.cfg.height, layers, s["pts"], s["ids"], s["tracks"], s["lines"], s["line_ids"], s["rel_ptr"], s["rel_id"],
                              s["line_db_ids"], **kw)


def _check_state_is_a_picture(s, small=False):
    n_obs = sum(len(v) for v in s["tracks"].values())
    assert len(s["ids"]) >= (40 if small else 100) and n_obs >= 5 * len(s["ids"]), (len(s["ids"]), n_obs)    # tracks with a history
    assert len(s["lines"]) >= 3 and s["rel_ptr"][-1] >= 3 and len(s["rel_ptr"]) == len(s["lines"]) + 1          # lines with points on them
    assert set(int(v) for v in s["line_ids"]) & set(int(v) for v in s["line_db_ids"])


CASES = [("history", R.HISTORY, {}), ("active", R.ACTIVE, {}), ("lines", R.LINES, {}), ("mask", R.MASK, {}), ("all", ALL, {}),
         ("highlighted", R.HISTORY, {"hi": True}), ("flagged", R.HISTORY, {"fl": True}), ("all_marked", ALL, {"hi": True, "fl": True}),
         ("colours_and_cut", R.HISTORY | R.ACTIVE, {"colors": (90, 300, 255, 200, 40, 255), "max_tracks": 4})]


def _run_case(c, s, mask, layers, opts):
    hi, fl = _subsets(s)
    kw = {}
    if opts.get("hi"):
        kw["highlighted"] = hi
    if opts.get("fl"):
        kw["flagged"] = fl
    for k in ("colors", "max_tracks"):
        if k in opts:
            kw[k] = opts[k]
    want_list = _expect_list(c, s, layers, **kw)
    got_list = c.track_image_primitives(layers, **kw)
    assert got_list.dtype == R.PRIM_DTYPE and len(got_list) == len(want_list), (len(got_list), len(want_list))
    assert got_list.tobytes() == want_list.tobytes(), np.nonzero(got_list != want_list)[0][:5]
    grey = c.pyramid_level(0, 0)
    want = R.render(grey, want_list, mask if layers & R.MASK else None)
    got = c.track_image(layers, **kw)
    assert np.array_equal(got, want), int((got != want).sum())
    return want_list, got


@pytest.mark.parametrize("name,layers,opts", CASES, ids=[x[0] for x in CASES])
def test_track_image_on_the_street_drive(full, name, layers, opts):
    c, s, mask = full
    _check_state_is_a_picture(s)
    prims, img = _run_case(c, s, mask, layers, opts)
    grey = c.pyramid_level(0, 0)
    if layers & (R.HISTORY | R.ACTIVE):
        assert len(prims) >= 2 * len(s["ids"])                   # at least a disc and a box or a segment per tracked point
    if layers & R.LINES:
        assert (prims["a"] == 2).sum() >= 3 and ((prims["a"] == 49) & (prims["b"] == 81)).sum() >= 3    # segments and line markers
    if layers & ~R.MASK:
        assert (img != grey[:, :, None]).any()
    if opts.get("hi"):
        assert (prims["kind"] == R.BOX).sum() >= len(s["ids"]) // 3 - 1
    if opts.get("fl"):
        assert ((prims["rgb"][:, 0] == 0) & (prims["rgb"][:, 1] == 255)).any()
    if layers == R.MASK:                                          # the bonnet's rows are tinted, the middle of the picture is the grey image
        assert np.array_equal(img[H - 1, :, 2], R.mask_rule(grey[H - 1])) and np.array_equal(img[H // 2, :, 2], grey[H // 2])


@pytest.mark.parametrize("name,layers,opts", CASES, ids=[x[0] for x in CASES])
def test_track_image_on_a_small_context(small, name, layers, opts):
    c, s, mask = small
    assert min(c.cfg.width, c.cfg.height) < 400
    _check_state_is_a_picture(s, small=True)
    prims, _ = _run_case(c, s, mask, layers, opts)
    if layers == R.HISTORY and not opts.get("fl"):
        assert set(prims["b"][prims["kind"] == R.RING].tolist()) == {1}            # discs of radius 1


def test_without_a_mask_the_mask_layer_does_nothing(pkg, frames):
    c = _drive(pkg, frames[:3], None)
    grey = c.pyramid_level(0, 0)
    assert np.array_equal(c.track_image(R.MASK), np.repeat(grey[:, :, None], 3, axis=2))
    c.close()


def test_before_the_first_feed(pkg):
    c = pkg.Context(pkg.default_config(W, H))
    w, h = C.c_int(), C.c_int()
    rc_pyr = c.lib.plv_pyramid_download(c.h, 0, 0, C.byref(w), C.byref(h), None)
    assert rc_pyr != pkg.PLV_OK
    opt = pkg.PlvTrackImageOptions()
    c.lib.plv_track_image_options_default(C.byref(opt))
    assert (opt.layers, opt.r1, opt.g1, opt.b1, opt.r2, opt.g2, opt.b2, opt.max_tracks, opt.n_highlighted, opt.n_flagged) == \
        (pkg.PLV_VIZ_HISTORY, 255, 255, 0, 255, 255, 255, 50, 0, 0)
    out = np.full((H, 3 * W), 0x5A, dtype=np.uint8)
    assert c.lib.plv_track_image(c.h, C.byref(opt), _u8(out), 3 * W) == rc_pyr
    assert np.all(out == 0x5A)
    c.close()


def test_track_image_refuses_bad_arguments(pkg, full):
    c, s, _ = full
    opt = pkg.PlvTrackImageOptions()
    c.lib.plv_track_image_options_default(C.byref(opt))
    out = np.full((H, 3 * W), 0x5A, dtype=np.uint8)
    assert c.lib.plv_track_image(c.h, C.byref(opt), _u8(out), 3 * W - 1) == pkg.PLV_E_BADARG
    assert c.lib.plv_track_image(c.h, None, _u8(out), 3 * W) == pkg.PLV_E_BADARG
    assert c.lib.plv_track_image(c.h, C.byref(opt), None, 3 * W) == pkg.PLV_E_BADARG
    opt.layers = 16
    assert c.lib.plv_track_image(c.h, C.byref(opt), _u8(out), 3 * W) == pkg.PLV_E_BADARG
    opt.layers, opt.n_highlighted = 1, 2
    assert c.lib.plv_track_image(c.h, C.byref(opt), _u8(out), 3 * W) == pkg.PLV_E_BADARG
    assert np.all(out == 0x5A)
    # the list with too little room: PLV_E_BADARG and the count
    opt.n_highlighted = 0
    n = C.c_int(-1)
    few = np.zeros(3, dtype=R.PRIM_DTYPE)
    rc = c.lib.plv_track_image_primitives(c.h, C.byref(opt), few.ctypes.data_as(C.POINTER(pkg.PlvDrawPrim)), 3, C.byref(n))
    assert rc == pkg.PLV_E_BADARG and n.value == len(_expect_list(c, s, R.HISTORY)) and not few.tobytes().strip(b"\0")


# ---------------------------------------------------------------------------------------------- 3. read-only
def _snapshot(c, n_cov):
    pts, ids = c.tracker_last()
    db = c.db_export(np.sort(c.db_select(1, 1e30)))
    lines, lids = c.line_tracker_last()
    rel = c.line_tracker_last_points()
    ldb = c.line_db_export(c.line_db_ids())
    parts = [pts, ids, *db, lines, lids, *rel, c.line_db_ids(), *[ldb[k] for k in sorted(ldb)], c.cov_download(n_cov),
             c.pyramid_level(0, 0), c.pyramid_level(1, 0)]
    return [np.ascontiguousarray(p).tobytes() for p in parts] + [c.db_size(), c.line_db_size(), c.pyramid_levels(0)]


def test_the_call_changes_nothing(full):
    c, s, _ = full
    rng = np.random.default_rng(9)
    A = rng.standard_normal((21, 21))
    c.cov_upload(A @ A.T + 21 * np.eye(21))
    before = _snapshot(c, 21)
    hi, fl = _subsets(s)
    for layers in (R.HISTORY, ALL):
        c.track_image(layers, highlighted=hi, flagged=fl)
        c.track_image_primitives(layers, highlighted=hi)
    opt = c._track_image_options(ALL, None, None, hi, None)[0]
    assert c.lib.plv_track_image(c.h, C.byref(opt), None, 3 * W) == -1             # a failing exit
    assert _snapshot(c, 21) == before


def _drive_system(pkg, dataset, tmp_path, name, with_images):
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    op = options.load_options(sd.write_config(str(tmp_path / f"config_{name}"), dataset, str(tmp_path / f"traj_{name}.txt")))
    end, pictures = {}, []

    def after_camera(system, frame, t):
        if with_images:
            rgb, overlay = system.get_track_img("history,active,lines,mask")
            pictures.append((rgb, overlay, system.state.initialized))
        c = system.ctx                                          # the last frame's state, read the same way in both drives
        end.update(frame=frame, last=[a.tobytes() for a in c.tracker_last()], db=c.db_size(), lines=[a.tobytes() for a in c.line_tracker_last()],
                   line_db=c.line_db_size(), n=system.state.n, imu=np.frombuffer(system.state.imu, dtype=np.float64).copy(),
                   cov=c.cov_download(system.state.n) if system.state.initialized else None)

    stats, times, poses = rp.replay(op, after_camera=after_camera)
    return stats, poses, end, pictures


def test_a_drive_with_the_picture_after_every_frame_ends_as_one_without(pkg, tmp_path):
    dataset = str(tmp_path / "data")
    sd.make_dataset(dataset, seconds=1.0)                                          # 10 camera frames
    sa, pa, ea, pictures = _drive_system(pkg, dataset, tmp_path, "a", True)
    sb, pb, eb, _ = _drive_system(pkg, dataset, tmp_path, "b", False)
    assert ea["frame"] == eb["frame"] == 9 and len(pictures) == 10
    assert sa["initialized"] and sa["cam_updates"] >= 1, sa                      # (updates ran between the pictures)
    timing = ("time_s", "time_camera_s", "time_after_camera_s", "image_route")
    assert {k: v for k, v in sa.items() if k not in timing} == {k: v for k, v in sb.items() if k not in timing}
    assert np.array_equal(pa, pb) and ea["n"] == eb["n"]
    assert np.array_equal(ea["cov"], eb["cov"]) and np.array_equal(ea["imu"], eb["imu"])
    assert ea["last"] == eb["last"] and ea["lines"] == eb["lines"] and (ea["db"], ea["line_db"]) == (eb["db"], eb["line_db"])
    assert all(rgb.shape == (H, W, 3) for rgb, _, _ in pictures)
    assert all(overlay == ("" if init else "init") for _, overlay, init in pictures) and pictures[0][1] == "init" and pictures[-1][1] == ""
    assert (pictures[-1][0][:, :, 0] != pictures[-1][0][:, :, 2]).any()             # something is drawn


# ---------------------------------------------------------------------------------------------- 4. the replay tool
def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    magic, dims, maxval, rest = data.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert magic == b"P6" and maxval == b"255" and len(rest) == 3 * w * h, path
    return np.frombuffer(rest, dtype=np.uint8).reshape(h, w, 3)


def test_replay_tool_writes_track_images(tmp_path):
    """tools/replay.py --synthetic 6 --track-images DIR: one P6 file of the camera's size per frame (rendering the 60 frames on the
    host is most of this test's time)"""
    out, pics = str(tmp_path / "res.json"), str(tmp_path / "pics")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--synthetic", "6", "--track-images", pics, "--out", out],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    names = sorted(os.listdir(pics))
    assert res["track_images_written"] == len(names) == res["stats"]["camera_messages"] == 60
    assert names == [f"{i:06d}.ppm" for i in range(60)]
    imgs = [_read_ppm(os.path.join(pics, n)) for n in names]
    assert all(im.shape == (H, W, 3) for im in imgs)
    assert (imgs[-1][:, :, 0] != imgs[-1][:, :, 2]).any() and not np.array_equal(imgs[10], imgs[-1])
