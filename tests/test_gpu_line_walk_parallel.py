"""plv_line_walk_mode 2 — one wave per 8-connected component of the edge map for the chain walk, the kept chains ordered by their seeds,
one wave per chain for the segment fit — against the CPU, through the C-ABI.

References: the edge map is the oracle's Canny of the half-resolution equalised image; the chains are a plain-Python restatement of
FastLineDetector's seed loop and getPointChain on that map (float32 arithmetic through numpy scalars, so the running mean of the
direction rounds as the oracle's does); the segments are the oracle's detect_lines."""
import numpy as np
import pytest
from scipy import ndimage

import oracle_lib
import synth
from line_restatement import LEN_THR, edge_map, walk_chains      # the CPU references: the detector's edge map, the chain walk

pytestmark = pytest.mark.gpu

SEG_TOL = 2e-3        # the contract of the device fit in test_detect_lines_parity (float rounding of the fit's atan2 / cos / sin)
_EIGHT = np.ones((3, 3), dtype=int)


@pytest.fixture(scope="module")
def lo():
    return oracle_lib.load_line()


# ------------------------------------------------------------------------------------------------ the drawings (320 x 240)
DW, DH = 320, 240


def _blank(w=DW, h=DH, v=30):
    return np.full((h, w), v, dtype=np.uint8)


def draw_bars():
    """(a) two bars side by side over the same rows: their edge components interleave in raster order"""
    img = _blank()
    img[60:100, 24:150] = 220
    img[80:130, 176:300] = 200
    return img


def draw_disc():
    """(b) a bright disc: its edge component is a closed ring; a bar beside it is the second component"""
    img = _blank()
    yy, xx = np.mgrid[0:DH, 0:DW]
    img[(xx - 120) ** 2 + (yy - 120) ** 2 <= 80 ** 2] = 215
    img[40:200, 250:280] = 180
    return img


def draw_t_and_cross():
    """(c) a T and a cross out of bars of different brightness: three tones meet, the edge components have junctions and leave
    several chains with several seeds each"""
    img = _blank()
    img[30:60, 20:140] = 225          # T: the roof ...
    img[60:200, 65:95] = 130          # ... and the stem, darker
    img[100:130, 170:310] = 225       # cross: the horizontal bar ...
    img[30:100, 225:255] = 120        # ... and the vertical one in two darker halves
    img[130:220, 225:255] = 120
    return img


def draw_ring_around_bar():
    """(d) a ring with a bar inside: the ring's walk leaves its lower part to later seeds, which lie below the first seed of the bar's
    component — ordering by seed, not by component"""
    img = _blank()
    yy, xx = np.mgrid[0:DH, 0:DW]
    r2 = (xx - 160) ** 2 + (yy - 120) ** 2
    img[(r2 <= 100 ** 2) & (r2 >= 84 ** 2)] = 220
    img[100:140, 110:210] = 200
    return img


def draw_bar_and_stub():
    """(e) two bars and a 10 x 10 stub whose edge component has fewer than length_threshold + 1 pixels: dropped before the walk"""
    img = _blank()
    img[50:90, 30:200] = 220
    img[140:190, 90:290] = 190
    img[110:120, 250:260] = 220
    return img


def draw_spiral():
    """(f) an Archimedean spiral band: one edge component (both flanks of the band, joined at its ends) of more than 1500 pixels"""
    img = _blank()
    yy, xx = np.mgrid[0:DH, 0:DW].astype(np.float64)
    dx, dy = xx - 160.0, yy - 120.0
    r, th = np.hypot(dx, dy), np.arctan2(dy, dx)
    pitch = 22.0
    m = np.zeros(img.shape, dtype=bool)
    for k in range(0, 6):
        t = th + 2 * np.pi * k                       # the spiral r = pitch * t / (2 pi), t in [2 pi, 10 pi]
        m |= (np.abs(r - pitch * t / (2 * np.pi)) < 4.0) & (t >= 2 * np.pi) & (t <= 10 * np.pi)
    img[m] = 220
    return img


DRAWINGS = {"bars": draw_bars, "disc": draw_disc, "t_and_cross": draw_t_and_cross, "ring_around_bar": draw_ring_around_bar,
            "bar_and_stub": draw_bar_and_stub, "spiral": draw_spiral}


# ------------------------------------------------------------------------------------------------ helpers
_ctxs = {}


@pytest.fixture(scope="module")
def ctx_of(pkg):
    """one context per image size, shared by the module's tests"""
    def get(w, h):
        if (w, h) not in _ctxs:
            _ctxs[(w, h)] = pkg.Context(pkg.default_config(w, h))
        return _ctxs[(w, h)]
    yield get
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()


def detect_in_mode(ctx, mode):
    """(segments, chains, info) of the current image in a device mode; mode 0 is restored"""
    ctx.line_walk_mode(mode)
    try:
        segs = ctx.detect_lines(0)
        return segs, ctx.line_chains(), ctx.line_walk_info()
    finally:
        ctx.line_walk_mode(0)


def assert_same_chains(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for c, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and np.array_equal(g, r), (what, "chain", c, g.shape, r.shape)


def check_frame(ctx, lo, img, what, min_components=2, min_segments=1):
    """Cases 1 and 2 on one image: the chains of modes 2 and 1 against the Python walk, bit for bit; the segments of mode 2 against
    mode 1's (bit for bit) and the oracle's (count, order, SEG_TOL).  Returns what the tests of the single drawings look at."""
    ctx.feed_image(img)
    eq = ctx.pyramid_level(0, 0)
    edges = edge_map(lo, eq)
    ref_chains = walk_chains(edges)
    ref_segs = lo.detect_lines(eq)
    s2, c2, i2 = detect_in_mode(ctx, 2)
    s1, c1, i1 = detect_in_mode(ctx, 1)
    print(what, "mode 2:", i2, "| mode 1:", i1, "| reference chains", len(ref_chains), "segments", len(ref_segs))
    assert i2["mode"] == 2 and i2["fell_back"] == 0, (what, i2)
    assert i1["mode"] == 1 and i1["fell_back"] == 0 and i1["n_components"] == 0, (what, i1)
    assert i2["n_components"] >= min_components and i2["n_chains"] > 0, (what, i2)
    assert i2["n_chains"] == len(ref_chains) == i1["n_chains"], (what, i2, i1, len(ref_chains))
    assert_same_chains(c2, ref_chains, what + ": mode 2")
    assert_same_chains(c1, ref_chains, what + ": mode 1")
    # the components the device lists are the components of the reference map that can hold a kept chain
    lab, n_lab = ndimage.label(edges, structure=_EIGHT)
    sizes = np.bincount(lab.ravel())[1:]
    assert i2["n_components"] == int((sizes >= LEN_THR + 1).sum()), (what, i2, sizes)
    assert i2["longest_component"] == int(sizes.max()), (what, i2, int(sizes.max()))
    assert len(ref_segs) >= min_segments, (what, len(ref_segs))
    assert s2.shape == s1.shape and np.array_equal(s2, s1), (what, s2.shape, s1.shape)
    assert s2.shape == ref_segs.shape, (what, s2.shape, ref_segs.shape)
    assert np.abs(s2 - ref_segs).max() < SEG_TOL, (what, float(np.abs(s2 - ref_segs).max()))
    return dict(edges=edges, lab=lab, sizes=sizes, chains=ref_chains, info=i2)


# ------------------------------------------------------------------------------------------------ 1, 2: drawings
@pytest.mark.parametrize("name", list(DRAWINGS))
def test_drawings_chains_and_segments(ctx_of, lo, name):
    r = check_frame(ctx_of(DW, DH), lo, DRAWINGS[name](), name, min_components=1 if name == "spiral" else 2)
    seed_comp = [int(r["lab"][c[0][1], c[0][0]]) for c in r["chains"]]      # component of every kept chain's seed, in output order
    if name == "bars":
        # the two bars' components take turns in the output: neither comes out in one piece
        assert len(set(seed_comp)) >= 2 and any(seed_comp[i] != seed_comp[i + 1] and seed_comp[i] in seed_comp[i + 2:] for i in range(len(seed_comp) - 2)), seed_comp
    if name == "t_and_cross":
        # junctions: a component leaves several kept chains
        assert max(seed_comp.count(k) for k in set(seed_comp)) >= 3, seed_comp
    if name == "ring_around_bar":
        # A ... B ... A: a later seed of one component lies behind the first seed of another
        first = {k: seed_comp.index(k) for k in set(seed_comp)}
        assert any(first[b] > first[a] and a in seed_comp[first[b]:] for a in first for b in first if a != b), seed_comp
    if name == "bar_and_stub":
        assert (r["sizes"] < LEN_THR + 1).any() and r["info"]["n_components"] < len(r["sizes"]), r["sizes"]
    if name == "spiral":
        assert r["sizes"].max() > 1500 and r["info"]["longest_component"] > 1500, r["sizes"]


# ------------------------------------------------------------------------------------------------ 2: the textured frames
def test_textured_frames_segments(ctx_of, lo):
    """the two textured 752 x 480 frames of test_gpu_linefront.py: mode 2's segments are mode 1's bit for bit, the oracle's in count and
    order and within SEG_TOL"""
    W, H = 752, 480
    canvas = synth.texture_canvas(W, H, seed=11, blobs=200, lines=120)
    ctx = ctx_of(W, H)
    for i in range(2):
        ctx.feed_image(synth.render_frame(canvas, W, H, tx=3.0 * i, ty=-2.0 * i, rot_deg=0.2 * i))
        ref = lo.detect_lines(ctx.pyramid_level(0, 0))
        s2, _, i2 = detect_in_mode(ctx, 2)
        s1, _, i1 = detect_in_mode(ctx, 1)
        print("textured frame", i, i2, len(ref))
        assert i2["mode"] == 2 and i2["fell_back"] == 0 and i2["n_components"] >= 2 and i2["n_chains"] == i1["n_chains"] > 0, (i2, i1)
        assert len(ref) > 20 and s2.shape == s1.shape == ref.shape, (s2.shape, s1.shape, ref.shape)
        assert np.array_equal(s2, s1)
        assert np.abs(s2 - ref).max() < SEG_TOL


# ------------------------------------------------------------------------------------------------ 3: sizes
def _boxes_image(w, h, seed):
    """slanted two-tone strips over a ramp: components of all sizes, long and short chains"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = 60.0 + 40.0 * xx / w + 30.0 * yy / h
    for _ in range(24):
        a = rng.uniform(0, np.pi)
        c, s_ = np.cos(a), np.sin(a)
        u = c * (xx - rng.uniform(0, w)) + s_ * (yy - rng.uniform(0, h))
        v = -s_ * (xx - rng.uniform(0, w)) + c * (yy - rng.uniform(0, h))
        img[(np.abs(u) < rng.uniform(3, 0.12 * w)) & (np.abs(v) < rng.uniform(10, 0.35 * w))] = rng.uniform(20, 235)
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("w,h", [(1280, 720), (750, 478)])
def test_other_sizes(ctx_of, lo, w, h):
    """1280 x 720: the half-resolution map is 230 KB of bytes — more than LDS holds — and 29 KB of bits; 750 x 478: 375 x 239 is no
    multiple of the Canny tile (16) nor of the bit map's word (64).  The assertions of the drawings."""
    check_frame(ctx_of(w, h), lo, _boxes_image(w, h, 5), f"{w}x{h}", min_segments=10)


# ------------------------------------------------------------------------------------------------ 4: fallback
def test_fallback_above_the_root_list(ctx_of, lo):
    """more 8-connected components than the device lists (4096): mode 2 runs mode 1's kernels, says so, and gives mode 1's segments"""
    w, h = 1280, 720
    img = _blank(w, h)
    img[8:h - 8:8, 8:w - 8:8] = 230            # a field of dots, one every 4 half-resolution pixels ...
    img[9:h - 8:8, 8:w - 8:8] = 230
    img[8:h - 8:8, 9:w - 8:8] = 230
    img[9:h - 8:8, 9:w - 8:8] = 230
    img[300:420, 200:1000] = 200               # ... and a bar, so that there are segments to compare
    ctx = ctx_of(w, h)
    ctx.feed_image(img)
    eq = ctx.pyramid_level(0, 0)
    n_comp = ndimage.label(edge_map(lo, eq), structure=_EIGHT)[1]
    assert n_comp > 4096, n_comp
    ref = lo.detect_lines(eq)
    s2, c2, i2 = detect_in_mode(ctx, 2)
    s1, c1, i1 = detect_in_mode(ctx, 1)
    print("fallback:", n_comp, "components", i2, len(ref))
    assert i2["fell_back"] == 1 and i2["mode"] == 1 and i2["n_components"] == 0, i2
    assert i1["fell_back"] == 0 and i1["mode"] == 1, i1
    assert len(s1) >= 2 and s2.shape == s1.shape and np.array_equal(s2, s1)
    assert s2.shape == ref.shape and np.abs(s2 - ref).max() < SEG_TOL
    assert_same_chains(c2, c1, "fallback")
    # the next detection with fewer components walks by components again
    ctx.feed_image(_boxes_image(w, h, 6))
    _, _, i3 = detect_in_mode(ctx, 2)
    assert i3["mode"] == 2 and i3["fell_back"] == 0 and i3["n_components"] >= 2, i3


# ------------------------------------------------------------------------------------------------ 5: capacities and refusals
def test_line_chains_capacities_and_refusals(pkg, ctx_of):
    import ctypes as C
    ctx = ctx_of(DW, DH)
    lib, ip = ctx.lib, C.POINTER(C.c_int)
    ctx.feed_image(draw_t_and_cross())
    ctx.line_walk_mode(0)
    ctx.detect_lines(0)
    n = C.c_int(-7)
    assert lib.plv_line_chains(ctx.h, 0, 0, None, None, C.byref(n)) == pkg.PLV_E_BADARG      # after a mode-0 detection
    assert ctx.line_walk_info()["mode"] == 0
    assert lib.plv_line_walk_info(ctx.h, None, None, None, None, None) == pkg.PLV_OK         # every pointer is nullable
    try:
        ctx.line_walk_mode(2)
        ctx.detect_lines(0)
        chains = ctx.line_chains()
        assert lib.plv_line_chains(ctx.h, 0, 0, None, None, C.byref(n)) == pkg.PLV_OK and n.value == len(chains) >= 2    # the query
        assert lib.plv_line_chains(ctx.h, 0, 0, None, None, None) == pkg.PLV_OK
        total = sum(len(c) for c in chains)
        guard = np.int32(-12345)
        ptr = np.full(len(chains) + 1, guard, dtype=np.int32)
        pts = np.full(2 * total, guard, dtype=np.int32)
        # one chain too few, one point too few: PLV_E_CAPACITY and nothing written
        assert lib.plv_line_chains(ctx.h, len(chains) - 1, total, ptr.ctypes.data_as(ip), pts.ctypes.data_as(ip), C.byref(n)) == pkg.PLV_E_CAPACITY
        assert n.value == len(chains) and (ptr == guard).all() and (pts == guard).all()
        assert lib.plv_line_chains(ctx.h, len(chains), total - 1, ptr.ctypes.data_as(ip), pts.ctypes.data_as(ip), C.byref(n)) == pkg.PLV_E_CAPACITY
        assert (ptr == guard).all() and (pts == guard).all()
        # exactly enough: everything written, nothing past it
        ptr = np.full(len(chains) + 3, guard, dtype=np.int32)
        pts = np.full(2 * total + 4, guard, dtype=np.int32)
        assert lib.plv_line_chains(ctx.h, len(chains), total, ptr.ctypes.data_as(ip), pts.ctypes.data_as(ip), C.byref(n)) == pkg.PLV_OK
        assert ptr[0] == 0 and ptr[len(chains)] == total and (ptr[len(chains) + 1:] == guard).all() and (pts[2 * total:] == guard).all()
        assert np.array_equal(pts[:2 * total].reshape(-1, 2), np.concatenate(chains))
        assert lib.plv_line_chains(ctx.h, -1, 0, ptr.ctypes.data_as(ip), None, None) == pkg.PLV_E_BADARG
        # modes: True and False stay 1 and 0, any other non-zero value means 1
        for arg, ran in ((True, 1), (5, 1), (2, 2), (False, 0)):
            ctx.line_walk_mode(arg)
            ctx.detect_lines(0)
            assert ctx.line_walk_info()["mode"] == ran, (arg, ctx.line_walk_info())
    finally:
        ctx.line_walk_mode(0)
    # a fresh context: nothing detected yet
    c2 = pkg.Context(pkg.default_config(DW, DH))
    try:
        assert c2.lib.plv_line_chains(c2.h, 0, 0, None, None, C.byref(n)) == pkg.PLV_E_BADARG
        assert c2.line_walk_info() == dict(mode=0, n_components=0, longest_component=0, n_chains=0, fell_back=0)
    finally:
        c2.close()


# ------------------------------------------------------------------------------------------------ 6: through the tracker
def test_tracker_feed_in_mode_2_matches_mode_1(pkg, lo):
    """three frames of test_line_tracker_stream's input through plv_line_tracker_feed: the same track store in mode 2 as in mode 1"""
    W, H = 752, 480
    canvas = synth.texture_canvas(W, H, seed=11, blobs=200, lines=120)
    frames = [synth.render_frame(canvas, W, H, tx=3.0 * i, ty=-2.0 * i, rot_deg=0.2 * i) for i in range(3)]
    cfg = pkg.default_config(W, H)
    vps = lo.vanishing_points(np.eye(3), np.array(list(cfg.intrinsics)))
    a, b = pkg.Context(pkg.default_config(W, H)), pkg.Context(pkg.default_config(W, H))
    try:
        a.line_walk_mode(2)
        b.line_walk_mode(1)
        for i, img in enumerate(frames):
            t = 10.0 + 0.05 * i
            for c in (a, b):
                c.tracker_feed(t, img)
                c.line_tracker_feed(t, vps)
            assert a.line_walk_info()["mode"] == 2 and a.line_walk_info()["fell_back"] == 0 and b.line_walk_info()["mode"] == 1
            (la, ia), (lb, ib) = a.line_tracker_last(), b.line_tracker_last()
            assert len(ia) > 0 and np.array_equal(ia, ib) and np.array_equal(la, lb)
        assert a.line_db_size() == b.line_db_size() > 0
        ids = a.line_db_ids()
        assert np.array_equal(ids, b.line_db_ids())
        ea, eb = a.line_db_export(ids), b.line_db_export(ids)
        for k in ("obs_ptr", "obs_time", "seg_uv", "seg_uvn", "D", "pts_ptr", "pt_ids"):
            assert np.array_equal(ea[k], eb[k]), k
        assert len(ea["pt_ids"]) > 0
    finally:
        a.line_walk_mode(0), b.line_walk_mode(0)
        a.close(), b.close()
