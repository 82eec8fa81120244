"""Camera images in the sensor's encoding (PLV_ENC_*: mono8, the four 8-bit Bayer patterns, bgr8 / rgb8 / bgra8 / rgba8) converted to
grey on the device (grey_from_encoded_kernel), everything through the C-ABI: plv_image_convert, plv_image_stage_encoded,
plv_raw_image_buffer, plv_tracker_feed_encoded and the replay driver's device route.  The yardstick is tests/image_encodings_ref.py, a
numpy restatement of the contract; the arithmetic is integer, so every comparison is exact."""
import copy
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import image_encodings_ref as ref
import kaist_synth
import oracle_lib
import synth
import synth_dataset as sd

pytestmark = pytest.mark.gpu

W, H = 752, 480
NAMES = list(ref.ENCODINGS)
SIZES = [(752, 480), (1280, 560), (1280, 720), (753, 481), (67, 35), (3, 3)]


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _colourise(grey):
    """an H x W x 3 RGB image with the structure of a grey frame: three different, monotone renderings of it"""
    g = grey.astype(np.int32)
    return np.stack([g, (g * 3) // 4 + 20, 255 - g // 2], axis=2).astype(np.uint8)


def _encode(rgb, name, rng=None):
    """the RGB image as a camera with that encoding would deliver it"""
    if name == "mono8":
        return ref.colour_to_grey(rgb, "rgb8")
    if name in ref.BAYER:
        return ref.mosaic(rgb, name)
    bgr = name.startswith("bgr")
    img = rgb[:, :, ::-1] if bgr else rgb
    if ref.BPP[name] == 4:
        alpha = rng.integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8) if rng is not None else np.full(rgb.shape[:2] + (1,), 255, np.uint8)
        img = np.concatenate([img, alpha], axis=2)
    return np.ascontiguousarray(img)


@pytest.fixture(scope="module")
def frames():
    """30 rendered frames of the street drive (tests/synth_dataset.py), 752 x 480, grey"""
    return sd.render_frames(np.arange(30) * 0.1, style="street", workers=min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------------------------------------- 1. plv_image_convert
@pytest.mark.parametrize("name", NAMES)
def test_image_convert_equals_the_reference(pkg, ctx, name):
    rng = np.random.default_rng(100 + ref.ENCODINGS[name])
    bpp = ref.BPP[name]
    for (w, h) in SIZES:
        img = ref.random_image(rng, h, w, name)
        want = ref.to_grey(img, name)
        got = ctx.image_convert(img, name)                       # packed rows
        assert got.shape == want.shape and np.array_equal(got, want), (name, w, h, "packed", int((got != want).sum()))
        pad = 13 if bpp == 1 else 5                               # padded rows: a slice of a wider array keeps its stride
        wide = rng.integers(0, 256, (h, w + pad) + (() if bpp == 1 else (bpp,)), dtype=np.uint8)
        wide[:, :w] = img
        view = wide[:, :w]
        assert view.strides[0] == (w + pad) * bpp
        got = ctx.image_convert(view, name)
        assert np.array_equal(got, want), (name, w, h, "padded", int((got != want).sum()))
        # a padded output: the bytes between the rows are left alone
        out = np.full((h, w + 7), 0xA5, dtype=np.uint8)
        a = np.ascontiguousarray(img)
        rc = ctx.lib.plv_image_convert(ctx.h, _u8(a), w * bpp, ref.ENCODINGS[name], w, h, _u8(out), w + 7)
        assert rc == pkg.PLV_OK and np.array_equal(out[:, :w], want) and np.all(out[:, w:] == 0xA5)


@pytest.mark.parametrize("name", NAMES)
def test_image_convert_of_a_rendered_frame(pkg, ctx, frames, name):
    """a rendered frame of tests/synth_dataset.py, coloured and re-mosaicked / re-packed in the encoding"""
    rng = np.random.default_rng(7)
    img = _encode(_colourise(frames[11]), name, rng)
    want = ref.to_grey(img, name)
    assert want.std() > 10                                       # (a picture, not a flat field)
    assert np.array_equal(ctx.image_convert(img, name), want)


# ---------------------------------------------------------------------------------------------- 2. the staged and the fed routes
def _tracker_state(c):
    pts, ids = c.tracker_last()
    sel = np.unique(np.concatenate([c.db_select(0, 1e9), c.db_select(1, 1e9), ids]))
    ptr, t, uv, uvn = c.db_export(sel)
    return dict(level0=c.pyramid_level(0, 0), pts=pts, ids=ids, db_ids=sel, db_size=c.db_size(), ptr=ptr, t=t, uv=uv, uvn=uvn)


def _same_state(a, b, what):
    assert a["db_size"] == b["db_size"] and len(a["ids"]) > 50, what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", NAMES)
def test_encoded_routes_equal_the_grey_routes(pkg, frames, name):
    rng = np.random.default_rng(3)
    enc = [_encode(_colourise(f), name, rng) for f in frames]
    grey = [ref.to_grey(e, name) for e in enc]
    routes = ["image_stage + tracker_feed_staged", "tracker_feed", "image_stage_encoded + tracker_feed_staged", "tracker_feed_encoded",
              "raw_image_buffer + image_stage_encoded + tracker_feed_staged", "raw_image_buffer + tracker_feed_encoded"]
    cs = [pkg.Context(pkg.default_config(W, H)) for _ in routes]
    for k in range(len(frames)):
        t = 0.1 * k
        cs[0].image_stage(k % 8, grey[k])
        cs[0].tracker_feed_staged(t, k % 8)
        cs[1].tracker_feed(t, grey[k])
        cs[2].image_stage_encoded(k % 8, enc[k], name)
        cs[2].tracker_feed_staged(t, k % 8)
        cs[3].tracker_feed_encoded(t, enc[k], name)
        blk = cs[4].raw_image_buffer(k % 4, name)
        blk[...] = enc[k]
        cs[4].image_stage_encoded(k % 8, blk, name)
        cs[4].tracker_feed_staged(t, k % 8)
        blk = cs[5].raw_image_buffer(k % 4, name)
        blk[...] = enc[k]
        cs[5].tracker_feed_encoded(t, blk, name)
        if k in (0, 1, 14, 29):
            want = _tracker_state(cs[0])
            for c, r in zip(cs[1:], routes[1:]):
                _same_state(want, _tracker_state(c), (name, k, r))
    assert want["db_size"] > 100
    for c in cs:
        c.close()


# ---------------------------------------------------------------------------------------------- 3. the one-call frame
TRI = dict(max_cond=1e7, max_dist=100.0, max_baseline=1e3)


def _filled_context(pkg, sc, fo):
    """the hand-made database and covariance of tests/test_gpu_one_call.py; its features get ids the tracker will not hand out"""
    ctx = pkg.Context(pkg.default_config(W, H))
    for f in range(len(sc["obs_ptr"]) - 1):
        a, b = sc["obs_ptr"][f], sc["obs_ptr"][f + 1]
        uv = sc["obs_uv"][a:b].astype(np.float32)
        ctx.db_append_measurements(1000000 + f, sc["obs_time"][a:b].copy(), uv, fo.undistort(sc["K8"], uv))
    ctx.cov_upload(synth.spd_cov(sc["n_state"], seed=4) * 1e-4)
    return ctx


def _scene_state(pkg, sc):
    st, _ = synth.scene_views(pkg, copy.deepcopy(sc))
    K = np.array(st.c.intrinsics)
    base = C.addressof(st.c)
    ent = [("vec", int(st.ids[i]) + 3, st.p[i], None, None) for i in range(len(st.ids))]
    ent.append(("vec", sc["intr_id"], K, None, base + pkg.PlvStateView.intrinsics.offset))
    return st, K, pkg.BoxPlus(ent)


@pytest.mark.parametrize("name", ["bayer_rggb8", "bgr8"])
def test_camera_frame_from_an_encoded_slot(pkg, name):
    """plv_camera_frame with slot >= 0 after plv_image_stage_encoded against plv_camera_frame with the converted host image, on the drive
    of tests/test_gpu_one_call.py (hand-made database + rendered canvas frames): two feeds without an update, then a frame with the update"""
    fo = oracle_lib.load_front()
    sc = synth.vio_scene(F=60, M=15, noise_px=0.4, seed=11)
    n, t = sc["n_state"], sc["t"]
    canvas = synth.texture_canvas(W, H, seed=42)
    a, b = _filled_context(pkg, sc, fo), _filled_context(pkg, sc, fo)
    st_a, K_a, plus_a = _scene_state(pkg, sc)
    st_b, K_b, plus_b = _scene_state(pkg, sc)
    K0 = K_a.copy()
    dt = float(t[-1] - t[-2])
    kw = dict(n=n, max_msckf=40, max_obs=15, t_prev_frame=float(t[-2]), state_time=float(t[-1]), window_full=True, lines=False, **TRI)
    for k in range(3):
        frame = synth.render_frame(canvas, W, H, tx=2.0 * k, ty=-1.0 * k)
        enc = _encode(_colourise(frame), name)
        grey = ref.to_grey(enc, name)
        last = k == 2
        stamp = float(t[-1]) if last else float(t[-3]) + 0.25 * dt * (k + 1)
        ra = a.camera_frame(st_a, stamp, img=grey, update=dict(plus=plus_a, **kw) if last else None)
        b.image_stage_encoded(3, enc, name)
        rb = b.camera_frame(st_b, stamp, slot=3, update=dict(plus=plus_b, **kw) if last else None)
        a.synchronize(), b.synchronize()
        assert ra[2] == rb[2]
        if last:
            assert ra[0]["status"] == rb[0]["status"] == 0 and ra[0]["n_accepted"] == rb[0]["n_accepted"] > 20
            for key in ("ids", "accepted", "dx", "p_FinG", "n_pool", "n_rows"):
                assert np.array_equal(ra[0][key], rb[0][key]), key
            assert np.abs(ra[0]["dx"]).max() > 0
        assert np.array_equal(a.cov_download(n), b.cov_download(n)), k
        assert np.array_equal(st_a.p, st_b.p) and np.array_equal(K_a, K_b) and np.array_equal(np.array(st_a.c.intrinsics), np.array(st_b.c.intrinsics))
        pa, ia = a.tracker_last()
        pb, ib = b.tracker_last()
        assert len(ia) > 50 and np.array_equal(ia, ib) and np.array_equal(pa, pb)
    assert not np.array_equal(K_a, K0)      # (the update moved the state)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------- 4. KAIST-layout replay
def test_kaist_layout_replay_device_route_equals_host_route(pkg, tmp_path):
    options, rp, kaist = (importlib.import_module("plviwo_amd." + m) for m in ("options", "replay", "kaist"))
    src = str(tmp_path / "street_src")
    sd.make_dataset(src, seconds=5.0, cam_hz=10.0, style="street", workers=min(16, os.cpu_count() or 1))
    kdir = kaist_synth.convert(src, str(tmp_path / "urban_synth"), sd.RL, sd.RR, sd.BASE, t0_ns=1000 * 10**9)
    ds = rp.open_dataset(kdir)
    assert isinstance(ds, kaist.KaistDataset) and ds.encoding == "bayer_rggb8"
    assert np.array_equal(ref.to_grey(ds.raw_image(2), ds.encoding), ds.image(2))
    runs = {}
    for route, host in (("device", False), ("host", True)):
        op = options.load_options(sd.write_config(str(tmp_path / "config"), kdir, str(tmp_path / f"traj_{route}.txt"), use_wheel=True))
        stats, times, poses = rp.replay(op, host_images=host)
        assert stats["initialized"] and stats["not_psd"] == 0 and stats["image_route"] == route, stats
        runs[route] = (stats, times, poses)
    (sa, ta, pa), (sb, tb, pb) = runs["device"], runs["host"]
    assert len(ta) >= 30 and np.array_equal(ta, tb) and np.array_equal(pa, pb)
    timing = ("time_s", "time_camera_s", "image_route")
    assert {k: v for k, v in sa.items() if k not in timing} == {k: v for k, v in sb.items() if k not in timing}
    assert sa["cam_accepted"] >= 300 and sa["camera_messages"] == sb["camera_messages"] >= 45
    assert open(str(tmp_path / "traj_device.txt")).read() == open(str(tmp_path / "traj_host.txt")).read()


# ---------------------------------------------------------------------------------------------- 5. mono8
def test_mono8_staging_equals_image_stage(pkg, frames):
    a, b = pkg.Context(pkg.default_config(W, H)), pkg.Context(pkg.default_config(W, H))
    for k in range(3):
        a.image_stage(k, frames[k])
        a.tracker_feed_staged(0.1 * k, k)
        b.image_stage_encoded(k, frames[k], "mono8")
        b.tracker_feed_staged(0.1 * k, k)
    _same_state(_tracker_state(a), _tracker_state(b), "mono8")
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------- 6. refused arguments
def test_refused_arguments_leave_slot_and_tracker_alone(pkg, frames):
    e = ref.ENCODINGS
    rng = np.random.default_rng(9)
    c, twin = pkg.Context(pkg.default_config(W, H)), pkg.Context(pkg.default_config(W, H))
    bayer = [ref.mosaic(_colourise(f), "bayer_rggb8") for f in frames[:3]]
    bgr = _encode(_colourise(frames[1]), "bgr8")
    for x in (c, twin):
        x.image_stage_encoded(2, bayer[0], "bayer_rggb8")
        x.tracker_feed_encoded(0.0, bayer[0], "bayer_rggb8")
        x.image_stage_encoded(2, bayer[1], "bayer_rggb8")          # what slot 2 holds from here on
    other = np.ascontiguousarray(bayer[2])
    lib, h = c.lib, c.h
    refused = [
        ("null image", lambda: lib.plv_image_stage_encoded(h, 2, None, W, e["bayer_rggb8"])),
        ("slot -1", lambda: lib.plv_image_stage_encoded(h, -1, _u8(other), W, e["bayer_rggb8"])),
        ("slot 8", lambda: lib.plv_image_stage_encoded(h, 8, _u8(other), W, e["bayer_rggb8"])),
        ("encoding 9", lambda: lib.plv_image_stage_encoded(h, 2, _u8(other), W, 9)),
        ("encoding -1", lambda: lib.plv_image_stage_encoded(h, 2, _u8(other), W, -1)),
        ("stride below width", lambda: lib.plv_image_stage_encoded(h, 2, _u8(other), W - 1, e["bayer_rggb8"])),
        ("stride below width * 3", lambda: lib.plv_image_stage_encoded(h, 2, _u8(bgr), 3 * W - 1, e["bgr8"])),
        ("stride below width * 4", lambda: lib.plv_image_stage_encoded(h, 2, _u8(bgr), 3 * W, e["rgba8"])),
        ("null context", lambda: lib.plv_image_stage_encoded(None, 2, _u8(other), W, e["bayer_rggb8"])),
        ("feed: null image", lambda: lib.plv_tracker_feed_encoded(h, 0.1, None, W, e["bayer_rggb8"], None)),
        ("feed: encoding 9", lambda: lib.plv_tracker_feed_encoded(h, 0.1, _u8(other), W, 9, None)),
        ("feed: stride below width", lambda: lib.plv_tracker_feed_encoded(h, 0.1, _u8(other), W - 1, e["bayer_rggb8"], None)),
        ("buffer: index 4", lambda: lib.plv_raw_image_buffer(h, 4, e["bgr8"], C.byref(C.POINTER(C.c_uint8)()), None)),
        ("buffer: encoding 9", lambda: lib.plv_raw_image_buffer(h, 0, 9, C.byref(C.POINTER(C.c_uint8)()), None)),
        ("buffer: null pointer", lambda: lib.plv_raw_image_buffer(h, 0, e["bgr8"], None, None)),
        ("convert: null output", lambda: lib.plv_image_convert(h, _u8(other), W, e["bayer_rggb8"], W, H, None, W)),
        ("convert: null image", lambda: lib.plv_image_convert(h, None, W, e["bayer_rggb8"], W, H, _u8(np.zeros((H, W), np.uint8)), W)),
        ("convert: 2 x 2 mosaic", lambda: lib.plv_image_convert(h, _u8(other), W, e["bayer_rggb8"], 2, 2, _u8(np.zeros((H, W), np.uint8)), W)),
        ("convert: output stride", lambda: lib.plv_image_convert(h, _u8(other), W, e["bayer_rggb8"], W, H, _u8(np.zeros((H, W), np.uint8)), W - 1)),
        ("convert: encoding", lambda: lib.plv_image_convert(h, _u8(other), W, 17, W, H, _u8(np.zeros((H, W), np.uint8)), W)),
    ]
    for what, call in refused:
        assert call() == pkg.PLV_E_BADARG, what
        if what != "null context":
            assert len(lib.plv_last_error()) > 0, what
    # the tracker is where the one accepted feed left it, and slot 2 still holds the second mosaic
    pc, ic = c.tracker_last()
    pt, it = twin.tracker_last()
    assert len(ic) > 50 and np.array_equal(ic, it) and np.array_equal(pc, pt) and c.db_size() == twin.db_size()
    for x in (c, twin):
        x.tracker_feed_staged(0.1, 2)
    _same_state(_tracker_state(twin), _tracker_state(c), "after the refused calls")
    fresh = pkg.Context(pkg.default_config(W, H))
    fresh.tracker_feed(0.0, ref.to_grey(bayer[0], "bayer_rggb8"))
    fresh.tracker_feed(0.1, ref.to_grey(bayer[1], "bayer_rggb8"))
    _same_state(_tracker_state(fresh), _tracker_state(c), "the grey route fed the two images")
    for x in (c, twin, fresh):
        x.close()
    assert pkg.encoding_from_name("mono16") == -1 and rng is not None


# ---------------------------------------------------------------------------------------------- 7. nothing is allocated ahead
def test_raw_blocks_are_allocated_on_first_use(pkg, frames):
    c = pkg.Context(pkg.default_config(W, H))
    for k in range(4):
        c.tracker_feed(0.1 * k, frames[k])
    c.synchronize()
    m0, a0 = pkg.memory_bytes(), pkg.alloc_count()
    assert pkg.encoding_from_name("bayer_rggb8") == 1 and pkg.encoding_bytes_per_pixel(1) == 1
    assert pkg.memory_bytes() == m0 and pkg.alloc_count() == a0      # grey frames and the name table: no raw block
    blk = c.raw_image_buffer(0, "bgr8")
    m1, a1 = pkg.memory_bytes(), pkg.alloc_count()
    assert blk.shape == (H, W, 3) and m1["pinned"] >= m0["pinned"] + W * H * 3 and m1["device"] == m0["device"] and a1 > a0
    blk[...] = _encode(_colourise(frames[4]), "bgr8")
    c.image_stage_encoded(0, blk, "bgr8")                              # the first encoded image: slot 0 comes into being
    m2, a2 = pkg.memory_bytes(), pkg.alloc_count()
    assert a2 > a1 and m2["pinned"] == m1["pinned"] and m2["device"] >= m1["device"] + W * H
    c.image_stage_encoded(0, blk, "bgr8")
    c.tracker_feed_staged(0.4, 0)
    c.synchronize()
    assert pkg.alloc_count() == a2 and pkg.memory_bytes()["pinned"] == m2["pinned"] and pkg.memory_bytes()["device"] == m2["device"]
    # an image that lies anywhere else: the library's own blocks at the first call, nothing at the second
    arr = _encode(_colourise(frames[5]), "bgr8")
    c.image_stage_encoded(0, arr, "bgr8")
    m3, a3 = pkg.memory_bytes(), pkg.alloc_count()
    assert a3 > a2 and m3["pinned"] >= m2["pinned"] + W * H * 3
    c.image_stage_encoded(0, arr, "bgr8")
    c.image_stage_encoded(0, arr, "bgr8")
    c.synchronize()
    m4 = pkg.memory_bytes()
    assert pkg.alloc_count() == a3 and m4["pinned"] == m3["pinned"] and m4["device"] == m3["device"]
    c.close()
