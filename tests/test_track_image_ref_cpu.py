"""CPU tests: tests/track_image_ref.py — the numpy restatement the device's track image is held to — against answers written out by
hand from the rules of include/plviwo.h "track image"."""
import numpy as np

import track_image_ref as R


def _pixels(p, W=32, H=32):
    xs, ys = R.coverage(p, W, H)
    return sorted(zip(xs.tolist(), ys.tolist()))


def test_disc_sizes():
    assert len(_pixels(R.disc(10, 10, 1, (1, 2, 3)))) == 5
    assert _pixels(R.disc(10, 10, 1, (1, 2, 3))) == [(9, 10), (10, 9), (10, 10), (10, 11), (11, 10)]
    px = _pixels(R.disc(10, 10, 2, (1, 2, 3)))
    assert len(px) == 13
    assert (12, 10) in px and (11, 11) in px and (12, 11) not in px
    # clipped at the corner: the quarter that lies inside
    assert _pixels(R.disc(0, 0, 2, (1, 2, 3))) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)]


def test_segment_x_major_and_reverse():
    # dx = 5, dy = 2: y = floor((4 i + 5) / 10) = 0 0 1 1 2 2
    want = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]
    assert _pixels(R.prim(R.SEG, 0, 0, 5, 2, a=1)) == want
    # from the other end: x = 5 - i, y = 2 - floor((4 i + 5) / 10)
    assert _pixels(R.prim(R.SEG, 5, 2, 0, 0, a=1)) == sorted([(5, 2), (4, 2), (3, 1), (2, 1), (1, 0), (0, 0)])
    # a slope where the two directions differ: dx = 3, dy = 1: floor((2 i + 3) / 6) = 0 0 1 1 forwards, 1 - (0 0 1 1) backwards
    assert _pixels(R.prim(R.SEG, 0, 0, 3, 1, a=1)) == [(0, 0), (1, 0), (2, 1), (3, 1)]
    assert _pixels(R.prim(R.SEG, 3, 1, 0, 0, a=1)) == [(0, 0), (1, 0), (2, 1), (3, 1)]
    # downwards: sign(dy) = -1
    assert _pixels(R.prim(R.SEG, 0, 4, 5, 2, a=1)) == [(0, 4), (1, 4), (2, 3), (3, 3), (4, 2), (5, 2)]


def test_segment_y_major_and_zero_length():
    # dx = 1, dy = 4: x = 1 + floor((2 i + 4) / 8) = 1 1 2 2 2
    assert _pixels(R.prim(R.SEG, 1, 0, 2, 4, a=1)) == [(1, 0), (1, 1), (2, 2), (2, 3), (2, 4)]
    assert _pixels(R.prim(R.SEG, 3, 3, 3, 3, a=1)) == [(3, 3)]
    assert _pixels(R.prim(R.SEG, 3, 3, 3, 3, a=2)) == [(3, 3), (3, 4)]
    assert _pixels(R.prim(R.SEG, -4, 3, -4, 3, a=1)) == []
    # |dx| = |dy| counts as x-major
    assert _pixels(R.prim(R.SEG, 0, 0, 2, 2, a=2)) == [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3)]


def test_segment_thickness_two():
    want = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)] + [(0, 1), (1, 1), (2, 2), (3, 2), (4, 3), (5, 3)]
    assert _pixels(R.prim(R.SEG, 0, 0, 5, 2, a=2)) == sorted(want)
    # y-major: the extra pixel lies at x + 1
    assert _pixels(R.prim(R.SEG, 1, 0, 2, 4, a=2)) == sorted([(1, 0), (1, 1), (2, 2), (2, 3), (2, 4), (2, 0), (2, 1), (3, 2), (3, 3), (3, 4)])


def test_line_marker_ring():
    px = _pixels(R.prim(R.RING, 16, 16, a=49, b=81))
    # lattice points within radius 9 (253) less those within 48 < 7^2 (149 - 4 on the circle of radius 7)
    assert len(px) == 253 - 145 == 108
    rel = {(x - 16, y - 16) for x, y in px}
    assert (7, 0) in rel and (9, 0) in rel and (5, 5) in rel and (-6, -4) in rel
    assert (6, 3) not in rel and (9, 1) not in rel and (0, 0) not in rel and (7, 6) not in rel


def test_box_orders_its_corners():
    want = [(x, y) for x in range(1, 5) for y in range(1, 4) if x in (1, 4) or y in (1, 3)]
    assert len(want) == 10
    for c in ((1, 1, 4, 3), (4, 3, 1, 1), (4, 1, 1, 3), (1, 3, 4, 1)):
        assert _pixels(R.prim(R.BOX, *c)) == sorted(want)
    assert _pixels(R.prim(R.BOX, 2, 2, 2, 2)) == [(2, 2)]
    # half outside: the edges that remain
    assert _pixels(R.prim(R.BOX, -2, -2, 1, 1)) == [(0, 1), (1, 0), (1, 1)]


def test_paint_order_and_base():
    grey = np.arange(64, dtype=np.uint8).reshape(8, 8)
    a, b = R.disc(3, 3, 1, (10, 20, 30)), R.disc(4, 3, 1, (40, 50, 60))
    img = R.render(grey, R.prims_array([a, b]))
    assert tuple(img[3, 3]) == (40, 50, 60) and tuple(img[3, 4]) == (40, 50, 60) and tuple(img[3, 2]) == (10, 20, 30)
    img = R.render(grey, R.prims_array([b, a]))
    assert tuple(img[3, 3]) == (10, 20, 30) and tuple(img[3, 4]) == (10, 20, 30) and tuple(img[3, 5]) == (40, 50, 60)
    assert tuple(img[0, 0]) == (0, 0, 0) and tuple(img[7, 7]) == (63, 63, 63)
    assert np.array_equal(R.render(grey, R.prims_array([]))[:, :, 1], grey)


def test_colour_ramp_n7():
    c1, c2 = (255, 255, 0), (255, 255, 255)
    # 255 / 7 * z = 36.43 72.86 109.29 145.71 182.14 218.57, truncated
    want = {1: (219, 219, 255), 2: (183, 183, 255), 3: (146, 146, 255), 4: (110, 110, 255), 5: (73, 73, 255), 6: (37, 37, 255)}
    for z, rgb in want.items():
        assert R.ramp_color(c1, c2, 7, z) == rgb
    assert R.ramp_color((600, -600, 0), (100, 100, 7), 2, 1) == (0, 255, 7)  # clamped
    assert R.flagged_color(7, 6) == (0, 255, 37) and R.flagged_color(7, 1) == (0, 255, 219)


def test_history_layer_layout_and_max_tracks():
    uv = np.stack([np.arange(60, dtype=np.float32) * 5 + 20, np.full(60, 100, dtype=np.float32)], axis=1)
    out = R.history_layer(752, 480, [(315.0, 100.0)], [7], {7: uv})
    # z = 59 .. 10 (n - z <= 50): 50 discs; every one but the newest has a segment to its successor
    assert len(out) == 99
    assert [int(p["kind"]) for p in out[:3]] == [R.RING, R.RING, R.SEG]
    assert (int(out[0]["x0"]), int(out[0]["b"])) == (315, 4) and (int(out[-2]["x0"]), int(out[-1]["x0"]), int(out[-1]["x1"])) == (70, 70, 75)
    assert tuple(out[0]["rgb"]) == R.ramp_color((255, 255, 0), (255, 255, 255), 60, 59) == (5, 5, 255)
    small = R.history_layer(320, 240, [(315.0, 100.0)], [7], {7: uv}, highlighted=[7])
    assert [int(p["kind"]) for p in small[:3]] == [R.BOX, R.RING, R.RING] and int(small[1]["b"]) == 1
    assert (int(small[0]["x0"]), int(small[0]["x1"]), int(small[0]["y0"]), int(small[0]["y1"])) == (312, 318, 97, 103)
    flagged = R.history_layer(320, 240, [(315.0, 100.0)], [7], {7: uv[:3]}, flagged=[7])
    assert [(int(p["kind"]), int(p["b"])) for p in flagged] == [(R.RING, 4), (R.RING, 4), (R.SEG, 0)]
    assert tuple(flagged[0]["rgb"]) == (0, 255, 85) and tuple(flagged[1]["rgb"]) == (0, 255, 170)
    assert R.history_layer(752, 480, [(1.0, 1.0)], [3], {7: uv}) == []


def test_mask_rule():
    assert R.mask_rule([0, 1, 254, 255, 228, 229, 230, 231]).tolist() == [26, 26, 255, 255, 254, 254, 255, 255]
    grey = np.full((2, 2), 9, dtype=np.uint8)
    img = R.render(grey, R.prims_array([R.disc(0, 0, 0, (1, 2, 4))]), mask=np.array([[255, 0], [1, 0]], dtype=np.uint8))
    assert img[0, 0].tolist() == [1, 2, 30] and img[1, 0].tolist() == [9, 9, 34] and img[0, 1].tolist() == [9, 9, 9]


def test_rne_and_truncation():
    assert [R.rne(v) for v in (0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 2.4999, 2.5001)] == [0, 2, 2, 4, 0, -2, -2, 2, 3]
    assert R.rne(2.0 ** 20) == 1 << 20 and R.rne(2.0 ** 20 + 1) is None and R.rne(-2.0 ** 20 - 1) is None
    assert R.rne(float("nan")) is None and R.rne(float("inf")) is None
    assert [R.trunc_half(v) for v in (0.5, 1.5, 2.49, -0.4, -0.6, -1.5, -1.6)] == [1, 2, 2, 0, 0, -1, -1]


def test_nan_observation_drops_its_primitives():
    uv = np.array([[10, 10], [20, 10], [np.nan, 10], [40, 10]], dtype=np.float32)
    out = R.history_layer(752, 480, [(40.0, 10.0)], [1], {1: uv})
    # z = 3: disc; z = 2: disc and segment dropped; z = 1: disc, its segment to z = 2 dropped
    assert [(int(p["kind"]), int(p["x0"])) for p in out] == [(R.RING, 40), (R.RING, 20)]
    assert R.active_layer(752, 480, [(np.inf, 3.0)]) == []


def test_lines_layer():
    pts = np.array([[100.5, 50.5], [200.0, 60.0]], dtype=np.float32)
    lines = np.array([[10.4, 10.6, 90.5, 20.2], [5, 5, 50, 50], [0, 0, 9, 9]], dtype=np.float32)
    out = R.lines_layer(pts, [11, 12], lines, [1, 2, 3], [0, 0, 2, 3], [12, 99, 11], line_db_ids=[2, 3])
    got = [(int(p["kind"]), int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"]), int(p["a"]), int(p["b"]), tuple(int(c) for c in p["rgb"])) for p in out]
    assert got == [(R.SEG, 5, 5, 50, 50, 2, 0, (128, 53, 23)), (R.RING, 200, 60, 0, 0, 49, 81, (128, 53, 23)),
                   (R.SEG, 0, 0, 9, 9, 2, 0, (1, 106, 46)), (R.RING, 100, 50, 0, 0, 49, 81, (1, 106, 46))]
