"""The case matrix of the line detector off its shipped settings (plv_config: line_length_threshold, line_distance_threshold, canny_th1,
canny_th2, line_min_length_px; shipped 20, sqrt 2, 50, 50, 40 — canny_aperture can only be 3).

A case is an image and a set of settings, and what it is there for.  Every image is fed with histogram_method = 0, so that level 0 of
the pyramid is the image as drawn and the references can be formed from the drawing alone.  tests/test_line_setting_cases_cpu.py proves
on the oracle alone that every case still does what it says; tests/test_gpu_line_settings.py holds the device to the oracle on all of
them, through every route of the detector.  Nothing here needs a GPU; the oracle is handed in where a reference is formed.

Sizes: 320 x 240 (half image 160 x 120: ten by seven and a half 16 x 16 tiles of the edge kernel), 333 x 251 (half image 166 x 125: the
last row and column of the full image are unused, partial tiles on both sides) and 98 x 70 (half image 49 x 35, where only short length
thresholds find anything).  They are the smallest at which the tiling, the two cleared corners and the buffers sized by the length
threshold can go wrong; 1280 x 720 is covered at the shipped settings elsewhere.
"""
import numpy as np

import synth
from line_restatement import edge_map, walk_chains
from test_gpu_line_walk_parallel import DRAWINGS as WALK_DRAWINGS

SHIPPED = dict(length=20, dist=1.414213562, c1=50, c2=50, min_len=40.0)
CHAIN_CAP = 4096       # kChainCap (line_host.hpp) and the `cap` of Context.detect_lines


def _s(**kw):
    assert set(kw) <= set(SHIPPED), kw
    return dict(SHIPPED, **kw)


SETTINGS = {
    "shipped": _s(),                                   # the control
    "canny30_90": _s(c1=30, c2=90),                    # hysteresis
    "canny20_200": _s(c1=20, c2=200),                  # hysteresis, wide
    "canny90_30": _s(c1=90, c2=30),                    # swapped: must equal 30 / 90
    "canny120_120": _s(c1=120, c2=120),                # equal but not shipped: the no-hysteresis path still moves
    "canny5000_5000": _s(c1=5000, c2=5000),            # no edge at all
    "canny30_48": _s(c1=30, c2=48),                    # the faint band's gradient is 4 * 12 = 48: AT the high threshold is weak, not strong
    "canny30_320": _s(c1=30, c2=320),                  # the corner drawings: strong only inside a cleared corner
    "len5": _s(length=5),                              # many short chains, small components survive min_px
    "len8": _s(length=8),
    "len60": _s(length=60),                            # drops most chains
    "dist0.5": _s(dist=0.5),                           # breaks chains into many segments
    "dist3": _s(dist=3.0),                             # merges them
    "min0": _s(min_len=0.0),
    "min12": _s(min_len=12.0),
    "min100": _s(min_len=100.0),
    # FastLineDetector itself drops a segment shorter than its length threshold, 20 half-resolution pixels = 40 full-resolution ones at
    # the shipped value: a minimum length below 40 decides something only next to a shorter length threshold (at 5: segments from 10 px)
    "len5_min0": _s(length=5, min_len=0.0),
    "len5_min12": _s(length=5, min_len=12.0),
    "len8_min0": _s(length=8, min_len=0.0),            # the small texture: the shipped settings find nothing there
    "combined": _s(length=7, dist=0.7, c1=25, c2=110, min_len=12.0),   # everything off its default
}
HYSTERESIS = ("canny30_90", "canny20_200", "canny90_30", "combined")   # on the fading bars: something promoted, something left out


# ------------------------------------------------------------------------------------------------ the images
def fading_bars():
    """320 x 240 on a background of 100: a bar whose contrast fades from 130 to 0 along its length (its flanks are strong at one end, weak
    further on — promoted by hysteresis as far as they stay above the low threshold — and nothing at the other), a faint bar (contrast
    12: weak at a low threshold of 30 or less, attached to nothing strong, so hysteresis leaves it out) and a bright stub inside the
    faint bar (strong, a few pixels away from the faint flanks)."""
    img = np.full((240, 320), 100.0)
    fade = np.linspace(130.0, 0.0, 280)
    img[40:80, 20:300] += fade[None, :]
    img[150:200, 30:290] += 12.0
    img[168:182, 140:176] += 110.0
    return np.rint(img).astype(np.uint8)


def faint_band():
    """320 x 240 on a background of 100: a band of contrast 12 from the left border to the right one — no corner, so |gx| + |gy| is
    4 * 12 = 48 on every pixel of its two flanks, exactly a high threshold of 48 — and a bright bar below it"""
    img = np.full((240, 320), 100, dtype=np.uint8)
    img[60:100, :] += 12
    img[150:190, 40:280] = 220
    return img


_CORNER_C = [120, 120, 120, 90, 60, 40, 25, 18] + [14] * 200


def _diagonal(c):
    y, x = np.mgrid[0:120, 0:160]
    half = np.where(x > y, 100 + np.array(c)[np.minimum(x, y)], 100).astype(np.uint8)
    return np.repeat(np.repeat(half, 2, axis=0), 2, axis=1)


def corner_top_left():
    """320 x 240, each pixel of a 160 x 120 drawing doubled: background 100 and 100 + c[min(x, y)] where x > y — a diagonal edge that is
    strong (above a high threshold of 320) only inside FastLineDetector's cleared top-left 6 x 6 corner and weak along the rest"""
    return _diagonal(_CORNER_C)


def corner_bottom_right():
    """the same drawing turned by 180 degrees, its strong part one pixel shorter: strong only inside the cleared bottom-right 5 x 5 corner"""
    return np.ascontiguousarray(_diagonal(_CORNER_C[1:])[::-1, ::-1])


def texture_333x251():
    canvas = synth.texture_canvas(333, 251, seed=21, blobs=60, lines=40)
    return synth.render_frame(canvas, 333, 251)


def texture_98x70():
    canvas = synth.texture_canvas(98, 70, seed=1, blobs=20, lines=6)
    return synth.render_frame(canvas, 98, 70)


IMAGES = {"fading_bars": fading_bars, "faint_band": faint_band, "corner_tl": corner_top_left, "corner_br": corner_bottom_right, "tex333": texture_333x251,
          "tex98": texture_98x70}
IMAGES.update({"walk_" + k: v for k, v in WALK_DRAWINGS.items()})
CORNERS = {"corner_tl": (slice(0, 6), slice(0, 6)), "corner_br": (slice(-5, None), slice(-5, None))}   # (rows, columns) of the half image

_image_cache = {}


def image(name):
    """the image of a case (uint8 [h][w]); drawn once, never written to"""
    if name not in _image_cache:
        img = np.ascontiguousarray(IMAGES[name](), dtype=np.uint8)
        img.setflags(write=False)
        _image_cache[name] = img
    return _image_cache[name]


# ------------------------------------------------------------------------------------------------ the matrix
LENGTH_SETTINGS = ("len5", "len8", "len60")
DIST_SETTINGS = ("dist0.5", "dist3")
MIN_SETTINGS = ("min0", "min12", "min100", "len5_min0", "len5_min12")
MIN_DRAWINGS = ("t_and_cross", "ring_around_bar", "spiral")

CASES = []      # (image, setting)
CASES += [("fading_bars", s) for s in ("shipped", "canny30_90", "canny20_200", "canny90_30", "canny120_120", "canny5000_5000", "len8", "combined")]
CASES += [("faint_band", s) for s in ("canny30_48", "shipped")]
CASES += [(c, s) for c in ("corner_tl", "corner_br") for s in ("canny30_320", "shipped")]
CASES += [("walk_" + d, s) for d in WALK_DRAWINGS for s in LENGTH_SETTINGS + DIST_SETTINGS + ("combined",)]
CASES += [("walk_" + d, s) for d in MIN_DRAWINGS for s in MIN_SETTINGS]
CASES += [("tex333", s) for s in ("shipped", "canny30_90", "canny120_120", "canny5000_5000", "len5", "len60", "dist0.5", "dist3", "min0", "min100", "len5_min12", "combined")]
CASES += [("tex98", s) for s in ("len8_min0", "len5_min0", "len5_min12", "combined")]
CASE_IDS = [f"{i}-{s}" for i, s in CASES]


def oracle_args(setting):
    """the settings as LineOracle.detect_lines / fld take them: (length, dist, c1, c2, min_len)"""
    s = SETTINGS[setting]
    return s["length"], s["dist"], s["c1"], s["c2"], s["min_len"]


def config(pkg, image_name, setting):
    """the plv_config of a case: the image's size, histogram_method 0, the five settings"""
    h, w = image(image_name).shape
    s = SETTINGS[setting]
    cfg = pkg.default_config(w, h)
    cfg.histogram_method = 0
    cfg.line_length_threshold, cfg.line_distance_threshold = s["length"], s["dist"]
    cfg.canny_th1, cfg.canny_th2, cfg.line_min_length_px = s["c1"], s["c2"], s["min_len"]
    return cfg


# ------------------------------------------------------------------------------------------------ the references
_ref_cache = {}


def reference(lo, image_name, setting):
    """What the device is held to on a case, formed once per (image, settings) and shared by the tests (never written to):
    `segs` the oracle's detect_lines on the image as drawn, `edges` the detector's edge map (bool, half resolution) and `chains` the
    restated walk on it.  lo: oracle_lib.load_line()."""
    key = (image_name, setting)
    if key not in _ref_cache:
        length, dist, c1, c2, min_len = oracle_args(setting)
        img = image(image_name)
        segs = lo.detect_lines(img, length, dist, c1, c2, min_len, cap=2 * CHAIN_CAP)
        edges = edge_map(lo, img, c1, c2)
        chains = walk_chains(edges, length)
        segs.setflags(write=False), edges.setflags(write=False)
        for c in chains:
            c.setflags(write=False)
        _ref_cache[key] = dict(segs=segs, edges=edges, chains=chains)
    return _ref_cache[key]
