"""The case matrix of the corner detector (test infrastructure; tests/test_detect_cases_cpu.py states on the oracle alone what each
case must contain, tests/test_gpu_detect_edges.py runs them through Context.perform_detection).

fast_tiles_kernel, fast_topk_kernel and subpix_kernel behind det_pre / det_launch / det_post were held to the oracle on rendered
textures with a few hundred local maxima per cell.  The cases below are the inputs on which those kernels take another branch:

  overflow       uniform noise in cells of 320x240, 376x240, 640x360 and 768x432: 7 000 .. 26 000 local maxima per cell, more than the
                 4096 keys fast_topk_kernel stages in LDS (it used to drop the rest, in the order the atomics arrived)
  near_cap       1280x720 at 5x5 (BASELINE configs[3]): 3 400 .. 3 600 maxima per 256x144 cell, the fullest the staged path gets
  seam_mirror    an image mirrored about x = 31|32 (y = 31|32): equal scores face each other across the 32x32 tile seam and must
                 suppress each other; with the grid line on the axis both columns lie in the cells' dead border
  all_ties       a lattice of single bright pixels: > 1 000 keys of score 254, the top-k is decided by raster order alone; the large
                 lattice has > 4096 of them (the selection over the stored list resolves a mass tie)
  few / none     fewer keys than slots per cell, no key at all, one textured cell among flat ones
  thresholds     fast_threshold 1 and 254; pixels exactly at the threshold and one grey level above it
  cell_sizes     cells of 7 pixels (one admissible pixel), of 6 (nothing runs), of 33 (one pixel into the second tile), with a remainder
  boxes          > 300 existing points: winners at exactly min_px_dist and min_px_dist + 1 from one, in x and in y, behind the
                 256th painted box; a point too near the border to paint a box; mask values 127 / 128; a point either side of a
                 grid line
  subpix_exits   detections within 6 pixels of every image border, refinements that end in each of subpix_kernel's exits
  cap_cut        the caller's capacity ends the list a few entries early

Every case uses histogram_method = PLV_HIST_NONE: the detector sees the image as given and the oracle gets the same array.
Everything here runs on numpy and the CPU oracle; no case needs a device to be built.

subpix_exits: on its 96x72 image the oracle reaches the window clamp at all four borders, the convergence test, the iteration limit,
the revert (moved more than the half-window) and the left-the-image break, the last both with and without the revert behind it (a
wedge whose edges meet three pixels outside the left border pulls the detection at x = 3 to x < 0 in one step).  The `det` break is not
reached from a FAST detection on any image tried (noise, sparse dots, noise islands on black, edges that converge on a flat region; 32x40
.. 128x96): it needs a 13x13 window without any gradient product, |det| <= 4.9e-32, and a FAST corner always has gradient in both
directions next to it, while a refinement step that jumps clear of all structure did not occur.  subpix_trace reaches it on a flat
window; test_detect_cases_cpu.test_subpix_exits states the exits the committed image reaches and fails if that set shrinks."""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib

LDS_KEYS = 4096          # keys fast_topk_kernel stages in LDS (written out: the tests do not read it from the library)
PLV_HIST_NONE = 0

Case = namedtuple("Case", "name img num_features grid_x grid_y min_px_dist fast_threshold pts ids currid mask cap")

_NO_PTS = np.zeros((0, 2), np.float32)
_NO_IDS = np.zeros(0, np.uint64)


def _case(name, img, nf, gx, gy, mpd=10, thr=20, pts=_NO_PTS, ids=_NO_IDS, currid=0, mask=None, cap=None):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return Case(name, img, nf, gx, gy, mpd, thr, np.asarray(pts, np.float32).reshape(-1, 2), np.asarray(ids, np.uint64), currid, mask, cap)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def lattice(w, h, off, step=4):
    img = np.zeros((h, w), np.uint8)
    img[off::step, off::step] = 255
    return img


# ------------------------------------------------------------------------------------------------ the oracle's view of a case
def extraction_grid(case):
    """Grider_GRID.h:88-98: (gx, gy, cell_w, cell_h, nfg) of the grid the corners are extracted on"""
    h, w = case.img.shape
    gx, gy = case.grid_x, case.grid_y
    if case.num_features < gx * gy:
        ratio = gx / gy
        gy = int(np.ceil(np.sqrt(case.num_features / ratio)))
        gx = int(np.ceil(gy * ratio))
    return gx, gy, w // gx, h // gy, int(case.num_features / (gx * gy)) + 1


def cell_bound(cw, ch):
    """most local maxima a cell can hold: a 3-pixel border is skipped, strict 3x3 suppression leaves one per 2x2 block"""
    return 0 if cw < 7 or ch < 7 else ((cw - 5) // 2) * ((ch - 5) // 2)


def cell_keypoints(case, x, y):
    """fast_roi of grid cell (x, y): positions in cell coordinates (raster order) and scores"""
    _, _, cw, ch, _ = extraction_grid(case)
    return oracle_lib.load_detect().fast_roi(case.img, x * cw, y * ch, cw, ch, case.fast_threshold, cap=cell_bound(cw, ch) + 1)


def cell_winners(case, x, y):
    """the first nfg of the cell's keypoints by score, ties in raster order: integer image positions and scores, in output order"""
    _, _, cw, ch, nfg = extraction_grid(case)
    xy, r = cell_keypoints(case, x, y)
    order = np.argsort(-r, kind="stable")[:nfg]
    return (xy[order] + np.array([x * cw, y * ch], np.float32)).astype(np.int64), r[order]


def run_oracle(case, pts=None, ids=None, mask="case", cap="case"):
    do = oracle_lib.load_detect()
    pts = case.pts if pts is None else np.asarray(pts, np.float32).reshape(-1, 2)
    ids = case.ids if ids is None else np.asarray(ids, np.uint64)
    return do.perform_detection(case.img, case.mask if isinstance(mask, str) else mask, pts, ids, case.currid, case.num_features, case.grid_x,
                                case.grid_y, case.min_px_dist, case.fast_threshold, cap=case.cap if isinstance(cap, str) else cap)


def refined(case, xy_int):
    """where the oracle's sub-pixel refinement leaves integer positions"""
    return oracle_lib.load_detect().corner_subpix(case.img, np.asarray(xy_int, np.float32).reshape(-1, 2))


def contains(result_pts, p):
    return bool(((result_pts[:, 0] == np.float32(p[0])) & (result_pts[:, 1] == np.float32(p[1]))).any())


# ------------------------------------------------------------------------------------------------ cornerSubPix, exit by exit
@functools.lru_cache(maxsize=None)
def _subpix_window(win):
    """the window weights as the oracle and the library compute them: float exp(-y * y) times float exp(-x * x), the C library's expf"""
    import ctypes
    import ctypes.util
    expf = ctypes.CDLL(ctypes.util.find_library("m")).expf
    expf.argtypes, expf.restype = [ctypes.c_float], ctypes.c_float
    t = np.arange(-win, win + 1, dtype=np.float32) / np.float32(win)
    v = np.array([expf(float(-(u * u))) for u in t], dtype=np.float32)
    return np.outer(v, v).astype(np.float32)


def subpix_trace(img, x, y, win=5, max_iters=20, eps=0.001):
    """cv::cornerSubPix for one point as the oracle states it (float32 samples, double sums in raster order), with the way it ended:
    (x, y, exit, clamped) where exit is one of "det", "left", "iters", "eps", reverted is appended as "+revert", and clamped says
    whether a sample was ever taken from outside the image (replicated border).  test_detect_cases_cpu holds its positions to
    orc_corner_subpix bit for bit, so the exit it names is the oracle's."""
    import math
    f32 = np.float32
    img = np.asarray(img)
    h, w = img.shape
    ww, sw = 2 * win + 1, 2 * win + 3
    mask = _subpix_window(win)
    cTx, cTy = f32(x), f32(y)
    cIx, cIy = cTx, cTy
    eps2 = eps * eps
    it, err, clamped, ended = 0, 0.0, False, None
    pxx = np.tile(np.arange(ww, dtype=np.float64) - win, (ww, 1))
    pyy = pxx.T
    while True:
        cx, cy = f32(cIx - f32((sw - 1) * 0.5)), f32(cIy - f32((sw - 1) * 0.5))
        ix, iy = int(math.floor(cx)), int(math.floor(cy))
        a, b = f32(cx - f32(ix)), f32(cy - f32(iy))
        a11, a12, a21, a22 = f32(f32(1 - a) * f32(1 - b)), f32(a * f32(1 - b)), f32(f32(1 - a) * b), f32(a * b)
        xs, ys = np.arange(ix, ix + sw + 1), np.arange(iy, iy + sw + 1)
        clamped |= bool(xs[0] < 0 or xs[-1] > w - 1 or ys[0] < 0 or ys[-1] > h - 1)
        patch = img[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)].astype(np.float32)
        sub = ((patch[:-1, :-1] * a11 + patch[:-1, 1:] * a12) + patch[1:, :-1] * a21) + patch[1:, 1:] * a22
        tgx = sub[1:-1, 2:] - sub[1:-1, :-2]
        tgy = sub[2:, 1:-1] - sub[:-2, 1:-1]
        gxx = ((tgx * tgx) * mask).astype(np.float64)
        gxy = ((tgx * tgy) * mask).astype(np.float64)
        gyy = ((tgy * tgy) * mask).astype(np.float64)
        seq = lambda t: float(np.cumsum(t.ravel())[-1])        # added up in raster order, one at a time
        A, B, Cc = seq(gxx), seq(gxy), seq(gyy)
        bb1, bb2 = seq(gxx * pxx + gxy * pyy), seq(gxy * pxx + gyy * pyy)
        det = A * Cc - B * B
        if abs(det) <= 2.220446049250313e-16 ** 2:
            ended = "det"
            break
        scale = 1.0 / det
        nx = f32(float(cIx) + Cc * scale * bb1 - B * scale * bb2)
        ny = f32(float(cIy) - B * scale * bb1 + A * scale * bb2)
        err = float(f32(nx - cIx)) ** 2 + float(f32(ny - cIy)) ** 2
        cIx, cIy = nx, ny
        if cIx < 0 or cIx >= w or cIy < 0 or cIy >= h:
            ended = "left"
            break
        it += 1
        if not it < max_iters:
            ended = "iters"
            break
        if not err > eps2:
            ended = "eps"
            break
    if abs(f32(cIx - cTx)) > win or abs(f32(cIy - cTy)) > win:
        cIx, cIy, ended = cTx, cTy, ended + "+revert"
    return float(cIx), float(cIy), ended, clamped


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def overflow(which):
    w, h, g, seed = {"320x240-1x1": (320, 240, 1, 0), "752x480-2x2": (752, 480, 2, 1), "640x360-1x1": (640, 360, 1, 2),
                     "768x432-1x1": (768, 432, 1, 3)}[which]
    return _case("overflow-" + which, noise(w, h, seed), 100, g, g)


OVERFLOW = ("320x240-1x1", "752x480-2x2", "640x360-1x1", "768x432-1x1")


@functools.lru_cache(maxsize=None)
def near_cap():
    return _case("near_cap", noise(1280, 720, 1), 500, 5, 5)


def mirrored(seed=3, n=96):
    left = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([left, left[:, ::-1]], axis=1))


@functools.lru_cache(maxsize=None)
def seam_mirror(which):
    """64 wide, the right half the mirror image of the left (columns 31 | 32 carry equal scores); `t`: transposed, rows 31 | 32;
    `split`: the grid line falls on the mirror axis"""
    img = mirrored()
    gx, gy = (2, 1) if "split" in which else (1, 1)
    if which.startswith("t"):
        img, gx, gy = np.ascontiguousarray(img.T), gy, gx
    return _case("seam_mirror-" + which, img, 40, gx, gy, mpd=3)


SEAM = ("x", "x-split", "t", "t-split")


@functools.lru_cache(maxsize=None)
def all_ties(off):
    if off == "big":
        return _case("all_ties-big", lattice(320, 264, 3), 60, 1, 1, mpd=4)
    return _case(f"all_ties-{off}", lattice(160, 120, off), 60, 1, 1, mpd=4)


TIES = (0, 1, 2, 3, "big")


def _dots(w, h, at):
    img = np.zeros((h, w), np.uint8)
    for x, y in at:
        img[y, x] = 255
    return img


@functools.lru_cache(maxsize=None)
def few(which):
    if which == "dots":          # five keys, 61 slots
        return _case("few-dots", _dots(120, 90, [(3, 3), (40, 20), (41, 60), (100, 86), (116, 45)]), 60, 1, 1)
    if which == "dots-2x2":      # cells with 3, 0, 1 and 2 keys, 16 slots each
        return _case("few-dots-2x2", _dots(120, 90, [(10, 10), (30, 30), (50, 12), (20, 70), (70, 50), (110, 80)]), 60, 2, 2)
    if which == "none":          # a constant image: the input points come back, the id counter stays
        pts = np.array([[20.5, 30.25], [60.0, 40.0], [61.0, 41.0], [100.0, 70.0], [4.0, 50.0]], np.float32)
        return _case("none", np.full((90, 120), 128, np.uint8), 60, 2, 2, pts=pts, ids=np.arange(7, 12), currid=11)
    if which == "one-textured":  # one textured cell among flat ones
        img = np.full((100, 150), 90, np.uint8)
        img[0:50, 50:100] = noise(50, 50, 5)
        return _case("one-textured", img, 60, 3, 2)
    raise KeyError(which)


FEW = ("dots", "dots-2x2", "none", "one-textured")


@functools.lru_cache(maxsize=None)
def thresholds(which):
    if which == "thr1":
        return _case("thr1", noise(100, 80, 6), 60, 2, 2, thr=1)
    if which == "equal":
        # pixels exactly `threshold` above their circle are no corners (the test is `>`), one grey level more makes one.  The four
        # compass pixels of each circle are darker still, so that the cheap pre-test of fast_tiles_kernel lets both kinds through
        # and the full score decides.
        img = np.full((90, 120), 100, np.uint8)
        for i, (x, y) in enumerate(EQUAL_DOTS):
            img[y, x] = 120 + (i % 2)
            for dx, dy in ((0, 3), (0, -3), (3, 0), (-3, 0)):
                img[y + dy, x + dx] = 90
        return _case("thr-equal", img, 60, 1, 1)
    return _case("thr254-lattice", lattice(160, 120, 1), 60, 1, 1, mpd=4, thr=254)


EQUAL_DOTS = ((20, 20), (50, 20), (80, 20), (103, 20), (20, 60), (50, 60), (80, 60), (110, 60))   # even: equal to, odd: one above
THRESHOLDS = ("thr1", "thr254", "equal")


@functools.lru_cache(maxsize=None)
def cell_sizes(which):
    w, h, gx, gy, nf = {"7px": (105, 70, 15, 10, 300), "6px": (90, 60, 15, 10, 300), "33px": (165, 99, 5, 3, 150),
                        "remainder": (100, 75, 3, 2, 60)}[which]
    return _case("cells-" + which, noise(w, h, 7), nf, gx, gy, mpd=3)


CELL_SIZES = ("7px", "6px", "33px", "remainder")


# ---- boxes: existing points against the winners of an empty start
BoxesCase = namedtuple("BoxesCase", "case base at_dist_x at_dist_y past_dist_x past_dist_y border mask127 mask128 first_special")


@functools.lru_cache(maxsize=None)
def boxes():
    """752x480 noise at 5x5, min_px_dist 12 (above the 10-pixel edge rule, so that a kept point can be too near the border to paint its
    box).  `base` is the same case from an empty start; the named winners are integer positions (x, y) of `base`'s per-cell winners:
      at_dist_x / at_dist_y     an existing point sits exactly min_px_dist from them in x / in y: inside its box, dropped
      past_dist_x / past_dist_y an existing point sits min_px_dist + 1 away: outside, kept
      border                    a winner within min_px_dist of an existing point at x = 11, which paints no box: kept
      mask127 / mask128         the mask holds 127 / 128 under them: kept / dropped
    The special points come last, behind 340 random ones: their boxes lie past the 256th (first_special counts the boxes before)."""
    w, h, mpd = 752, 480, 12
    img = noise(w, h, 11)
    base = _case("boxes-base", img, 1000, 5, 5, mpd=mpd)
    res0 = run_oracle(base)[0]
    rng = np.random.default_rng(12)
    rnd = np.column_stack([rng.uniform(0, w, 340), rng.uniform(0, h, 340)]).astype(np.float32)
    rnd[:3] = [[4.0, 4.0], [w - 3.0, 50.0], [100.0, h - 2.0]]   # edge points are dropped
    occupied = {(int(p[0] / np.float32(mpd)), int(p[1] / np.float32(mpd))) for p in rnd}
    taken = []

    def pick(ok):
        """a winner of `base` that survives to its result, far from every random point and from the winners picked before"""
        for cx in range(5):
            for cy in range(5):
                wxy, _ = cell_winners(base, cx, cy)
                ref = refined(base, wxy)
                for (x, y), r in zip(wxy, ref):
                    if not contains(res0, r) or not ok(x, y):
                        continue
                    if np.abs(rnd - [x, y]).max(axis=1).min() <= 2 * mpd or any(max(abs(x - a), abs(y - b)) <= 4 * mpd for a, b in taken):
                        continue
                    cells = {(int(r[0] / np.float32(mpd)) + i, int(r[1] / np.float32(mpd)) + j) for i in (-1, 0, 1) for j in (-1, 0, 1)}
                    if cells & occupied:
                        continue
                    taken.append((x, y))
                    return int(x), int(y)
        raise AssertionError("no winner fits")

    inner = lambda x, y: 40 <= x < w - 40 and 40 <= y < h - 40
    ax, ay, px, py = pick(inner), pick(inner), pick(inner), pick(inner)
    m127, m128 = pick(inner), pick(inner)
    # the border winner: an existing point at x = 11 keeps (11 >= the 10-pixel edge) and paints no box (11 - 12 < 0)
    taken_before = list(taken)
    bord = None
    for cy in range(5):
        wxy, _ = cell_winners(base, 0, cy)
        for (x, y), r in zip(wxy, refined(base, wxy)):
            if 13 <= x <= 22 and 30 <= y < h - 30 and contains(res0, r) and int(r[0] / np.float32(mpd)) == 1 and \
                    np.abs(rnd - [x, y]).max(axis=1).min() > 2 * mpd and all(max(abs(x - a), abs(y - b)) > 4 * mpd for a, b in taken_before):
                bord = (int(x), int(y))
                break
        if bord:
            break
    assert bord is not None
    special = np.array([[ax[0] + mpd + 0.5, ax[1] + 0.25], [ay[0] + 0.75, ay[1] - mpd + 0.5],
                        [px[0] - (mpd + 1) + 0.5, px[1] + 0.5], [py[0] + 0.25, py[1] + mpd + 1 + 0.75],
                        [11.5, bord[1] + 0.5]], np.float32)
    pts = np.concatenate([rnd, special])
    mask = np.zeros((h, w), np.uint8)
    mask[m127[1], m127[0]] = 127
    mask[m128[1], m128[0]] = 128
    case = _case("boxes", img, 1000, 5, 5, mpd=mpd, pts=pts, ids=np.arange(100, 100 + len(pts)), currid=2000, mask=mask)
    return BoxesCase(case, base, ax, ay, px, py, bord, m127, m128, len(rnd))


@functools.lru_cache(maxsize=None)
def grid_line(side):
    """one existing point at x = 150.39 / 150.41: either side of the grid line 752 / 5 = 150.4.  With 50 features on 5x5 a cell that
    holds one point asks for none, so the point decides whether cell (0, 0) or cell (1, 0) is extracted from."""
    x = {"left": 150.39, "right": 150.41}[side]
    return _case("grid_line-" + side, noise(752, 480, 13), 50, 5, 5, pts=np.array([[x, 48.0]], np.float32), ids=np.array([5]), currid=5)


def wedge(w, h, apex_x, y0, slope, x_end, ss=8):
    """an anti-aliased bright wedge on black: |y - y0| <= slope * (x - apex_x) up to x_end.  The refinement of a corner on its edges
    solves for the point the two edges meet in: the apex, wherever it lies"""
    ys, xs = np.mgrid[0:h * ss, 0:w * ss]
    x, y = (xs + 0.5) / ss - 0.5, (ys + 0.5) / ss - 0.5
    inside = (np.abs(y - y0) <= slope * (x - apex_x)) & (x <= x_end)
    return np.clip(np.rint((inside * 255.0).reshape(h, ss, w, ss).mean(axis=(1, 3))), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def subpix_exits():
    """bright single pixels and 3x3 blobs on black, 3 .. 5 pixels from each border and in the corners (the refinement window of 13x13
    samples reaches over the border: replicated), a patch of noise (refinements that wander: revert, iteration limit) and a wedge
    whose apex lies outside the left border, with a faint pixel beside it (refinements that leave the image)"""
    w, h = 96, 72
    img = wedge(w, h, -3, 36, 0.15, 20)
    img[39, 4] = 40
    img[20:52, 40:76] = noise(36, 32, 17)
    for x, y in [(3, 10), (5, 60), (w - 4, 12), (w - 5, 40), (w - 6, 62), (12, 3), (50, 4), (80, 5), (14, h - 4), (48, h - 5),
                 (78, h - 6), (3, 3), (w - 4, h - 4)]:
        img[y, x] = 255
    img[60:63, 20:23] = 200
    img[8:11, 60:63] = 180
    return _case("subpix_exits", img, 200, 1, 1, mpd=3)


@functools.lru_cache(maxsize=None)
def cap_cut():
    """the caller's buffers end four entries before the list the oracle returns uncapped"""
    base = _case("cap_cut-base", noise(200, 150, 19), 120, 2, 2, pts=np.array([[50.0, 50.0], [120.5, 80.5]], np.float32), ids=np.array([3, 4]),
                 currid=9)
    n = len(run_oracle(base)[0])
    return base, base._replace(name="cap_cut", cap=n - 4)


def gpu_cases():
    """every case the device runs, by name"""
    out = [overflow(k) for k in OVERFLOW] + [near_cap()] + [seam_mirror(k) for k in SEAM] + [all_ties(k) for k in TIES]
    out += [few(k) for k in FEW] + [thresholds(k) for k in THRESHOLDS] + [cell_sizes(k) for k in CELL_SIZES]
    out += [boxes().case, boxes().base, grid_line("left"), grid_line("right"), subpix_exits(), cap_cut()[1]]
    assert len({c.name for c in out}) == len(out)
    return out
