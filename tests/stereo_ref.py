"""TrackKLT::feed_stereo and perform_detection_stereo restated in Python on the CPU oracle's primitives
(REF: open_vins/ov_core/src/track/TrackKLT.cpp:202-393, 530-827; Grider_GRID::perform_griding, Grider_GRID.h:74-180).

The right camera's stage cannot be composed from DetectOracle.perform_detection: its pruning spares a point whose id the left list
holds (`grid_2d_close1 > 127 && !is_stereo`, :754-759) and its corners are tested against a mask cloned from mask0 (:721) while its
points and grid cells are tested against mask1.  So the grid extraction is restated here from fast_roi + corner_subpix, and
test_stereo_ref_cpu.py holds that restatement, run as a monocular detection, to perform_detection itself.

`stats` counts what a stream exercised (the CPU test asserts that the GPU test's streams reach every branch)."""
import functools
import math
from collections import Counter

import numpy as np

import cam_equi
import oracle_lib
import synth

F32 = np.float32


class Settings:
    """the tracker settings the restatement reads (the names of plv_config)"""

    def __init__(self, num_features, grid_x, grid_y, min_px_dist, fast_threshold=20):
        self.num_features, self.grid_x, self.grid_y = num_features, grid_x, grid_y
        self.min_px_dist, self.fast_threshold = min_px_dist, fast_threshold


def points_array(a):
    return np.asarray(a, dtype=F32).reshape(-1, 2)


def ids_array(a):
    return np.asarray(a, dtype=np.uint64).reshape(-1)


class Detection:
    """the pruning loop and the grid top-up that perform_detection_monocular and both halves of perform_detection_stereo share"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.do = oracle_lib.load_detect()

    def prune(self, w, h, mask, pts, ids, spared=None):
        """:411-464 / :547-600 / :724-780 -> kept indices, close grid, cell counts, the kept points' boxes (top_up paints them on
        its mask), number of points kept only because their id is in `spared`"""
        c = self.cfg
        mpd = c.min_px_dist
        cw, ch = int(F32(w) / F32(mpd)), int(F32(h) / F32(mpd))
        close = np.zeros((ch, cw), np.uint8)
        grid = np.zeros((c.grid_y, c.grid_x), np.uint8)
        size_x, size_y = F32(w) / F32(c.grid_x), F32(h) / F32(c.grid_y)
        keep, boxes, by_exception = [], [], 0
        for i in range(len(ids)):
            fx, fy = F32(pts[i, 0]), F32(pts[i, 1])
            x, y = int(fx), int(fy)
            if x < 10 or x >= w - 10 or y < 10 or y >= h - 10:
                continue
            xc, yc = int(fx / F32(mpd)), int(fy / F32(mpd))
            if xc < 0 or xc >= cw or yc < 0 or yc >= ch:
                continue
            xg, yg = int(math.floor(fx / size_x)), int(math.floor(fy / size_y))
            if xg < 0 or xg >= c.grid_x or yg < 0 or yg >= c.grid_y:
                continue
            if close[yc, xc] > 127:
                if spared is None or int(ids[i]) not in spared:
                    continue
                if mask is None or mask[y, x] <= 127:
                    by_exception += 1
            if mask is not None and mask[y, x] > 127:
                continue
            close[yc, xc] = 255
            if grid[yg, xg] < 255:
                grid[yg, xg] += 1
            if x - mpd >= 0 and x + mpd < w and y - mpd >= 0 and y + mpd < h:
                boxes.append((x, y))
            keep.append(i)
        return keep, close, grid, boxes, by_exception

    def valid_cells(self, w, h, grid, mask):
        """:478-492: cells short of features whose nearest-neighbour sample of the mask is not 255, x outer, y inner"""
        c = self.cfg
        nfg_req = max(1, int(0.5 * (int(c.num_features / (c.grid_x * c.grid_y)) + 1)))
        out = []
        for x in range(c.grid_x):
            for y in range(c.grid_y):
                sx, sy = min(int(math.floor(x * w / c.grid_x)), w - 1), min(int(math.floor(y * h / c.grid_y)), h - 1)
                if int(grid[y, x]) < nfg_req and (mask is None or int(mask[sy, sx]) != 255):
                    out.append((x, y))
        return out

    def griding(self, img, mask_updated, valid):
        """Grider_GRID::perform_griding: per valid cell the nfg strongest FAST corners (ties in raster order), those on
        mask_updated > 127 dropped, then cornerSubPix of all of them"""
        c = self.cfg
        h, w = img.shape
        if not valid:
            return points_array([])
        gx, gy = c.grid_x, c.grid_y
        if c.num_features < gx * gy:
            ratio = gx / gy
            gy = int(math.ceil(math.sqrt(c.num_features / ratio)))
            gx = int(math.ceil(gy * ratio))
        nfg = int(c.num_features / (gx * gy)) + 1
        sxp, syp = w // gx, h // gy
        ext = []
        for cx, cy in valid:
            x, y = cx * sxp, cy * syp
            if x + sxp > w or y + syp > h:
                continue
            xy, resp = self.do.fast_roi(img, x, y, sxp, syp, c.fast_threshold)
            for k in np.argsort(-resp, kind="stable")[:nfg]:
                px, py = F32(xy[k, 0]) + F32(x), F32(xy[k, 1]) + F32(y)
                if int(px) < 0 or int(px) > w or int(py) < 0 or int(py) > h:
                    continue
                if mask_updated[int(py), int(px)] > 127:
                    continue
                ext.append((px, py))
        if not ext:
            return points_array([])
        return self.do.corner_subpix(img, points_array(ext))

    def top_up(self, img, mask_cells, mask_corners, close, grid, boxes):
        """the extraction and the rejection near existing points (:478-512 / :617-650 / :793-825): accepted corners in order;
        mask_cells: the mask the grid cells are sampled from, mask_corners: the one the boxes are painted on"""
        h, w = img.shape
        mpd = self.cfg.min_px_dist
        upd = np.zeros((h, w), np.uint8) if mask_corners is None else np.array(mask_corners, dtype=np.uint8)
        for x, y in boxes:
            upd[y - mpd:y + mpd + 1, x - mpd:x + mpd + 1] = 255
        ext = self.griding(img, upd, self.valid_cells(w, h, grid, mask_cells))
        ch, cw = close.shape
        out = []
        for px, py in ext:
            xg, yg = int(F32(px) / F32(mpd)), int(F32(py) / F32(mpd))
            if xg < 0 or xg >= cw or yg < 0 or yg >= ch:
                continue
            if close[yg, xg] > 127:
                continue
            close[yg, xg] = 255
            out.append((px, py))
        return points_array(out)

    def least(self):
        return min(20, int(0.5 * self.cfg.num_features))

    def monocular(self, img, mask, pts, ids, currid):
        """perform_detection_monocular (:395-528), for the comparison with DetectOracle.perform_detection"""
        h, w = img.shape
        pts, ids = points_array(pts), ids_array(ids)
        keep, close, grid, boxes, _ = self.prune(w, h, mask, pts, ids)
        pts, ids = pts[keep], ids[keep]
        if self.cfg.num_features - len(ids) < self.least():
            return pts, ids, currid
        new = self.top_up(img, mask, mask, close, grid, boxes)
        new_ids = np.arange(currid + 1, currid + 1 + len(new), dtype=np.uint64)
        return np.vstack([pts, new]), np.concatenate([ids, new_ids]), currid + len(new)


MODELS = ("radtan", "equidistant")  # (the values of PLV_CAM_*)


class StereoRef:
    """models: the camera model of each camera; undistort(cam, uv) -> normalised float32 points: by default the CPU oracle's radtan
    undistortion or cam_equi.undistort on the camera's present K8 (the device's is held to 1 ulp of the latter, so a test may hand in
    the device's own).  jitter: a numpy Generator that moves every normalised coordinate by -1, 0 or +1 ulp before RANSAC reads it
    (test_stereo_ref_cpu.py: a run none of whose decisions hangs on the last bit gives the same lists with it)."""

    def __init__(self, cfg, K8_left, K8_right, models=("radtan", "radtan"), undistort=None, jitter=None):
        self.cfg, self.K8 = cfg, [np.array(K8_left, dtype=np.float64), np.array(K8_right, dtype=np.float64)]
        assert all(m in MODELS for m in models)
        self.models, self.undistort, self.jitter = tuple(models), undistort or self.model_undistort, jitter
        self.matchings = []  # per matching that ran: (feed, camera, points handed to RANSAC, its inliers, points kept)
        self.fo = oracle_lib.load_front()
        self.det = Detection(cfg)
        self.pts = [points_array([]), points_array([])]
        self.ids = [ids_array([]), ids_array([])]
        self.currid = 0
        self.prev = None  # ((eq, pyramid, mask) left, (...) right) of the last pair
        self.db = {}      # id -> ([(t, u, v, un, vn) ...] camera 0, [...] camera 1)
        self.stats = Counter()
        self.frames = []  # per feed: the set of things that happened in it

    # ---- perform_detection_stereo
    def detect(self, left, right, pts0, ids0, pts1, ids1, events):
        (eq0, pyr0, mask0), (eq1, pyr1, mask1) = left, right
        h, w = eq0.shape
        nf = self.cfg.num_features
        pts0, ids0, pts1, ids1 = points_array(pts0), ids_array(ids0), points_array(pts1), ids_array(ids1)
        keep, close, grid, boxes, _ = self.det.prune(w, h, mask0, pts0, ids0)
        pts0, ids0 = pts0[keep], ids0[keep]
        if nf - len(ids0) > self.det.least():  # :609
            events.add("left top-up")
            new = self.det.top_up(eq0, mask0, mask0, close, grid, boxes)
            if len(new):
                tracked, status, _ = self.fo.lk_track(pyr0, pyr1, new, new)  # :671, no undistortion, no RANSAC
                add0, id0, add1, id1 = [], [], [], []
                for i in range(len(new)):
                    oob = lambda p: int(p[0]) < 0 or int(p[0]) >= w or int(p[1]) < 0 or int(p[1]) >= h
                    if oob(new[i]):
                        continue
                    self.currid += 1
                    add0.append(new[i]), id0.append(self.currid)
                    if not oob(tracked[i]) and status[i] == 1:
                        add1.append(tracked[i]), id1.append(self.currid)
                        self.stats["new stereo features"] += 1
                    else:
                        self.stats["new left-only features"] += 1
                pts0, ids0 = np.vstack([pts0, points_array(add0)]), np.concatenate([ids0, ids_array(id0)])
                pts1, ids1 = np.vstack([pts1, points_array(add1)]), np.concatenate([ids1, ids_array(id1)])
        keep, close, grid, boxes, spared = self.det.prune(w, h, mask1, pts1, ids1, spared={int(i) for i in ids0})  # :724-780
        self.stats["right points kept by the is_stereo exception"] += spared
        pts1, ids1 = pts1[keep], ids1[keep]
        if nf - len(ids1) > self.det.least():  # :785
            events.add("right top-up")
            new = self.det.top_up(eq1, mask1, mask0, close, grid, boxes)  # (:721: boxes painted on a clone of mask0)
            if mask1 is not None:
                self.stats["right corners under mask_right"] += sum(1 for p in new if mask1[int(p[1]), int(p[0])] > 127)
            self.stats["new right-only features"] += len(new)
            new_ids = np.arange(self.currid + 1, self.currid + 1 + len(new), dtype=np.uint64)
            self.currid += len(new)
            pts1, ids1 = np.vstack([pts1, new]), np.concatenate([ids1, new_ids])
        return pts0, ids0, pts1, ids1

    def model_undistort(self, cam, uv):
        if self.models[cam] == "equidistant":
            return cam_equi.undistort(self.K8[cam], uv)
        return self.fo.undistort(self.K8[cam], uv)

    def _normalised(self, cam, uv):
        un = np.ascontiguousarray(self.undistort(cam, uv), dtype=F32).reshape(-1, 2)
        if self.jitter is not None:
            step = self.jitter.integers(-1, 2, un.shape)
            un = np.where(step == 0, un, np.nextafter(un, np.where(step > 0, F32(np.inf), F32(-np.inf)).astype(F32))).astype(F32)
        return un

    # ---- perform_matching of one camera (:829-886), composed as the oracle's orc_perform_matching is: LK with the old positions as
    # the initial flow, the camera's undistortion of both lists, RANSAC at 2 px over max(fx, fy), mask = status & inlier
    def match(self, cam, prev_pyr, pyr, pts_old):
        n = len(pts_old)
        if n == 0:
            return pts_old, None, None
        if n < 10:
            return pts_old.copy(), np.zeros(n, np.uint8), None
        pts_new, status, _ = self.fo.lk_track(prev_pyr, pyr, pts_old, pts_old)
        n0, n1 = self._normalised(cam, pts_old), self._normalised(cam, pts_new)
        inlier, _, _ = self.fo.ransac(n0, n1, 2.0 / max(self.K8[cam][0], self.K8[cam][1]))
        mask = ((status != 0) & (inlier != 0)).astype(np.uint8)
        self.matchings.append((len(self.frames) - 1, cam, n, int((inlier != 0).sum()), int(mask.sum())))
        return pts_new, mask, n1

    def match_oracle(self, cam, prev_pyr, pyr, pts_old):
        """the same through FrontOracle.perform_matching (radtan only): what the composition is held to"""
        n = len(pts_old)
        if n == 0:
            return pts_old, None, None
        if n < 10:
            return pts_old.copy(), np.zeros(n, np.uint8), None
        rc, pts_new, mask, n0, n1 = self.fo.perform_matching(prev_pyr, pyr, pts_old, pts_old, self.K8[cam])
        return pts_new, mask, n1

    # ---- feed_new_camera with two images + feed_stereo
    def feed(self, t, img_left, img_right, mask_left=None, mask_right=None):
        events = set()
        self.frames.append(events)
        cur = []
        for img, mask in ((img_left, mask_left), (img_right, mask_right)):
            eq = self.fo.equalize_hist(img)
            cur.append((eq, self.fo.pyramid(eq), None if mask is None else np.asarray(mask, dtype=np.uint8)))
        h, w = img_left.shape
        if len(self.ids[0]) == 0 and len(self.ids[1]) == 0:  # :221-240
            events.add("detection on the current pair")
            p0, i0, p1, i1 = self.detect(cur[0], cur[1], self.pts[0], self.ids[0], self.pts[1], self.ids[1], events)
            self.pts, self.ids, self.prev = [p0, p1], [i0, i1], cur
            return
        p0, i0, p1, i1 = self.detect(self.prev[0], self.prev[1], self.pts[0], self.ids[0], self.pts[1], self.ids[1], events)
        if not events:
            events.add("no top-up")
        n0, m0, un0 = self.match(0, self.prev[0][1], cur[0][1], p0)
        n1, m1, un1 = self.match(1, self.prev[1][1], cur[1][1], p1)
        if 0 < len(p0) < 10 or 0 < len(p1) < 10:
            events.add("fewer than 10 points")
        if m0 is None and m1 is None:  # :285-299
            events.add("reset")
            self.pts, self.ids, self.prev = [points_array([]), points_array([])], [ids_array([]), ids_array([])], cur
            return
        good = ([], [])   # (point, id, normalised point) per camera
        right_index = {}
        for k in range(len(i1)):
            right_index.setdefault(int(i1[k]), k)
        for i in range(len(i0)):  # :306-338
            x, y = n0[i]
            if x < 0 or y < 0 or int(x) > w or int(y) > h:
                continue
            k = right_index.get(int(i0[i]))
            if m0[i] and k is not None and m1[k]:
                xr, yr = n1[k]
                if xr < 0 or yr < 0 or int(xr) >= w or int(yr) >= h:
                    continue
                good[0].append((n0[i], i0[i], un0[i]))
                good[1].append((n1[k], i1[k], un1[k]))
                self.stats["stereo tracks"] += 1
            elif m0[i]:
                good[0].append((n0[i], i0[i], un0[i]))
                self.stats["left-only tracks"] += 1
        added = {int(g[1]) for g in good[1]}
        for i in range(len(i1)):  # :341-354
            x, y = n1[i]
            if x < 0 or y < 0 or int(x) >= w or int(y) >= h:
                continue
            if m1[i] and int(i1[i]) not in added:
                good[1].append((n1[i], i1[i], un1[i]))
                added.add(int(i1[i]))
                self.stats["right-only tracks"] += 1
        for cam in (0, 1):  # :357-366
            for p, fid, un in good[cam]:
                self.db.setdefault(int(fid), ([], []))[cam].append((t, p[0], p[1], un[0], un[1]))
        self.pts = [points_array([g[0] for g in good[cam]]) for cam in (0, 1)]
        self.ids = [ids_array([g[1] for g in good[cam]]) for cam in (0, 1)]
        self.prev = cur


# ---- the streams the GPU test feeds (and the CPU test checks the coverage of)
def intrinsics(w, h, f):
    return np.array([f, f * 1.01, w / 2.0 - 0.5, h / 2.0 + 0.25, -0.28, 0.07, 2e-4, -1e-4])


class Stream:
    def __init__(self, name, w, h, cfg, disparity, offsets, K_left, K_right, mask_right=None, cut=None):
        self.name, self.w, self.h, self.cfg, self.disparity, self.offsets = name, w, h, cfg, disparity, offsets
        self.K_left, self.K_right, self.mask_right, self.cut = K_left, K_right, mask_right, cut

    def frames(self):
        """(t, left, right, mask_left, mask_right) per frame: one textured plane seen at a uniform horizontal disparity; offsets:
        per frame (tx, ty) of the left view and the extra (dx, dy) of the right one.  `cut`: frame -> a mask on both images of that
        frame (the next frame's detection on the then-last pair prunes with it)."""
        canvas = synth.texture_canvas(self.w, self.h, seed=42)
        for f, (tx, ty, dx, dy) in enumerate(self.offsets):
            left = synth.render_frame(canvas, self.w, self.h, tx=tx, ty=ty)
            right = synth.render_frame(canvas, self.w, self.h, tx=tx + self.disparity + dx, ty=ty + dy)
            ml = np.zeros((self.h, self.w), np.uint8) if self.mask_right is not None else None
            mr = self.mask_right
            if self.cut is not None and f in self.cut:
                ml = mr = self.cut[f]
            yield 10.0 + 0.05 * f, left, right, ml, mr


def streams():
    out = []
    w, h = 320, 240
    cfg = Settings(60, 5, 4, 10)
    band = np.zeros((h, w), np.uint8)
    band[:, 80:112] = 255  # (between the grid cells' sample points at x = 0, 64, 128, ...: no cell is skipped for it)
    # a jump of the right view alone (frame 3) starves the right list, a jump of both (frame 5) the left one
    offs = [(0, 0, 0, 0), (2, 1, 0, 0), (4, 1, 0, 0), (5, 2, 40, 25), (6, 2, 40, 25), (60, 45, 40, 25), (61, 46, 40, 25), (63, 46, 40, 25)]
    out.append(Stream("band", w, h, cfg, 6.0, offs, intrinsics(w, h, 230.0), intrinsics(w, h, 230.0), mask_right=band))
    out.append(Stream("two cameras", w, h, cfg, 6.0, offs[:6], intrinsics(w, h, 230.0), intrinsics(w, h, 150.0) + np.array([0, 0, 3, -2, 0.1, 0, 0, 0])))
    w, h = 256, 192
    cfg = Settings(40, 4, 3, 8)
    nearly_all = np.full((h, w), 255, np.uint8)
    nearly_all[60:100, 60:120] = 0
    offs = [(0, 0, 0, 0), (1, 1, 0, 0), (2, 1, 0, 0), (3, 2, 0, 0), (4, 2, 0, 0), (5, 3, 0, 0), (6, 3, 0, 0), (7, 3, 0, 0)]
    # frame 2's mask leaves a handful of points to frame 3's matching (fewer than 10: all-zero masks, empty lists), frame 4 detects
    # anew; frame 5's mask leaves none to frame 6 (both masks empty: the reset), frame 7 detects anew
    out.append(Stream("cut", w, h, cfg, 4.0, offs, intrinsics(w, h, 190.0), intrinsics(w, h, 190.0), cut={2: nearly_all, 5: np.full((h, w), 255, np.uint8)}))
    return out


# ---- the model pairings (camera 0, camera 1) and the equidistant coefficient sets (MILD and STRONG of test_gpu_equidistant.py)
PAIRINGS = {"RR": ("radtan", "radtan"), "RE": ("radtan", "equidistant"), "ER": ("equidistant", "radtan"), "EE": ("equidistant", "equidistant")}
EQUI_SETS = {"mild": (3.2e-3, -1.1e-3, 2.4e-3, -6.0e-4), "strong": (-0.35, 0.12, -0.03, 0.004)}
# what test_gpu_stereo_tracker.py feeds beside the three RR streams ("cut" keeps every point under any model: it stays RR)
PAIRING_RUNS = [("two cameras", "RE", "strong"), ("two cameras", "ER", "strong"), ("two cameras", "EE", "strong"), ("band", "EE", "strong"),
                ("two cameras", "EE", "mild")]


def paired_intrinsics(s, pairing, coeffs):
    """the stream's K8 per camera, an equidistant camera's K8[4:] replaced by the coefficient set (its fx fy cx cy stay)"""
    out = []
    for K, model in zip((s.K_left, s.K_right), PAIRINGS[pairing]):
        K = np.array(K, dtype=np.float64)
        if model == "equidistant":
            K[4:] = EQUI_SETS[coeffs]
        out.append(K)
    return out


def run_stream(s, ref, K8_at=None):
    """feeds the stream to `ref`; K8_at: frame -> (camera, K8) set before that frame is fed.  Returns the lists after every frame."""
    after = []
    for f, (t, left, right, ml, mr) in enumerate(s.frames()):
        if K8_at and f in K8_at:
            cam, K = K8_at[f]
            ref.K8[cam] = np.array(K, dtype=np.float64)
        ref.feed(t, left, right, ml, mr)
        after.append((ref.pts[0].copy(), ref.ids[0].copy(), ref.pts[1].copy(), ref.ids[1].copy()))
    return after


@functools.lru_cache(maxsize=None)
def reference_run(name, pairing="RR", coeffs=None):
    """the restatement over one of the streams under one model pairing, computed once:
    (stream, [(pts0, ids0, pts1, ids1) after every frame], StereoRef); the intrinsics it ran with are the StereoRef's K8"""
    s = {x.name: x for x in streams()}[name]
    K8 = paired_intrinsics(s, pairing, coeffs)
    ref = StereoRef(s.cfg, K8[0], K8[1], models=PAIRINGS[pairing])
    return s, run_stream(s, ref), ref


# ---- an intrinsics change between two pairs (plv_stereo_set_intrinsics): "two cameras" under EE strong, one camera's K8 replaced
# before pair CHANGE_AT is fed
CHANGE_AT = 3


def changed_intrinsics(K8):
    """a calibration step far larger than an update makes, so that the threshold 2 / max(fx, fy) and the undistortion both show"""
    return np.array(K8, dtype=np.float64) * np.array([1.25, 1.25, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5]) + np.array([0, 0, 4.0, -3.0, 0, 0, 0, 0])


@functools.lru_cache(maxsize=None)
def changed_run(cam):
    s, _, plain = reference_run("two cameras", "EE", "strong")
    K8 = paired_intrinsics(s, "EE", "strong")
    ref = StereoRef(s.cfg, K8[0], K8[1], models=PAIRINGS["EE"])
    return s, run_stream(s, ref, {CHANGE_AT: (cam, changed_intrinsics(K8[cam]))}), ref
