"""TrackKLT::feed_new_camera / feed_monocular restated in Python on the CPU oracle's primitives
(REF: open_vins/ov_core/src/track/TrackKLT.cpp:34-200), with the feature database calls the library answers (plv_db_*) restated on
the restatement's own `db`.  Device-free: test_mono_ref_cpu.py holds it to the compiled oracle/frame_oracle.cpp and shows that the
streams below reach every branch; test_gpu_tracker*.py hold the library to it.

`stats` counts what a stream exercised, `frames` what happened in every feed.  `variant` switches in one mistake a mirror of
feed_monocular could make (VARIANTS): the CPU test shows that the streams tell each of them from the restatement."""
import functools
from collections import Counter

import numpy as np

import oracle_lib
import synth
from stereo_ref import Settings, ids_array, intrinsics, points_array

F32 = np.float32
NONE, HISTOGRAM, CLAHE = 0, 1, 2   # TrackBase::HistogramMethod / PLV_HIST_*

VARIANTS = ("top-up with the current mask",          # perform_detection on the last image with this frame's mask (:130 takes img_mask_last)
            "keep loop with the last mask",          # :166 reads message.masks, the current one
            "keep loop with >= 127",                 # :166 is > 127
            "mask not stored on the early exits",    # :147 stores the mask on the reset; the fewer-than-10 frame stores it at :186
            "detection on the last image after a loss")  # :114 detects on the current pyramid

# what stats / frames may hold (test_mono_ref_cpu.py asks for every one of them)
BRANCHES = ("first-frame detection", "detection after a loss, with a mask", "detection after a loss, without a mask", "top-up adds",
            "top-up adds nothing", "top-up prunes", "top-up keeps all", "fewer than 10 points", "n == 0 reset", "dropped as out of image",
            "dropped on the current mask", "dropped as unmatched", "everything lost")


class OracleTracker:
    """cfg: anything with num_features, grid_x, grid_y, min_px_dist, fast_threshold (a plv_config or stereo_ref.Settings);
    histogram_method None: cfg.histogram_method where cfg has one, else HISTOGRAM (the library's default)."""

    def __init__(self, cfg, K8, histogram_method=None, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.cfg, self.K8, self.variant = cfg, np.asarray(K8, dtype=np.float64), variant
        self.method = histogram_method if histogram_method is not None else getattr(cfg, "histogram_method", HISTOGRAM)
        self.fo, self.do = oracle_lib.load_front(), oracle_lib.load_detect()
        self.pts, self.ids = points_array([]), ids_array([])
        self.currid = 0
        self.prev = None       # (equalised image, pyramid) of the last feed
        self.mask_last = None  # img_mask_last
        self.fed = 0
        self.db = {}           # id -> [(t, u, v, un, vn) ...]
        self.stats = Counter()
        self.frames = []       # per feed: the set of branches taken in it

    def _equalise(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if self.method == HISTOGRAM:
            return self.fo.equalize_hist(img)  # :59
        if self.method == CLAHE:
            return self.fo.clahe(img)          # :61-64 createCLAHE(10.0, 8x8)
        assert self.method == NONE, self.method
        return img                             # :66

    def _detect(self, eq, mask, pts, ids):
        c = self.cfg
        p, i, self.currid = self.do.perform_detection(eq, mask, pts, ids, self.currid, c.num_features, c.grid_x, c.grid_y, c.min_px_dist,
                                                      c.fast_threshold)
        return p, i

    def _took(self, events, what, n=1):
        events.add(what)
        self.stats[what] += n

    def feed_image(self, img):
        """an image fed past the tracker (plv_feed_image between two tracker feeds): it becomes the last image the next feed tops up
        on and tracks from; points, ids and the stored mask stay"""
        eq = self._equalise(img)
        self.prev = (eq, self.fo.pyramid(eq))

    def feed(self, t, img, mask=None):
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        events = set()
        self.frames.append(events)
        eq = self._equalise(img)
        pyr = self.fo.pyramid(eq)  # :71
        h, w = eq.shape
        early_exit = False
        try:
            if len(self.ids) == 0:  # :110-123
                if self.fed == 0:
                    self._took(events, "first-frame detection")
                else:
                    self._took(events, "detection after a loss, with a mask" if mask is not None else "detection after a loss, without a mask")
                on = self.prev[0] if self.variant == "detection on the last image after a loss" and self.prev is not None else eq
                self.pts, self.ids = self._detect(on, mask, self.pts, self.ids)
                return
            # :127-130 top-up on the last image with the last mask
            n_in, newest = len(self.ids), self.currid
            top_mask = mask if self.variant == "top-up with the current mask" else self.mask_last
            pts_old, ids_old = self._detect(self.prev[0], top_mask, self.pts, self.ids)
            kept = int((ids_old <= newest).sum())
            self._took(events, "top-up adds" if len(ids_old) > kept else "top-up adds nothing")
            self._took(events, "top-up prunes" if kept < n_in else "top-up keeps all")
            n = len(ids_old)
            if n == 0:  # :836-837 perform_matching returns at once, :143-152
                self._took(events, "n == 0 reset")
                self.pts, self.ids = points_array([]), ids_array([])
                early_exit = True
                return
            if n < 10:  # :848-852 an all-zero mask, the points where they were: the loop below keeps none
                self._took(events, "fewer than 10 points")
                early_exit = True
                pts_new, ok, n1 = pts_old.copy(), np.zeros(n, np.uint8), None
            else:
                rc, pts_new, ok, n0, n1 = self.fo.perform_matching(self.prev[1], pyr, pts_old, pts_old, self.K8)
            keep_mask = self.mask_last if self.variant == "keep loop with the last mask" else mask
            on_mask = (lambda v: v >= 127) if self.variant == "keep loop with >= 127" else (lambda v: v > 127)
            good, gid = [], []
            for i in range(n):  # :159-173
                x, y = pts_new[i]
                if x < 0 or y < 0 or int(x) >= w or int(y) >= h:
                    self._took(events, "dropped as out of image")
                    continue
                if keep_mask is not None and on_mask(int(keep_mask[int(y), int(x)])):
                    self._took(events, "dropped on the current mask")
                    continue
                if not ok[i]:
                    self._took(events, "dropped as unmatched")
                    continue
                good.append(pts_new[i])
                gid.append(ids_old[i])
                self.db.setdefault(int(ids_old[i]), []).append((t, x, y, n1[i, 0], n1[i, 1]))  # :176-179
            if not good:
                self._took(events, "everything lost")
            self.pts, self.ids = points_array(good), ids_array(gid)
        finally:  # :116-121 / :144-149 / :182-189
            self.prev = (eq, pyr)
            if not (early_exit and self.variant == "mask not stored on the early exits"):
                self.mask_last = mask
            self.fed += 1


# ---- the database calls (plv_db_*), on a db as OracleTracker keeps it
def db_select(db, mode, t):
    """mode 0: features_not_containing_newer(t), no observation at or after t (FeatureDatabase.cpp:147-186); mode 1:
    features_containing_older(t), the first observation before t (:188-227); ids ascending"""
    if mode == 0:
        out = [fid for fid, obs in db.items() if obs and not obs[-1][0] >= t]
    else:
        out = [fid for fid, obs in db.items() if obs and obs[0][0] < t]
    return ids_array(sorted(out))


def db_cleanup_measurements(db, t):
    """observations older than t go, then the tracks with none left (FeatureDatabase.cpp:286-303), in place.  "Older" is `< t`
    as the library and the compiled oracle have it: an observation at t itself stays (Feature::clean_older_measurements of the
    reference drops that one too; the next update's remove_unusable_measurements drops it either way)."""
    for fid in list(db):
        db[fid] = [o for o in db[fid] if not o[0] < t]
        if not db[fid]:
            del db[fid]


def db_remove(db, ids):
    for fid in ids:
        db.pop(int(fid), None)


def db_export(db, ids):
    """(obs_ptr, times, uv, uvn) of plv_db_export_tracks: an id the database does not hold has no observations"""
    ptr, t, uv, uvn = [0], [], [], []
    for fid in ids:
        for o in db.get(int(fid), []):
            t.append(o[0]), uv.append(o[1:3]), uvn.append(o[3:5])
        ptr.append(len(t))
    return np.array(ptr, dtype=np.int32), np.array(t, dtype=np.float64), points_array(uv), points_array(uvn)


def db_disparity(db, time0, time1):
    """FeatureHelper::compute_disparity as plv_db_disparity documents it: the raw-pixel difference and its norm in float, mean and
    standard deviation (n - 1) in double over the tracks in ascending id, (-1, -1, 0) below two tracks"""
    disp = []
    for fid in sorted(db):
        times = [o[0] for o in db[fid]]
        if time0 not in times or time1 not in times:
            continue
        o0, o1 = db[fid][times.index(time0)], db[fid][times.index(time1)]
        du, dv = F32(o1[1]) - F32(o0[1]), F32(o1[2]) - F32(o0[2])
        disp.append(float(np.sqrt(F32(F32(du * du) + F32(dv * dv)))))
    if len(disp) < 2:
        return -1.0, -1.0, 0
    mean = 0.0
    for d in disp:
        mean += d
    mean /= float(len(disp))
    var = 0.0
    for d in disp:
        var += (d - mean) * (d - mean)
    return mean, float(np.sqrt(var / float(len(disp) - 1))), len(disp)


def assert_database(ctx, db):
    """the library's whole database is `db` (a mono_ref database): ids, and times, uv and uvn of every observation"""
    ids = np.array(sorted(db), dtype=np.uint64)
    assert ctx.db_size() == len(ids)
    assert np.array_equal(ctx.db_select(1, np.inf), ids)
    got, want = ctx.db_export(ids), db_export(db, ids)
    for g, w, what in zip(got, want, ("obs_ptr", "times", "uv", "uvn")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


# ---- the streams the GPU tests feed (and the CPU test checks the coverage of)
class Stream:
    def __init__(self, name, w, h, cfg, K, offsets, masks):
        self.name, self.w, self.h, self.cfg, self.K, self.offsets, self.masks = name, w, h, cfg, K, offsets, masks

    def times(self):
        return [10.0 + 0.05 * f for f in range(len(self.offsets))]

    def frames(self):
        """(t, image, mask or None) per frame: one textured plane under the frame's (tx, ty)"""
        canvas = synth.texture_canvas(self.w, self.h, seed=42)
        for f, (tx, ty) in enumerate(self.offsets):
            yield 10.0 + 0.05 * f, synth.render_frame(canvas, self.w, self.h, tx=tx, ty=ty), self.masks.get(f)


def streams():
    out = []
    w, h = 320, 240
    cfg = Settings(60, 5, 4, 10)
    # one band just above the threshold and one just at it: a point on the second is kept (`> 127`), the jumps of frames 4 and 5
    # carry points out of the image and leave most unmatched
    band = np.zeros((h, w), np.uint8)
    band[:, 80:112] = 128
    band[:, 200:230] = 127
    offs = [(0, 0), (2, 1), (4, 1), (5, 2), (30, 2), (60, 45), (61, 46), (63, 46)]
    out.append(Stream("band", w, h, cfg, intrinsics(w, h, 230.0), offs, {f: band for f in range(len(offs))}))
    w, h = 256, 192
    nearly_all = np.full((h, w), 255, np.uint8)
    nearly_all[60:100, 60:120] = 0
    # frame 2's mask leaves a handful of points to frame 3's matching (fewer than 10: nothing kept), frame 4 detects anew without a
    # mask; frame 5's mask leaves none, frame 6 detects anew
    out.append(Stream("cut", w, h, Settings(40, 4, 3, 8), intrinsics(w, h, 190.0), [(i, (i + 1) // 2) for i in range(8)],
                      {2: nearly_all, 5: np.full((h, w), 255, np.uint8)}))
    w, h = 320, 240
    strip = np.full((h, w), 255, np.uint8)
    strip[:, 1:10] = 0
    # frame 2 keeps the few points inside x < 10; frame 3's top-up prunes them all (closer than 10 px to the border) and finds no
    # valid cell (every cell's sample point is 255 in the last mask): the n == 0 reset; frame 4 detects anew
    out.append(Stream("strip", w, h, Settings(60, 5, 4, 10), intrinsics(w, h, 230.0), [(0, 0), (-2, 1), (-22, 1), (-23, 1), (-24, 2)], {2: strip}))
    w, h = 256, 192
    partly = np.zeros((h, w), np.uint8)
    partly[:, 100:140] = 200
    # frame 1's mask leaves nothing, frame 2 detects anew under a mask (the three streams above regain their tracks without one),
    # frame 3 tracks without a mask: its top-up prunes with frame 2's
    out.append(Stream("regain", w, h, Settings(40, 4, 3, 8), intrinsics(w, h, 190.0), [(i, (i + 1) // 2) for i in range(4)],
                      {1: np.full((h, w), 255, np.uint8), 2: partly}))
    return out


STREAMS = ("band", "cut", "strip", "regain")


def stream(name):
    return {s.name: s for s in streams()}[name]


@functools.lru_cache(maxsize=None)
def reference_run(name, histogram_method=HISTOGRAM, variant=None):
    """the restatement over one of the streams, computed once: (stream, [(points, ids, stored mask) after every frame], the
    OracleTracker).  Shared between tests: nobody changes what it returns (the database calls above work on copies, db_copy)."""
    s = stream(name)
    ref = OracleTracker(s.cfg, s.K, histogram_method, variant)
    after = []
    for t, img, mask in s.frames():
        ref.feed(t, img, mask)
        after.append((ref.pts.copy(), ref.ids.copy(), ref.mask_last))
    return s, after, ref


def db_copy(db):
    return {fid: list(obs) for fid, obs in db.items()}


# ---- CLAHE (createCLAHE(10.0, 8x8), TrackKLT.cpp:60-64) off the one size the front-end test feeds
# (w, h) -> the clip max(int(10 * tile area / 256), 1) its 8 x 8 tiles give.  1280 x 560 is the KAIST camera's size; 40 x 40 (tiles
# of 5 x 5, a pyramid of two levels) is the one size here whose clip is the floor: 10 * 25 / 256 < 1.
CLAHE_SIZES = {(40, 40): 1, (64, 64): 2, (256, 192): 30, (320, 240): 46, (1280, 560): 437}
CLAHE_IMAGES = ("texture", "noise", "constant", "checker")


@functools.lru_cache(maxsize=None)
def clahe_image(w, h, kind):
    if kind == "texture":
        return synth.render_frame(synth.texture_canvas(w, h, seed=42), w, h, tx=3.0, ty=-2.0)
    if kind == "noise":  # low contrast: a few grey values hold every pixel of a tile
        return np.clip(100.0 + 10.0 * np.random.default_rng(w + h).normal(size=(h, w)), 0, 255).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w), 93, np.uint8)
    assert kind == "checker"
    ys, xs = np.mgrid[0:h, 0:w]
    return np.where(((xs // 3) + (ys // 3)) % 2 == 0, 60, 190).astype(np.uint8)


def clahe_tile_residuals(img, clip_limit=10.0, tiles=8):
    """per tile what CLAHE's redistribution works with: (clip, [(clipped total, residual, stride) ...]) — the excess over the clip
    is spread in batches of 256, the residual over bins `stride` apart"""
    h, w = img.shape
    tw, th = w // tiles, h // tiles
    assert tw * tiles == w and th * tiles == h
    clip = max(int(clip_limit * tw * th / 256), 1)
    out = []
    for j in range(tiles):
        for i in range(tiles):
            hist = np.bincount(img[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256)
            clipped = int(np.maximum(hist - clip, 0).sum())
            residual = clipped % 256
            out.append((clipped, residual, max(256 // residual, 1) if residual else 0))
    return clip, out
