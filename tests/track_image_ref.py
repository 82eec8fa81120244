"""The track image restated in numpy (include/plviwo.h "track image", DESIGN.md "The track image"): the rasterisation rules and the
layers that turn tracker state into a primitive list.  Integer arithmetic throughout (int64), so every comparison against the device
is exact.  A primitive is painted over its clipped bounding box with array operations; a few thousand take well under a second."""
import math

import numpy as np

RING, BOX, SEG = 0, 1, 2
HISTORY, ACTIVE, LINES, MASK = 1, 2, 4, 8

PRIM_DTYPE = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("a", "<i4"), ("b", "<i4"),
                       ("rgb", "u1", (3,)), ("pad", "u1")])
assert PRIM_DTYPE.itemsize == 32

GET_TRACK_IMG_COLORS = (255, 255, 0, 255, 255, 255)


def prim(kind, x0, y0, x1=0, y1=0, a=0, b=0, rgb=(0, 0, 0)):
    p = np.zeros((), dtype=PRIM_DTYPE)
    p["kind"], p["x0"], p["y0"], p["x1"], p["y1"], p["a"], p["b"] = kind, x0, y0, x1, y1, a, b
    p["rgb"] = rgb
    return p


def prims_array(items):
    out = np.zeros(len(items), dtype=PRIM_DTYPE)
    for i, p in enumerate(items):
        out[i] = p
    return out


def disc(x, y, r, rgb):
    return prim(RING, x, y, a=0, b=r * r, rgb=rgb)


# ---------------------------------------------------------------- rasterisation
def _window(W, H, xa, ya, xb, yb):
    """The part of the inclusive box [xa, xb] x [ya, yb] that lies in the image, as coordinate grids; None when empty."""
    xa, xb, ya, yb = max(xa, 0), min(xb, W - 1), max(ya, 0), min(yb, H - 1)
    if xa > xb or ya > yb:
        return None
    ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1].astype(np.int64)
    return xs, ys


def coverage(p, W, H):
    """(xs, ys) int64 arrays of the pixels of primitive p inside a W x H image."""
    kind, x0, y0, x1, y1, a, b = (int(p[k]) for k in ("kind", "x0", "y0", "x1", "y1", "a", "b"))
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    if kind == RING:
        if b < 0 or a > b:
            return none
        r = math.isqrt(b) + 1
        win = _window(W, H, x0 - r, y0 - r, x0 + r, y0 + r)
        if win is None:
            return none
        xs, ys = win
        d = (xs - x0) ** 2 + (ys - y0) ** 2
        hit = (d >= a) & (d <= b)
        return xs[hit], ys[hit]
    if kind == BOX:
        xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        win = _window(W, H, xa, ya, xb, yb)
        if win is None:
            return none
        xs, ys = win
        hit = (xs == xa) | (xs == xb) | (ys == ya) | (ys == yb)
        return xs[hit], ys[hit]
    if kind == SEG:
        if a < 1:
            return none
        dx, dy = x1 - x0, y1 - y0
        swap = abs(dx) < abs(dy)  # y-major: the same rule with the roles of x and y swapped
        if swap:
            u0, v0, u1, dmaj, dmin, Umax, Vmax = y0, x0, y1, abs(dy), abs(dx), H, W
            s = 1 if dx >= 0 else -1
        else:
            u0, v0, u1, dmaj, dmin, Umax, Vmax = x0, y0, x1, abs(dx), abs(dy), W, H
            s = 1 if dy >= 0 else -1
        lo, hi = max(min(u0, u1), 0), min(max(u0, u1), Umax - 1)
        if lo > hi:
            return none
        u = np.arange(lo, hi + 1, dtype=np.int64)
        i = np.abs(u - u0)
        if dmaj == 0:
            v = np.full_like(u, v0)
        else:
            v = v0 + s * ((2 * i * dmin + dmaj) // (2 * dmaj))
        # thickness: the minor coordinates v .. v + a - 1, of which only those inside the image matter
        t = np.arange(0, min(a, Vmax + max(0, -int(v.min()))), dtype=np.int64)
        us = np.repeat(u[None, :], len(t), axis=0).ravel()
        vs = (v[None, :] + t[:, None]).ravel()
        keep = (vs >= 0) & (vs < Vmax)
        us, vs = us[keep], vs[keep]
        return (vs, us) if swap else (us, vs)
    raise ValueError(f"unknown primitive kind {kind}")


def mask_rule(c):
    """Channel 2 under a set mask byte: cv::addWeighted(255 * 0.1 + c) = c + 25.5, rounded half to even, saturated."""
    c = np.asarray(c, dtype=np.int64)
    return np.minimum(255, c + np.where(c % 2 == 0, 26, 25)).astype(np.uint8)


def render(grey, prims, mask=None):
    """[H, W, 3] u8: the primitives painted in order over (g, g, g), then the mask rule."""
    grey = np.asarray(grey, dtype=np.uint8)
    H, W = grey.shape
    out = np.repeat(grey[:, :, None], 3, axis=2).copy()
    for p in prims:
        xs, ys = coverage(p, W, H)
        if len(xs):
            out[ys, xs] = p["rgb"]
    if mask is not None:
        m = np.asarray(mask) != 0
        out[:, :, 2][m] = mask_rule(out[:, :, 2][m])
    return out


# ---------------------------------------------------------------- float -> pixel
LIMIT = np.float32(2.0 ** 20)


def rne(v):
    """Round-half-to-even of the float32 value; None for a coordinate that drops its primitive."""
    v = np.float32(v)
    if not np.isfinite(v) or abs(v) > LIMIT:
        return None
    return int(np.rint(v))


def trunc_half(v):
    """(int)((double)v + 0.5), truncated towards zero (TrackLSD.cpp:865-866); None as rne."""
    v = np.float32(v)
    if not np.isfinite(v) or abs(v) > LIMIT:
        return None
    return int(math.trunc(float(v) + 0.5))


def _px(*vals, conv=rne):
    out = [conv(v) for v in vals]
    return None if any(o is None for o in out) else out


def ramp_color(c1, c2, n, z):
    """Colour of observation z of a track of n: clamp(c2[k] - (int)(1.0 * c1[k] / n * z), 0, 255)"""
    return tuple(min(255, max(0, int(c2[k]) - int(1.0 * c1[k] / n * z))) for k in range(3))


def flagged_color(n, z):
    return (0, 255, 255 - int(1.0 * 255 / n * z))


def _disc_f(out, x, y, r, rgb):
    c = _px(x, y)
    if c is not None:
        out.append(disc(c[0], c[1], r, rgb))


def _box_f(out, x, y, d, rgb):
    x, y, d = np.float32(x), np.float32(y), np.float32(d)
    c = _px(x - d, y - d, x + d, y + d)  # the subtraction in float32
    if c is not None:
        out.append(prim(BOX, c[0], c[1], c[2], c[3], rgb=rgb))


def _seg_f(out, xa, ya, xb, yb, rgb):
    c = _px(xa, ya, xb, yb)
    if c is not None:
        out.append(prim(SEG, c[0], c[1], c[2], c[3], a=1, rgb=rgb))


# ---------------------------------------------------------------- layers
def history_layer(W, H, pts, ids, tracks, highlighted=(), flagged=(), colors=GET_TRACK_IMG_COLORS, max_tracks=50):
    """tracks: id -> [n, 2] float32 observations (oldest first); an id without an entry has no track."""
    small = min(W, H) < 400
    rad = 1 if small else 2
    c1, c2 = colors[:3], colors[3:]
    highlighted, flagged = set(int(i) for i in highlighted), set(int(i) for i in flagged)
    out = []
    for (x, y), fid in zip(pts, ids):
        fid = int(fid)
        if fid in highlighted:
            _box_f(out, x, y, 3 if small else 5, (0, 255, 0))
            _disc_f(out, x, y, rad, (0, 255, 0))
        uv = tracks.get(fid)
        if uv is None or len(uv) == 0:
            continue
        n = len(uv)
        z = n - 1
        while z > 0:
            if n - z > max_tracks:
                break
            if fid in flagged:
                rgb, r = flagged_color(n, z), 2
            else:
                rgb, r = ramp_color(c1, c2, n, z), rad
            _disc_f(out, uv[z][0], uv[z][1], r, rgb)
            if z + 1 < n:
                _seg_f(out, uv[z][0], uv[z][1], uv[z + 1][0], uv[z + 1][1], rgb)
            z -= 1
    return out


def active_layer(W, H, pts, colors=GET_TRACK_IMG_COLORS):
    rad = 1 if min(W, H) < 400 else 2
    clamp = lambda c: tuple(min(255, max(0, int(v))) for v in c)
    out = []
    for x, y in pts:
        _disc_f(out, x, y, rad, clamp(colors[:3]))
        _box_f(out, x, y, 3, clamp(colors[3:]))
    return out


def lines_layer(pts, ids, lines, line_ids, rel_ptr, rel_id, line_db_ids):
    where = {int(fid): i for i, fid in enumerate(ids)}
    in_db = set(int(i) for i in line_db_ids)
    out = []
    for i, (ln, lid) in enumerate(zip(lines, line_ids)):
        if int(lid) not in in_db:
            continue
        rgb = ((i * 128) % 255, (i * 53) % 255, (i * 23) % 255)
        c = _px(*ln, conv=trunc_half)
        if c is not None:
            out.append(prim(SEG, c[0], c[1], c[2], c[3], a=2, rgb=rgb))
        for q in range(int(rel_ptr[i]), int(rel_ptr[i + 1])):
            k = where.get(int(rel_id[q]))
            if k is None:
                continue
            p = _px(pts[k][0], pts[k][1])
            if p is not None:
                out.append(prim(RING, p[0], p[1], a=49, b=81, rgb=rgb))
    return out


def track_image_list(W, H, layers, pts, ids, tracks, lines=(), line_ids=(), rel_ptr=(0,), rel_id=(), line_db_ids=(), highlighted=(),
                     flagged=(), colors=GET_TRACK_IMG_COLORS, max_tracks=50):
    """The list plv_track_image paints for the chosen layers: the point layers, then the lines."""
    out = []
    if layers & HISTORY:
        out += history_layer(W, H, pts, ids, tracks, highlighted, flagged, colors, max_tracks)
    if layers & ACTIVE:
        out += active_layer(W, H, pts, colors)
    if layers & LINES:
        out += lines_layer(pts, ids, lines, line_ids, rel_ptr, rel_id, line_db_ids)
    return prims_array(out)
