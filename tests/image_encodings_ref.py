"""numpy restatement of the image-encoding contract of include/plviwo.h (PLV_ENC_*), for all nine encodings: the yardstick of
tests/test_image_encodings_cpu.py and tests/test_gpu_image_encodings.py.  A vectorised form of the per-site rule, written from the
contract and not from the library: integers only, weights R 4899, G 9617, B 1868 over 2^14.

    colour   Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14, alpha ignored
    Bayer    interior site of colour c in {R, B}, o the other:  (diag4*w[o] + cross4*w[G] + centre*4*w[c] + 2^15) >> 16
             site G:  ((left+right)*w[colour of left] + (up+down)*w[colour of up] + centre*2*w[G] + 2^14) >> 15
             row 0 copies row 1, row H-1 copies row H-2; then column 0 copies column 1, column W-1 copies column W-2
    mono8    a copy
"""
import numpy as np

ENCODINGS = {"mono8": 0, "bayer_rggb8": 1, "bayer_bggr8": 2, "bayer_gbrg8": 3, "bayer_grbg8": 4, "bgr8": 5, "rgb8": 6, "bgra8": 7,
             "rgba8": 8}
BAYER = ("bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8")
COLOUR = ("bgr8", "rgb8", "bgra8", "rgba8")
BPP = {"mono8": 1, "bayer_rggb8": 1, "bayer_bggr8": 1, "bayer_gbrg8": 1, "bayer_grbg8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}
W = {"r": 4899, "g": 9617, "b": 1868}


def bayer_colours(name, h, w):
    """[h][w] array of 'r' / 'g' / 'b': the colour of every site; the name's letters are the sites (0,0), (0,1), (1,0), (1,1)"""
    letters = name[len("bayer_"):len("bayer_") + 4]
    cell = np.array(list(letters)).reshape(2, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    return cell[yy % 2, xx % 2]


def bayer_to_grey(m, name):
    m = np.asarray(m)
    assert m.ndim == 2 and m.dtype == np.uint8
    h, w = m.shape
    assert h >= 3 and w >= 3, "a Bayer mosaic is 3 x 3 at least"
    p = m.astype(np.int64)
    col = bayer_colours(name, h, w)
    wmap = np.zeros((h, w), dtype=np.int64)
    for k, v in W.items():
        wmap[col == k] = v
    c = p[1:-1, 1:-1]
    diag4 = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    horz, vert = p[1:-1, :-2] + p[1:-1, 2:], p[:-2, 1:-1] + p[2:, 1:-1]
    w_c, w_left, w_up, w_diag = wmap[1:-1, 1:-1], wmap[1:-1, :-2], wmap[:-2, 1:-1], wmap[:-2, :-2]
    colour_site = (diag4 * w_diag + (horz + vert) * W["g"] + c * 4 * w_c + (1 << 15)) >> 16   # the diagonal neighbours of R are B and v.v.
    green_site = (horz * w_left + vert * w_up + c * 2 * W["g"] + (1 << 14)) >> 15
    out = np.zeros((h, w), dtype=np.int64)
    out[1:-1, 1:-1] = np.where(col[1:-1, 1:-1] == "g", green_site, colour_site)
    out[0, :] = out[1, :]
    out[h - 1, :] = out[h - 2, :]
    out[:, 0] = out[:, 1]
    out[:, w - 1] = out[:, w - 2]
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def colour_to_grey(img, name):
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == BPP[name] and img.dtype == np.uint8
    p = img.astype(np.int64)
    r, g, b = (p[:, :, 0], p[:, :, 1], p[:, :, 2]) if name.startswith("rgb") else (p[:, :, 2], p[:, :, 1], p[:, :, 0])
    return ((r * W["r"] + g * W["g"] + b * W["b"] + 8192) >> 14).astype(np.uint8)


def to_grey(img, name):
    """the grey image of `img` in encoding `name` (H x W for the 1-byte encodings, H x W x 3 / 4 for the colour ones)"""
    if name == "mono8":
        return np.array(img, dtype=np.uint8)
    if name in BAYER:
        return bayer_to_grey(img, name)
    if name in COLOUR:
        return colour_to_grey(img, name)
    raise ValueError(name)


def mosaic(rgb, name):
    """samples an H x W x 3 RGB image at the sites of the Bayer pattern `name`: what the sensor would have delivered"""
    rgb = np.asarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    col = bayer_colours(name, h, w)
    return np.where(col == "r", rgb[:, :, 0], np.where(col == "g", rgb[:, :, 1], rgb[:, :, 2])).astype(np.uint8)


def random_image(rng, h, w, name):
    shape = (h, w) if BPP[name] == 1 else (h, w, BPP[name])
    return rng.integers(0, 256, size=shape, dtype=np.uint8)
