"""What the case matrix of the corner detector (tests/detect_cases.py) must contain, asserted on the CPU oracle alone: no case of
tests/test_gpu_detect_edges.py can pass vacuously.  The overflowing cells really hold more keys than fast_topk_kernel stages, the
near-full ones stay below; equal scores really face each other across the tile seam and neither survives; the lattices are all ties
and touch the first admissible column and the tile seams; the few / none cases have fewer keys than slots; the 7-pixel cells have one
admissible pixel and the 6-pixel ones none; every special point of the boxes case changes the oracle's result where it is meant to;
the sub-pixel image ends refinements by every exit it names; the capacity really cuts the list."""
import collections

import numpy as np
import pytest

import detect_cases as dc


def _counts(case):
    gx, gy, _, _, _ = dc.extraction_grid(case)
    return np.array([[len(dc.cell_keypoints(case, x, y)[0]) for x in range(gx)] for y in range(gy)])


@pytest.mark.parametrize("which", dc.OVERFLOW)
def test_overflow_cells_hold_more_keys_than_are_staged(which):
    case = dc.overflow(which)
    _, _, cw, ch, nfg = dc.extraction_grid(case)
    n = _counts(case)
    assert n.max() > 4096, n
    assert n.max() <= dc.cell_bound(cw, ch)
    assert nfg == {1: 101, 2: 26}[case.grid_x]
    # the cut-off is not at the top score: keys of several scores are among the first nfg, so dropping any stored key can show
    _, r = dc.cell_winners(case, 0, 0)
    assert len(np.unique(r)) > 5
    assert len(dc.run_oracle(case)[0]) > 10


def test_overflow_covers_the_sizes():
    sizes = {dc.extraction_grid(dc.overflow(k))[2:4] for k in dc.OVERFLOW}
    assert {(320, 240), (376, 240), (640, 360)} <= sizes and any(cw > 640 and ch > 360 for cw, ch in sizes)


def test_near_cap_cells_are_nearly_full():
    case = dc.near_cap()
    assert dc.extraction_grid(case)[:4] == (5, 5, 256, 144)
    n = _counts(case)
    assert n.max() <= 4096 and n.max() > 3000, n


@pytest.mark.parametrize("which", dc.SEAM)
def test_seam_mirror_scores_face_each_other(which):
    case = dc.seam_mirror(which)
    do = dc.oracle_lib.load_detect()
    img = case.img if which.startswith("x") else case.img.T            # (scores of the transposed image: the circle is symmetric)
    img = np.ascontiguousarray(img)
    assert np.array_equal(img[:, :32], img[:, 63:31:-1])
    pairs = 0
    for y in range(3, img.shape[0] - 3):
        a, b = do.fast_score(img, 31, y, case.fast_threshold), do.fast_score(img, 32, y, case.fast_threshold)
        assert a == b
        pairs += a > 0
    assert pairs >= 10, pairs
    gx, gy, cw, ch, _ = dc.extraction_grid(case)
    axis = 0 if which.startswith("x") else 1
    total = 0
    for x in range(gx):
        for y in range(gy):
            xy, _ = dc.cell_keypoints(case, x, y)
            pos = xy[:, axis] + (x * cw, y * ch)[axis]
            assert not np.isin(pos, (31, 32)).any()
            total += len(xy)
    assert total > 20
    assert (cw, ch)[axis] == (32 if "split" in which else 64)


@pytest.mark.parametrize("off", dc.TIES)
def test_all_ties(off):
    case = dc.all_ties(off)
    xy, r = dc.cell_keypoints(case, 0, 0)
    assert len(xy) > 1000 and (r == 254).all()
    assert dc.extraction_grid(case)[4] == 61
    if off == 3:
        assert len(xy) == 1131 and xy[:, 0].min() == 3 and np.isin(xy[:, 0] % 32, (0, 31)).sum() == 116
    if off == "big":
        assert len(xy) > 4096 and xy[:, 0].min() == 3
    # the winners are the first 61 in raster order and nothing else tells them from the rest
    wxy, _ = dc.cell_winners(case, 0, 0)
    assert np.array_equal(wxy, xy[:61].astype(np.int64))


def test_few_and_none():
    c = dc.few("dots")
    assert 0 < len(dc.cell_keypoints(c, 0, 0)[0]) < dc.extraction_grid(c)[4]
    assert len(dc.run_oracle(c)[0]) == len(dc.cell_keypoints(c, 0, 0)[0]) == 5
    c = dc.few("dots-2x2")
    n = _counts(c)
    assert sorted(n.ravel()) == [0, 1, 2, 3] and dc.extraction_grid(c)[4] == 16
    c = dc.few("none")
    assert _counts(c).sum() == 0
    p, i, cid = dc.run_oracle(c)
    assert cid == c.currid and len(p) == 3 and list(i) == [7, 8, 10]        # the point next to another and the edge point are dropped
    c = dc.few("one-textured")
    n = _counts(c)
    assert n[0, 1] > 20 and n.sum() == n[0, 1] and n.shape == (2, 3)


def test_thresholds():
    c = dc.thresholds("thr1")
    assert c.fast_threshold == 1
    r = np.concatenate([dc.cell_keypoints(c, x, y)[1] for x in range(2) for y in range(2)])
    assert r.min() == 1                                                       # a score the default threshold would have cut
    c = dc.thresholds("thr254")
    xy, r = dc.cell_keypoints(c, 0, 0)
    assert c.fast_threshold == 254 and len(xy) > 1000 and (r == 254).all()   # 255 above the ring: the corner test is `> threshold`
    c = dc.thresholds("equal")
    do = dc.oracle_lib.load_detect()
    xy, r = dc.cell_keypoints(c, 0, 0)
    assert sorted(map(tuple, xy.astype(int))) == sorted(dc.EQUAL_DOTS[1::2]) and (r == 20).all()    # one above the threshold: corners
    for x, y in dc.EQUAL_DOTS[0::2]:                                                               # exactly at it: none, by one level
        assert do.fast_score(c.img, x, y, 20) == 0 and do.fast_score(c.img, x, y, 19) == 19
        assert c.img[y, x] - c.img[y + 3, x] > 20 and c.img[y, x] - c.img[y, x + 3] > 20         # (the pre-test of the kernel passes)


def test_cell_sizes():
    c = dc.cell_sizes("7px")
    assert dc.extraction_grid(c)[:4] == (15, 10, 7, 7)
    n = _counts(c)
    assert n.max() == 1 and n.sum() > 5
    for x in range(15):
        for y in range(10):
            xy, _ = dc.cell_keypoints(c, x, y)
            assert all(tuple(p) == (3, 3) for p in xy)
    c = dc.cell_sizes("6px")
    assert dc.extraction_grid(c)[:4] == (15, 10, 6, 6) and _counts(c).sum() == 0 and len(dc.run_oracle(c)[0]) == 0
    c = dc.cell_sizes("33px")
    assert dc.extraction_grid(c)[:4] == (5, 3, 33, 33)
    c = dc.cell_sizes("remainder")
    assert dc.extraction_grid(c)[:4] == (3, 2, 33, 37) and c.img.shape == (75, 100)
    for k in ("33px", "remainder"):
        c = dc.cell_sizes(k)
        assert _counts(c).min() > dc.extraction_grid(c)[4]                  # every cell is cut to its first nfg


def test_boxes_change_the_result_where_intended():
    b = dc.boxes()
    case, mpd = b.case, b.case.min_px_dist
    assert len(case.pts) >= 300 and mpd > 10
    res0 = dc.run_oracle(b.base)[0]
    res = dc.run_oracle(case)
    special = case.pts[b.first_special:]
    # the specials are kept as existing points, and at least 256 boxes are painted before theirs
    kept_before = dc.run_oracle(case._replace(num_features=10), pts=case.pts[:b.first_special], ids=case.ids[:b.first_special])[0]
    h, w = case.img.shape
    xi, yi = kept_before[:, 0].astype(int), kept_before[:, 1].astype(int)
    assert ((xi - mpd >= 0) & (xi + mpd < w) & (yi - mpd >= 0) & (yi + mpd < h)).sum() >= 256
    for p in special:
        assert dc.contains(res[0], p)
    assert res[2] > case.currid
    ref = lambda q: dc.refined(case, [q])[0]
    for q in (b.at_dist_x, b.at_dist_y, b.past_dist_x, b.past_dist_y, b.border, b.mask127, b.mask128):
        assert dc.contains(res0, ref(q)), q                                   # every named winner is in the result of the empty start
    d = lambda q, p: (abs(q[0] - int(p[0])), abs(q[1] - int(p[1])))
    assert d(b.at_dist_x, special[0]) == (mpd, 0) and d(b.at_dist_y, special[1]) == (0, mpd)
    assert d(b.past_dist_x, special[2]) == (mpd + 1, 0) and d(b.past_dist_y, special[3]) == (0, mpd + 1)
    assert int(special[4][0]) - mpd < 0 and d(b.border, special[4])[0] <= mpd and d(b.border, special[4])[1] == 0
    assert case.mask[b.mask127[1], b.mask127[0]] == 127 and case.mask[b.mask128[1], b.mask128[0]] == 128
    assert not dc.contains(res[0], ref(b.at_dist_x)) and not dc.contains(res[0], ref(b.at_dist_y))
    assert dc.contains(res[0], ref(b.past_dist_x)) and dc.contains(res[0], ref(b.past_dist_y))
    assert dc.contains(res[0], ref(b.border))
    assert dc.contains(res[0], ref(b.mask127)) and not dc.contains(res[0], ref(b.mask128))
    # without the mask the 128 winner is back; without the special points the two boxed winners are
    assert dc.contains(dc.run_oracle(case, mask=None)[0], ref(b.mask128))
    r2 = dc.run_oracle(case, pts=case.pts[:b.first_special], ids=case.ids[:b.first_special])[0]
    assert dc.contains(r2, ref(b.at_dist_x)) and dc.contains(r2, ref(b.at_dist_y))


def test_grid_line_point_decides_the_cell():
    new = {}
    for side in ("left", "right"):
        c = dc.grid_line(side)
        p, i, cid = dc.run_oracle(c)
        assert i[0] == 5 and cid > 5
        q = p[1:]
        new[side] = (int(((q[:, 0] < 147) & (q[:, 1] < 93)).sum()), int(((q[:, 0] >= 153) & (q[:, 0] < 297) & (q[:, 1] < 93)).sum()))
    assert new["left"][0] == 0 and new["left"][1] > 0, new        # x = 150.39 fills cell (0, 0): cell (1, 0) is extracted from
    assert new["right"][0] > 0 and new["right"][1] == 0, new      # x = 150.41 fills cell (1, 0)


def test_subpix_trace_is_the_oracle():
    for c in (dc.subpix_exits(), dc.thresholds("thr1"), dc.cell_sizes("33px")):
        xy, _ = dc.cell_keypoints(c, 0, 0)
        ref = dc.refined(c, xy)
        for p, q in zip(xy, ref):
            x, y, _, _ = dc.subpix_trace(c.img, p[0], p[1])
            assert np.float32(x) == q[0] and np.float32(y) == q[1]
    assert dc.subpix_trace(np.full((40, 40), 7, np.uint8), 20, 20)[:3] == (20.0, 20.0, "det")


def test_subpix_exits():
    c = dc.subpix_exits()
    h, w = c.img.shape
    xy, _ = dc.cell_keypoints(c, 0, 0)
    res = dc.run_oracle(c)[0]
    ends = collections.Counter()
    near = collections.Counter()
    for p in xy:
        x, y, end, clamped = dc.subpix_trace(c.img, p[0], p[1])
        if not dc.contains(res, (x, y)):
            continue                                        # (dropped by the min_px_dist grid: the device result cannot show it)
        ends[end] += 1
        ends["clamped"] += clamped
        for side, on in (("left", p[0] < 6), ("right", p[0] >= w - 6), ("top", p[1] < 6), ("bottom", p[1] >= h - 6)):
            near[side] += bool(on and clamped)
    assert all(near[s] >= 1 for s in ("left", "right", "top", "bottom")), near
    assert ends["eps"] >= 1 and ends["iters"] >= 1
    assert ends["iters+revert"] + ends["eps+revert"] >= 1
    assert ends["left"] >= 1 and ends["left+revert"] >= 1, ends
    assert res[:, 0].min() < 0                              # the refinement that left the image is returned where it ended
    assert ends["det"] + ends["det+revert"] == 0            # not reached from a detection (module docstring of detect_cases)


def test_cap_cuts_the_list():
    base, case = dc.cap_cut()
    full, cut = dc.run_oracle(base), dc.run_oracle(case)
    assert len(cut[0]) == case.cap == len(full[0]) - 4 and len(base.pts) == 2
    assert np.array_equal(cut[0], full[0][:case.cap]) and cut[2] == full[2] - 4


def test_every_case_uses_the_image_as_given():
    names = [c.name for c in dc.gpu_cases()]
    assert len(names) == len(set(names)) >= 29
    assert dc.PLV_HIST_NONE == 0
