"""What the cases of tests/line_setting_cases.py must contain, proven on the oracle alone (no device), so that a later edit of the drawings
cannot hollow them out: hysteresis that promotes and leaves out, a corner drawing that is strong only inside a cleared corner, length /
distance / minimum-length settings that move the result, chains that exist only because min_px moved, and counts below the device's
capacities.  The restated edge map and chain walk (line_restatement.py) are held to the oracle's own FastLineDetector here too."""
import numpy as np
import pytest
from scipy import ndimage

import line_setting_cases as lc
import oracle_lib

_EIGHT = np.ones((3, 3), dtype=int)


@pytest.fixture(scope="module")
def lo():
    return oracle_lib.load_line()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _canny(lo, image_name, low, high):
    return lo.canny(lo.resize_half(lc.image(image_name)), low, high) != 0


def test_matrix_names_what_it_uses():
    assert len(set(lc.CASES)) == len(lc.CASES)
    for im, s in lc.CASES:
        assert im in lc.IMAGES and s in lc.SETTINGS, (im, s)
    used = {s for _, s in lc.CASES}
    assert used == set(lc.SETTINGS), set(lc.SETTINGS) - used
    assert {im for im, _ in lc.CASES} == set(lc.IMAGES)
    shapes = {lc.image(im).shape for im in lc.IMAGES}
    assert shapes == {(240, 320), (251, 333), (70, 98)}, shapes
    # the small texture only with settings that find something on it
    assert all(lc.SETTINGS[s]["length"] <= 8 for im, s in lc.CASES if im == "tex98")


@pytest.mark.parametrize("setting", lc.HYSTERESIS)
def test_hysteresis_cases_promote_and_leave_out(lo, setting):
    s = lc.SETTINGS[setting]
    low, high = min(s["c1"], s["c2"]), max(s["c1"], s["c2"])
    assert low < high and ("fading_bars", setting) in lc.CASES
    both, strong, weak = _canny(lo, "fading_bars", low, high), _canny(lo, "fading_bars", high, high), _canny(lo, "fading_bars", low, low)
    print(setting, "strong", int(strong.sum()), "promoted", int((both & ~strong).sum()), "left out", int((weak & ~both).sum()))
    assert not (strong & ~both).any() and not (both & ~weak).any()
    assert (both & ~strong).sum() >= 20, "nothing promoted"
    assert (weak & ~both).sum() >= 20, "nothing left out"


def test_swapped_thresholds_give_the_same_bytes(lo):
    half = lo.resize_half(lc.image("fading_bars"))
    assert np.array_equal(lo.canny(half, 90, 30), lo.canny(half, 30, 90))
    a, b = lc.reference(lo, "fading_bars", "canny90_30"), lc.reference(lo, "fading_bars", "canny30_90")
    assert len(a["segs"]) > 0 and _same(a["segs"], b["segs"]) and np.array_equal(a["edges"], b["edges"])


def test_gradient_at_the_high_threshold_is_weak(lo):
    """30 / 48 on the faint band: its flanks (|gx| + |gy| = 48 everywhere) are weak and attached to nothing strong, so they are left out;
    one step lower (30 / 47) they are strong and their two segments come back"""
    at, below = _canny(lo, "faint_band", 30, 48), _canny(lo, "faint_band", 30, 47)
    print("edge pixels at 30 / 48:", int(at.sum()), "at 30 / 47:", int(below.sum()))
    assert at.any() and not (at & ~below).any() and (below & ~at).sum() >= 300
    a = lc.reference(lo, "faint_band", "canny30_48")["segs"]
    b = lo.detect_lines(lc.image("faint_band"), 20, lc.SHIPPED["dist"], 30, 47, 40.0)
    assert 0 < len(a) and len(a) + 2 == len(b), (len(a), len(b))


def test_controls(lo):
    """120 / 120 moves the edge map without hysteresis; 5000 / 5000 leaves no edge; the shipped control finds something"""
    for im in ("fading_bars", "tex333"):
        ship, c120, none = (lc.reference(lo, im, s) for s in ("shipped", "canny120_120", "canny5000_5000"))
        assert len(ship["segs"]) > 0 and len(c120["segs"]) > 0
        assert not np.array_equal(ship["edges"], c120["edges"]) and c120["edges"].any()
        assert not none["edges"].any() and len(none["segs"]) == 0 and len(none["chains"]) == 0


@pytest.mark.parametrize("name", list(lc.CORNERS))
def test_corner_cases_are_strong_only_inside_the_cleared_corner(lo, name):
    s = lc.SETTINGS["canny30_320"]
    low, high = s["c1"], s["c2"]
    strong = _canny(lo, name, high, high)
    rows, cols = lc.CORNERS[name]
    inside = np.zeros_like(strong)
    inside[rows, cols] = True
    assert (strong & inside).sum() >= 1 and not (strong & ~inside).any(), (int((strong & inside).sum()), int((strong & ~inside).sum()))
    ref = lc.reference(lo, name, "canny30_320")
    print(name, "strong", int(strong.sum()), "edges", int(ref["edges"].sum()), "segments", ref["segs"].tolist())
    assert ref["edges"].sum() >= 100 and len(ref["segs"]) >= 1
    # ... so clearing the corners in FRONT of the hysteresis leaves nothing: every edge of the finished map was promoted from the corner
    both = _canny(lo, name, low, high)
    assert both.sum() > strong.sum() and not (ref["edges"] & strong).any()


def _groups():
    return dict(length=lc.LENGTH_SETTINGS, dist=lc.DIST_SETTINGS, min_len=("min100", "len5_min0", "len5_min12"), combined=("combined", "len8_min0"))


@pytest.mark.parametrize("setting", [s for g in _groups().values() for s in g])
def test_setting_moves_the_result_somewhere(lo, setting):
    images = [im for im, s in lc.CASES if s == setting]
    assert images
    moved = [im for im in images if not _same(lc.reference(lo, im, setting)["segs"], lc.reference(lo, im, "shipped")["segs"])]
    print(setting, "moves", len(moved), "of", len(images))
    assert moved, images
    assert any(len(lc.reference(lo, im, setting)["segs"]) > 0 for im in images)


def test_minimum_length_below_the_length_threshold(lo):
    """A minimum length of 0 or 12 px next to the shipped length threshold changes nothing (FastLineDetector drops what is shorter than 20
    half-resolution pixels itself): those cases hold the device to the shipped result.  Next to a length threshold of 5 the three values
    0, 12 and 40 give three different results somewhere."""
    for im, s in lc.CASES:
        if s in ("min0", "min12"):
            assert _same(lc.reference(lo, im, s)["segs"], lc.reference(lo, im, "shipped")["segs"]), (im, s)
    images = [im for im, s in lc.CASES if s == "len5_min12"]
    n = {im: [len(lc.reference(lo, im, s)["segs"]) for s in ("len5_min0", "len5_min12", "len5")] for im in images}
    print(n)
    assert any(a > b > c for a, b, c in n.values()), n


@pytest.mark.parametrize("setting", ["len5", "len8"])
def test_short_lengths_keep_chains_and_components_the_shipped_min_px_drops(lo, setting):
    length = lc.SETTINGS[setting]["length"]
    short_chain = small_comp = 0
    for im in [im for im, s in lc.CASES if s == setting]:
        ref = lc.reference(lo, im, setting)
        short_chain += sum(1 for c in ref["chains"] if len(c) < 21)
        lab, n_lab = ndimage.label(ref["edges"], structure=_EIGHT)
        sizes = np.bincount(lab.ravel())[1:]
        small_comp += int(((sizes >= length + 1) & (sizes <= 20)).sum())
    print(setting, "kept chains shorter than 21 points:", short_chain, "components of", length + 1, "to 20 pixels:", small_comp)
    assert short_chain >= 1 and small_comp >= 1


def test_len60_drops_most_chains(lo):
    n60 = n20 = 0
    for im in [im for im, s in lc.CASES if s == "len60"]:
        a, b = len(lc.reference(lo, im, "len60")["chains"]), len(lc.reference(lo, im, "shipped")["chains"])
        assert a <= b, im
        n60, n20 = n60 + a, n20 + b
    print("kept chains at 60:", n60, "at 20:", n20)
    assert 0 < n60 < n20 / 2


@pytest.mark.parametrize("image_name,setting", lc.CASES, ids=lc.CASE_IDS)
def test_case_fits_the_device_and_the_restatement_is_the_oracle(lo, image_name, setting):
    """fewer than 4096 segments and chains (kChainCap, the cap of detect_lines); the restated edge map is the one the oracle's
    FastLineDetector walks, and the restated walk keeps a chain for every chain the oracle grows segments on"""
    ref = lc.reference(lo, image_name, setting)
    length, dist, c1, c2, min_len = lc.oracle_args(setting)
    assert len(ref["segs"]) < lc.CHAIN_CAP and len(ref["chains"]) < lc.CHAIN_CAP, (len(ref["segs"]), len(ref["chains"]))
    segs, edges = lo.fld(lo.resize_half(lc.image(image_name)), length, dist, c1, c2, cap=2 * lc.CHAIN_CAP, want_edges=True)
    assert np.array_equal(edges != 0, ref["edges"])
    if len(segs):
        assert len(ref["chains"]) >= 1
    # the final filter: the kept segments are the detector's, doubled, longer than min_len
    full = segs * np.float32(2)
    keep = (full[:, 2] - full[:, 0]) ** 2 + (full[:, 3] - full[:, 1]) ** 2 > np.float32(min_len) * np.float32(min_len)
    assert _same(full[keep], ref["segs"])
