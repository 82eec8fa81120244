"""The corner detector on the GPU, held to the oracle on the case matrix of tests/detect_cases.py: fast_tiles_kernel, fast_topk_kernel
and subpix_kernel behind det_pre / det_launch / det_post, through Context.perform_detection.  Positions are compared bit for bit, ids
and the id counter must be equal (FAST scores, suppression, top-k and the id assignment are integer-exact; the sub-pixel refinement
adds its sums up in raster order on both sides).

What this module found.  With 4096 keys per cell the library dropped every further local maximum in the order the atomics arrived:
on the commit before, the four `overflow` cases, test_overflow_is_stable_from_run_to_run and
test_nothing_is_left_dirty_between_frames failed (92 .. 97 points where the oracle has 96 .. 101, other points on other runs), near_cap
passed.  Now every maximum a cell can hold is stored (fast_cell_bound keys per cell in global memory) and a cell with more than 4096
of them selects its nfg largest keys by radix from the stored list before the usual ranking; a cell that counts more than was stored
ends the call in PLV_E_CAPACITY (det_check, also for a detection started ahead of time).  Storage is the cell's own upper bound, so
that refusal needs a counter that did not start at zero: the mutation "counter reset removed" below is what reaches it.

Twelve one-line mutations of csrc/detect_kernels.hip (comparisons and arithmetic only: no index, bound or size changes), each built
into a library of its own on a scratch copy and run once on the MI355X against this module and against the three files the suite had
before (test_gpu_detect.py, test_gpu_tracker.py, test_gpu_frontend.py):

  mutation                                                              caught here by (first of N failing tests)           before
  fast_tiles_kernel   suppression q[1] >= s -> q[1] > s                 test_case_matches_the_oracle[cells-33px] (3, with   yes
                                                                        seam_mirror-x)
  fast_tiles_kernel   key: raster order reversed (idx for ~idx)         test_case_matches_the_oracle[all_ties-0] (29)       yes
  fast_topk_kernel    cut-off: score >= cut -> score > cut              test_case_matches_the_oracle[all_ties-0] (9+)       (*)
  fast_topk_kernel    box test in x: <= min_px_dist -> <                test_case_matches_the_oracle[boxes] (2)             yes
  fast_topk_kernel    box test in y: <= min_px_dist -> <                test_case_matches_the_oracle[boxes] (1)             yes
  fast_topk_kernel    mask > 127 -> mask > 128                          test_case_matches_the_oracle[boxes] (1)             no
  fast_topk_kernel    cand_n[cell] = 0 removed                          test_case_matches_the_oracle[all_ties-0] (29)       one test
  fast_topk_kernel    selection: k < prefix -> k <= prefix              test_case_matches_the_oracle[all_ties-big] (7)      no
  fast_topk_kernel    selection: want -= above removed                  none: equivalent (**)                               no
  subpix_kernel       revert test removed                               test_case_matches_the_oracle[boxes] (22)            yes
  subpix_kernel       left-the-image break removed                      test_case_matches_the_oracle[subpix_exits] (1)      no
  fast_score_lds      a <= thr -> a < thr                               test_case_matches_the_oracle[thr-equal] (1)         no

(*) The cut-off mutant leaves the slots of the ranks it drops unwritten.  Their valid flag then held what the freshly allocated buffer
held, subpix_kernel refined such a slot from a stale position, and the run ended in a device fault in cells-remainder, the tenth case
(nine had failed by assertion before it; what the older files would have said was lost with the run).  fast_topk_kernel now clears
the valid flag of every slot of its cell before it ranks, so a slot is valid only if this launch wrote it; the mutant, rebuilt, then
fails cells-remainder by assertion (56 points for 61).  The unmutated library never faulted.
(**) Without the subtraction the selection keeps the `above` keys of higher bytes on top of the nfg it wants; the ranking behind it
takes any survivor list up to 4096 keys and ranks it exactly, so the result is the same, a little later.

The threshold mutant passed the whole matrix at first (a pixel exactly at the threshold fails the kernel's cheap pre-test unless its
compass pixels are stronger); the case thr-equal was added for it.

The `det` break of subpix_kernel is not reached by any case (module docstring of detect_cases.py says why); every other exit is.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import detect_cases as dc
import synth

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in dc.gpu_cases()}


def _context(pkg, case):
    h, w = case.img.shape
    cfg = pkg.default_config(w, h)
    cfg.histogram_method = dc.PLV_HIST_NONE
    cfg.num_features, cfg.grid_x, cfg.grid_y = case.num_features, case.grid_x, case.grid_y
    cfg.min_px_dist, cfg.fast_threshold = case.min_px_dist, case.fast_threshold
    return pkg.Context(cfg)


@functools.lru_cache(maxsize=None)
def _expected(name):
    return dc.run_oracle(CASES[name])


def _same(got, want):
    assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]))
    assert np.array_equal(got[1], want[1]) and got[2] == want[2], (got[2], want[2])
    bad = np.flatnonzero((got[0].view(np.uint32) != want[0].view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], got[0][bad[:5]], want[0][bad[:5]])


def _detect(c, case):
    c.feed_image(case.img)
    return c.perform_detection(0, case.pts, case.ids, case.currid, mask=case.mask, cap=case.cap)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_the_oracle(pkg, name):
    case = CASES[name]
    c = _context(pkg, case)
    c.feed_image(case.img)
    before = pkg.counters()["launches"]
    got = c.perform_detection(0, case.pts, case.ids, case.currid, mask=case.mask, cap=case.cap)
    launched = pkg.counters()["launches"] - before
    if name == "cells-6px":         # cells below 7 pixels have no admissible pixel: nothing is detected and no kernel is launched for it
        assert launched == 0 and len(got[0]) == 0 and got[2] == case.currid
    else:
        assert launched > 0
    _same(got, _expected(name))
    if name == "none":
        assert got[2] == case.currid and len(got[0]) == 3
    if name == "cap_cut":
        assert len(got[0]) == case.cap
    # the same image again in the same context: nothing of the first call is left behind
    _same(c.perform_detection(0, case.pts, case.ids, case.currid, mask=case.mask, cap=case.cap), _expected(name))
    c.close()


def test_overflow_is_stable_from_run_to_run(pkg):
    """a cell with more keys than the staged list: which keys arrive first differs from launch to launch, the result may not"""
    case = CASES["overflow-320x240-1x1"]
    c = _context(pkg, case)
    for _ in range(4):
        _same(_detect(c, case), _expected(case.name))
    c.close()


def test_nothing_is_left_dirty_between_frames(pkg):
    """overflow, then all ties, then an ordinary texture, then overflow again, in ONE context (320x240, one cell, 101 slots): a
    candidate counter or a buffer left dirty by one frame shows in the next"""
    over = CASES["overflow-320x240-1x1"]
    ties = over._replace(name="ties-320x240", img=dc.lattice(320, 240, 3))
    tex = over._replace(name="texture-320x240", img=synth.render_frame(synth.texture_canvas(320, 240, seed=5), 320, 240))
    assert len(dc.cell_keypoints(ties, 0, 0)[0]) > 4096 and 101 < len(dc.cell_keypoints(tex, 0, 0)[0]) < 4096
    c = _context(pkg, over)
    for case in (over, ties, tex, over, tex, ties):
        _same(_detect(c, case), dc.run_oracle(case))
    c.close()


def test_too_many_slots_per_cell_are_refused_untouched(pkg):
    """2001 slots per cell do not fit fast_topk_kernel's winner list: the call is refused on the host (launch_fast_cells, before a
    kernel is launched) with PLV_E_CAPACITY and a message; points, ids and the id counter stay as they were"""
    case = CASES["thr1"]._replace(num_features=2000, grid_x=1, grid_y=1)
    c = _context(pkg, case)
    c.feed_image(case.img)
    P = np.full((4200, 2), 7.5, np.float32)
    I = np.full(4200, 99, np.uint64)
    P[:2] = [[30.0, 30.0], [60.0, 50.0]]
    I[:2] = [4, 5]
    P0, I0 = P.copy(), I.copy()
    cid, n_out = C.c_uint64(17), C.c_int(-1)
    before = pkg.counters()["launches"]
    rc = c.lib.plv_perform_detection(c.h, 0, None, P.ctypes.data_as(C.POINTER(C.c_float)), I.ctypes.data_as(C.POINTER(C.c_uint64)), 2, 4200,
                                     C.byref(cid), C.byref(n_out))
    assert rc == pkg.PLV_E_CAPACITY and b"FAST" in c.lib.plv_last_error()
    assert pkg.counters()["launches"] == before
    assert np.array_equal(P, P0) and np.array_equal(I, I0) and cid.value == 17 and n_out.value == -1
    c.close()
