"""CPU proof that the RANSAC case matrix (tests/ransac_cases.py) is not vacuous: on the oracle alone, every case runs, its trace shows
the branch or exit the case names, and the iteration count and the inliers are the ones written down.  tests/test_gpu_ransac.py then
holds the device to the oracle on the same cases."""
import numpy as np
import pytest

import oracle_lib
import ransac_cases
from oracle_lib import RANSAC_TRACE

CASES = ransac_cases.cases()
CUBIC_EXITS = ("c1_zero", "linear", "quad_neg", "quad", "three", "double", "one")


@pytest.fixture(scope="module")
def fo():
    return oracle_lib.load_front()


@pytest.fixture(scope="module")
def runs(fo):
    """every case once through the traced gate and once through the traced per-hypothesis export"""
    out = {}
    for c in CASES:
        gate = fo.ransac_traced(c["m1"], c["m2"], c["thr"], c["conf"], c["max_iters"], c["seed"])
        hyp = fo.ransac_hypotheses_traced(c["m1"], c["m2"], c["thr"], c["seed"], ransac_cases.nhyp(c))
        out[c["name"]] = gate, hyp
    return out


def test_two_view_recipe_is_the_one_the_front_end_test_used():
    """the recipe moved here from test_gpu_frontend.py: same draws in the same order (first and last numbers of one set)"""
    m1, m2 = ransac_cases.two_view(40, 4, 5)
    assert m1.dtype == m2.dtype == np.float32 and m1.shape == m2.shape == (40, 2)
    rng = np.random.default_rng(4)
    X = np.column_stack([rng.uniform(-4, 4, 40), rng.uniform(-3, 3, 40), rng.uniform(4, 12, 40)])
    noise = rng.normal(0, 0.3 / 458, (40, 2))
    assert np.array_equal(m1, (X[:, :2] / X[:, 2:] + noise).astype(np.float32))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_does_what_it_says(runs, case):
    (mask, good, iters, tr), _ = runs[case["name"]]
    n = len(case["m1"])
    assert case["iters"] is not None, "a case states its iteration count"
    assert iters == case["iters"], (iters, tr)
    if case["inliers"] is not None:
        assert good == case["inliers"]
    assert int(mask.sum()) == good and (good == 0 or good >= 7)
    for slot in case["reach"]:
        assert tr[slot] > 0, (slot, tr)
    for slot in case["never"]:
        assert tr[slot] == 0, (slot, tr)
    for slot, v in case["trace"].items():
        assert tr[slot] == v, (slot, tr)
    # the trace adds up: one cubic exit per hypothesis that got a subset and passed the rank test
    assert tr["hypotheses"] == iters and (n > 7 or iters == 1)
    assert sum(tr[k] for k in CUBIC_EXITS) == tr["hypotheses"] - tr["no_subset"] - tr["rank_fail"]
    assert (tr["rank_step"] >= 0) == (tr["rank_fail"] > 0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hypothesis_export_agrees_with_the_gate(runs, case):
    """orc_ransac_hypotheses is the loop's own body: replaying RANSACPointSetRegistrator::run over its counts gives the gate's answer"""
    (mask, good, iters, _), (F, nm, cnt, tr) = runs[case["name"]]
    n, nh = len(case["m1"]), ransac_cases.nhyp(case)
    assert tr["hypotheses"] == nh
    assert ((cnt >= 0).sum(axis=1) == nm).all() and (np.sort(cnt >= 0, axis=1)[:, ::-1] == (cnt >= 0)).all()
    assert (F.reshape(nh, 3, 9)[np.arange(3)[None, :] >= nm[:, None]] == 0).all()
    if case["max_iters"] > nh:
        return          # (a cap above the export's: the replay below would run out of hypotheses)
    best, niters, it, bestF = 0, (1 if n == 7 else case["max_iters"]), 0, None
    while it < niters:
        for k in range(nm[it]):
            if cnt[it, k] > max(best, 6):
                best, bestF = int(cnt[it, k]), F[it, k]
                niters = _update_iters(case["conf"], (n - best) / n, niters)
        it += 1
    assert (best, it) == (good, iters)
    assert (bestF is None) == (good == 0)


def _update_iters(p, ep, max_iters):
    """cv::RANSACUpdateNumIters for seven model points"""
    import math
    tiny = np.finfo(np.float64).tiny
    num = max(1.0 - min(max(p, 0.0), 1.0), tiny)
    denom = 1.0 - (1.0 - min(max(ep, 0.0), 1.0)) ** 7
    if denom < tiny:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(np.rint(num / denom))


def test_every_named_branch_is_reached_somewhere(runs):
    """each slot of the trace, over all cases: reached, except the two the case file names as unreached within its search budget"""
    total = dict.fromkeys(RANSAC_TRACE, 0)
    for gate, hyp in runs.values():
        for k in RANSAC_TRACE:
            if k != "rank_step":
                total[k] += gate[3][k] + hyp[3][k]
    unreached = sorted(k for k, v in total.items() if v == 0 and k != "rank_step")
    assert unreached == ["nonfinite", "xr_clamp"], total
    assert "never reached" in ransac_cases.SEARCHED


def test_matrix_covers_the_sizes_stops_and_settings():
    names = {c["name"] for c in CASES}
    for n in (7, 8, 9, 10, 12, 63, 64, 65, 511, 512, 513, 600, 1100):
        c = next(c for c in CASES if c["name"] == f"size-{n}")
        assert len(c["m1"]) == n
    assert {c["iters"] for c in CASES if c["name"].startswith("stop-")} >= {1, 64, 65, 127, 128, 129, 1000}
    assert any(1 < c["iters"] <= 63 for c in CASES if c["name"].startswith("stop-"))
    assert {c["max_iters"] for c in CASES if c["name"].startswith("cap-")} == {1, 2, 63, 64, 65, 128, 129, 2000}
    assert {c["conf"] for c in CASES if c["name"].startswith("conf-")} == {0.0, 0.5, 0.99, 0.999999, 1.0}
    assert next(c for c in CASES if c["name"] == "conf-0.0")["iters"] == 1        # stops after one hypothesis
    assert next(c for c in CASES if c["name"] == "conf-1.0")["iters"] == 1000     # never stops
    for branch in ("c1_zero", "linear", "quad", "double", "f8_zero"):
        assert sum(c["name"].startswith(f"crafted-{branch}-") for c in CASES) >= 5, branch
    assert {"identical", "grid-shift", "one-line", "nan-rows", "thr-0", "thr-10-noiseless", "outliers-90"} <= names


def test_slot_tie_cases_tie(runs):
    """the hypothesis that wins has two models with the winning count, and no earlier one reaches it"""
    ties = [c for c in CASES if c["name"].startswith("slot-tie-")]
    assert len(ties) >= 3
    for c in ties:
        (mask, good, iters, _), (F, nm, cnt, _) = runs[c["name"]]
        first = int(np.flatnonzero((cnt[:iters] == good).any(axis=1))[0])
        assert cnt[:iters].max() == good and (cnt[first] == good).sum() >= 2, (c["name"], cnt[first])


def test_degenerate_outcomes(runs):
    """what the oracle does where the geometry gives out: identical images and a pure shift lose every track (rank 6, all 1000
    hypotheses fail the rank test at the last elimination step); 1e-4 px of noise and the first hypothesis takes all 250 points; points
    on one line never get a subset; counts below seven never become a mask"""
    for name in ("identical", "grid-shift"):
        (mask, good, iters, tr), (F, nm, cnt, _) = runs[name]
        assert (good, iters, int(mask.sum())) == (0, 1000, 0)
        assert tr["rank_fail"] == 1000 and tr["rank_step"] == 6 and (nm == 0).all() and (cnt == -1).all()
    for name in ("identical-noise-1e-4", "identical-noise-0.05"):
        (mask, good, iters, tr), _ = runs[name]
        assert (good, iters) == (250, 1) and mask.all()
    (mask, good, iters, tr), (F, nm, cnt, _) = runs["one-line"]
    assert (good, iters) == (0, 1000) and tr["no_subset"] == 1000 and tr["retry"] == 16000 and (nm == 0).all()
    (mask, good, iters, tr), (F, nm, cnt, _) = runs["thr-tiny"]
    assert good == 0 and not mask.any() and 1 <= cnt.max() <= 6
    (mask, good, iters, tr), (F, nm, cnt, _) = runs["thr-0"]
    assert good == 0 and not mask.any() and iters == 1000
    (mask, good, iters, tr), _ = runs["thr-10-noiseless"]
    assert (good, iters) == (100, 1) and mask.all()
    (mask, good, iters, tr), (F, nm, cnt, _) = runs["nan-rows"]
    assert not mask[::9].any() and np.isfinite(F).all()
