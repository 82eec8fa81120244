"""What the case matrix of the blocked factorisation (tests/chol_cases.py) must contain, asserted without a GPU: no case of
tests/test_gpu_blocked_chol.py can pass vacuously — the widths reach every (instantiation, tile count) pair, more rows are accepted
than there are columns, the dependent columns give dead pivots and nothing else does, the factor form stays below its hand-over, the
not-PSD constructions fail at the pivot they name, the chi2 systems are conditioned well enough for their tolerance, and the CPU
oracle alone is inside every floor the device comparison uses.  Where a case's outcome has a second cause besides the one it is
there for (section 3's "block" construction), the test below says so and says what the device test asserts instead."""
import numpy as np
import pytest

import chol_cases as cc

FLOOR = 1e-9           # the default route's stated agreement (test_gpu_update_hard.py): floor of sections 1 and 5
FLOOR_FACTOR = 1e-8    # the factor form's (test_replay_captured_batches_in_the_factor_form): floor of section 2
CHI2_RTOL = 1e-9       # test_chi2_batch_parity


def _pair(size):
    """(NT, tiles) from the launch thresholds, restated: launch_bchol_ekf / launch_bchol_prior in csrc/blocked_chol.hip"""
    nt = 2 if size <= 32 else 4 if size <= 64 else 7 if size <= 112 else 8 if size <= 128 else 10 if size <= 160 else 12
    return nt, -(-size // 16)


def test_widths_reach_every_instantiation_and_tile_count():
    want = {(2, 1), (2, 2), (4, 3), (4, 4), (7, 5), (7, 6), (7, 7), (8, 8), (10, 9), (10, 10), (12, 11), (12, 12)}
    got = {}
    for k in cc.WHITENED_K:
        got.setdefault(_pair(k), []).append(k)
        assert cc.launch_nt(k) == _pair(k)[0] and cc.tiles(k) == _pair(k)[1]
    assert set(got) == want and len(cc.WHITENED_K) == len(set(cc.WHITENED_K)) == 36
    for (nt, t), ks in got.items():     # one column in the last tile, one short of full, full
        assert sorted(ks) == ([3, 15, 16] if t == 1 else [16 * t - 15, 16 * t - 1, 16 * t]), (nt, t, ks)
    assert {_pair(k) for k in cc.HOUSEHOLDER_K} == {(7, 5), (12, 11)} and set(cc.HOUSEHOLDER_K) <= set(cc.WHITENED_K)
    # section 2: every instantiation with all its tiles, the last one partly filled
    assert [_pair(k) for k in cc.DEPENDENT_K] == [(2, 2), (4, 4), (7, 7), (8, 8), (10, 10), (12, 12)] and all(k % 16 == 13 for k in cc.DEPENDENT_K)
    # section 5: n + 1 border rows end a strip (n = 15, 31, 47) or start one with the residual row alone (16, 32, 48)
    assert [(n + 1) % 16 for n in cc.BORDER_N] == [0, 1, 0, 1, 0, 1]


def _check_stacked(c, floor):
    o = c["oracle"]
    assert o["rc"] == 0 and o["acc"].all() and o["n_rows"] == c["H"].shape[0] == len(c["rows"]) * cc.ROWS_PROJ
    assert o["n_rows"] > c["k"]                                   # compressed: the update factors k x k, not rows x rows
    assert len(c["rows"]) * cc.ROWS_PROJ > c["k"]                 # (what the library decides the route on: slots x rows per slot)
    assert np.abs(o["dx"]).max() > 1e-6 and cc.rel(o["P"], c["P"]) > 1e-3   # the update does something
    assert c["e_oracle"] < floor, c["e_oracle"]


@pytest.mark.parametrize("k", cc.WHITENED_K)
def test_whitened_case_conditions(k):
    c = cc.whitened_case(k)
    assert c["n"] == k + 15 and c["k"] == k
    _check_stacked(c, FLOOR)
    piv, _ = cc.unit_factor(c["P"][np.ix_(c["cols"], c["cols"])])
    assert piv.min() > cc.PLV_PRIOR_AMB          # no near or dead pivot: the whitened form, not the factor form
    print(f"k {k}: NT {_pair(k)[0]}, {_pair(k)[1]} tiles, {len(c['rows'])} features, {c['oracle']['n_rows']} rows, smallest prior pivot {piv.min():.1e}, "
          f"oracle vs restatement {c['e_oracle']:.2e}")


@pytest.mark.parametrize("k", cc.WHITENED_K)
def test_a_wrong_panel_of_either_factor_would_miss_the_bound(k):
    """The bound of section 1 put to work on the CPU: the whitened form in fp64 meets it, and with ANY single 16-column panel of the
    prior factor or of B's factor off by a relative 1e-5 it does not (the miscompilation csrc/blocked_chol.hpp records left dx off by
    1e-3).  The measurements of these cases are weaker than the prior (B's diagonal is about 1.1), so an error of the prior factor
    reaches P' and dx reduced by up to 1e-3: relative 1e-5 is what every panel still shows.  One exception, not held to anything
    here: at k = 16 t - 15 the last panel of the prior factor is a single entry, the last state's conditional standard deviation,
    and 1e-5 of it moves P' and dx by 7e-13 .. 7e-10 only (measured over the seven widths where it stays under the bound)."""
    c = cc.whitened_case(k)
    Pt, dxt = c["truth"]
    bound = max(10 * c["e_oracle"], FLOOR)
    P1, dx1 = cc.whitened_form(c)
    assert max(cc.rel(P1, Pt), cc.rel(dx1, dxt)) < bound
    for factor in ("M", "B"):
        for p in range(cc.tiles(k)):
            if factor == "M" and p == cc.tiles(k) - 1 and k % 16 == 1:
                continue
            P1, dx1 = cc.whitened_form(c, factor, p, 1e-5)
            assert max(cc.rel(P1, Pt), cc.rel(dx1, dxt)) > bound, (factor, p)


def test_information_form_is_the_gain_form():
    """the k x k restatement against the rows x rows one test_gpu_update_hard.py has used (long double both)"""
    c = cc.whitened_case(33)
    Pt, dxt = cc.truth(c["P"], c["rows"], c["Hf"], c["Hx"], c["res"], c["cols"], c["oracle"]["acc"])
    assert cc.rel(c["truth"][0], Pt) < 1e-15 and cc.rel(c["truth"][1], dxt) < 1e-15


@pytest.mark.parametrize("place", cc.DEPENDENT_PLACES)
@pytest.mark.parametrize("k", cc.DEPENDENT_K)
def test_dependent_case_conditions(k, place):
    c = cc.dependent_case(k, place)
    dep, cols, P = c["dep"], c["cols"], c["P"]
    t = cc.tiles(k)
    if place == "first_tile":
        assert dep[0] >= 6 and dep[-1] < 16
    elif place == "last_boundary":
        assert [d // 16 for d in dep] == [t - 2] * 3 + [t - 1] * 3
    else:
        assert dep == list(range(k - 6, k))
    for i, d in enumerate(dep):      # rows and columns exactly equal
        assert np.array_equal(P[cols[d]], P[cols[i]]) and np.array_equal(P[:, cols[d]], P[:, cols[i]])
    assert np.array_equal(P, P.T)
    piv, _ = cc.unit_factor(P[np.ix_(cols, cols)])
    live = np.ones(k, dtype=bool)
    live[dep] = False
    assert np.abs(piv[dep]).max() < cc.PLV_PRIOR_TAU and piv[live].min() > cc.PLV_PRIOR_AMB, (piv[dep], piv[live].min())
    lam = cc.lambda_max(P[np.ix_(cols, cols)], c["H"])
    assert lam < 0.25 * cc.PLV_WHITEN_LAMBDA_MAX, lam
    _check_stacked(c, FLOOR_FACTOR)
    print(f"k {k} {place}: dead pivots at {dep[0]} .. {dep[-1]} (|pivot| <= {np.abs(piv[dep]).max():.1e}), smallest live one {piv[live].min():.1e}, sigma x {c['sigma']:g}, "
          f"largest diagonal entry of B {lam:.3g}, oracle vs restatement {c['e_oracle']:.2e}")


@pytest.mark.parametrize("n", cc.BORDER_N)
def test_border_case_conditions(n):
    c = cc.whitened_case(n - 3, n)
    assert c["n"] == n and c["k"] == n - 3
    _check_stacked(c, FLOOR)
    e = cc.border_ekf_case(n)
    assert e["oracle"]["rc"] == 0 and e["H"].shape == (10, n - 3) and e["e_oracle"] < FLOOR


def test_not_psd_cases_fail_where_they_say(oracle):
    """Every case names the first pivot that is not positive, and the CPU oracle rejects it.  What else would reject it: with the
    dead column dropped — the factorisation as the device carries it on — the "block" construction leaves the gain's diagonal above
    P's, so the negative-diagonal test rejects those updates too and only the library's error text tells that the factorisation
    reported them; the "noise" construction keeps the diagonal of P - K M^T positive, so an unreported pivot there would come back
    as status 0 with P changed."""
    cases = cc.not_psd_cases()
    assert {r: cc.launch_nt(r) for r in cc.NOT_PSD_R} == {20: 2, 40: 4, 100: 7, 128: 8}
    assert len(cases) == len(set(cases)) == 2 * (2 + 3 + 3 + 3)
    for r, p, pivot in cases:
        assert pivot // 16 == p and (pivot % 16 in (0, 15) or pivot in (1, r - 1))
        for how in cc.NOT_PSD_HOW:
            c = cc.not_psd_case(r, pivot, how)
            first, dmin = cc.dropped_column_diagonal(c)
            assert first == pivot, (r, pivot, how, first)
            if how == "block":
                assert dmin < -0.1, (r, pivot, dmin)
            else:
                assert dmin > 0 and np.all(np.linalg.eigvalsh(c["P"]) > 0), (r, pivot, dmin)
            rc, _, _ = oracle.ekf_update(c["P"], c["H"], c["cols"], c["res"], c["Rd"])
            assert rc == -3, (r, pivot, how, rc)
    # the first pivot of a later panel (the chain's separate first read) and the last one of a panel chosen through map7 / map8
    assert (100, 3, 48) in cases and (100, 6, 99) in cases and (128, 4, 64) in cases and (128, 7, 127) in cases


@pytest.mark.parametrize("mp_most", cc.CHI2_ROWS)
@pytest.mark.parametrize("k", cc.CHI2_K)
def test_chi2_case_conditions(k, mp_most):
    c = cc.chi2_case(k, mp_most)
    assert list(c["rows"]) == list(range(1, mp_most + 1)) and c["Hx"].shape == (mp_most, k, cc.CHI2_LD)
    assert (c["ref"] > 0).all()
    eps = np.finfo(np.float64).eps
    assert (c["rows"] * eps * c["cond"]).max() < CHI2_RTOL                 # fp64 can hold the value to the tolerance
    d = np.abs(c["oracle"] - c["ref"])
    assert (d <= CHI2_RTOL * c["ref"]).all() and (d <= cc.chi2_bound(c)).all()
    print(f"k {k}, 1 .. {mp_most} rows: chi2 {c['ref'].min():.3g} .. {c['ref'].max():.3g}, cond(S) up to {c['cond'].max():.3g}, oracle vs restatement "
          f"{(d / c['ref']).max():.2e}")
