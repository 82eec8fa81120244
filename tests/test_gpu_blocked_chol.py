"""Every instantiation and exit of the blocked factorisation (csrc/blocked_chol.hpp) through the public C-ABI wrappers, held to
extended precision.  The cases are tests/chol_cases.py's (tests/test_chol_cases_cpu.py proves what they contain); the reference of
every numeric comparison is the long-double restatement there, and the CPU oracle, run beside the library on every case, is the
yardstick: the library may be ten times as far from the restatement as the oracle is, or as far as the project's stated agreement
of the route (1e-9 for the default route, 1e-8 for the factor form), whichever is larger.

  1  whitened update, route 4 asserted: bchol_prior_kernel<NT> and bchol_ekf_kernel<NT> with r = k at all twelve (NT, tiles) pairs;
     the widths of five and eleven tiles also through mode 1 (Householder compression, route 2, then bchol_ekf_kernel with r = k);
  2  six exactly dependent columns in the prior block, in the first tile, across the last tile boundary and at the end: dead pivots
     of bchol_prior_kernel, the update in the factor form.  The C ABI reports the route (4 for both forms) and not which form the
     device chose, so that it took the factor form rests on the numeric comparison: with a zero column in M the whitened form's
     W0 = M^-1 P[cols, :] has a zero row and its result is wrong by multiples of P (csrc/dense_kernels.hip "whitened update");
  3  PLV_E_NOT_PSD from the first and the last pivot of the first, a middle and the last panel of bchol_ekf_kernel<2|4|7|8>, with
     the library's error text naming the factorisation as the one that rejected, for an indefinite block of the covariance (the
     issue's construction) and for a negative noise entry, where nothing else would reject.
     bchol_ekf_kernel<10|12> only ever factor B = I + M^T G M of the whitened route (plv_ekf_update applies more than 128 rows block
     after block), which is positive definite by construction: there is no input that makes them report it, and no case here;
  4  chi2 by value at every projected row count: chi2_gate_kernel<2> (1 .. 32 rows) and <4> (1 .. 63, small systems inside the
     four-strip kernel), and the refusal of 64 rows;
  5  border strips: the residual row as the last row of a full strip and alone in a strip, through plv_ekf_update and the whitened
     route.
Every case prints one line: case, route, library vs restatement, oracle vs restatement."""
import ctypes as C

import numpy as np
import pytest

import chol_cases as cc

pytestmark = pytest.mark.gpu

FLOOR = 1e-9           # the default route's stated agreement (test_gpu_update_hard.py)
FLOOR_FACTOR = 1e-8    # the factor form's (test_replay_captured_batches_in_the_factor_form)
CHI2_RTOL = 1e-9       # test_chi2_batch_parity


def _stacked(ctx, c, label, mode, route_want, floor):
    """one stacked update with the gate open, in compression mode `mode`: section 1's assertion"""
    ctx.update_compression_mode(mode)
    try:
        rc, P1, dx1, acc, nr = ctx.msckf_update(c["P"], c["rows"], c["Hf"], c["Hx"], c["res"], c["cols"], cc.SIGMA2, 1e6, 0.0)
        _, route, _ = ctx.update_compression_mode()
    finally:
        ctx.update_compression_mode(0)
    o, (Pt, dxt) = c["oracle"], c["truth"]
    e_lib = max(cc.rel(P1, Pt), cc.rel(dx1, dxt))
    print(f"{label}: rc {rc}, route {route}, library vs restatement {e_lib:.2e}, oracle vs restatement {c['e_oracle']:.2e}, "
          f"ratio {e_lib / max(c['e_oracle'], 1e-300):.1f}")
    assert rc == 0 and o["rc"] == 0
    assert np.array_equal(acc, o["acc"]) and nr == o["n_rows"]
    assert nr > c["k"]
    assert route == route_want, route
    assert np.array_equal(P1, P1.T)
    assert e_lib < max(10 * c["e_oracle"], floor), (e_lib, c["e_oracle"])


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", cc.WHITENED_K)
def test_whitened_update_every_instantiation_and_tile_count(ctx, k):
    _stacked(ctx, cc.whitened_case(k), f"whitened k {k} NT {cc.launch_nt(k)} tiles {cc.tiles(k)}", 0, 4, FLOOR)


@pytest.mark.parametrize("k", cc.HOUSEHOLDER_K)
def test_householder_route_five_and_eleven_tiles(ctx, k):
    _stacked(ctx, cc.whitened_case(k), f"householder k {k} NT {cc.launch_nt(k)} tiles {cc.tiles(k)}", 1, 2, FLOOR)


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("place", cc.DEPENDENT_PLACES)
@pytest.mark.parametrize("k", cc.DEPENDENT_K)
def test_dead_prior_pivots_panel_by_panel(ctx, k, place):
    c = cc.dependent_case(k, place)
    _stacked(ctx, c, f"dependent k {k} NT {cc.launch_nt(k)} {place} (pivots {c['dep'][0]} .. {c['dep'][-1]})", 0, 4, FLOOR_FACTOR)


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("how", cc.NOT_PSD_HOW)
@pytest.mark.parametrize("r,panel,pivot", cc.not_psd_cases())
def test_not_psd_from_every_panel(ctx, pkg, oracle, r, panel, pivot, how):
    """plv_ekf_update returns PLV_E_NOT_PSD for either rejection, the factorisation's report (status bit 2) or a negative diagonal of
    P - K M^T (bit 1), and leaves the state alone for both.  That the FACTORISATION reported the pivot is what the error text shows:
    "S not positive definite" is chosen on bit 2.  With the "noise" construction the status alone shows it too: the diagonal test
    does not fire there (test_chol_cases_cpu.py), so an unreported pivot would return 0 and change P."""
    c = cc.not_psd_case(r, pivot, how)
    rc0, _, _ = oracle.ekf_update(c["P"], c["H"], c["cols"], c["res"], c["Rd"])
    ctx.cov_upload(c["P"])
    rc1, P1, dx1 = ctx.ekf_update(c["P"], c["H"], c["cols"], c["res"], c["Rd"])
    why = ctx.lib.plv_last_error()
    Pd = ctx.cov_download(r)
    print(f"not PSD ({how}) r {r} NT {cc.launch_nt(r)} panel {panel} pivot {pivot}: oracle {rc0}, library {rc1}, {why.decode()!r}")
    assert rc0 == -3
    assert rc1 == pkg.PLV_E_NOT_PSD
    assert b"S not positive definite" in why
    assert np.array_equal(P1, c["P"])
    assert np.all(dx1 == 0)
    assert np.array_equal(Pd, c["P"])


# ------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("mp_most", cc.CHI2_ROWS)
@pytest.mark.parametrize("k", cc.CHI2_K)
def test_chi2_by_value_at_every_row_count(ctx, k, mp_most):
    c = cc.chi2_case(k, mp_most)
    chi = ctx.chi2_batch(c["P"], c["rows"], c["Hx"], c["res"], c["cols"], cc.SIGMA2)
    ref, bound = c["ref"], cc.chi2_bound(c)
    d, d_o = np.abs(chi - ref), np.abs(c["oracle"] - ref)
    for f in range(len(ref)):
        print(f"chi2 k {k} kernel <{2 if mp_most <= 32 else 4}> rows {c['rows'][f]}: library vs restatement {d[f] / ref[f]:.2e}, oracle vs restatement "
              f"{d_o[f] / ref[f]:.2e}, bound {bound[f] / ref[f]:.2e}")
    worst = int(np.argmax(d / bound))
    print(f"chi2 k {k} kernel <{2 if mp_most <= 32 else 4}>: worst |library - restatement| / bound {d[worst] / bound[worst]:.2f} at {c['rows'][worst]} rows")
    assert np.isfinite(chi).all()
    assert (d <= bound).all(), [(int(c["rows"][f]), d[f], bound[f]) for f in np.nonzero(d > bound)[0]]
    assert (d <= CHI2_RTOL * ref).all()


def test_chi2_refuses_64_rows_and_leaves_the_output(ctx, pkg):
    c = cc.chi2_case(17, 63)
    rows = c["rows"].copy()
    rows[-1] = 64
    F, k, ld = c["Hx"].shape
    n = c["P"].shape[0]
    P = np.asfortranarray(c["P"])
    chi = np.full(F, -7.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = ctx.lib.plv_chi2_batch(ctx.h, P.ctypes.data_as(dp), n, n, F, k, ld, rows.ctypes.data_as(ip), c["Hx"].ctypes.data_as(dp), c["res"].ctypes.data_as(dp),
                                c["cols"].ctypes.data_as(ip), C.c_double(cc.SIGMA2), chi.ctypes.data_as(dp))
    assert rc == pkg.PLV_E_CAPACITY
    assert np.all(chi == -7.0)
    with pytest.raises(pkg.PlvError) as e:
        ctx.chi2_batch(c["P"], rows, c["Hx"], c["res"], c["cols"], cc.SIGMA2)
    assert e.value.code == pkg.PLV_E_CAPACITY


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("n", cc.BORDER_N)
def test_border_strips_whitened(ctx, n):
    _stacked(ctx, cc.whitened_case(n - 3, n), f"borders whitened n {n} ({n + 1} border rows) k {n - 3}", 0, 4, FLOOR)


@pytest.mark.parametrize("n", cc.BORDER_N)
def test_border_strips_ekf_update(ctx, n):
    c = cc.border_ekf_case(n)
    rc, P1, dx1 = ctx.ekf_update(c["P"], c["H"], c["cols"], c["res"], c["Rd"])
    Pt, dxt = c["truth"]
    e_lib = max(cc.rel(P1, Pt), cc.rel(dx1, dxt))
    print(f"borders ekf n {n} ({n + 1} border rows) k {n - 3} r 10: rc {rc}, route ekf_update, library vs restatement {e_lib:.2e}, oracle vs restatement "
          f"{c['e_oracle']:.2e}, ratio {e_lib / max(c['e_oracle'], 1e-300):.1f}")
    assert rc == 0 and c["oracle"]["rc"] == 0
    assert np.array_equal(P1, P1.T)
    assert e_lib < max(10 * c["e_oracle"], FLOOR), (e_lib, c["e_oracle"])
