"""Column order of the stacked Jacobians without a device: plv_jacobian_columns and plv_line_jacobian_columns take no context
(host-side integer logic only), so the order of the point and of the line batch is held against the oracle here, on the scenes of
the GPU parity tests (test_gpu_jacobian.py, test_gpu_lines.py), together with the capacity and argument errors."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import synth


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


def _columns(pkg, fn, st, tr, cap):
    """(status, columns) of plv_jacobian_columns / plv_line_jacobian_columns with room for cap columns"""
    cols = np.full(max(cap, 1), -7, dtype=np.int32)
    k = C.c_int(-1)
    rc = getattr(pkg.load_library(), fn)(C.byref(st.c), C.byref(tr.c), cols.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(k))
    return rc, cols[:max(k.value, 0)].copy()


@pytest.mark.parametrize("kw,k", [(dict(), 98), (dict(obs_offset=0.017), 98), (dict(n_clones=20, F=150, M=20), 128),
                                  (dict(n_clones=6, F=5, M=4), 44)])
def test_point_columns_equal_the_oracle(pkg, jo, kw, k):
    sc = synth.vio_scene(**kw)
    extra = dict(use_pol_cov=1, intr_ori_cov=1e-6, intr_pos_cov=1e-6) if "obs_offset" in kw else {}
    st, tr = synth.scene_views(pkg, sc, **extra)
    rc, cols = _columns(pkg, "plv_jacobian_columns", st, tr, 1024)
    assert rc == 0 and len(cols) == k
    assert np.array_equal(cols, jo.columns(st, tr))
    assert _columns(pkg, "plv_jacobian_columns", st, tr, k)[0] == 0
    assert _columns(pkg, "plv_jacobian_columns", st, tr, k - 1)[0] == pkg.PLV_E_CAPACITY


def _variant_scene(pkg):
    """the views of test_build_jacobians_variants: every calibration block has columns, one observation has no bounding clones"""
    sc = synth.vio_scene(n_clones=10, F=12, M=8, obs_offset=0.011)
    sc["obs_time"] = sc["obs_time"].copy()
    sc["obs_time"][3] = sc["t"][0] - 5.0
    st = pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], sc["R_ItoC"], sc["p_IinC"], sc["K8"], intrinsic_state_id=15,
                       extrinsic_state_id=sc["n_state"], dt_state_id=sc["n_state"] + 6, cam_dt=0.003, sigma_pix=1.0,
                       use_pol_cov=1, intr_ori_cov=1e-6, intr_pos_cov=1e-6, feat_rep=1)
    return sc, st, pkg.Tracks(sc["obs_ptr"], sc["obs_time"], sc["obs_uv"], sc["pts"])


def test_point_columns_with_calibration_blocks(pkg, jo):
    sc, st, tr = _variant_scene(pkg)
    rc, cols = _columns(pkg, "plv_jacobian_columns", st, tr, 1024)
    assert rc == 0 and len(cols) == 6 + 8 + 1 + 54   # clone 0 is never interpolated over
    assert np.array_equal(cols, jo.columns(st, tr))
    n = sc["n_state"]
    assert np.array_equal(cols[:15], np.r_[n:n + 6, 15:23, n + 6])   # extrinsics, intrinsics, time offset lead
    assert _columns(pkg, "plv_jacobian_columns", st, tr, len(cols) - 1)[0] == pkg.PLV_E_CAPACITY


def _line_scene(pkg, calib_dt, fej_noise, offset, pol):
    sc = synth.vio_scene(F=4, calib_int=True, fej_noise=fej_noise, obs_offset=offset)
    ls = synth.line_scene(sc, L=80, noise_px=0.7)
    ls["obs_time"] = ls["obs_time"] + np.where(ls["obs_time"] < sc["t"][-1], offset, 0.0)
    st, _ = synth.scene_views(pkg, sc, use_pol_cov=pol, intr_ori_cov=1e-5, intr_pos_cov=2e-5, dt_state_id=14 if calib_dt else -1)
    return st, pkg.LineTracks(ls["obs_ptr"], ls["obs_time"], ls["seg_uv"], seg_uvn=ls["seg_uvn"], line_FinG=ls["lines"])


@pytest.mark.parametrize("calib_dt,fej_noise,offset,pol", [(False, 0.0, 0.0, 0), (True, 1e-3, 0.013, 1), (False, 2e-3, 0.02, 1)])
def test_line_columns_equal_the_oracle(pkg, jo, calib_dt, fej_noise, offset, pol):
    st, lt = _line_scene(pkg, calib_dt, fej_noise, offset, pol)
    rc, cols = _columns(pkg, "plv_line_jacobian_columns", st, lt, 512)
    assert rc == 0 and len(cols) == 90 + (1 if calib_dt else 0)
    assert np.array_equal(cols, jo.line_columns(st, lt))
    if calib_dt:
        assert cols[24] == 14 and 14 not in cols[:24]   # the time offset follows the first window's four poses
    assert _columns(pkg, "plv_line_jacobian_columns", st, lt, len(cols))[0] == 0
    assert _columns(pkg, "plv_line_jacobian_columns", st, lt, len(cols) - 1)[0] == pkg.PLV_E_CAPACITY


@pytest.mark.parametrize("fn,prefix", [("plv_jacobian_columns", "jacobians: "), ("plv_line_jacobian_columns", "line jacobians: ")])
def test_bad_views_are_refused_with_the_callers_prefix(pkg, fn, prefix):
    lines = fn == "plv_line_jacobian_columns"

    def views():
        return _line_scene(pkg, False, 0.0, 0.0, 0) if lines else _variant_scene(pkg)[1:]

    last_error = lambda: pkg.load_library().plv_last_error().decode()
    st, tr = views()
    st.c.clone_time = None
    assert _columns(pkg, fn, st, tr, 1024)[0] == pkg.PLV_E_BADARG
    assert last_error() == prefix + "null view field"
    st, tr = views()
    st.c.intr_order = 2
    assert _columns(pkg, fn, st, tr, 1024)[0] == pkg.PLV_E_BADARG
    assert last_error() == prefix + "only intr_order = 3 is built (got 2)"
