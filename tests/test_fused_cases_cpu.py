"""What the case matrix of the fused launches (tests/fused_cases.py) must contain, asserted on the CPU oracle alone: no case of
tests/test_gpu_fused_launches.py can pass vacuously — the gate decides both ways where it should, NaN blocks sit next to healthy ones,
blocks with nothing left after the projection occur, and chi2 / the residual norm are conditioned well enough to be compared by
value (the oracle against its restatement with LAPACK's QR and numpy.linalg.solve)."""
import numpy as np
import pytest

import fused_cases as fc
import oracle_lib

S_MAX = 1e-10          # spread of chi2 / residual norm between the oracle and its restatement (measured: 4e-13 worst in the matrix,
#                        1.4e-11 worst over the one-call scenes)


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


def _nan_blocks(systems):
    _, rows, Hf, Hx, res = systems
    return np.array([np.isnan(Hf[f]).any() or np.isnan(Hx[f]).any() or np.isnan(res[f]).any() for f in range(len(rows))])


def test_every_axis_value_occurs_twice_and_the_hard_combinations_once():
    for kind, cases in fc.CASES.items():
        assert 12 <= len(cases) <= 16 and len({c.name for c in cases}) == len(cases)
        count = lambda pred: sum(1 for c in cases if pred(c))
        for shape in (fc.A, fc.B, fc.C3, fc.ONE, fc.SHORT):
            assert count(lambda c: (c.n_clones, c.F, c.M) == shape) >= 2, (kind, shape)
        for ld_extra in (0, 2):
            assert count(lambda c: c.ld_extra == ld_extra) >= 2
        for off in (0.0, 0.013, 0.037):
            assert count(lambda c: c.obs_offset == off and c.cam_dt == 0.0) >= 2, (kind, off)
        assert count(lambda c: c.cam_dt != 0.0) >= 1
        for fej in (0.0, 1e-3, 2e-3):
            assert count(lambda c: c.fej_noise == fej) >= 2, (kind, fej)
        for flag in (True, False):
            assert count(lambda c: c.calib_dt == flag) >= 2
        for noise in ("none", "pol", "imu_cov", "res_pose"):
            assert count(lambda c: c.noise == noise) >= 2, (kind, noise)
        for noise in ("pol", "imu_cov", "res_pose"):   # ... each once with off-clone times AND first estimates that differ
            assert count(lambda c: c.noise == noise and c.obs_offset > 0 and c.fej_noise > 0) >= 1, (kind, noise)
        assert all(c.obs_offset > 0 for c in cases if c.noise == "pol")
        if kind == "points":
            for flag in (True, False):
                assert count(lambda c: c.calib_ext == flag) >= 2 and count(lambda c: c.calib_intr == flag) >= 2
            assert count(lambda c: c.model == "equidistant") >= 2 and count(lambda c: c.outlier_px > 0) >= 4
            assert count(lambda c: c.outlier_px == 2.0 and c.M == 6) == 1
    assert sum(1 for c in fc.ONE_CALL_LINE_CASES if c.dt_clone == 0.5) >= 3


@pytest.mark.parametrize("case", fc.LINE_CASES + fc.POINT_CASES, ids=lambda c: f"{c.kind}-{c.name}")
def test_case_conditions(pkg, oracle, jo, case):
    b = fc.build(pkg, case)
    tr = b["tr"]
    assert len(tr.ptr) - 1 == case.F and b["ld"] == 2 * case.M + case.ld_extra
    if not b["has_oracle"]:
        # the CPU oracle has no fisheye model: the case is held to the unfused device route; here only that the scene is a fisheye one
        # (the observations are not what the radtan model makes of the same landmarks)
        assert case.model == "equidistant" and np.abs(tr.uv - fc.build(pkg, case._replace(model="radtan"))["tr"].uv).max() > 20.0
        return
    systems = fc.oracle_systems(jo, b)
    cols, rows, Hf, Hx, res = systems
    assert rows.max() <= b["ld"] and (rows.max() == 2 * case.M or case.F == 1)    # (a scene's first track is one of its shorter ones)
    up = fc.oracle_update(oracle, b, systems)
    acc = up["accepted"].astype(bool)
    assert up["rc"] == 0 and np.abs(up["dx"]).max() > 1e-6
    nan = _nan_blocks(systems)
    vo, vq = fc.gate_values_oracle(oracle, b, systems), fc.gate_values_qr(b, systems)
    reach = fc.reaches_gate(b, rows)
    s = fc.spread(vo, vq)
    print(f"{case.kind} {case.name}: k = {len(cols)}, {acc.sum()} of {case.F} accepted, {nan.sum()} NaN blocks, {(rows == b['fdim']).sum()} with rows == fdim, "
          f"chi2 {np.nanmin(vo[:, 0]):.2g} .. {np.nanmax(vo[:, 0]):.2g}, |Hx| up to {np.nanmax(np.abs(Hx)):.2g}, spread {s:.2g}")
    # the oracle's own verdicts are the ones its values give; a NaN block is NaN in the value too and is rejected
    gate = (vo[:, 0] < vo[:, 1]) & ((b["res_norm_gate"] <= 0) | (vo[:, 2] < b["res_norm_gate"]))
    assert np.array_equal(gate, acc) and np.array_equal(np.isnan(vo[:, 0]), ~reach | nan) and not acc[nan].any()
    assert s < S_MAX, s
    if case.F > 1:
        assert acc.sum() >= 0.5 * case.F
    else:
        assert acc.sum() == 1
    if case.kind == "points" and case.outlier_px > 0:
        assert (~acc).sum() >= 0.1 * case.F and b["outlier"].sum() >= 0.1 * case.F
        if case.outlier_px == 2.0:     # verdicts near the threshold: some of the noisy tracks pass
            assert 0 < (acc & b["outlier"]).sum() < b["outlier"].sum()
    if case.kind == "lines" and case.noise == "pol":
        assert 0.10 * case.F <= nan.sum() <= 0.40 * case.F, nan.sum()
    if case.kind == "lines" and case.noise == "imu_cov":
        assert 0.10 * case.F <= nan.sum() <= 0.40 * case.F, nan.sum()
    if case.kind == "lines" and (case.n_clones, case.F, case.M) == fc.SHORT:
        assert (rows == b["fdim"]).sum() >= 1 and not acc[rows == b["fdim"]].any()
    if case.fej_noise > 0:
        assert np.abs(b["st"].Rf - b["st"].R).max() > 1e-4
    if case.calib_dt:
        assert b["st"].c.dt_state_id in list(cols)


@pytest.mark.parametrize("case", fc.ONE_CALL_LINE_CASES + fc.ONE_CALL_POINT_CASES, ids=lambda c: f"{c.kind}-{c.name}")
def test_one_call_scene_conditions(pkg, oracle, jo, case):
    """The scenes of the one-call entry points: the compiled CPU frame's recorded values are the ones the oracle's pieces give on the
    batch rebuilt from its outputs (so the spread measured on that batch is the spread of what the device is compared with), enough
    features reach the gate, and for lines the anchored triangulation (D > 0 and a point) and the plane-pair one both occur."""
    fo = oracle_lib.load_front()
    b = fc.build(pkg, case)
    tracks, used = fc.one_call_tracks(b, fo.undistort)
    r = fc.one_call_oracle(pkg, b, tracks, used)
    out = r["out"]
    assert out["status"] == 0 and len(out["ids"]) >= 15 and out["accepted"].sum() >= 3 and np.abs(out["dx"]).max() > 1e-6
    b2, systems = fc.one_call_systems(pkg, jo, b, tracks, out)
    vo, vq = fc.gate_values_oracle(oracle, b2, systems), fc.gate_values_qr(b2, systems)
    pos = {int(i): q for q, i in enumerate(r["ids"])}
    fv = np.array([r["vals"][pos[int(i)]] for i in out["ids"]])
    if case.kind == "points":
        fv = fv[:, [8, 9, 10]]
    assert np.array_equal(fv[:, 1], vo[:, 1]) and fc.rel_diff(fv[:, 0], vo[:, 0]) < 1e-12 and fc.rel_diff(fv[:, 2], vo[:, 2]) < 1e-12
    s = fc.spread(vo, vq)
    print(f"{case.kind} {case.name}: pool {out['n_pool']}, {len(out['ids'])} at the gate, {out['accepted'].sum()} accepted, chi2 {np.nanmin(vo[:, 0]):.2g} .. "
          f"{np.nanmax(vo[:, 0]):.2g}, spread {s:.2g}")
    assert s < S_MAX, s
    if case.kind == "lines":
        anchored = [int(i) for i in out["ids"] if tracks[int(i)][3] > 0 and tracks[int(i)][4][1] in used]
        assert len(anchored) >= 3 and len(out["ids"]) - len(anchored) >= 5
    elif case.outlier_px == 2.0:
        assert 0 < out["accepted"].sum() < len(out["ids"])
