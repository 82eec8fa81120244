"""The restatement of the stereo point update with a CPI table (tests/stereo_cpi_ref.py) and the scene
tests/test_gpu_stereo_try_update.py holds the library to, pinned without a device: the served / unserved rule against the oracle's
pose function, and the branches the scene must reach under the restatement alone."""
import numpy as np
import pytest

import oracle_lib
import stereo_cpi_ref as scr
import stereo_update_ref as sr
import synth


@pytest.fixture(scope="module")
def jo(pkg):
    return oracle_lib.load_jac(pkg)


@pytest.fixture(scope="module")
def fo():
    return oracle_lib.load_front()


def test_served_rule_is_the_oracles(pkg, jo):
    """`servable` (times alone) == the ok of orc_cpi_poses: at records, between records of one clone, between two clones' runs, outside
    the table, and on a window that has lost the clones the records hang on"""
    sc = synth.vio_scene(n_clones=8, F=4)
    cp = scr.cut_table(synth.cpi_scene(sc), sc)
    tab = scr.table(pkg, cp)
    st, _ = synth.scene_views(pkg, sc)
    t = cp["t"]
    last_of_run = t[:-1][np.diff(cp["clone_t"]) != 0]
    tq = np.concatenate([sc["t"], t[::4], t[:-1:3] + 0.002, last_of_run + 1e-4, [t[0] - 0.01, t[-1] + 0.01, t[-1], t[0]]])
    want = jo.cpi_poses(st, tab, tq)[2]
    got = np.array([scr.servable(sc["t"], cp, x) for x in tq], np.uint8)
    assert np.array_equal(got, want) and want.any() and not want.all()
    assert not scr.servable(sc["t"], cp, sc["t"][0]) and scr.servable(sc["t"], cp, sc["t"][1])      # the cut: the oldest frame
    st2 = pkg.StateView(sc["t"][3:], sc["R"][3:], sc["p"][3:], sc["ids"][3:], sc["R_ItoC"], sc["p_IinC"], sc["K8"])
    tq2 = np.array([sc["t"][1], sc["t"][2] + 0.002, sc["t"][3], sc["t"][4] + 0.0125])
    assert [scr.servable(sc["t"][3:], cp, x) for x in tq2] == [bool(v) for v in jo.cpi_poses(st2, tab, tq2)[2]] == [False, False, True, True]


@pytest.mark.parametrize("pairing", list(sr.PAIRINGS))
def test_scene_reaches_every_branch(pkg, oracle, jo, fo, pairing):
    model0, model1 = sr.PAIRINGS[pairing]
    sc, pair, tracks, names, opt, cp = scr.update_scene(pkg, fo.undistort, model1=model1, model0=model0)
    P = synth.spd_cov(sc["n_state"], seed=4) * 1e-4
    out = scr.update_points(jo, oracle, pair, tracks, P, cp, scr.table(pkg, cp), **opt)
    plain = sr.update_points(jo, oracle, pair, tracks, P, **opt)
    # observations of each camera handed back as unserved (the oldest frame's), among the features the loop examined
    assert out["unserved"][0] >= 1 and out["unserved"][1] >= 1, out["unserved"]
    assert not (out["times"] == sc["t"][0] + pair.dt).any() and (out["times"] == sc["t"][1] + pair.dt).any()
    # a feature drops below two usable observations because of that — and is selected without the table
    assert names["two then one"] in out["below_two"], out["below_two"]
    assert out["trace"]["n_valid"][names["two then one"]] == (1, 0) and plain["trace"]["n_valid"][names["two then one"]] == (2, 0)
    # a left and a right observation of one frame share a pose
    shared = 0
    for fid, po in out["pose_of"].items():
        if 0 in po and 1 in po:
            for i, x in enumerate(out["kept_t"][fid][0]):
                for j, y in enumerate(out["kept_t"][fid][1]):
                    if x == y:
                        assert po[0][i] == po[1][j], fid
                        shared += 1
    assert shared >= 100
    assert len(out["times"]) <= 14 + 15        # (one pose per distinct time: 14 served clone times and the late observations')
    # the selection reaches the cap, the gate rejects, enough are accepted
    assert len(out["ids"]) == opt["max_msckf"] and out["status"] == 0
    assert (out["accepted"] == 0).any() and out["accepted"].sum() >= 10, out["accepted"]
    # point_used: every triangulated feature the loop examined, selected or dynamic; nothing behind the cap
    tr = out["trace"]
    assert set(out["used"]) == {fid for fid in tr["ok"] if tr["ok"][fid] and sum(tr["n_valid"][fid]) >= 2}
    assert set(int(i) for i in out["ids"]) < set(out["used"]) and names["biased"] in out["used"]
    assert len(tr["ok"]) < len(tr["order"])
    # the table changes the update: other poses, fewer rows
    assert out["n_rows"] < plain["n_rows"] and np.abs(out["dx"] - plain["dx"]).max() > 1e-6
    if model0 == sr.EQUI:  # camera 0 read as radtan: other verdicts (the argument of test_stereo_update_ref_cpu.py, with the table)
        wrong = scr.update_points(jo, oracle, sr.read_as_radtan(pair), tracks, P, cp, scr.table(pkg, cp), **opt)
        assert list(wrong["ids"]) != list(out["ids"]) or list(wrong["accepted"]) != list(out["accepted"])
