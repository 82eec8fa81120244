"""The zero-velocity updater inside the driver: one short rendered drive (752 x 480, the replay tests' size) that drives, brakes to
a stop, stands for two seconds and pulls away, with wheels, replayed with `zupt.enabled` and without it.  The speed profile and the
sensor noise of the frames are this file's own, installed over synth_dataset.arc / Renderer.render for the duration of the fixture."""
import importlib
import os

import numpy as np
import pytest

import synth_dataset as sd

# 2 m/s; braking at 2 m/s^2 from T_BRAKE to T_STOP, standing until T_GO, pulling away at 2 m/s^2 for T_PULL.  Frames are stamped
# x.x517 and the encoders x.xx31: the window that holds the stop and the one that holds the start hold encoder samples of 0.09 m/s
# and more, so the wheels veto them.
V0, T_BRAKE, T_STOP, T_GO, T_PULL, SECONDS = 2.0, 1.81, 2.81, 4.79, 1.0, 6.6
MAX_WHEEL_SPEED, MAX_VELOCITY = 0.05, 1.0                                    # the defaults of zupt.max_wheel_speed / max_velocity


def stop_and_go(t):
    """arc length and speed: V0, a constant deceleration to a stop, standing (speed exactly 0), a constant acceleration back to V0"""
    x = np.asarray(t, dtype=np.float64)
    b, p = T_STOP - T_BRAKE, T_PULL
    ub, up = np.clip((x - T_BRAKE) / b, 0.0, 1.0), np.clip((x - T_GO) / p, 0.0, 1.0)
    s = V0 * np.minimum(x, T_BRAKE) + V0 * b * (ub - 0.5 * ub * ub) + 0.5 * V0 * p * up * up + V0 * np.maximum(x - T_GO - p, 0.0)
    v = np.where(x < T_BRAKE, V0, np.where(x < T_STOP, V0 * (1 - ub), np.where(x < T_GO, 0.0, np.where(x < T_GO + p, V0 * up, V0))))
    return (float(s), float(v)) if np.ndim(t) == 0 else (s, v)


def noisy_render(render, sigma=1.5):
    """Renderer.render with independent sensor noise on every frame (sigma grey levels, seeded by the frame's time): two frames of a
    standing camera are never the same image"""
    def f(self, t):
        img = render(self, t).astype(np.float64)
        rng = np.random.default_rng(int(round(float(t) * 1e6)))
        return np.clip(np.rint(img + rng.normal(0.0, sigma, img.shape)), 0, 255).astype(np.uint8)
    return f


def _standing_frames(tc):
    """indices of the frames whose window (previous stamp, stamp] lies inside the standing interval shrunk by 0.1 s at each end"""
    return [k for k in range(1, len(tc)) if tc[k - 1] >= T_STOP + 0.1 and tc[k] <= T_GO - 0.1]


def _rim_speed(sim, k):
    """the largest absolute rim speed of the dataset's own encoder samples (Wheel3DAng: angular velocity x radius) over the window
    of frame k: (previous stamp, the newest IMU stamp when the frame arrives]"""
    tc, (tw, m1, m2), t_imu = sim["cam_times"], sim["wheel"], sim["imu"][0]
    t0, t1 = tc[k - 1], min(tc[k], t_imu[t_imu <= tc[k]].max())
    m = (tw > t0) & (tw <= t1)
    return max(np.abs(m1[m]).max() * sd.RL, np.abs(m2[m]).max() * sd.RR) if m.any() else -1.0


def test_standing_frames_keep_their_tracks_on_the_cpu(pkg, monkeypatch):
    """The other thing the GPU test rests on: four consecutive rendered frames of the standing camera, with their sensor noise, through
    the CPU oracle's front end (the library's is bit-identical to it): at least 20 points are tracked from each frame into the
    next, and their mean raw displacement stays under the default max_disparity of 1 px."""
    import oracle_context as oc
    monkeypatch.setattr(sd, "arc", stop_and_go)
    monkeypatch.setattr(sd.Renderer, "render", noisy_render(sd.Renderer.render))
    tc = sd.simulate(SECONDS, seed=0)["cam_times"]
    ks = _standing_frames(tc)[:3]
    times = [tc[ks[0] - 1]] + [tc[k] for k in ks]
    imgs = sd.render_frames(times)
    assert not np.array_equal(imgs[0], imgs[1])
    cfg = pkg.default_config(752, 480)
    cfg.num_features, cfg.fast_threshold, cfg.grid_x, cfg.grid_y, cfg.min_px_dist, cfg.histogram_method = 250, 20, 5, 5, 10, 1   # write_config's
    for i in range(8):
        cfg.intrinsics[i] = float(sd.K8[i])
    ctx = oc.OracleContext(cfg)
    try:
        prev = None
        for t, img in zip(times, imgs):
            ctx.tracker_feed(float(t), img)
            pts, ids = ctx.tracker_last()
            pts, ids = np.array(pts, dtype=np.float64).reshape(-1, 2), [int(i) for i in ids]
            if prev is not None:
                d = [np.linalg.norm(p - prev[i]) for p, i in zip(pts, ids) if i in prev]
                print(f"t {t:.4f}: {len(d)} points tracked from the previous frame, mean displacement {np.mean(d) if d else -1:.3f} px")
                assert len(d) >= 20 and np.mean(d) < 1.0, (t, len(d))
            prev = dict(zip(ids, pts))
    finally:
        ctx.close()


def test_drive_profile_on_the_cpu(monkeypatch):
    """what the GPU test rests on, checked without a GPU: the profile is continuous and stands exactly still, the synthetic encoder noise
    (0.02 rad/s times the radius) stays under max_wheel_speed while standing and the rim speed is far above it while driving, and
    the shrunk standing interval holds a good number of frames"""
    monkeypatch.setattr(sd, "arc", stop_and_go)
    x = np.linspace(0.0, SECONDS, 6601)
    s, v = stop_and_go(x)
    assert np.abs(np.diff(s) / np.diff(x) - 0.5 * (v[1:] + v[:-1])).max() < 1e-3 and np.all(np.diff(s) >= 0)      # s' = v (kinks: 2 m/s^2 x 1 ms / 8)
    still = (x >= T_STOP) & (x <= T_GO)
    assert np.all(v[still] == 0.0) and np.ptp(s[still]) == 0.0 and v[0] == V0 and v[-1] == V0
    assert stop_and_go(3.0) == (float(s[3000]), 0.0)
    sim = sd.simulate(SECONDS, seed=0)
    tc = sim["cam_times"]
    frames = _standing_frames(tc)
    assert len(frames) >= 15
    for k in range(1, len(tc)):
        r = _rim_speed(sim, k)
        if k in frames:
            assert 0 <= r < 0.6 * MAX_WHEEL_SPEED, (k, r)
        if tc[k - 1] < T_STOP < tc[k] or tc[k - 1] < T_GO < tc[k]:      # the windows that hold the stop and the start are vetoed
            assert r > 1.5 * MAX_WHEEL_SPEED, (k, r)
        if tc[k] < T_BRAKE or tc[k - 1] > T_GO + T_PULL:
            assert r > 20 * MAX_WHEEL_SPEED, (k, r)
    t, wm, am = sim["imu"]
    m = (t > T_STOP + 0.01) & (t < T_GO - 0.01)      # at rest the IMU reads its biases, gravity and noise
    assert np.abs(wm[m].mean(0) - sd.BG).max() < 1e-3 and abs(np.linalg.norm((am[m] - sd.BA).mean(0)) - 9.81) < 1e-2


@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stop_and_go"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(sd, "arc", stop_and_go)
        mp.setattr(sd.Renderer, "render", noisy_render(sd.Renderer.render))
        sim = sd.simulate(SECONDS, seed=0)
        sd.make_dataset(d, seconds=SECONDS, workers=min(8, os.cpu_count() or 1))
    sim["cam_times"] = np.array([float(f"{x:.9f}") for x in sim["cam_times"]])      # as the dataset's files hold them
    return d, sim


def _replay(pkg, dataset, cfg_dir, zupt, monkeypatch):
    """the drive through replay(); per camera frame (stamp, cam_updates and zupt_updates before and after, |v| and p after), and every
    call of the library's zero-velocity entry points (name, arguments of interest, result)"""
    options, rp, system = (importlib.import_module("plviwo_amd." + m) for m in ("options", "replay", "system"))
    cfg = sd.write_config(cfg_dir, dataset, os.path.join(cfg_dir, "traj.txt"))
    if zupt:
        with open(cfg, "a") as f:
            f.write('config_zupt: "config_zupt.yaml"\n')
        with open(os.path.join(cfg_dir, "config_zupt.yaml"), "w") as f:
            f.write("%YAML:1.0\n\nzupt:\n  enabled: true\n")
    op = options.load_options(cfg)
    assert op.est.zupt.enabled == zupt and op.est.wheel.enabled
    assert (op.est.zupt.max_wheel_speed, op.est.zupt.max_velocity) == (MAX_WHEEL_SPEED, MAX_VELOCITY)
    calls, frames = [], []
    for name in ("zupt_system", "zupt_update", "db_disparity", "zupt_try_update"):
        orig = getattr(pkg.Context, name)

        def wrapper(self, *a, _orig=orig, _name=name, **kw):
            out = _orig(self, *a, **kw)
            calls.append((_name, a, kw, out))
            return out
        monkeypatch.setattr(pkg.Context, name, wrapper)
    feed = system.SystemManager.feed_measurement_camera

    def feed_and_note(self, t, *a, **kw):
        before = (self.stats["cam_updates"], self.stats["zupt_updates"])
        out = feed(self, t, *a, **kw)
        frames.append(dict(t=float(t), before=before, after=(self.stats["cam_updates"], self.stats["zupt_updates"]),
                           speed=float(np.linalg.norm(self.state.imu.v)), p=np.array(self.state.imu.p), initialized=self.state.initialized,
                           points=len(self.ctx.tracker_last()[1])))
        return out
    monkeypatch.setattr(system.SystemManager, "feed_measurement_camera", feed_and_note)
    stats, times, poses = rp.replay(op)
    return stats, frames, calls


def _drift(frames, tc):
    ks = _standing_frames(tc)
    by_t = {f["t"]: f for f in frames}
    return float(np.linalg.norm(by_t[float(tc[ks[-1]])]["p"] - by_t[float(tc[ks[0]])]["p"]))


@pytest.mark.gpu
def test_standing_frames_take_zero_velocity_updates(pkg, drive, tmp_path, monkeypatch):
    dataset, sim = drive
    tc = sim["cam_times"]
    stats, frames, calls = _replay(pkg, dataset, str(tmp_path / "on"), True, monkeypatch)
    assert stats["initialized"] and stats["startup_time"] < T_BRAKE and stats["frames"] == len(tc) == len(frames)
    assert stats["not_psd"] == 0
    assert [f["t"] for f in frames] == [float(x) for x in tc]
    tried = {a[8]: (a, out) for name, a, kw, out in calls if name == "zupt_try_update"}       # by the frame's stamp (cam_time1)
    standing = _standing_frames(tc)
    assert len(standing) >= 15
    # every standing frame takes a zero-velocity update, on at least 20 points tracked from the previous frame whose disparity passes
    by = {"disparity": 0, "imu": 0}
    for k in standing:
        a, (rc, res, dx) = tried[float(tc[k])]
        assert a[7] == float(tc[k - 1]) and rc == 0 and res["stationary"] == 1 and res["updated"] == 1, (k, res)
        assert res["wheel_vetoed"] == 0 and res["disparity_n"] >= 20 and res["disparity_passed"] == 1, (k, res)
        assert 0 <= res["disparity_mean"] < 1.0 and frames[k]["points"] >= 20, (k, res)
        by["disparity"] += res["disparity_passed"]
        by["imu"] += res["imu_passed"]
        f = frames[k]
        assert f["after"][1] == f["before"][1] + 1, (k, f)
    print(f"{len(standing)} standing frames: the disparity passed in {by['disparity']}, the IMU test in {by['imu']}; points held by the "
          f"tracker after them {min(frames[k]['points'] for k in standing)} .. {max(frames[k]['points'] for k in standing)}; largest chi2 "
          f"{max(tried[float(tc[k])][1][1]['chi2'] for k in standing):.2f} against {tried[float(tc[standing[0]])][1][1]['chi2_threshold']:.2f}")
    # no frame whose window holds a rim speed above max_wheel_speed takes one (the dataset's own encoder samples)
    fast = 0
    for k in range(1, len(tc)):
        f = frames[k]
        if _rim_speed(sim, k) > MAX_WHEEL_SPEED:
            fast += 1
            assert f["after"][1] == f["before"][1], (k, f)
            if float(tc[k]) in tried:
                assert tried[float(tc[k])][1][1]["wheel_vetoed"] == 1
    assert fast >= 20
    # the camera update is left out on a frame that took a zero-velocity update, and runs on the others
    for f in frames:
        if f["after"][1] > f["before"][1]:
            assert f["after"][0] == f["before"][0], f
    assert stats["zupt_updates"] == sum(f["after"][1] - f["before"][1] for f in frames) >= len(standing)
    assert stats["cam_updates"] >= 20 and stats["wheel_accepted"] >= 30
    assert frames[standing[-1]]["speed"] <= MAX_VELOCITY
    print("speed after the last standing frame %.3g m/s; position drift over the standing interval with zero-velocity updates %.3g m"
          % (frames[standing[-1]]["speed"], _drift(frames, tc)))
    assert not [c for c in calls if c[0] in ("zupt_system", "zupt_update")]      # the driver goes through plv_zupt_try_update alone


@pytest.mark.gpu
def test_without_the_option_nothing_calls_the_updater(pkg, drive, tmp_path, monkeypatch):
    dataset, sim = drive
    stats, frames, calls = _replay(pkg, dataset, str(tmp_path / "off"), False, monkeypatch)
    assert stats["initialized"] and stats["frames"] == len(sim["cam_times"]) and stats["not_psd"] == 0
    assert stats["zupt_updates"] == 0 and calls == []
    assert stats["cam_updates"] >= 20
    print("position drift over the standing interval without zero-velocity updates %.3g m" % _drift(frames, sim["cam_times"]))
