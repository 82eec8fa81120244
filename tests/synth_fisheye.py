"""A fisheye version of synth_dataset's drive: the same trajectory, IMU, wheel and scene, rendered through an equidistant camera
(Kalibr `distortion_model: equidistant`, four `distortion_coeffs`).  synth_dataset itself is not edited and its module globals
(K8, W, H) are left as they are: the renderer is synth_dataset.Renderer with its per-pixel rays replaced by the equidistant
model's exact inverse (cam_equi.unproject).  Test helper, not a test."""
import os
import re

import numpy as np

import cam_equi
import synth_dataset as sd

W, H = 752, 480
# fx fy cx cy k1 k2 k3 k4 (TUM-VI-like; the corners sit at theta_d ~ 1.27 rad, ~73 degrees, well below pi/2)
K8 = np.array([350.0, 350.0, 376.0, 240.0, 0.012, -0.006, 0.002, -0.0005])


class FisheyeRenderer(sd.Renderer):
    def __init__(self, seed=7, style="room"):
        assert (sd.W, sd.H) == (W, H), "synth_dataset renders 752x480 here"
        super().__init__(seed=seed, style=style)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        self.rays = cam_equi.unproject(K8, np.stack([xs.ravel(), ys.ravel()], axis=1))
        self.f = 0.5 * (K8[0] + K8[1])


def render_frames(times, seed=7):
    rd = FisheyeRenderer(seed=seed)
    return [rd.render(t) for t in times]


def make_dataset(out_dir, seconds=8.0, cam_hz=10.0, seed=0):
    """synth_dataset.make_dataset's streams and ground truth, with the camera images rendered through the fisheye camera."""
    sd.make_dataset(out_dir, seconds=seconds, cam_hz=cam_hz, seed=seed, render=False)
    rd = FisheyeRenderer()
    for line in open(os.path.join(out_dir, "cam0", "data.csv")):
        if line.startswith("#"):
            continue
        t, name = line.strip().split(",")
        sd.write_pgm(os.path.join(out_dir, "cam0", "data", name), rd.render(float(t)))
    return out_dir


def write_config(cfg_dir, dataset_dir, traj_path, model="equidistant", **kw):
    """synth_dataset.write_config with the camera of this dataset: `equidistant` with K8, or — the control — the same fx fy cx cy
    under a `radtan` model with zero coefficients."""
    cfg = sd.write_config(cfg_dir, dataset_dir, traj_path, **kw)
    p = os.path.join(cfg_dir, "config_camera.yaml")
    text = open(p).read()
    coeffs = K8[4:] if model == "equidistant" else np.zeros(4)
    text = re.sub(r"distortion_coeffs: *\[[^\]]*\]", "distortion_coeffs: [" + ", ".join(f"{x:.10g}" for x in coeffs) + "]", text)
    text = re.sub(r"distortion_model: *\S+", f"distortion_model: {model}", text)
    text = re.sub(r"intrinsics: *\[[^\]]*\]", "intrinsics: [" + ", ".join(f"{x:.10g}" for x in K8[:4]) + "]", text)
    open(p, "w").write(text)
    return cfg


# ---- the same drive seen by a stereo pair of such cameras (synth_stereo_dataset's mounts: camera 1 0.5 m to camera 0's right)
def make_stereo_dataset(out_dir, seconds=4.0, cam_hz=10.0, seed=0):
    """make_dataset + cam1/: the right camera's images at the left camera's stamps, rendered through the same fisheye camera from
    camera 1's mount."""
    import synth_stereo_dataset as ssd
    make_dataset(out_dir, seconds=seconds, cam_hz=cam_hz, seed=seed)
    os.makedirs(os.path.join(out_dir, "cam1", "data"), exist_ok=True)
    rd = FisheyeRenderer()
    left = sd.P_CINI
    sd.P_CINI = ssd.p_cini_right()   # (Renderer.render reads the mount when it renders)
    try:
        with open(os.path.join(out_dir, "cam1", "data.csv"), "w") as f:
            f.write("# t file\n")
            for line in open(os.path.join(out_dir, "cam0", "data.csv")):
                if line.startswith("#"):
                    continue
                t, name = line.strip().split(",")
                f.write(f"{t},{name}\n")
                sd.write_pgm(os.path.join(out_dir, "cam1", "data", name), rd.render(float(t)))
    finally:
        sd.P_CINI = left
    return out_dir


def write_stereo_config(cfg_dir, dataset_dir, traj_path, model="equidistant", **kw):
    """synth_stereo_dataset.write_config with this dataset's camera in both blocks (cam0 and cam1): `equidistant` with K8, or — the
    control — fx fy cx cy under `radtan` with zero coefficients."""
    import synth_stereo_dataset as ssd
    cfg = ssd.write_config(cfg_dir, dataset_dir, traj_path, **kw)
    p = os.path.join(cfg_dir, "config_camera.yaml")
    text = open(p).read()
    coeffs = K8[4:] if model == "equidistant" else np.zeros(4)
    text, n1 = re.subn(r"distortion_coeffs: *\[[^\]]*\]", "distortion_coeffs: [" + ", ".join(f"{x:.10g}" for x in coeffs) + "]", text)
    text, n2 = re.subn(r"distortion_model: *\S+", f"distortion_model: {model}", text)
    text, n3 = re.subn(r"intrinsics: *\[[^\]]*\]", "intrinsics: [" + ", ".join(f"{x:.10g}" for x in K8[:4]) + "]", text)
    assert (n1, n2, n3) == (2, 2, 2), "one block per camera"
    open(p, "w").write(text)
    return cfg
