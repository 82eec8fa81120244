"""synth_dataset.make_dataset for a stereo pair: camera 1 is camera 0 moved 0.5 m to its right (P_CINI shifted along the camera's x
axis, the same R_CTOI), rendered with the same Renderer at the same stamps into cam1/; the configuration synth_dataset.write_config
writes is patched to max_n: 2, use_stereo: true, stereo_pair: [0, 1] with a cam1 block."""
import os

import numpy as np

import synth_dataset as sd

BASELINE = 0.5


def p_cini_right():
    return sd.P_CINI + sd.R_CTOI @ np.array([BASELINE, 0.0, 0.0])


def render_right(times, style="room", workers=1):
    """the right camera's images at `times` (synth_dataset.render_frames from camera 1's mount)"""
    left = sd.P_CINI
    sd.P_CINI = p_cini_right()
    try:
        return sd.render_frames(times, style, workers)
    finally:
        sd.P_CINI = left


def make_dataset(out_dir, seconds=12.0, cam_hz=10.0, style="room", workers=1, drop_right=(), **kw):
    """make_dataset + cam1/data.csv, cam1/data/*.pgm at the left camera's stamps; drop_right: frame numbers the right camera misses"""
    out = sd.make_dataset(out_dir, seconds=seconds, cam_hz=cam_hz, style=style, workers=workers, **kw)
    tc = out["cam_times"]
    os.makedirs(os.path.join(out_dir, "cam1", "data"), exist_ok=True)
    imgs = render_right(tc, style, workers)
    with open(os.path.join(out_dir, "cam1", "data.csv"), "w") as f:
        f.write("# t file\n")
        for k, x in enumerate(tc):
            if k in drop_right:
                continue
            name = f"{k:06d}.pgm"
            f.write(f"{x:.9f},{name}\n")
            sd.write_pgm(os.path.join(out_dir, "cam1", "data", name), imgs[k])
    return out


def write_config(cfg_dir, dataset_dir, traj_path, **kw):
    path = sd.write_config(cfg_dir, dataset_dir, traj_path, **kw)
    cam = os.path.join(cfg_dir, "config_camera.yaml")
    text = open(cam).read()
    assert "  max_n: 1\n  use_stereo: false\n" in text
    text = text.replace("  max_n: 1\n  use_stereo: false\n", "  max_n: 2\n  use_stereo: true\n  stereo_pair: [0, 1]\n")
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = sd.R_CTOI, p_cini_right()
    rows = "\n".join("    - [" + ", ".join(f"{x:.12g}" for x in row) + "]" for row in T)
    text += f'''cam1:
  timeoffset: 0.0
  T_imu_cam:
{rows}
  distortion_coeffs: [{", ".join(f"{x:.10g}" for x in sd.K8[4:])}]
  distortion_model: radtan
  intrinsics: [{", ".join(f"{x:.10g}" for x in sd.K8[:4])}]
  resolution: [{sd.W}, {sd.H}]
  topic: "cam1"
'''
    with open(cam, "w") as f:
        f.write(text)
    return path
