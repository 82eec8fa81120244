"""File-based replay in place of the reference's rosbag player: a directory of images plus IMU / wheel
CSV files is merged into one time-ordered message stream and fed to the SystemManager; poses are logged in the reference's
trajectory format.

REF: PL-VIWO/src/run_bag.cpp:51-144 (message loop: IMU -> feed_measurement_imu (+ trajectory line when a clone was made), camera ->
     feed_measurement_camera, wheel -> feed_measurement_wheel; bag_start / bag_durr window), :272-340 (mono camera message ->
     CameraData with an all-zero mask unless use_mask); PL-VIWO/src/core/ROSHelper.cpp:151-216 (image / JointState conversions);
     PL-VIWO/src/utils/State_Logger.h:188-205 (trajectory line).

Dataset layout (`sys.path_bag` names the directory):
    imu.csv              t, wx, wy, wz, ax, ay, az          ('#' comment lines; t in seconds, or integer nanoseconds as EuRoC)
    wheel.csv            t, m1, m2                          (the two readings of the configured wheel type; optional)
    cam0/data.csv        t, file name                       (optional: without it the file stem is the time stamp)
    cam0/data/*          8-bit grey images: .pgm (P5), .png (grey / RGB, not interlaced) or .npy
    cam1/data.csv, cam1/data/*   the right camera of a stereo pair, laid out like cam0 (optional): a left and a right frame with one
                         time stamp are a pair; a frame without its partner is skipped by a stereo replay and counted
A directory in the EuRoC MAV (ASL) layout is read as it is: mav0/imu0/data.csv, mav0/cam0/data.csv + mav0/cam0/data/*.png (and
mav0/cam1); a KAIST Complex Urban raw directory (sensor_data/xsens_imu.csv, encoder.csv, image/stereo_left, image/stereo_right)
through kaist.KaistDataset (open_dataset).
"""
import os
import struct
import time
import zlib

import numpy as np

from . import traj_format, traj_header
from .options import OptionsError
from .system import SystemManager

IMU, WHEEL, CAM = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------ images
def _read_pgm(path):
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] != b"P5":
        raise ValueError(f"{path}: not a binary PGM")
    vals, pos = [], 2
    while len(vals) < 3:   # width, height, maxval with '#' comments
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        vals.append(int(data[pos:end]))
        pos = end
    w, h, maxval = vals
    pos += 1
    if maxval > 255:
        img = np.frombuffer(data, dtype=">u2", count=w * h, offset=pos).reshape(h, w)
        return (img >> 8).astype(np.uint8)
    return np.frombuffer(data, dtype=np.uint8, count=w * h, offset=pos).reshape(h, w).copy()


def _read_png(path):
    """8-bit grey / grey+alpha / RGB / RGBA, non-interlaced (what cv_bridge's MONO8 conversion would be handed)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            break
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    ch = {0: 1, 2: 3, 4: 2, 6: 4}.get(ctype)
    if depth != 8 or ch is None or interlace:
        raise ValueError(f"{path}: only 8-bit non-interlaced grey / RGB PNGs are read")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), dtype=np.uint8)
    prev = np.zeros(w * ch, dtype=np.int32)
    for y in range(h):
        ft, line = raw[y, 0], raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:   # 1 (sub), 3 (average), 4 (Paeth) depend on the pixel to the left: byte-serial
            cur = np.zeros_like(line)
            for x in range(w * ch):
                a = cur[x - ch] if x >= ch else 0
                b = prev[x]
                c = prev[x - ch] if x >= ch else 0
                if ft == 1:
                    pr = a
                elif ft == 3:
                    pr = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pr = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[x] = (line[x] + pr) & 255
        out[y] = cur
        prev = cur
    img = out.reshape(h, w, ch)
    if ch <= 2:
        return img[:, :, 0].copy()
    rgb = img[:, :, :3].astype(np.float64)   # OpenCV's RGB -> grey weights
    return np.clip(np.rint(0.299 * rgb[:, :, 0] + 0.587 * rgb[:, :, 1] + 0.114 * rgb[:, :, 2]), 0, 255).astype(np.uint8)


def read_image(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == ".pgm":
        return _read_pgm(path)
    if ext == ".png":
        return _read_png(path)
    if ext == ".npy":
        return np.ascontiguousarray(np.load(path), dtype=np.uint8)
    raise ValueError(f"{path}: unsupported image format")


# ----------------------------------------------------------------------------------------------------------- dataset
def _read_csv(path, ncol):
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            parts = [x for x in line.replace(",", " ").split()]
            if len(parts) < ncol:
                raise ValueError(f"{path}: expected {ncol} columns: {line}")
            rows.append(parts[:ncol])
    return rows


def _stamp(s):
    """seconds as a decimal number, or integer nanoseconds (EuRoC)"""
    if "." not in s and "e" not in s.lower() and len(s.lstrip("-")) > 12:
        return int(s) * 1e-9
    return float(s)


class Dataset:
    """The time-ordered message list of a dataset directory (the rosbag::View of run_bag.cpp)."""

    def __init__(self, root, cam_dir="cam0", use_wheel=True, use_cam=True, right_dir="cam1"):
        self.root = root
        imu_path = os.path.join(root, "imu.csv")
        if not os.path.exists(imu_path) and os.path.isdir(os.path.join(root, "mav0")):   # EuRoC MAV (ASL) layout
            imu_path = os.path.join(root, "mav0", "imu0", "data.csv")
            cam_dir, right_dir = os.path.join("mav0", cam_dir), os.path.join("mav0", right_dir)
        imu = _read_csv(imu_path, 7)
        self.imu = np.array([[_stamp(r[0])] + [float(x) for x in r[1:]] for r in imu])
        self.wheel = np.zeros((0, 3))
        wp = os.path.join(root, "wheel.csv")
        if use_wheel and os.path.exists(wp):
            self.wheel = np.array([[_stamp(r[0]), float(r[1]), float(r[2])] for r in _read_csv(wp, 3)])
        self.frames = self._frames_of(os.path.join(root, cam_dir)) if use_cam else []
        # the right camera of a stereo pair, matched to the left frames by time stamp
        self.right_dir = os.path.join(root, right_dir)
        right = self._frames_of(self.right_dir) if use_cam else []
        pair_frames(self, right)
        msgs = [(t, IMU, i) for i, t in enumerate(self.imu[:, 0])] + [(t, WHEEL, i) for i, t in enumerate(self.wheel[:, 0])] + \
               [(t, CAM, i) for i, (t, _) in enumerate(self.frames)]
        msgs.sort(key=lambda m: (m[0], m[1]))
        self.msgs = msgs

    @staticmethod
    def _frames_of(cdir):
        """[(stamp, path)] of one camera directory (data.csv, or the file stems as stamps); empty without the directory"""
        if not os.path.isdir(cdir):
            return []
        listing = os.path.join(cdir, "data.csv")
        if os.path.exists(listing):
            return [(_stamp(r[0]), os.path.join(cdir, "data", r[1])) for r in _read_csv(listing, 2)]
        return [(_stamp(os.path.splitext(name)[0]), os.path.join(cdir, "data", name)) for name in sorted(os.listdir(os.path.join(cdir, "data")))]

    def t_begin(self):
        return self.msgs[0][0]

    def image(self, i, cam=0):
        """frame i of the left camera (cam = 0), or its partner of the right camera (cam = 1)"""
        return read_image(self.frames[i][1] if cam == 0 else self.right_of[i])

    encoding = "mono8"      # what raw_image delivers (a ROS encoding string): these layouts hold grey images
    raw_image = image

    @staticmethod
    def to_grey(raw):
        """raw_image -> the grey image, on the host (image(i) = to_grey(raw_image(i)))"""
        return raw


def pair_frames(ds, right):
    """Matches the right camera's frames [(stamp, path)] to ds.frames by time stamp: ds.has_right (there is a right camera),
    ds.right_of [len(frames)] (the partner's path or None), ds.right_unpaired (right frames no left frame has the stamp of)"""
    by_stamp = {t: p for t, p in right}
    ds.has_right = len(right) > 0
    ds.right_of = [by_stamp.get(t) for t, _ in ds.frames]
    left_stamps = {t for t, _ in ds.frames}
    ds.right_unpaired = sum(1 for t, _ in right if t not in left_stamps)


def open_dataset(root, use_wheel=True, use_cam=True):
    """Dataset for this layout / EuRoC, or kaist.KaistDataset for a KAIST Complex Urban raw directory (sensor_data/xsens_imu.csv)"""
    from . import kaist
    if kaist.is_kaist_raw(root):
        return kaist.KaistDataset(root, use_wheel=use_wheel, use_cam=use_cam)
    return Dataset(root, use_wheel=use_wheel, use_cam=use_cam)


class TrajectoryLogger:
    """State_Logger::save_trajectory_to_file (REF: State_Logger.h:160-205)."""

    def __init__(self, path):
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        self.f = open(path, "w")
        self.f.write(traj_header())
        self.n = 0

    def save(self, sys):
        st = sys.state
        self.f.write(traj_format(st.time, np.array(st.imu.p), np.array(st.imu.q), sys.imu_pose_covariance()))
        self.n += 1

    def close(self):
        self.f.close()


def write_ppm(path, rgb):
    """an [H, W, 3] u8 image as a binary PPM (P6)"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


class MapAccumulator:
    """The map of a whole replay (SystemManager(line_map=True)): behind every camera message the MSCKF points and line segments the
    updates used are taken over (get_used_msckf / get_used_lines clear their lists) and the in-state landmarks' latest positions are
    noted by feature id.  `after_camera` has replay()'s callback signature."""
    KINDS = {"msckf": 0, "slam": 1, "line": 2}

    def __init__(self, accepted_only=True):
        self.accepted_only = accepted_only
        self.points, self.segments, self.landmarks = [], [], {}

    def after_camera(self, system, frame, t):
        self.points.append(system.get_used_msckf())
        self.segments.append(system.get_used_lines(self.accepted_only))
        for fid, lm in system.state.slam.items():
            self.landmarks[int(fid)] = np.array(lm.p, dtype=float)

    def arrays(self):
        """-> (msckf points [n, 3], landmark positions [m, 3], segments [k, 6])"""
        pts = np.concatenate(self.points) if self.points else np.zeros((0, 3))
        seg = np.concatenate(self.segments) if self.segments else np.zeros((0, 6))
        lms = np.array([self.landmarks[k] for k in sorted(self.landmarks)], dtype=float).reshape(-1, 3)
        return pts, lms, seg

    def stats(self):
        pts, lms, seg = self.arrays()
        length = np.linalg.norm(seg[:, 3:] - seg[:, :3], axis=1)
        return dict(map_points=int(len(pts) + len(lms)), map_lines=int(len(seg)),
                    map_line_length_p50=float(np.median(length)) if len(length) else 0.0)

    def write_ply(self, path):
        """ASCII PLY: a vertex per MSCKF point, landmark and segment end point (property `kind`: 0 / 1 / 2), an edge per segment"""
        pts, lms, seg = self.arrays()
        verts = [(p, self.KINDS["msckf"]) for p in pts] + [(p, self.KINDS["slam"]) for p in lms]
        first = len(verts)
        for s in seg:
            verts += [(s[:3], self.KINDS["line"]), (s[3:], self.KINDS["line"])]
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            f.write("ply\nformat ascii 1.0\ncomment kind: 0 MSCKF point, 1 in-state landmark, 2 line segment end point\n")
            f.write(f"element vertex {len(verts)}\nproperty double x\nproperty double y\nproperty double z\nproperty uchar kind\n")
            f.write(f"element edge {len(seg)}\nproperty int vertex1\nproperty int vertex2\nend_header\n")
            for p, kind in verts:
                f.write(f"{p[0]:.6f} {p[1]:.6f} {p[2]:.6f} {kind}\n")
            for i in range(len(seg)):
                f.write(f"{first + 2 * i} {first + 2 * i + 1}\n")


def replay(op, dataset=None, trajectory_path=None, device=0, progress=None, max_obs=24, host_images=False, after_camera=None, **system_kw):
    """run_bag's main loop.  Returns (SystemManager statistics, times, poses [n][7] = p, q).  after_camera(sys, frame, t), when given,
    is called behind every camera message (run_bag.cpp:287-296 publishes the track image there); its time is kept apart from the
    camera side's (time_after_camera_s).  A dataset whose frames are not grey
    (Dataset.encoding, e.g. the Bayer mosaics of a KAIST directory) hands them over as they are read and the library converts them
    on the device; host_images: the dataset converts them on the host (Dataset.image), as a context without the conversion has to."""
    ds = dataset if dataset is not None else open_dataset(op.sys.path_bag, use_wheel=op.est.wheel.enabled, use_cam=op.est.cam.enabled)
    stereo = bool(op.est.cam.enabled and op.est.cam.use_stereo and op.est.cam.max_n == 2)
    if stereo and not getattr(ds, "has_right", False):
        raise OptionsError(f"replay: the configuration has a stereo pair, the dataset has no right camera images ({getattr(ds, 'right_dir', 'cam1')})")
    sys = SystemManager(op, device=device, max_obs=max_obs, **system_kw)
    path = trajectory_path if trajectory_path is not None else (op.sys.path_trajectory if op.sys.save_trajectory else None)
    log = TrajectoryLogger(path) if path else None
    t_init = ds.t_begin() + op.sys.bag_start                               # run_bag.cpp:214-216
    t_finish = math_inf if op.sys.bag_durr < 0 else t_init + op.sys.bag_durr
    mask = None
    if op.est.cam.enabled and op.est.cam.use_mask.get(0):
        mask = read_image(op.est.cam.mask_path[0])
    mask_right = read_image(op.est.cam.mask_path[1]) if stereo and op.est.cam.use_mask.get(1) else None
    pairs_skipped = ds.right_unpaired if stereo else 0
    times, poses = [], []
    encoding = getattr(ds, "encoding", "mono8")
    has_raw = hasattr(ds, "raw_image") and hasattr(ds, "to_grey")
    device_images = not host_images and encoding != "mono8" and has_raw and hasattr(sys.ctx, "image_stage_encoded")
    cam_wall, cam_frames = 0.0, 0       # wall time of the camera messages past the file read: conversion + feed + update
    after_wall = 0.0
    for k, (t, kind, i) in enumerate(ds.msgs):
        if t > t_finish:
            break
        if t < t_init:
            continue
        if kind == IMU:
            r = ds.imu[i]
            if sys.feed_measurement_imu(r[0], r[1:4], r[4:7]):
                st = sys.state
                times.append(st.time), poses.append(np.concatenate([np.array(st.imu.p), np.array(st.imu.q)]))
                if log:
                    log.save(sys)
        elif kind == CAM and stereo:
            if ds.right_of[i] is None:       # a frame without its partner
                pairs_skipped += 1
                continue
            left, right = (ds.raw_image(i), ds.raw_image(i, 1)) if has_raw else (ds.image(i), ds.image(i, 1))
            on_device = not host_images and encoding != "mono8" and has_raw        # (plv_tracker_feed_stereo converts the pair itself)
            if has_raw and not on_device:
                left, right = ds.to_grey(left), ds.to_grey(right)
            t0 = time.perf_counter()
            sys.feed_measurement_stereo(t, left, right, mask, mask_right, encoding=encoding if on_device else "mono8")
            cam_wall, cam_frames = cam_wall + time.perf_counter() - t0, cam_frames + 1
            if after_camera is not None:
                t0 = time.perf_counter()
                after_camera(sys, cam_frames - 1, t)
                after_wall += time.perf_counter() - t0
        elif kind == CAM:
            raw = ds.raw_image(i) if has_raw else None       # (the file read is not the camera side's time)
            t0 = time.perf_counter()
            if device_images:
                sys.feed_measurement_camera_encoded(t, raw, encoding, mask)
            else:
                sys.feed_measurement_camera(t, ds.to_grey(raw) if has_raw else ds.image(i), mask)
            cam_wall, cam_frames = cam_wall + time.perf_counter() - t0, cam_frames + 1
            if after_camera is not None:
                t0 = time.perf_counter()
                after_camera(sys, cam_frames - 1, t)
                after_wall += time.perf_counter() - t0
        else:
            r = ds.wheel[i]
            sys.feed_measurement_wheel(r[0], r[1], r[2])
        if progress and k % 2000 == 0:
            progress(sys, t)
    if log:
        log.close()
    stats = dict(sys.stats)
    stats.update(distance_m=sys.distance, time_s={k: round(v, 4) for k, v in sys.tc.total.items()}, initialized=sys.state.initialized,
                 startup_time=sys.state.startup_time, end_time=sys.state.time, n_state=sys.state.n, clone_freq=op.est.clone_freq,
                 image_route="device" if device_images or (stereo and not host_images and encoding != "mono8" and has_raw) else "host",
                 time_camera_s=round(cam_wall, 6), camera_messages=cam_frames, stereo=stereo, pairs_skipped=pairs_skipped)
    if after_camera is not None:
        stats["time_after_camera_s"] = round(after_wall, 6)
    sys.close()
    return stats, np.array(times), np.array(poses).reshape(-1, 7)


math_inf = float("inf")
