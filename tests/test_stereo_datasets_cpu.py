"""The right camera in the dataset readers and in replay(): the plain layout (cam1/ beside cam0/), the EuRoC layout (mav0/cam1) and the
KAIST raw layout (image/stereo_right), pairs matched by time stamp, a frame without its partner skipped and counted, and a stereo
configuration on a left-only directory refused.  The images are rendered at 64 x 48: only the files and their stamps matter here."""
import importlib
import os
import shutil

import numpy as np
import pytest

import kaist_synth
import synth_dataset as sd
import synth_stereo_dataset as ssd
from oracle_context import OracleIwInitializer
from stereo_mirror_context import StereoMirrorContext

N_FRAMES, DROPPED = 6, 2


@pytest.fixture(scope="module")
def mods(pkg):
    name = pkg.__name__
    return tuple(importlib.import_module(name + m) for m in (".options", ".system", ".replay", ".kaist"))


@pytest.fixture(scope="module")
def pair_dir(tmp_path_factory):
    """0.6 s of the synthetic pair at 64 x 48 with the right camera missing frame 2, and its stereo configuration"""
    d = str(tmp_path_factory.mktemp("pair"))
    sd.set_camera(64, 48)
    try:
        ssd.make_dataset(d, seconds=0.6, cam_hz=10.0, drop_right=(DROPPED,))
        cfg = ssd.write_config(os.path.join(d, "config"), d, os.path.join(d, "out", "traj.txt"))
    finally:
        sd.set_camera(752, 480)
    return d, cfg


def _check_pairs(ds, n_right_only=0):
    assert ds.has_right and len(ds.frames) == N_FRAMES and len(ds.right_of) == N_FRAMES
    assert [p is None for p in ds.right_of] == [i == DROPPED for i in range(N_FRAMES)]
    assert ds.right_unpaired == n_right_only
    left, right = ds.image(0), ds.image(0, 1)
    assert left.shape == right.shape == (48, 64) and left.dtype == right.dtype == np.uint8 and not np.array_equal(left, right)
    assert np.array_equal(ds.to_grey(ds.raw_image(3, 1)), ds.image(3, 1))


def test_plain_layout_reads_the_right_camera(mods, pair_dir, tmp_path):
    _, _, rp, _ = mods
    d, _ = pair_dir
    _check_pairs(rp.Dataset(d))
    # a right frame whose stamp no left frame has is counted, and pairs are matched by stamp, not by position
    e = str(tmp_path / "extra")
    shutil.copytree(d, e)
    shutil.copy(os.path.join(e, "cam1", "data", "000000.pgm"), os.path.join(e, "cam1", "data", "000099.pgm"))
    with open(os.path.join(e, "cam1", "data.csv"), "a") as f:
        f.write("9.500000000,000099.pgm\n")
    _check_pairs(rp.Dataset(e), n_right_only=1)
    # without cam1 nothing changes for the left camera
    shutil.rmtree(os.path.join(e, "cam1"))
    ds = rp.Dataset(e)
    assert not ds.has_right and len(ds.frames) == N_FRAMES and ds.right_of == [None] * N_FRAMES and ds.right_unpaired == 0


def test_euroc_layout_reads_mav0_cam1(mods, pair_dir, tmp_path):
    _, _, rp, _ = mods
    d, _ = pair_dir
    e = str(tmp_path / "euroc")
    os.makedirs(os.path.join(e, "mav0", "imu0"))
    shutil.copy(os.path.join(d, "imu.csv"), os.path.join(e, "mav0", "imu0", "data.csv"))
    for cam in ("cam0", "cam1"):
        shutil.copytree(os.path.join(d, cam), os.path.join(e, "mav0", cam))
    ds = rp.open_dataset(e)
    assert isinstance(ds, rp.Dataset) and ds.right_dir == os.path.join(e, "mav0", "cam1")
    _check_pairs(ds)


def test_kaist_layout_reads_stereo_right(mods, pair_dir, tmp_path):
    _, _, rp, kaist = mods
    d, _ = pair_dir
    k = kaist_synth.convert(d, str(tmp_path / "kaist"), sd.RL, sd.RR, sd.BASE)
    left_only = rp.open_dataset(k)
    assert isinstance(left_only, kaist.KaistDataset) and not left_only.has_right
    src = rp.Dataset(d)
    os.makedirs(os.path.join(k, "image", "stereo_right"))
    for i, (t, _) in enumerate(src.frames):
        if src.right_of[i] is not None:
            kaist_synth.write_png(os.path.join(k, "image", "stereo_right", f"{kaist_synth.T0_NS + int(round(t * 1e9))}.png"), src.image(i, 1))
    ds = rp.open_dataset(k)
    assert ds.encoding == "bayer_rggb8" and ds.right_dir == os.path.join(k, "image", "stereo_right")
    _check_pairs(ds)
    assert np.array_equal(ds.raw_image(3, 1), src.image(3, 1)) and np.array_equal(ds.image(3, 1), kaist.bayer_rg_to_grey(src.image(3, 1)))


def test_replay_feeds_pairs_and_counts_the_frame_without_a_partner(mods, pair_dir, monkeypatch):
    options, system, rp, _ = mods
    d, cfg = pair_dir
    fed = []
    monkeypatch.setattr(system.SystemManager, "feed_measurement_stereo",
                        lambda self, t, left, right, ml=None, mr=None, encoding="mono8": fed.append((t, left.shape, right.shape, encoding, np.array_equal(left, right))))
    monkeypatch.setattr(system.SystemManager, "feed_measurement_camera", lambda self, *a, **k: pytest.fail("a stereo replay fed one image"))
    op = options.load_options(cfg)
    stats, _, _ = rp.replay(op, context_factory=StereoMirrorContext, iw_initializer_factory=OracleIwInitializer)
    assert stats["stereo"] is True and stats["pairs_skipped"] == 1 and stats["camera_messages"] == N_FRAMES - 1
    ds = rp.Dataset(d)
    assert [f[0] for f in fed] == [t for i, (t, _) in enumerate(ds.frames) if i != DROPPED]
    assert all(f[1:] == ((48, 64), (48, 64), "mono8", False) for f in fed)


def test_stereo_configuration_on_a_left_only_directory_is_refused(mods, pair_dir, tmp_path):
    options, _, rp, _ = mods
    d, cfg = pair_dir
    e = str(tmp_path / "left_only")
    shutil.copytree(d, e)
    shutil.rmtree(os.path.join(e, "cam1"))
    op = options.load_options(cfg)
    op.sys.path_bag = e
    with pytest.raises(options.OptionsError) as err:
        rp.replay(op, context_factory=StereoMirrorContext, iw_initializer_factory=OracleIwInitializer)
    assert os.path.join(e, "cam1") in str(err.value) and "right camera" in str(err.value)
