"""The image-encoding contract (include/plviwo.h PLV_ENC_*) without a device: tests/image_encodings_ref.py, the numpy restatement the
GPU suite holds the library to, against pl-viwo_amd/kaist.py's bayer_rg_to_grey (the project's host yardstick for RGGB) and against
the properties any demosaicing to grey must have; the library's two host-only entry points; the compiler's resource report of the
conversion kernel."""
import importlib
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import image_encodings_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SIZES = [(8, 8), (9, 11), (6, 7), (3, 3), (31, 20), (3, 5), (4, 3), (56, 128)]


def _kaist():
    # kaist.py imports nothing of the package at module level: loaded from its file, so that these tests run where the library is not built
    spec = importlib.util.spec_from_file_location("kaist_standalone", os.path.join(ROOT, "pl-viwo_amd", "kaist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rggb_is_bayer_rg_to_grey():
    kaist = _kaist()
    rng = np.random.default_rng(0)
    for (h, w) in SIZES:
        for _ in range(4):
            m = rng.integers(0, 256, (h, w), dtype=np.uint8)
            assert np.array_equal(ref.to_grey(m, "bayer_rggb8"), kaist.bayer_rg_to_grey(m)), (h, w)
    for v in (0, 255):
        m = np.full((7, 9), v, dtype=np.uint8)
        assert np.array_equal(ref.to_grey(m, "bayer_rggb8"), kaist.bayer_rg_to_grey(m))


def test_pattern_names_give_the_site_colours():
    assert ref.bayer_colours("bayer_rggb8", 2, 2).tolist() == [["r", "g"], ["g", "b"]]
    assert ref.bayer_colours("bayer_bggr8", 2, 2).tolist() == [["b", "g"], ["g", "r"]]
    assert ref.bayer_colours("bayer_gbrg8", 2, 2).tolist() == [["g", "b"], ["r", "g"]]
    assert ref.bayer_colours("bayer_grbg8", 2, 2).tolist() == [["g", "r"], ["b", "g"]]


@pytest.mark.parametrize("shifted, dy, dx", [("bayer_grbg8", 0, 1), ("bayer_gbrg8", 1, 0), ("bayer_bggr8", 1, 1)])
def test_shift_relations_between_the_patterns(shifted, dy, dx):
    """an RGGB mosaic with its first column (row, both) dropped is a GRBG (GBRG, BGGR) mosaic: same grey two pixels inside the border"""
    rng = np.random.default_rng(1)
    for (h, w) in [(12, 14), (13, 11), (31, 20)]:
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        full = ref.to_grey(m, "bayer_rggb8")[dy:, dx:]
        part = ref.to_grey(np.ascontiguousarray(m[dy:, dx:]), shifted)
        assert part.shape == full.shape and np.array_equal(part[2:-2, 2:-2], full[2:-2, 2:-2]), (shifted, h, w)


def test_constant_colour_planes():
    rng = np.random.default_rng(2)
    for _ in range(20):
        r, g, b = (int(x) for x in rng.integers(0, 256, 3))
        want = (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14
        rgb = np.zeros((10, 13, 3), dtype=np.uint8)
        rgb[:, :] = (r, g, b)
        for name in ref.BAYER:
            out = ref.to_grey(ref.mosaic(rgb, name), name).astype(int)
            assert np.abs(out - want).max() <= 1, (name, r, g, b)
        assert np.all(ref.to_grey(rgb, "rgb8") == want)
        assert np.all(ref.to_grey(rgb[:, :, ::-1], "bgr8") == want)
        rgba = np.concatenate([rgb, rng.integers(0, 256, (10, 13, 1), dtype=np.uint8)], axis=2)
        assert np.all(ref.to_grey(rgba, "rgba8") == want)
        assert np.all(ref.to_grey(np.concatenate([rgb[:, :, ::-1], rgba[:, :, 3:]], axis=2), "bgra8") == want)


def test_constant_mosaic_is_returned_unchanged_and_255_stays_255():
    for name in ref.BAYER:
        for v in (0, 1, 77, 128, 254, 255):
            for (h, w) in [(3, 3), (6, 6), (7, 10)]:
                assert np.all(ref.to_grey(np.full((h, w), v, dtype=np.uint8), name) == v), (name, v)
    for name in ref.COLOUR:
        assert np.all(ref.to_grey(np.full((5, 6, ref.BPP[name]), 255, dtype=np.uint8), name) == 255)
        assert np.all(ref.to_grey(np.zeros((5, 6, ref.BPP[name]), dtype=np.uint8), name) == 0)
    m = np.random.default_rng(3).integers(0, 256, (9, 9), dtype=np.uint8)
    assert np.array_equal(ref.to_grey(m, "mono8"), m)


def test_rgb_is_bgr_reversed_and_alpha_is_ignored():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    assert np.array_equal(ref.to_grey(img, "rgb8"), ref.to_grey(np.ascontiguousarray(img[:, :, ::-1]), "bgr8"))
    assert not np.array_equal(ref.to_grey(img, "rgb8"), ref.to_grey(img, "bgr8"))
    for name, base in (("rgba8", "rgb8"), ("bgra8", "bgr8")):
        a1 = np.concatenate([img, rng.integers(0, 256, (17, 23, 1), dtype=np.uint8)], axis=2)
        a2 = np.concatenate([img, rng.integers(0, 256, (17, 23, 1), dtype=np.uint8)], axis=2)
        assert np.array_equal(ref.to_grey(a1, name), ref.to_grey(a2, name)) and np.array_equal(ref.to_grey(a1, name), ref.to_grey(img, base))


def test_borders_replicate_rows_then_columns():
    m = np.random.default_rng(5).integers(0, 256, (9, 12), dtype=np.uint8)
    for name in ref.BAYER:
        g = ref.to_grey(m, name)
        assert np.array_equal(g[0], g[1]) and np.array_equal(g[-1], g[-2]) and np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, -1], g[:, -2])


def test_kaist_dataset_names_its_encoding():
    """library-free: the reader's class says what raw_image delivers, and its host conversion is the reference's"""
    kaist = _kaist()
    assert kaist.KaistDataset.encoding == "bayer_rggb8" and ref.ENCODINGS[kaist.KaistDataset.encoding] == 1
    m = np.random.default_rng(6).integers(0, 256, (56, 128), dtype=np.uint8)
    assert np.array_equal(ref.to_grey(m, kaist.KaistDataset.encoding), kaist.KaistDataset.to_grey(m))


def test_kaist_dataset_raw_image_through_the_package(pkg, tmp_path):
    """KaistDataset.raw_image converted by the reference equals KaistDataset.image (the package's own reader)"""
    import kaist_synth
    kaist, replay = importlib.import_module("plviwo_amd.kaist"), importlib.import_module("plviwo_amd.replay")
    root = str(tmp_path / "urban")
    os.makedirs(os.path.join(root, "sensor_data"))
    os.makedirs(os.path.join(root, "image", "stereo_left"))
    rng = np.random.default_rng(7)
    t0 = 1544590798000000000
    with open(os.path.join(root, "sensor_data", "xsens_imu.csv"), "w") as f:
        for i in range(4):
            f.write(",".join(str(x) for x in [t0 + i * 10000000, 0, 0, 0, 1, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 9.8, 0, 0, 0]) + "\n")
    imgs = [rng.integers(0, 256, (57, 129), dtype=np.uint8) for _ in range(2)]
    for i, img in enumerate(imgs):
        kaist_synth.write_png(os.path.join(root, "image", "stereo_left", f"{t0 + 5000000 + i * 100000000}.png"), img)
    ds = replay.open_dataset(root)
    assert isinstance(ds, kaist.KaistDataset) and ds.encoding == "bayer_rggb8" and len(ds.frames) == 2
    for i, img in enumerate(imgs):
        raw = ds.raw_image(i)
        assert np.array_equal(raw, img)
        assert np.array_equal(ref.to_grey(raw, ds.encoding), ds.image(i)) and np.array_equal(ds.to_grey(raw), ds.image(i))
    grey = replay.Dataset.__dict__["encoding"]
    assert grey == "mono8" and replay.Dataset.raw_image is replay.Dataset.image


def test_encoding_names_through_the_library(pkg):
    """plv_encoding_from_name / plv_encoding_bytes_per_pixel: host logic, no device needed"""
    assert pkg.ENCODINGS == ref.ENCODINGS
    for name, value in ref.ENCODINGS.items():
        assert pkg.encoding_from_name(name) == value
        assert pkg.encoding_bytes_per_pixel(value) == ref.BPP[name]
    for name in ("mono16", "bayer_rggb16", "yuv422", "", "MONO8", "bgr8 ", "rgb"):
        assert pkg.encoding_from_name(name) == -1, name
    assert pkg.load_library().plv_encoding_from_name(None) == -1
    for value in (-1, 9, 1000):
        assert pkg.encoding_bytes_per_pixel(value) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_conversion_kernel_uses_no_scratch(tmp_path):
    """every instance of grey_from_encoded_kernel (encoding class x source kind), cross-compiled for gfx950 with the Makefile's flags"""
    src = os.path.join(ROOT, "pl-viwo_amd", "csrc", "encoding_kernels.hip")
    out = str(tmp_path / "encoding_kernels.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-result",
                        "--cuda-device-only", "-S", "-o", out, src], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read()
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text):
        found[m.group(1)] = int(m.group(2))
    inst = {k: v for k, v in found.items() if "grey_from_encoded_kernel" in k}
    assert len(inst) == 8, sorted(found)          # copy, Bayer, 3-byte, 4-byte  x  HBM, pinned host block
    assert all(v == 0 for v in inst.values()), inst
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) >= 8 and max(spills) == 0
