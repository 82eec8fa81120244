"""The line map's definition (DESIGN.md "The line map") on its numpy restatement, tests/line_segments_ref.py — the reference the GPU
tests (tests/test_gpu_line_segments.py) hold plv_line_segments to.  No GPU here: ground truth on the synthetic line scene, every rule
of the definition on a hand-made case, the well-posedness of the scene the GPU test uses, and the library's new exports, bindings
and adapter methods."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_segments_ref as ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pl-viwo_amd", "host")
STUB = os.path.join(ROOT, "tests", "host_stub")


# ------------------------------------------------------------------------------------------------ ground truth
def scene_arrays(sc, ls, lines=None, **kw):
    return ref.line_segments(sc["t"], sc["R"], sc["p"], sc["R_ItoC"], sc["p_IinC"], kw.pop("cam_dt", 0.0), 0.01, ls["obs_ptr"], ls["obs_time"],
                             ls["seg_uvn"], ls["lines"] if lines is None else lines, **kw)


def test_end_points_lie_at_the_true_segment_ends():
    """The generator draws every view's visible half-length in half * [0.9, 1.1] on both sides, so the lower median of the views'
    extents lies in that interval too: P1 within 0.1 * half of a - half * d, P2 of a + half * d (the rays meet the true line exactly
    up to the float32 of seg_uvn, ~1e-6 m)."""
    sc = synth.vio_scene(F=4)
    ls = synth.line_scene(sc, L=40, noise_px=0)
    truth = ref.replay_line_scene(sc, L=40)
    assert np.allclose(ls["lines"], [np.concatenate([np.cross(a, d), d]) for a, d, _ in truth], rtol=0, atol=1e-12)
    ep, ext, nv, ok = scene_arrays(sc, ls)
    assert ok.all() and (nv == np.diff(ls["obs_ptr"])).all()
    for l, (a, d, half) in enumerate(truth):
        assert np.linalg.norm(ep[l, :3] - (a - half * d)) <= 0.1 * half, l
        assert np.linalg.norm(ep[l, 3:] - (a + half * d)) <= 0.1 * half, l
        assert ext[l, 1] - ext[l, 0] >= 1.8 * half - 1e-6


# ------------------------------------------------------------------------------------------------ the rules, one hand-made case each
T = 10.0 + 0.1 * np.arange(6)


def hand_case(cam_p, uvn, line, times=None, n_clones=6):
    """Identity rotations (IMU = camera), the cameras at cam_p [M, 3] — one observation each, at the clone times unless given — and
    the line's segments uvn [M, 4]"""
    t = 10.0 + 0.1 * np.arange(n_clones)
    cam_p = np.asarray(cam_p, float)
    M = len(cam_p)
    times = t[:M] if times is None else np.asarray(times, float)
    clone_p = np.zeros((n_clones, 3))
    clone_p[:min(M, n_clones)] = cam_p[:n_clones]
    return dict(clone_time=t, clone_R=np.tile(np.eye(3), (n_clones, 1, 1)), clone_p=clone_p, R_ItoC=np.eye(3), p_IinC=np.zeros(3), cam_dt=0.0,
                dt_exp=0.01, obs_ptr=np.array([0, M], np.int32), obs_time=times, seg_uvn=np.asarray(uvn, np.float32),
                line_FinG=np.asarray(line, float).reshape(1, 6), res_R=np.tile(np.eye(3), (M, 1, 1)), res_p=cam_p)


# the line x = s, y = 0, z = 5: direction e_x, through (0, 0, 5); moment = (0, 0, 5) x e_x = (0, 5, 0)
LINE_X = np.array([0.0, 5.0, 0.0, 1.0, 0.0, 0.0])


def view_of(cam, s1, s2, line_z=5.0):
    """normalised segment of the points (s1, 0, z) and (s2, 0, z) seen from `cam` (identity rotation)"""
    out = []
    for s in (s1, s2):
        pc = np.array([s, 0.0, line_z]) - cam
        out += [pc[0] / pc[2], pc[1] / pc[2]]
    return out


def test_one_view_gives_its_own_extent():
    c = hand_case([[0.5, 0.2, 0]], [view_of([0.5, 0.2, 0], -1.0, 2.0)], LINE_X)
    ep, ext, nv, ok = ref.line_segments(**c)
    assert ok[0] == 1 and nv[0] == 1
    assert np.allclose(ext[0], [-1.0, 2.0], atol=1e-6) and np.allclose(ep[0], [-1, 0, 5, 2, 0, 5], atol=1e-6)


def test_end_points_are_ordered_along_the_direction():
    c = hand_case([[0, 0.1, 0]], [view_of([0, 0.1, 0], 2.0, -1.0)], LINE_X)      # the detector's order is arbitrary
    ep, ext, _, _ = ref.line_segments(**c)
    assert ext[0, 0] < ext[0, 1] and np.allclose(ep[0], [-1, 0, 5, 2, 0, 5], atol=1e-6)


def test_no_counted_view_is_ok_zero_and_zeros():
    c = hand_case([[0, 0, 0]], [view_of([0, 0, 0], -1.0, 1.0)], LINE_X, times=[20.0])      # no bounding clones
    ep, ext, nv, ok = ref.line_segments(**c)
    assert ok[0] == 0 and nv[0] == 0 and not ep.any() and not ext.any()


def test_a_ray_parallel_to_the_line_is_rejected():
    # the line along the optical axis through (1, 0, *): the ray (0, 0, 1) is parallel to it
    line = np.concatenate([np.cross([1.0, 0, 0], [0, 0, 1.0]), [0, 0, 1.0]])
    cams = [[0, 0, 0], [0.3, 0, 0]]
    good = [1.0 / 4.0, 0.0, 1.0 / 8.0, 0.0]                # (1, 0, 4) and (1, 0, 8) from the origin
    bad = [0.0, 0.0, 1.0 / 8.0, 0.0]                       # first end point: the optical axis itself
    second = [0.7 / 4.0, 0.0, 0.7 / 8.0, 0.0]
    ep, ext, nv, ok = ref.line_segments(**hand_case(cams, [good, second], line))
    assert nv[0] == 2
    ep, ext, nv, ok = ref.line_segments(**hand_case(cams, [bad, second], line))
    assert nv[0] == 1 and ok[0] == 1 and np.allclose(ext[0], [4.0, 8.0], atol=1e-5)      # the whole first observation is out
    # just inside / outside 1e-3 rad: den / q = sin^2(angle)
    for ang, counted in ((2e-3, 2), (5e-4, 1)):
        near = [np.tan(ang), 0.0, 1.0 / 8.0, 0.0]
        assert ref.line_segments(**hand_case(cams, [near, second], line))[2][0] == counted


def test_an_end_point_behind_the_camera_drops_the_observation():
    # camera 1 looks along +z from z = 10: the line at z = 5 is behind it, its rays meet the line at negative range
    cams = [[0, 0.1, 0], [0, 0.1, 10.0]]
    views = [view_of(cams[0], -1.0, 1.0), view_of(cams[1], -3.0, 3.0)]
    ep, ext, nv, ok = ref.line_segments(**hand_case(cams, views, LINE_X))
    assert nv[0] == 1 and np.allclose(ext[0], [-1.0, 1.0], atol=1e-6)
    # one end point in front, one behind: a camera beside the line, looking across it, the line passing through its image plane
    line = np.concatenate([np.cross([0.0, 0, 1.0], [1.0, 0, 1.0]), [1.0, 0, 1.0]])     # through (0, 0, 1) along (1, 0, 1)
    cams = [[0, 0.1, 0], [0.2, 0.1, 0]]
    front = lambda cam, s: [(s - cam[0]) / (1.0 + s), (0.0 - cam[1]) / (1.0 + s)]            # point (s, 0, 1 + s)
    v_ok = front(cams[0], 0.5) + front(cams[0], 2.0)
    v_half = front(cams[1], 0.5) + front(cams[1], -3.0)                                     # (-3, 0, -2): behind
    ep, ext, nv, ok = ref.line_segments(**hand_case(cams, [v_ok, v_half], line))
    assert nv[0] == 1


def test_even_count_takes_the_lower_median():
    cams = [[0.1 * i, 0.1, 0] for i in range(4)]
    lows, highs = [-1.0, -1.4, -1.2, -1.1], [2.0, 2.6, 2.2, 2.4]
    views = [view_of(c, lo, hi) for c, lo, hi in zip(cams, lows, highs)]
    ep, ext, nv, ok = ref.line_segments(**hand_case(cams, views, LINE_X))
    assert nv[0] == 4
    assert np.allclose(ext[0], [sorted(lows)[1], sorted(highs)[1]], atol=1e-6)      # index (4 - 1) // 2 = 1 of each list on its own
    # odd: the median proper
    ep, ext, nv, ok = ref.line_segments(**hand_case(cams[:3], views[:3], LINE_X))
    assert np.allclose(ext[0], [-1.2, 2.2], atol=1e-6)


def test_zero_direction_or_non_finite_line_is_ok_zero():
    cams = [[0, 0.1, 0]]
    views = [view_of(cams[0], -1.0, 1.0)]
    for line in ([0, 5.0, 0, 0, 0, 0], [0, np.nan, 0, 1, 0, 0], [0, 5.0, 0, np.inf, 0, 0]):
        ep, ext, nv, ok = ref.line_segments(**hand_case(cams, views, line))
        assert ok[0] == 0 and nv[0] == 0 and not ep.any()


def test_of_65_usable_views_the_newest_64_count():
    n = 65
    t = 10.0 + 0.5 * np.arange(6)
    times = np.linspace(t[0], t[-1], n)
    cams = np.array([[0.01 * i, 0.1, 0] for i in range(n)])
    lows = np.full(n, -1.0)
    lows[0] = -50.0                                  # the oldest view alone reaches far out
    views = [view_of(cams[i], lows[i], 2.0 + 0.01 * i) for i in range(n)]
    c = hand_case(cams, views, LINE_X, times=times)
    c["clone_time"] = t
    ep, ext, nv, ok, det = ref.line_segments(detail=True, **c)
    assert nv[0] == 64 and np.allclose(det[0][0].min(), -1.0, atol=1e-6)      # -50 is not among the lows
    assert np.allclose(ext[0, 1], np.sort(2.0 + 0.01 * np.arange(1, n))[(64 - 1) // 2], atol=1e-6)
    # an unusable view in between does not use up one of the 64 places
    times2 = np.concatenate([times[:10], [99.0], times[10:]])
    cams2 = np.concatenate([cams[:10], [[0, 0.1, 0]], cams[10:]])
    views2 = views[:10] + [views[0]] + views[10:]
    c2 = hand_case(cams2, views2, LINE_X, times=times2)
    c2["clone_time"] = t
    assert np.array_equal(ref.line_segments(**c2)[1], ext)


def test_the_scale_of_the_pluecker_vector_does_not_matter():
    sc = synth.vio_scene(F=4)
    ls = synth.line_scene(sc, L=12, noise_px=0.5)
    a = scene_arrays(sc, ls)
    b = scene_arrays(sc, ls, lines=3.0 * ls["lines"])
    assert np.allclose(a[0], b[0], rtol=0, atol=1e-9) and np.allclose(a[1], b[1], rtol=0, atol=1e-9) and (a[2] == b[2]).all()


# ------------------------------------------------------------------------------------------------ the scene of the GPU test
def test_the_gpu_scene_has_no_near_ties_at_the_medians():
    """A selection that flips between two neighbours of the sorted list must show as an error far above the 1e-9 the GPU test allows,
    and rounding must not be able to flip it: at every line's median index the sorted lows (and highs) have neighbours more than 1e-6
    away.  The scene also holds every case the GPU test is after."""
    sc, ls = ref.gpu_scene()
    ep, ext, nv, ok, det = scene_arrays(sc, ls, detail=True)
    n_obs = np.diff(ls["obs_ptr"])
    assert {1, 2, 3, 63, 64}.issubset(set(nv.tolist())) and n_obs.max() >= 65 and (nv <= 64).all()
    assert (nv < n_obs).sum() >= 10 and ok.sum() >= 60      # unusable observations among usable ones
    for l in range(len(nv)):
        k = nv[l]
        for arr in det[l]:
            if k >= 2:
                i = (k - 1) // 2
                gaps = [abs(arr[i] - arr[j]) for j in (i - 1, i + 1) if 0 <= j < k]
                assert min(gaps) > 1e-6, (l, k, gaps)


# ------------------------------------------------------------------------------------------------ library, bindings, adapter
def test_the_library_exports_and_binds_the_line_map(pkg):
    lib = pkg.load_library()
    for name in ("plv_line_segments", "plv_line_map_mode", "plv_camera_used_lines"):
        assert hasattr(lib, name) and name in lib._plv_signatures, name
    for name in ("line_segments", "line_map_mode", "camera_used_lines"):
        assert callable(getattr(pkg.Context, name)), name
    from importlib import import_module
    sm = import_module(pkg.__name__ + ".system").SystemManager
    assert all(callable(getattr(sm, n)) for n in ("get_used_msckf", "get_used_lines", "get_slam_cloud"))


PUBLISHER = """
#include "UpdaterCameraHIP.h"
using namespace std;
using namespace Eigen;
// ROSPublisher::publish_cam_features' reads (REF: ROSPublisher.cpp:227, 238), the updater's class name changed and nothing else
size_t publish_cam_features(shared_ptr<viw::UpdaterCameraHIP> up_cam) {
  vector<Vector3d> feats_msckf = up_cam->get_used_msckf();
  vector<Matrix<double, 6, 1>> feats_line = up_cam->get_used_lines();
  up_cam->line_map(true);
  return feats_msckf.size() + feats_line.size();
}
"""


def test_the_publishers_reads_compile_against_the_adapter(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "publish_cam_features.cpp"
    src.write_text(PUBLISHER)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + STUB, "-I" + os.path.join(ROOT, "include"),
                        "-I" + HOST, str(src)], capture_output=True, text=True)
    errors = [l for l in r.stderr.splitlines() if "error" in l or "warning" in l]
    assert r.returncode == 0 and not errors, "\n".join(errors[:20])


def test_the_map_file_is_an_ascii_ply_with_an_edge_per_segment(pkg, tmp_path):
    """replay.MapAccumulator (tools/replay.py --map): vertices = MSCKF points, landmarks, segment end points with their `kind`, one
    edge per segment between its two end points; the statistics the tool adds to its result line."""
    from importlib import import_module
    rp = import_module(pkg.__name__ + ".replay")
    m = rp.MapAccumulator()
    m.points = [np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]), np.zeros((0, 3))]
    m.segments = [np.zeros((0, 6)), np.array([[0.0, 0, 0, 3.0, 4.0, 0], [1.0, 1, 1, 1.0, 1, 3.0]])]
    m.landmarks = {9: np.array([7.0, 8.0, 9.0])}
    assert m.stats() == dict(map_points=3, map_lines=2, map_line_length_p50=3.5)
    path = str(tmp_path / "out" / "map.ply")
    m.write_ply(path)
    lines = open(path).read().splitlines()
    assert lines[:2] == ["ply", "format ascii 1.0"] and "element vertex 7" in lines and "element edge 2" in lines
    body = lines[lines.index("end_header") + 1:]
    assert len(body) == 7 + 2
    assert [int(x.split()[3]) for x in body[:7]] == [0, 0, 1, 2, 2, 2, 2]
    assert [float(v) for v in body[2].split()[:3]] == [7.0, 8.0, 9.0] and [float(v) for v in body[4].split()[:3]] == [3.0, 4.0, 0.0]
    assert body[7:] == ["3 4", "5 6"]
    empty = rp.MapAccumulator()
    assert empty.stats() == dict(map_points=0, map_lines=0, map_line_length_p50=0.0)


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_line_segments_kernel_uses_no_scratch_and_no_lds(tmp_path):
    """The kernel keeps a line's vectors, a pose and two sort keys per lane in registers (an index that varies by lane into one of the
    vectors would send them to scratch memory): private_segment_fixed_size and group_segment_fixed_size of the compiler's metadata,
    cross-compiled for gfx950 with the flags of pl-viwo_amd/Makefile."""
    import re
    src = os.path.join(ROOT, "pl-viwo_amd", "csrc", "line_map_kernels.hip")
    out = str(tmp_path / "line_map_kernels.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-result",
                        "--cuda-device-only", "-S", "-o", out, src], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read()
    m = re.search(r"\.name:\s+(\S*line_segments_kernel\S*)\n", text)
    assert m, "line_segments_kernel is not in the assembly's metadata"
    start, end = text.rfind("\n  - .", 0, m.start()), text.find("\n  - .", m.end())
    meta = dict(re.findall(r"\.(\w+):\s+(\d+)\n", text[start:end if end > 0 else len(text)]))
    assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["group_segment_fixed_size"]) == 0, meta
    assert int(meta.get("vgpr_spill_count", 0)) == 0 and int(meta["vgpr_count"]) <= 128, meta      # (<= 128: four waves per SIMD)
