"""CPU tests: the track image's declarations — pl-viwo_amd/host/TrackImageHIP.h through a compiler against the stand-ins of
tests/host_stub (as tests/test_host_shims.py does for the other adapters), and the new entry points in include/plviwo.h, which
tests/test_abi.py then holds to the export table and the bindings."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pl-viwo_amd", "host")
STUB = os.path.join(ROOT, "tests", "host_stub")
SYMBOLS = ("plv_draw_primitives", "plv_track_image", "plv_track_image_primitives", "plv_track_image_options_default",
           "plv_line_tracker_last_points")


def _syntax_only(path, *flags):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", *flags, "-x", "c++", "-I" + STUB,
                        "-I" + os.path.join(ROOT, "include"), "-I" + HOST, path], capture_output=True, text=True)
    errors = [l for l in r.stderr.splitlines() if "error" in l or ("warning" in l and "#pragma once in main file" not in l)]
    return r.returncode, errors


def test_track_image_adapter_type_checks():
    rc, errors = _syntax_only(os.path.join(HOST, "TrackImageHIP.h"), "-DCV_8UC3=16")
    assert rc == 0 and not errors, "\n".join(errors[:20])


def test_a_display_override_compiles(tmp_path):
    """the use INTEGRATION.md describes: a caller-owned CV_8UC3 matrix handed to plv_host::track_image"""
    src = tmp_path / "use.cpp"
    src.write_text('#include "TrackImageHIP.h"\n'
                   'int picture(plv_ctx *ctx, const std::vector<size_t> &slam_ids, unsigned char *pixels, int w, int h) {\n'
                   '  cv::Mat out(h, w, CV_8UC3, pixels);\n'
                   '  return plv_host::track_image(ctx, slam_ids, PLV_VIZ_HISTORY | PLV_VIZ_LINES | PLV_VIZ_MASK, out);\n'
                   '}\n')
    rc, errors = _syntax_only(str(src), "-DCV_8UC3=16")
    assert rc == 0 and not errors, "\n".join(errors[:20])
    src.write_text('#include "TrackImageHIP.h"\nint f(plv_ctx *c, cv::Mat &m) { return plv_host::track_image(c, 3, 1, m); }\n')   # ids, not a count
    assert _syntax_only(str(src), "-DCV_8UC3=16")[0] != 0


def test_nothing_existing_includes_the_adapter():
    for name in os.listdir(HOST):
        if name.endswith(".h") and name != "TrackImageHIP.h":
            assert "TrackImageHIP.h" not in open(os.path.join(HOST, name)).read(), name


def test_header_declares_the_track_image():
    txt = open(os.path.join(ROOT, "include", "plviwo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    for name in ("PLV_DRAW_RING", "PLV_DRAW_BOX", "PLV_DRAW_SEG", "PLV_VIZ_HISTORY", "PLV_VIZ_ACTIVE", "PLV_VIZ_LINES", "PLV_VIZ_MASK",
                 "plv_draw_prim", "plv_track_image_options"):
        assert re.search(r"\b%s\b" % name, code), name


def test_primitive_is_32_bytes_and_the_header_stays_c11(pkg, tmp_path):
    import ctypes as C
    assert C.sizeof(pkg.PlvDrawPrim) == 32 == pkg.DRAW_PRIM_DTYPE.itemsize
    assert [f[0] for f in pkg.PlvTrackImageOptions._fields_] == ["layers", "r1", "g1", "b1", "r2", "g2", "b2", "max_tracks", "n_highlighted",
                                                                 "highlighted", "n_flagged", "flagged"]
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include "plviwo.h"\n_Static_assert(sizeof(plv_draw_prim) == 32, "plv_draw_prim");\n'
                   'int main(void) { plv_track_image_options o; plv_track_image_options_default(&o);\n'
                   '  return (o.layers == PLV_VIZ_HISTORY && o.max_tracks == 50 && o.r1 == 255 && o.b1 == 0 && o.b2 == 255 && !o.highlighted) ? 0 : 1; }\n')
    exe = tmp_path / "t"
    lib_dir = os.path.join(ROOT, "pl-viwo_amd", "lib")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", lib_dir, "-lplviwo_hip", "-Wl,-rpath," + lib_dir], check=True)
    assert subprocess.run([str(exe)]).returncode == 0                             # (host logic: needs no device)


def test_layer_names(pkg):
    assert pkg.viz_layers("history,lines, mask") == 1 | 4 | 8 and pkg.viz_layers(["active"]) == 2 and pkg.viz_layers(5) == 5
    with pytest.raises(ValueError):
        pkg.viz_layers("history,text")
