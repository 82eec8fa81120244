"""Jacobian parity block by block (test infrastructure of test_gpu_jacobian.py / test_gpu_lines.py).

The parity tests hold |device - oracle| to 1e-9 of the largest entry of the whole batch.  A line Jacobian's entries reach 7e7 (the
rotation blocks of a Pluecker line seen through pixel-scale intrinsics), so that bound lets a block of small entries — the time offset
column, a position block next to a rotation block — be wrong in its fourth digit.  Here every block of state columns is held to 1e-9
of the largest oracle entry OF THAT BLOCK over the batch: clone rotations, clone positions, time offset, extrinsic rotation, extrinsic
position, focal lengths + centre, distortion; Hf; the residual."""
import numpy as np


def state_blocks(st, cols):
    """{block name: column indices} of the Jacobian columns `cols` (state index per column) for the state view `st`"""
    c = st.c
    cols = np.asarray(cols)
    idx = {}

    def put(name, first, size):
        if first >= 0:
            j = np.nonzero((cols >= first) & (cols < first + size))[0]
            if len(j):
                idx[name] = np.concatenate([idx[name], j]) if name in idx else j
    for sid in st.ids:
        put("clone rotation", int(sid), 3)
        put("clone position", int(sid) + 3, 3)
    put("time offset", c.dt_state_id, 1)
    put("extrinsic rotation", c.extrinsic_state_id, 3)
    put("extrinsic position", c.extrinsic_state_id + 3 if c.extrinsic_state_id >= 0 else -1, 3)
    put("focal + centre", c.intrinsic_state_id, 4)
    put("distortion", c.intrinsic_state_id + 4 if c.intrinsic_state_id >= 0 else -1, 4)
    assert sum(len(j) for j in idx.values()) == len(cols), "a Jacobian column belongs to no block of the state view"
    return idx


def assert_blocks(st, cols, dev, orc, tol=1e-9, label=""):
    """dev, orc = (Hf [F][fdim][ld], Hx [F][k][ld], res [F][ld]).  NaN in the same places; every block to tol x its own largest oracle
    entry.  Returns {block: (difference / largest entry, largest entry)}."""
    (Hf, Hx, res), (Hf_o, Hx_o, res_o) = dev, orc
    parts = {"Hf": (Hf, Hf_o), "res": (res, res_o)}
    for name, j in state_blocks(st, cols).items():
        parts[name] = (Hx[:, j, :], Hx_o[:, j, :])
    out = {}
    for name, (a, b) in parts.items():
        assert np.array_equal(np.isnan(a), np.isnan(b)), (label, name)
        fin = ~np.isnan(b)
        if not fin.any():
            continue
        scale = np.abs(b[fin]).max()
        diff = np.abs(a[fin] - b[fin]).max()
        out[name] = (diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf), scale)
    print(f"{label}: " + ", ".join(f"{k} {v[0]:.1e} (of {v[1]:.2g})" for k, v in out.items()))
    for name, (rel, scale) in out.items():
        assert rel <= tol, (label, name, rel, scale)
    return out
