"""The line map's definition (DESIGN.md "The line map") restated in numpy: the reference of tests/test_line_segments_cpu.py and
tests/test_gpu_line_segments.py.  The reference project has no computation to compare with (LineHelper.cpp:476-493 is commented
out), so the definition is the library's own and this file is its second statement, written from DESIGN.md and not from the kernel.

Inputs are plain arrays; `segments_of(st, lt)` reads them out of a StateView / LineTracks pair."""
import numpy as np

import synth

MAX_VIEWS = 64


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _exp_so3(w):            # REF quat_ops.h:231-251
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = _skew(w)
    A, B = (1.0, 0.5) if th < 1e-7 else (np.sin(th) / th, (1 - np.cos(th)) / th ** 2)
    return np.eye(3) + A * K + B * K @ K


def _log_so3(R):            # REF quat_ops.h:273-313 (the branch for rotations away from pi: a clone window never turns that far)
    tr = np.trace(R)
    assert tr + 1.0 >= 1e-10
    if tr - 3.0 < -1e-7:
        th = np.arccos((tr - 1.0) / 2.0)
        mag = th / (2.0 * np.sin(th))
    else:
        mag = 0.5 - (tr - 3.0) / 12.0
    return mag * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def bounding_start(ct, t, dt_exp):
    """State::bounding_times + bounding_poses_n for order 3 (REF: State.cpp:1023-1136): first of the four clones, or -1"""
    N = len(ct)
    if N < 4 or t < ct[0] - dt_exp or t > ct[N - 1]:
        return -1
    nb = next((i for i in range(N - 1) if ct[i] - dt_exp <= t <= ct[i + 1] + dt_exp), -1)
    if nb < 0:
        return -1
    if nb - 1 < 0:
        return 0
    return N - 4 if nb + 2 >= N else nb - 1


def interpolated_pose(ct, cR, cp, s0, t):
    """State::get_interpolated_pose_poly (REF: State.cpp:979-1021): the cubic through clones s0 .. s0 + 3 on so(3) x R^3"""
    R0, p0 = cR[s0], cp[s0]
    th = np.array([_log_so3(cR[s0 + 1 + w] @ R0.T) for w in range(3)])
    dp = np.array([cp[s0 + 1 + w] - p0 for w in range(3)])
    d = np.array([ct[s0 + 1 + w] - ct[s0] for w in range(3)])
    V = np.stack([d, d ** 2, d ** 3], axis=1)
    lam = np.array([t - ct[s0], (t - ct[s0]) ** 2, (t - ct[s0]) ** 3]) @ np.linalg.inv(V)
    return _exp_so3(lam @ th) @ R0, p0 + lam @ dp


def line_segments(clone_time, clone_R, clone_p, R_ItoC, p_IinC, cam_dt, dt_exp, obs_ptr, obs_time, seg_uvn, line_FinG, res_R=None, res_p=None,
                  detail=False):
    """-> end_points [L, 6], extent [L, 2], n_views [L], ok [L]; with detail also the per-line ascending (lows, highs) lists"""
    ct = np.asarray(clone_time, float)
    cR, cp = np.asarray(clone_R, float).reshape(-1, 3, 3), np.asarray(clone_p, float).reshape(-1, 3)
    R_ItoC, p_IinC = np.asarray(R_ItoC, float).reshape(3, 3), np.asarray(p_IinC, float).reshape(3)
    uvn = np.asarray(seg_uvn, np.float32).reshape(-1, 4).astype(float)
    lines = np.asarray(line_FinG, float).reshape(-1, 6)
    L = len(lines)
    ep, ext, nv, ok, sorted_lists = np.zeros((L, 6)), np.zeros((L, 2)), np.zeros(L, np.int32), np.zeros(L, np.uint8), []
    for l in range(L):
        sorted_lists.append((np.zeros(0), np.zeros(0)))
        n, v = lines[l, :3], lines[l, 3:]
        vv = v @ v
        if not np.all(np.isfinite(lines[l])) or not (vv > 0) or not np.isfinite(vv):
            continue
        vh, p0 = v / np.sqrt(vv), np.cross(v, n) / vv
        usable = [o for o in range(obs_ptr[l], obs_ptr[l + 1]) if bounding_start(ct, obs_time[o] + cam_dt, dt_exp) >= 0]
        lows, highs = [], []
        for o in usable[-MAX_VIEWS:]:                       # the track is in time order: the newest 64
            tm = obs_time[o] + cam_dt
            if res_R is not None:
                R_GtoI, p_IinG = np.asarray(res_R, float).reshape(-1, 3, 3)[o], np.asarray(res_p, float).reshape(-1, 3)[o]
            else:
                R_GtoI, p_IinG = interpolated_pose(ct, cR, cp, bounding_start(ct, tm, dt_exp), tm)
            R_GtoC = R_ItoC @ R_GtoI
            c = p_IinG - R_GtoC.T @ p_IinC
            w = c - p0
            d = vh @ w
            s, kept = [], True
            for j in range(2):
                r = R_GtoC.T @ np.array([uvn[o, 2 * j], uvn[o, 2 * j + 1], 1.0])
                b, q, g = vh @ r, r @ r, r @ w
                den = q - b * b
                if den < 1e-6 * q:
                    kept = False
                    continue
                sj, uj = (q * d - b * g) / den, (b * d - g) / den
                kept = kept and uj > 0 and np.isfinite(sj)
                s.append(sj)
            if kept:
                lows.append(min(s)), highs.append(max(s))
        k = len(lows)
        nv[l] = k
        lows, highs = np.sort(lows), np.sort(highs)
        sorted_lists[-1] = (lows, highs)
        if k == 0:
            continue
        lo, hi = lows[(k - 1) // 2], highs[(k - 1) // 2]
        ep[l], ext[l], ok[l] = np.concatenate([p0 + lo * vh, p0 + hi * vh]), (lo, hi), 1
    return (ep, ext, nv, ok, sorted_lists) if detail else (ep, ext, nv, ok)


def segments_of(st, lt, line_FinG=None, detail=False):
    """the same from a StateView and a LineTracks (line_FinG: instead of the tracks' own)"""
    c = st.c
    return line_segments(st.t, st.R, st.p, np.array(c.R_ItoC[:]), np.array(c.p_IinC[:]), c.cam_dt, c.dt_exp, lt.ptr, lt.t, lt.uvn,
                         lt.lg if line_FinG is None else line_FinG, lt.rR, lt.rp, detail=detail)


# ------------------------------------------------------------------------------------------------ scenes the tests share
def replay_line_scene(sc, L=40, M=15, seed=5, w=752, h=480, depth=(6.0, 40.0)):
    """synth.line_scene's random draws, replayed with its seed: the (a, d, half) of every line it kept (the generator returns the
    Pluecker lines only).  The caller checks the replay against those."""
    rng = np.random.default_rng(seed)
    K8, R_ItoC, p_IinC = sc["K8"], sc["R_ItoC"], sc["p_IinC"]
    n_clones = len(sc["t"])
    out = []
    while len(out) < L:
        a = np.array([rng.uniform(-15, 15), rng.uniform(-10, 10), rng.uniform(*depth)])
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        half = rng.uniform(1.0, 4.0)
        m = M if len(out) % 3 else max(3, M - int(rng.integers(0, M // 2 + 1)))
        ok = True
        for ci in range(n_clones - m, n_clones):
            R, p = sc["R"][ci], sc["p"][ci]
            for sgn in (-1.0, 1.0):
                P3 = a + sgn * half * (1 + 0.1 * rng.uniform(-1, 1)) * d
                pc = R_ItoC @ (R @ (P3 - p)) + p_IinC
                xn = pc[:2] / pc[2]
                uv = np.array([K8[0] * xn[0] + K8[2], K8[1] * xn[1] + K8[3]])
                ok = ok and pc[2] > 1 and 5 < uv[0] < w - 5 and 5 < uv[1] < h - 5
        if not ok:
            continue
        for _ in range(m):
            rng.normal(0, 1.0, 4), rng.normal(0, 1.0, 4)      # (the two noise draws per view)
        out.append((a, d, half))
    return out


def gpu_scene():
    """The tracks tests/test_gpu_line_segments.py sends through plv_line_segments: 67 lines; observations per line 1, 2, 3, 63, 64, 65
    (and the generator's own counts); unusable observations — no bounding clones, a ray parallel to the line — interleaved among the
    usable ones; off-clone observation times so that the polynomial is evaluated.  Returns plain arrays (vio scene, line scene)."""
    sc = synth.vio_scene(n_clones=15, F=4, dt_clone=0.2, seed=3)
    base = synth.line_scene(sc, L=67, M=12, seed=11, noise_px=0.5)
    truth = replay_line_scene(sc, L=67, M=12, seed=11)      # (a, d, half) of the generator's lines
    rng = np.random.default_rng(7)
    t0, t1 = sc["t"][0], sc["t"][-1]
    counts = {0: 1, 1: 2, 2: 3, 3: 63, 4: 64, 5: 65, 66: 65}
    ptr, times, uvn = [0], [], []
    for l in range(67):
        a, b = base["obs_ptr"][l], base["obs_ptr"][l + 1]
        if l in counts:      # the line's first view, repeated with a little noise at ascending times across the window
            m = counts[l]
            tt = np.sort(rng.uniform(t0, t1, m))
            R_p = [sc["pose_fn"](x) for x in tt]
            a_, d_, half = truth[l]
            rows = []
            for (R, p), x in zip(R_p, tt):
                row = []
                for s in (half * rng.uniform(-1.1, -0.9), half * rng.uniform(0.9, 1.1)):
                    pc = sc["R_ItoC"] @ (R @ (a_ + s * d_ - p)) + sc["p_IinC"]
                    row += [pc[0] / pc[2], pc[1] / pc[2]]
                rows.append(row)
            tl, ul = list(tt), rows
        else:
            tl = list(base["obs_time"][a:b] + np.where(base["obs_time"][a:b] < t1, 0.013, 0.0))
            ul = [list(r) for r in base["seg_uvn"][a:b]]
        if l % 5 == 1 and len(tl) >= 2:      # an observation outside the window in the middle of the track
            tl.insert(len(tl) // 2, t1 + 1.0), ul.insert(len(ul) // 2, ul[0])
        if l % 7 == 6 and len(tl) >= 2:      # ... and one whose first ray is parallel to the line
            R, p = sc["pose_fn"](tl[1])
            r = (sc["R_ItoC"] @ R) @ base["lines"][l, 3:]
            if abs(r[2]) > 1e-3:
                ul[1] = [r[0] / r[2], r[1] / r[2], ul[1][2], ul[1][3]]
        times += tl
        uvn += ul
        ptr.append(len(times))
    ls = dict(lines=base["lines"].copy(), obs_ptr=np.array(ptr, np.int32), obs_time=np.array(times), seg_uvn=np.array(uvn, np.float32),
              seg_uv=np.zeros((len(times), 4), np.float32))
    return sc, ls
