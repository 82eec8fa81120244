"""The case matrix of the blocked factorisation (csrc/blocked_chol.hpp) behind its four launchers, and the extended-precision
restatements its results are held to.  tests/test_chol_cases_cpu.py proves on the CPU that every case contains what it claims;
tests/test_gpu_blocked_chol.py runs the cases on the device through the public C-ABI wrappers.

The launchers pick the instantiation (NT 16-row strips) from the size: <= 32 -> 2, 64 -> 4, 112 -> 7, 128 -> 8, 160 -> 10, 192 -> 12;
the number of tiles the matrix really has, ceil(size / 16), can be smaller than NT, which is when the `p < ntk` / `t < ntk` branches
and the strip maps of NT = 7 and 8 matter.  The sections:
  1  whitened update (prior factor and EKF solve with r = k) at every (NT, tiles) pair, three widths per tile count;
  2  exact dependencies in the prior block (a pose and its fresh clone), placed in the first tile, across the last tile boundary and
     as the last columns, one width per instantiation: the factor form;
  3  the not-positive-definite exit raised by the first and by the last pivot of the first, a middle and the last panel, by an
     indefinite block of the covariance and by a negative noise entry (which nothing but the factorisation's own report rejects);
  4  chi2 by value at every projected row count of both gate instantiations;
  5  border strips: the residual row as the last row of a full strip and alone in a strip of its own.
The reference of every numeric comparison is written out in numpy.longdouble (numpy's linalg has no extended precision)."""
import functools
import math

import numpy as np

import synth

PLV_PRIOR_TAU = 2e-13            # csrc/blocked_chol.hip: pivots of the unit-diagonal prior block below it are exact dependencies
PLV_PRIOR_AMB = 1e-4             # ... below it near dependencies
PLV_WHITEN_LAMBDA_MAX = 1e2      # ... B's largest diagonal entry beyond which the factor form hands the update over
THRESHOLDS = ((32, 2), (64, 4), (112, 7), (128, 8), (160, 10), (192, 12))   # launch_bchol_ekf / launch_bchol_prior
SIGMA2 = 2.25

ld_t = np.longdouble


def launch_nt(size):
    """the instantiation the launchers pick for a size x size factorisation"""
    for limit, nt in THRESHOLDS:
        if size <= limit:
            return nt
    raise ValueError(size)


def tiles(size):
    return (size + 15) // 16


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@functools.lru_cache(maxsize=None)
def q95():
    return synth.q95_table()


# ------------------------------------------------------------------------------------------ restatements
def truth(P, rows, Hf, Hx, res, cols, acc):
    """information-form update in extended precision on the accepted, projected rows: P' = (P^-1 + H^T H)^-1, dx = P' H^T r"""
    ld = np.longdouble
    n = P.shape[0]
    Hp, r = project(rows, Hf, Hx, res, acc)
    H = np.zeros((Hp.shape[0], n))
    H[:, cols] = Hp
    # K form in long double with a Cholesky solve written out (numpy's linalg has no extended precision)
    Hl, Pl, rl = H.astype(ld), P.astype(ld), r.astype(ld)
    S = Hl @ Pl @ Hl.T + np.eye(H.shape[0], dtype=ld)
    L = np.zeros_like(S)
    for i in range(S.shape[0]):
        for j in range(i + 1):
            v = S[i, j] - L[i, :j] @ L[j, :j]
            L[i, j] = np.sqrt(v) if i == j else v / L[j, j]
    M = Pl @ Hl.T

    def solve(B):   # S^-1 B
        Y = np.zeros_like(B)
        for i in range(L.shape[0]):
            Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
        X = np.zeros_like(B)
        for i in range(L.shape[0] - 1, -1, -1):
            X[i] = (Y[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
        return X
    KT = solve(M.T)
    return (Pl - M @ KT).astype(np.float64), (KT.T @ rl).astype(np.float64)


def project(rows, Hf, Hx, res, acc):
    """the accepted rows after the nullspace projection, stacked: H (m x k) and r (m).  Any orthonormal basis of Hf's left null space
    gives the same update; this one is LAPACK's."""
    Hs, rs = [], []
    for f in range(len(rows)):
        if not acc[f]:
            continue
        m = int(rows[f])
        q, _ = np.linalg.qr(Hf[f, :, :m].T, mode="complete")
        N = q[:, Hf.shape[1]:]
        Hs.append(N.T @ Hx[f, :, :m].T)
        rs.append(N.T @ res[f, :m])
    return np.vstack(Hs), np.concatenate(rs)


def lu_solve_ld(A, B):
    """A^-1 B in long double: Gaussian elimination with partial pivoting, one row operation per step on [A | B]"""
    k = A.shape[0]
    W = np.concatenate([A.astype(ld_t), B.astype(ld_t)], axis=1)
    for j in range(k):
        p = j + int(np.argmax(np.abs(W[j:, j])))
        if p != j:
            W[[j, p]] = W[[p, j]]
        W[j + 1:, j:] -= np.outer(W[j + 1:, j] / W[j, j], W[j, j:])
    X = np.zeros((k, B.shape[1]), dtype=ld_t)
    for j in range(k - 1, -1, -1):
        X[j] = (W[j, k:] - W[j, j + 1:k] @ X[j + 1:]) / W[j, j]
    return X


def truth_info(P, H, r, cols, Rdiag=None):
    """The EKF update of the rows H (m x k, on the columns `cols`) with residual r and diagonal noise (identity when None), in long
    double and in the information form, a k x k solve however many rows there are, valid for a singular prior block too:
        K = Pc (I + G Ps)^-1 H^T R^-1,  G = H^T R^-1 H,  Pc = P[:, cols],  Ps = P[cols, cols]
        P' = P - Pc (I + G Ps)^-1 G Pc^T,   dx = Pc (I + G Ps)^-1 H^T R^-1 r
    (I + G Ps has the eigenvalues of I + G^1/2 Ps G^1/2: real and >= 1)."""
    n, k = P.shape[0], len(cols)
    Hl, rl, Pl = H.astype(ld_t), r.astype(ld_t), P.astype(ld_t)
    if Rdiag is not None:
        w = 1 / np.sqrt(np.asarray(Rdiag).astype(ld_t))
        Hl, rl = Hl * w[:, None], rl * w
    G, g = Hl.T @ Hl, Hl.T @ rl
    Pc, Ps = Pl[:, cols], Pl[np.ix_(cols, cols)]
    X = lu_solve_ld(np.eye(k, dtype=ld_t) + G @ Ps, np.concatenate([G @ Pc.T, g[:, None]], axis=1))
    return (Pl - Pc @ X[:, :n]).astype(np.float64), (Pc @ X[:, n]).astype(np.float64)


def unit_factor(Ps, tau=PLV_PRIOR_TAU):
    """What bchol_prior_kernel computes, in long double: Ps scaled to unit diagonal, its pivots, and the factor M of Ps itself
    (Ps = M M^T) with a zero column wherever the pivot is <= tau."""
    k = Ps.shape[0]
    d = np.sqrt(np.diag(Ps).astype(ld_t))
    A = Ps.astype(ld_t) / np.outer(d, d)
    L = np.zeros((k, k), dtype=ld_t)
    piv = np.zeros(k)
    for j in range(k):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        piv[j] = float(col[0])
        if col[0] > tau:
            L[j:, j] = col / np.sqrt(col[0])
    return piv, L * d[:, None]


def lambda_max(Ps, H):
    """largest diagonal entry of B = I + M^T G M, G = H^T H"""
    _, M = unit_factor(Ps)
    HM = H.astype(ld_t) @ M
    return float(1 + np.max(np.sum(HM * HM, axis=0)))


# ------------------------------------------------------------------------------------------ sections 1, 2 and 5: stacked updates
M_OBS = 8
ROWS_PROJ = 2 * M_OBS - 3   # every feature is seen M_OBS times: 13 rows after the projection


def n_features(k):
    """enough features for more accepted rows than columns, with a margin of one tile and two features"""
    return math.ceil((k + 16) / ROWS_PROJ) + 2


def _batch(F, k, seed):
    """tests/synth.py's generator (as test_msckf_update_tile_boundaries uses it), every feature with all its rows and none of them an
    outlier; below two clone blocks of columns, where that generator has no layout, dense blocks"""
    if k >= 12:
        return synth.msckf_batch(F=F, M=M_OBS, k=k, seed=seed, ragged=False, outlier_frac=0.0)
    rng = np.random.default_rng(seed)
    ld = 2 * M_OBS
    return (np.full(F, ld, dtype=np.int32), rng.normal(size=(F, 3, ld)), rng.normal(size=(F, k, ld)), rng.normal(0, 0.35, (F, ld)))


def _whitened_ks():
    ks = []
    for t in range(1, 13):
        ks += [3, 15, 16] if t == 1 else [16 * t - 15, 16 * t - 1, 16 * t]
    return ks


WHITENED_K = _whitened_ks()                                    # section 1, mode 0
HOUSEHOLDER_K = [16 * t + d for t in (5, 11) for d in (-15, -1, 0)]   # ... and mode 1
BORDER_N = [15, 16, 31, 32, 47, 48]                            # section 5: k = n - 3
DEPENDENT_K = [29, 61, 109, 125, 157, 189]                     # section 2: 16 t - 3 with the largest tile count of every instantiation
DEPENDENT_PLACES = ("first_tile", "last_boundary", "last_columns")


def dependent_positions(k, place):
    """positions (in the update's column order) of the six columns that repeat columns 0 .. 5"""
    if place == "first_tile":
        first = 6
    elif place == "last_boundary":
        first = 16 * (tiles(k) - 1) - 3
    else:
        first = k - 6
    return list(range(first, first + 6))


def _finish(P, cols, batch):
    """oracle and restatement of a stacked update with the gate open: computed once per case (functools.lru_cache on the builders)"""
    import oracle_lib
    rows, Hf, Hx, res = batch
    orc = oracle_lib.load()
    rc, Po, dxo, acc, nr = orc.msckf_update(P, rows, Hf, Hx, res, cols, SIGMA2, q95(), 1e6, 0.0)
    H, r = project(rows, Hf, Hx, res, acc)
    Pt, dxt = truth_info(P, H, r, cols)
    return dict(P=P, cols=cols, rows=rows, Hf=Hf, Hx=Hx, res=res, H=H, r=r, k=len(cols), n=P.shape[0],
                oracle=dict(rc=rc, P=Po, dx=dxo, acc=acc, n_rows=nr), truth=(Pt, dxt),
                e_oracle=max(rel(Po, Pt), rel(dxo, dxt)))


@functools.lru_cache(maxsize=None)
def whitened_case(k, n=None):
    """sections 1 and 5: n = k + 15 states (or the given n), the update on k of them"""
    n = k + 15 if n is None else n
    P = synth.spd_cov(n, seed=k)
    cols = synth.col_map(n, k, seed=k, skip=15)
    return _finish(P, cols, _batch(n_features(k), k, k))


@functools.lru_cache(maxsize=None)
def dependent_case(k, place):
    """section 2: P = T P0 T^T with T copying the states of the update's columns 0 .. 5 onto those of six later columns — rows and
    columns of P are then equal bit for bit (every entry of the product is one term) — and the measurements' sigma doubled until the
    largest diagonal entry of B = I + M^T G M is below a quarter of PLV_WHITEN_LAMBDA_MAX"""
    n = k + 15
    P0 = synth.spd_cov(n, seed=k)
    cols = synth.col_map(n, k, seed=k, skip=15)
    dep = dependent_positions(k, place)
    T = np.eye(n)
    for i, pos in enumerate(dep):
        T[cols[pos]] = T[cols[i]]
    P = T @ P0 @ T.T
    rows, Hf, Hx, res = _batch(n_features(k), k, k)
    acc = np.ones(len(rows), dtype=bool)
    H, _ = project(rows, Hf, Hx, res, acc)
    Ps = P[np.ix_(cols, cols)]
    sigma = 1.0
    while lambda_max(Ps, H / sigma) >= 0.25 * PLV_WHITEN_LAMBDA_MAX:
        sigma *= 2.0
    c = _finish(P, cols, (rows, Hf, Hx / sigma, res / sigma))
    c.update(dep=dep, sigma=sigma, place=place)
    return c


@functools.lru_cache(maxsize=None)
def border_ekf_case(n, r=10):
    """section 5 through plv_ekf_update: r rows on k = n - 3 columns, the n + 1 border rows [M ; res^T] of the solve"""
    import oracle_lib
    k = n - 3
    P = synth.spd_cov(n, seed=n)
    cols = synth.col_map(n, k, seed=n, skip=15)
    rng = np.random.default_rng(n)
    H = rng.normal(size=(r, k))
    res = rng.normal(size=r)
    Rd = rng.uniform(0.5, 2.0, r)
    rc, Po, dxo = oracle_lib.load().ekf_update(P, H, cols, res, Rd)
    Pt, dxt = truth_info(P, H, res, cols, Rd)
    return dict(P=P, cols=cols, H=H, res=res, Rd=Rd, n=n, k=k, oracle=dict(rc=rc, P=Po, dx=dxo), truth=(Pt, dxt),
                e_oracle=max(rel(Po, Pt), rel(dxo, dxt)))


def whitened_form(c, factor=None, panel=None, delta=0.0):
    """The whitened form of the update (csrc/dense_kernels.hip "whitened update") in fp64 with LAPACK's factors, optionally with one
    16-column panel of the prior factor ("M") or of B's factor ("B") off by the relative error `delta`: what a wrong panel of either
    device factorisation does to P' and dx, for the CPU test that the bound would notice it."""
    from scipy.linalg import solve_triangular
    P, cols, H, r, k = c["P"], c["cols"], c["H"], c["r"], c["k"]
    M = np.linalg.cholesky(P[np.ix_(cols, cols)])
    if factor == "M":
        M[:, 16 * panel:16 * panel + 16] *= 1 + delta
    Lb = np.linalg.cholesky(np.eye(k) + M.T @ (H.T @ H) @ M)
    if factor == "B":
        Lb[:, 16 * panel:16 * panel + 16] *= 1 + delta
    W0 = solve_triangular(M, P[cols, :], lower=True)
    Vv = solve_triangular(Lb, np.column_stack([W0, M.T @ (H.T @ r)]), lower=True)
    V, v = Vv[:, :-1], Vv[:, -1]
    return P - W0.T @ W0 + V.T @ V, V.T @ v


# ------------------------------------------------------------------------------------------ section 3: not positive definite
NOT_PSD_R = [20, 40, 100, 128]


def not_psd_cases():
    """(r, panel, failing pivot): the first and the last pivot of the first, a middle and the last panel"""
    out = []
    for r in NOT_PSD_R:
        t = tiles(r)
        for p in sorted({0, t // 2, t - 1}):
            first = max(16 * p, 1)
            last = min(16 * p + 15, r - 1)
            out += [(r, p, first), (r, p, last)]
    return out


NOT_PSD_HOW = ("block", "noise")


def not_psd_case(r, pivot, how="block"):
    """S = P + R whose first pivot that is not positive is `pivot`, two ways.
    "block": test_ekf_update_not_psd_leaves_state's construction with the indefinite 2 x 2 block at (pivot - 1, pivot): the pivots are
        1e-4 .. and then 1e-4 - 25e-6 / 1e-4 < 0.  Here the rejection has a second witness: with the dead column dropped the gain's
        diagonal exceeds P's, so the negative-diagonal test rejects the update as well; what shows that the FACTORISATION reported it
        is the library's error text ("S not positive definite" is chosen ahead of "negative covariance diagonal").
    "noise": P = 1e-4 I stays positive definite and S is indefinite through one noise entry, R[pivot] = -2e-4.  With that column
        dropped P - K M^T keeps a positive diagonal (dropped_column_diagonal), so nothing but the factorisation's own report rejects
        the update: were it missing, the call would return 0 and change P."""
    P = np.eye(r) * 1e-4
    Rd = np.full(r, 1e-8)
    if how == "block":
        P[pivot - 1, pivot] = P[pivot, pivot - 1] = 5e-3
    else:
        Rd[pivot] = -2e-4
    return dict(P=P, cols=np.arange(r, dtype=np.int32), H=np.eye(r), res=np.ones(r), Rd=Rd)


def dropped_column_diagonal(c):
    """(first pivot that is not positive, smallest entry of diag(P - W W^T)) for the factorisation as the device carries it on past
    such a pivot without reporting it: a pivot <= 0 gives a zero column of L (blocked_chol.hpp: no elimination by it, and the border
    rows' column W[:, j] is zero), W = M L^-T with M = P[:, cols] H^T.  Long double."""
    P, H, cols = c["P"].astype(ld_t), c["H"].astype(ld_t), c["cols"]
    A = H @ P[np.ix_(cols, cols)] @ H.T + np.diag(c["Rd"].astype(ld_t))
    M = P[:, cols] @ H.T
    r = A.shape[0]
    W = np.zeros_like(M)
    first = -1
    for j in range(r):
        piv = A[j, j]
        if piv > 0:
            W[:, j] = M[:, j] / np.sqrt(piv)
            lcol = A[j + 1:, j] / np.sqrt(piv)
            M[:, j + 1:] -= np.outer(W[:, j], lcol)
            A[j + 1:, j + 1:] -= np.outer(lcol, lcol)
        elif first < 0:
            first = j
    return first, float(np.min(np.diag(P) - np.sum(W * W, axis=1)))


# ------------------------------------------------------------------------------------------ section 4: chi2 by value
CHI2_K = [17, 98]
CHI2_ROWS = [32, 63]      # mp = 1 .. 32 launches chi2_gate_kernel<2>, 1 .. 63 <4>
CHI2_LD = 64


@functools.lru_cache(maxsize=None)
def chi2_case(k, mp_most):
    """one feature per projected row count 1 .. mp_most; per feature the restatement r^T (H Ps H^T + sigma^2 I)^-1 r in long double
    and cond(S)"""
    import oracle_lib
    n = k + 15
    P = synth.spd_cov(n, seed=k)
    cols = synth.col_map(n, k, seed=k, skip=15)
    _, _, Hx, res = synth.msckf_batch(F=mp_most, M=CHI2_LD // 2, k=k, seed=k + mp_most, ragged=False, ld=CHI2_LD)
    rows = np.arange(1, mp_most + 1, dtype=np.int32)
    Ps = P[np.ix_(cols, cols)].astype(ld_t)
    ref, cond = np.zeros(mp_most), np.zeros(mp_most)
    for f, m in enumerate(rows):
        H, r = Hx[f, :, :m].T.astype(ld_t), res[f, :m].astype(ld_t)
        S = H @ Ps @ H.T + SIGMA2 * np.eye(m, dtype=ld_t)
        ref[f] = float(r @ lu_solve_ld(S, r[:, None])[:, 0])
        cond[f] = np.linalg.cond(S.astype(np.float64))
    chi_o = oracle_lib.load().chi2_batch(P, rows, Hx, res, cols, SIGMA2)
    return dict(P=P, cols=cols, rows=rows, Hx=Hx, res=res, ref=ref, cond=cond, oracle=chi_o)


def chi2_bound(c):
    """per feature: ten times the oracle's own distance from the restatement, or what fp64 can hold of it: mp eps cond(S) ref"""
    return np.maximum(10 * np.abs(c["oracle"] - c["ref"]), c["rows"] * np.finfo(np.float64).eps * c["cond"] * c["ref"])
