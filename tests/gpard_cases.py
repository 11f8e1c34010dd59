"""Checks of the per-coordinate length-scale gradient (automatic relevance determination) of a kept kernel ridge regression fit:
hssk_kernel_matmul_coord, Kernel<double>::log_marginal_likelihood_gradient_coords and its C and Python forms, and the `widths`
convenience of KernelRegression.  Shared by the CPU emulator tests (tests/test_gpard_emu.py) and the GPU tests
(tests/test_gpard_gpu.py); the helpers of tests/gpgrad_cases.py are reused.

The formulas.  k_l(x, y) = k(x / l, y / l), theta_j = ln l_j at l = 1,
    dk/dtheta_j = k D_j,   D_j = (x_j - y_j)^2 / h^2 (Gauss), |x_j - y_j| / h (Laplace),   sum_j k D_j = h dk/dh,
    dL/dtheta_j = 1/2 alpha^T K_j alpha - 1/2 tr(H^-1 K_j),   K_j = K o D_j,   dL/dw_j = (dL/dtheta_j) / w_j for a fit on X / w.
check_oracle compares them with central differences of the dense L in plain numpy: the formulas themselves, no library code.

The product kernel.  The reference is kernel_cases.kernel_ref in long double (k and the exponent's magnitude a) times D_j in long
double from the double coordinates.  The kernel computes k^ as hssk_kernel_matmul does, within b = kernel_entry_bound(lambda = 0)
of k, and g_j^ = fl(fl(k^ fl(df df)) c^) with df = fl(x_j - y_j) and c^ = fl(1 / fl(h h)) (Laplace: |df| and c^ = fl(1 / h)).
Relative roundings: df one (two in its square), the square one, the two products one each, the constant two: seven (Laplace
four), so to first order |g_j^ - g_j| <= D_j (b + 7 u k).  The form asserted, with c = 8:
    b'_j = D_j (kernel_entry_bound(a, A, type, d, 0) + 8 u k).
An entry of the product:  |out_j(i, c) - ref| <= sum_r (b'_j + n u |g_j|) |B(r, c)|  (gpgrad_cases.product_bound).
Equal points have df = 0 exactly, so g_j = k^ 0 c^ = 0 exactly.  (1 / h) sum_j out_j against hssk_kernel_matmul(deriv = 1): both are
within their own product bounds of the same long double matrix h^-1 sum_j g_j = dk/dh, so they differ by at most
(1 / h) sum_j E_j + E' (the sum over j is taken in long double here).

The gradient of a kept model.  As in gpgrad_cases: Hd the dense form of the matrix the handle writes, S = solve(Hd, Z), the
library's S^ within EPS_F cond_2(Hd) ||s_k|| of it, its products within E_j.  Per coordinate j and probe k
    |tc^_jk - tc_jk| <= EPS_F cond_2(Hd) ||s_k|| ||(K_j z)_k|| + sum_i |s_ik| E_j,ik,
    |quad_j^ - quad_j| <= 1/2 sum_i |alpha_i| E_j,i(alpha),
trace_j the mean over the probes with the mean of the bounds, dtheta_j = quad_j - trace_j / 2 with the sum.  A case only proves
something while, for EVERY coordinate,  bound(dtheta_j) <= 1e-4 min(|trace_j|, |quad_j|);  that is asserted from the reference
side alone.  Per probe, sum_j tc^_jk and h th^_k of the existing gradient are each within their bounds of the same number."""
import ctypes

import numpy as np

import gp_cases as GP
import gpgrad_cases as GG
import kernel_cases as KC
from strumpack_amd import hssk as K

LD = np.longdouble
U = KC.U53
KT = GG.KT
C_ROUND = 8


# ---- 1. the formulas themselves ---------------------------------------------------------------------------------------------------
def dense_dj(X, ktype, h):
    """D_j for every j: d x n x n (float64)"""
    df = X[:, None, :] - X[None, :, :]
    D = df ** 2 / h ** 2 if ktype == 0 else np.abs(df) / h
    return np.moveaxis(D, -1, 0)


def dense_gradient_coords(X, y, ktype, h, lam):
    n = len(X)
    idx = np.arange(n)
    Kd = KC.kernel_np(X, idx, idx, ktype, h, 0.0)
    Hi = np.linalg.inv(Kd + lam * np.eye(n))
    alpha = Hi @ y
    return np.array([0.5 * alpha @ (Kd * Dj) @ alpha - 0.5 * np.trace(Hi @ (Kd * Dj)) for Dj in dense_dj(X, ktype, h)])


def check_oracle(kern, d, n=200, lam=4.0, step=1e-5):
    """dL/dtheta_j of the dense L against central differences in ln l_j (relative 1e-5, as gpgrad_cases.check_oracle argues), their
    sum against h dL/dh, and dL/dw_j at a w != 1 against central differences in w_j"""
    X, y, _ = GP.model_data(d, n, 2)
    ktype = KT[kern]
    h = float(KC.kernel_widths(d)[ktype])
    g = dense_gradient_coords(X, y, ktype, h, lam)
    for j in range(d):
        lp, lm = np.ones(d), np.ones(d)
        lp[j], lm[j] = np.exp(step), np.exp(-step)
        fd = (GG.dense_lml(X / lp, y, ktype, h, lam) - GG.dense_lml(X / lm, y, ktype, h, lam)) / (2 * step)
        print("oracle %s R^%d: dL/dtheta_%d %.9g (differences %.9g)" % (kern, d, j, g[j], fd))
        assert abs(g[j] - fd) <= 1e-5 * abs(g[j]), (j, g[j], fd)
    dh, _ = GG.dense_gradient(X, y, ktype, h, lam)
    print("oracle %s R^%d: sum_j dL/dtheta_j %.12g, h dL/dh %.12g" % (kern, d, g.sum(), h * dh))
    assert abs(g.sum() - h * dh) <= 1e-10 * np.abs(g).sum()
    w = 0.6 + 0.2 * np.arange(1, d + 1)
    gw = dense_gradient_coords(X / w, y, ktype, h, lam) / w
    for j in range(d):
        wp, wm = w.copy(), w.copy()
        wp[j] += step
        wm[j] -= step
        fd = (GG.dense_lml(X / wp, y, ktype, h, lam) - GG.dense_lml(X / wm, y, ktype, h, lam)) / (2 * step)
        assert abs(gw[j] - fd) <= 1e-5 * abs(gw[j]), (j, gw[j], fd)


# ---- 2. hssk_kernel_matmul_coord on its own -----------------------------------------------------------------------------------------
def g_reference(X, ktype, h, d, j):
    """(g_j, b'_j) in long double over all pairs of the rows of X"""
    idx = np.arange(len(X))
    k, a, A = KC.kernel_ref(X, idx, idx, ktype, h, 0.0)
    x = X[:, j].astype(LD)
    df = x[:, None] - x[None, :]
    D = df * df / (LD(h) * LD(h)) if ktype == 0 else np.abs(df) / LD(h)
    return k * D, D * (KC.kernel_entry_bound(a, A, ktype, d, 0.0) + C_ROUND * U * k)


def nj_max(hk):
    return hk.lib.hssk_kernel_matmul_coord_max()


def coord(hk, dX, n, d, ktype, h, j0, nj, B, splits=0, pad=(3, 5, 7)):
    """one call on a padded B into pre-filled padded output blocks with a gap between them: returns nj results of n x nc after
    checking that nothing else was written"""
    nc = B.shape[1]
    ldb, ldo = n + pad[0], n + pad[1]
    stride = ldo * nc + pad[2]
    Bp = np.full((ldb, nc), 1e300)
    Bp[:n] = B
    dB, dO = hk.array(Bp), hk.array(np.full(nj * stride + 11, KC.SENTINEL))
    spec = K.KernelSpec(dX.ptr, n, d, ktype, 1, h, 123.0)       # (lambda must not appear anywhere)
    hk.check(hk.lib.hssk_kernel_matmul_coord(hk.ctx, ctypes.byref(spec), j0, nj, dB.ptr, ldb, nc, dO.ptr, ldo, stride, splits))
    hk.sync()
    got = dO.get()
    dB.free()
    dO.free()
    assert np.all(got[nj * stride:] == KC.SENTINEL), "hssk_kernel_matmul_coord wrote behind its blocks"
    blocks = got[:nj * stride].reshape(nj, stride)
    assert np.all(blocks[:, ldo * nc:] == KC.SENTINEL), "hssk_kernel_matmul_coord wrote between its blocks"
    out = blocks[:, :ldo * nc].reshape(nj, nc, ldo)
    assert np.all(out[:, :, n:] == KC.SENTINEL), "hssk_kernel_matmul_coord wrote below a block"
    return np.ascontiguousarray(out[:, :, :n].transpose(0, 2, 1))


def runs(d):
    """the coordinates a case computes: all of them up to R^8, the first and the last four beyond"""
    return [list(range(d))] if d <= 8 else [list(range(4)), list(range(d - 4, d))]


def groups(d, nj):
    """(j0, count) covering runs(d) with groups of nj, the last group of a run ragged (d = 7, nj = 2: .., (6, 1))"""
    return [(r[i], min(nj, len(r) - i)) for r in runs(d) for i in range(0, len(r), nj)]


# (n, nc, d, kernel, splits; -1: one split per stage of 16 points): every d of {1, 2, 7, 8, 64}, every n of {1, 15 (below a stage),
# 64 (one tile), 150, 333 (ragged tiles and stages)}, every nc of {1, 17, 64}, splits 0, 1, 3 and one per stage, both kernels
COORD_CASES = [
    (1, 1, 1, "gauss", 0),
    (15, 17, 2, "laplace", 1),
    (64, 64, 7, "gauss", 3),
    (150, 17, 8, "laplace", -1),
    (150, 64, 8, "gauss", 3),
    (333, 64, 8, "gauss", 0),
    (333, 1, 7, "laplace", -1),
    (150, 17, 64, "gauss", 1),
    (64, 1, 64, "laplace", 3),
    (333, 17, 2, "gauss", 3),
]


def check_coord(hk, n, nc, d, kern, splits, seed=13):
    """every built nj over the groups of groups(d, nj): coordinate by coordinate (nj = 1) against the long double reference under
    the bound of the module docstring, every larger nj bit for bit what nj = 1 gave (whichever group computed it); two calls bit
    for bit; splits = 0 bit for bit the forced hssk_kernel_matmul_splits(n); the sum over the coordinates against deriv = 1"""
    rng = np.random.default_rng(seed + n + d)
    X, B = rng.standard_normal((n, d)), rng.standard_normal((n, nc))
    ktype = KT[kern]
    h = float(KC.kernel_widths(d)[ktype])
    if splits < 0:
        splits = (n + 15) // 16
    dX = hk.array(X.T)
    one, worst, Esum = {}, 0.0, 0
    for j0, _ in groups(d, 1):
        one[j0] = coord(hk, dX, n, d, ktype, h, j0, 1, B, splits)[0]
        g, bp = g_reference(X, ktype, h, d, j0)
        ref, E = g @ B.astype(LD), GG.product_bound(g, bp, B)
        err = np.abs(one[j0].astype(LD) - ref)
        assert np.all(err <= E), (kern, n, nc, d, j0, splits, float((err / E).max()))
        assert np.all(np.diag(np.asarray(g, dtype=np.float64)) == 0.0)
        worst = max(worst, float((err / np.where(E > 0, E, 1)).max()))
        Esum = Esum + E
    print("kernel_matmul_coord %s n=%d nc=%d d=%d splits=%d: largest error / bound %.3f" % (kern, n, nc, d, splits, worst))
    top = nj_max(hk)
    assert top >= 2
    for nj in range(2, top + 1):
        for j0, cnt in groups(d, nj):
            got = coord(hk, dX, n, d, ktype, h, j0, cnt, B, splits)
            for jj in range(cnt):
                assert np.array_equal(got[jj], one[j0 + jj]), ("coordinate %d differs between nj = 1 and nj = %d" % (j0 + jj, cnt))
    j0, cnt = groups(d, top)[0]
    a = coord(hk, dX, n, d, ktype, h, j0, cnt, B, splits)
    assert np.array_equal(a, coord(hk, dX, n, d, ktype, h, j0, cnt, B, splits)), "two calls differ"
    auto = hk.lib.hssk_kernel_matmul_splits(n)
    assert np.array_equal(coord(hk, dX, n, d, ktype, h, j0, cnt, B, 0), coord(hk, dX, n, d, ktype, h, j0, cnt, B, auto)), "splits = 0"
    if d <= 8:   # all coordinates at hand: (1 / h) sum_j out_j is the deriv = 1 product
        dh = GG.matmul(hk, dX, n, d, ktype, h, 0.0, 1, B, splits)
        gp, bpp = GG.g_reference(X, ktype, h, d, 1, 0.0)
        total = sum(one[j].astype(LD) for j in range(d)) / LD(h)
        assert np.all(np.abs(total - dh.astype(LD)) <= Esum / LD(h) + GG.product_bound(gp, bpp, B)), (kern, n, d, "sum over the coordinates")
    dX.free()
    return worst


def check_entries(hk, seed=3):
    """B = I at n = 64: the product IS the matrix, so every entry of g_j is within b'_j of the long double reference (no sum)"""
    n, d = 64, 7
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    dX = hk.array(X.T)
    for kern, ktype in KT.items():
        h = float(KC.kernel_widths(d)[ktype])
        got = np.concatenate([coord(hk, dX, n, d, ktype, h, j0, cnt, np.eye(n)) for j0, cnt in groups(d, nj_max(hk))])
        for j in range(d):
            g, bp = g_reference(X, ktype, h, d, j)
            err = np.abs(got[j].astype(LD) - g)
            assert np.all(err <= bp), (kern, j, float((err / np.where(bp > 0, bp, 1)).max()))
            assert np.all(np.diag(got[j]) == 0.0) and np.count_nonzero(got[j]) == n * (n - 1)
    dX.free()


def check_properties(hk, seed=5):
    """duplicated points contribute exactly 0 in every coordinate; a column does not depend on the other columns"""
    rng = np.random.default_rng(seed)
    n, d, nc = 130, 8, 17
    top = nj_max(hk)
    for kern, ktype in KT.items():
        h = float(KC.kernel_widths(d)[ktype])
        X = rng.standard_normal((n, d))
        X[77] = X[3]
        X[129] = X[64]
        dX = hk.array(X.T)
        B = np.zeros((n, 4))
        B[77, 0], B[3, 1], B[129, 2], B[64, 3] = 1.5, -2.0, 3.0, 0.25
        for splits in (1, 3):
            for j0, cnt in groups(d, top):
                got = coord(hk, dX, n, d, ktype, h, j0, cnt, B, splits)
                for jj in range(cnt):
                    for col, (i, j) in enumerate([(3, 77), (77, 3), (64, 129), (129, 64)]):
                        assert got[jj][i, col] == 0.0 and got[jj][j, col] == 0.0, (kern, splits, j0 + jj, i, j)
                    assert np.count_nonzero(got[jj]) == 4 * (n - 2)
        B = rng.standard_normal((n, nc))
        B2 = rng.standard_normal((n, nc))
        B2[:, 5] = B[:, 5]
        for splits in (0, 3):
            a, b = coord(hk, dX, n, d, ktype, h, 2, top, B, splits), coord(hk, dX, n, d, ktype, h, 2, top, B2, splits)
            assert np.array_equal(a[:, :, 5], b[:, :, 5]) and not np.array_equal(a[:, :, 4], b[:, :, 4]), "a column depends on its neighbours"
            c = coord(hk, dX, n, d, ktype, h, 2, top, B[:, 5:6], splits)
            assert np.array_equal(a[:, :, 5], c[:, :, 0]), "a column depends on the column count"
        dX.free()


def check_refusals(hk):
    n, d, nc = 40, 8, 5
    rng = np.random.default_rng(1)
    top = nj_max(hk)
    dX, dB = hk.array(rng.standard_normal((65, n))), hk.array(rng.standard_normal((n, 65)))
    fill = np.full((n, 65 * (top + 1)), KC.SENTINEL)
    dO = hk.array(fill)
    f = hk.lib.hssk_kernel_matmul_coord
    sp = lambda t, dd=d, nn=n: ctypes.byref(K.KernelSpec(dX.ptr, nn, dd, t, 2 if t == 2 else 1, 1.3, 0.0))
    st = n * nc
    assert f(hk.ctx, sp(2), 0, 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 2 and "ANOVA" in hk.error()
    assert f(hk.ctx, sp(3), 0, 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 2                  # Matern 3/2
    assert f(hk.ctx, sp(4), 0, 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 2                  # Matern 5/2
    assert f(hk.ctx, sp(0, 65), 0, 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 2             # d > 64
    assert f(hk.ctx, sp(1, 65), 64, 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 2
    assert f(hk.ctx, sp(0), 0, 1, dB.ptr, n, 65, dO.ptr, n, n * 65, 0) == 1             # more than 64 columns
    assert f(hk.ctx, sp(0), 0, 1, dB.ptr, n, -1, dO.ptr, n, st, 0) == 1
    assert f(hk.ctx, sp(0), -1, 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 1                # j0 < 0
    assert f(hk.ctx, sp(0), 0, 0, dB.ptr, n, nc, dO.ptr, n, st, 0) == 1                 # nj < 1
    assert f(hk.ctx, sp(0), 0, top + 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 1           # nj > max
    assert f(hk.ctx, sp(0), d - 1, 2, dB.ptr, n, nc, dO.ptr, n, st, 0) == 1             # j0 + nj > d
    assert f(hk.ctx, sp(0), d, 1, dB.ptr, n, nc, dO.ptr, n, st, 0) == 1
    assert f(hk.ctx, sp(0), 0, 2, dB.ptr, n - 1, nc, dO.ptr, n, st, 0) == 1             # ldb < n
    assert f(hk.ctx, sp(0), 0, 2, dB.ptr, n, nc, dO.ptr, n - 1, st, 0) == 1             # ldo < n
    assert f(hk.ctx, sp(0), 0, 2, dB.ptr, n, nc, dO.ptr, n, st - 1, 0) == 1             # stride below n nc
    assert f(hk.ctx, sp(0), 0, 2, None, n, nc, dO.ptr, n, st, 0) == 1
    assert f(hk.ctx, sp(0), 0, 2, dB.ptr, n, nc, None, n, st, 0) == 1
    assert f(hk.ctx, None, 0, 2, dB.ptr, n, nc, dO.ptr, n, st, 0) == 1
    assert f(hk.ctx, sp(0), 0, 2, dB.ptr, n, nc, dB.ptr, n, st, 0) == 1                 # out aliases B
    assert f(hk.ctx, sp(0), 0, 2, dB.at(0, 6), n, nc, dB.ptr, n, st, 0) == 1            # B inside the second output block
    assert f(hk.ctx, sp(0), 0, 2, dB.ptr, n, nc, dO.ptr, n, st, -1) == 1
    # nothing to do
    assert f(hk.ctx, sp(0), 0, 2, None, n, 0, None, n, 0, 0) == 0
    assert f(hk.ctx, sp(0, d, 0), 0, 2, None, 0, nc, None, 0, 0, 0) == 0
    hk.sync()
    assert np.array_equal(dO.get(), fill), "a refused call wrote its output"
    # more splits than stages: every split at least one stage
    B = rng.standard_normal((n, nc))
    a = coord(hk, dX, n, d, 0, 1.3, 1, 2, B, 50)
    assert np.array_equal(a, coord(hk, dX, n, d, 0, 1.3, 1, 2, B, 3))
    for v in (dX, dB, dO):
        v.free()


# ---- 3. the gradient of a kept model ----------------------------------------------------------------------------------------------
# (kernel, d, lambda, factor on the width): Gauss R^8 and Laplace R^2 at the fit settings of gp_cases.fit_model (n = 700)
MODEL_CASES = [("gauss", 8, 4.0, 1.0), ("laplace", 2, 4.0, 1.0)]


def coords_matrices(kr, kind):
    """[(g_j, b'_j + n u |g_j|)] in long double for the model's points: computed once per model, shared by its probe blocks"""
    ktype, _, h = kind
    X = kr.model_points()
    n, d = X.shape
    out = []
    for j in range(d):
        g, bp = g_reference(X, ktype, h, d, j)
        out.append((g, bp + n * U * np.abs(g)))
    return out


def coords_reference(kr, Hd, sv, mats, Z):
    """reference terms and their bounds (module docstring) for the probes Z (n x m, cluster order)"""
    alpha = kr.weights()
    cond = sv[0] / sv[-1]
    S = np.linalg.solve(Hd, Z)
    F = np.linalg.norm
    al = alpha.astype(LD)
    ref = dict(tc=[], quad=[], trace=[], dtheta=[])
    bound = dict(tc=[], quad=[], trace=[], dtheta=[])
    for g, W in mats:
        Gz = np.asarray(g @ Z.astype(LD), dtype=np.float64)
        E = np.asarray(W @ np.abs(Z).astype(LD), dtype=np.float64)
        tc = (S * Gz).sum(0)
        btc = GP.EPS_F * cond * F(S, axis=0) * F(Gz, axis=0) + (np.abs(S) * E).sum(0)
        q, bq = float(0.5 * (al @ (g @ al))), float(0.5 * (np.abs(al) @ (W @ np.abs(al))))
        for name, r, b in (("tc", tc, btc), ("quad", q, bq), ("trace", tc.mean(), btc.mean()),
                           ("dtheta", q - 0.5 * tc.mean(), bq + 0.5 * btc.mean())):
            ref[name].append(r)
            bound[name].append(b)
    return {k: np.array(v) for k, v in ref.items()}, {k: np.array(v) for k, v in bound.items()}


def raw_coords(lib, kr, m, Z=None, seed=0):
    """the C entry point on the raw handle: (grad, terms)"""
    d = kr.d
    grad, terms = np.zeros(d), np.zeros(2 * d + d * m)
    zp = None if Z is None else np.asfortranarray(Z).ctypes.data
    assert lib.SPX_kernel_lml_gradient_coords(kr.K, m, zp, seed, grad.ctypes.data, terms.ctypes.data) == 0
    return grad, terms


def check_model_gradient(KM, lib, kern, d, lam, hscale, path, ms=(63, 70)):
    """one kept fit (n = 700): the coordinate gradient with 63 explicit Rademacher probes (one block with alpha) and with 70 (two
    blocks); the long double matrices are computed once for both"""
    kr, _, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    try:
        Hd, sv, _ = GP.dense_model(kr, path)
        mats = coords_matrices(kr, kind)
        return max(check_model_probes(lib, kr, Hd, sv, kind, mats, m) for m in ms)
    finally:
        kr.destroy()


def check_model_probes(lib, kr, Hd, sv, kind, mats, m):
    """m explicit probes term by term under their bounds, the proof assertion for every coordinate, per probe the sum over the
    coordinates against h th of the existing gradient, a second call and the raw C call bit for bit, the model undisturbed"""
    d = kr.d
    tag = "%s R^%d lambda=%g h=%.3g m=%d" % (("gauss", "laplace")[kind[0]], d, kr.lam, kind[2], m)
    ld = kr.logabsdet()
    Z = GG.rademacher(kr.n, m)
    ref, bound = coords_reference(kr, Hd, sv, mats, Z)
    for j in range(d):
        print("coords %s j=%d: dtheta %.9g bound %.3g trace %.6g quad %.6g" % (tag, j, ref["dtheta"][j], bound["dtheta"][j],
                                                                             ref["trace"][j], ref["quad"][j]))
    assert np.all(bound["dtheta"] <= 1e-4 * np.minimum(np.abs(ref["trace"]), np.abs(ref["quad"]))), (tag, "the case proves nothing")
    g, t = kr.log_marginal_likelihood_gradient_coords(Z=Z, terms=True)
    assert g.shape == (d,) and t["tc"].shape == (d, m) and np.array_equal(g, t["dtheta"])
    worst = 0.0
    for name in ("tc", "quad", "trace", "dtheta"):
        err = np.abs(t[name] - ref[name])
        ratio = float(np.max(err / bound[name]))
        worst = max(worst, ratio)
        print("coords %s %s: largest error %.3g largest bound %.3g error / bound %.3g" % (tag, name, float(err.max()),
                                                                                         float(bound[name].max()), ratio))
        assert np.all(err <= bound[name]), (tag, name, ratio)
    # per probe: the coordinates add up to h times the derivative in h
    _, _, th = kr.log_marginal_likelihood_gradient(Z=Z, terms=True)
    _, bh = GG.gradient_reference(kr, Hd, sv, kind, Z)
    h = kind[2]
    assert np.all(np.abs(t["tc"].astype(LD).sum(0) - LD(h) * th["th"].astype(LD)) <= bound["tc"].sum(0) + h * bh["th"]), (tag, "sum over j")
    g2, t2 = kr.log_marginal_likelihood_gradient_coords(Z=Z, terms=True)
    assert np.array_equal(g, g2) and all(np.array_equal(t[k], t2[k]) for k in t), "two calls differ"
    gc, tcr = raw_coords(lib, kr, m, Z)
    assert np.array_equal(gc, g) and np.array_equal(tcr, np.concatenate([t["quad"], t["trace"], t["tc"].ravel()])), "C and Python differ"
    assert np.array_equal(kr.log_marginal_likelihood_gradient_coords(Z=Z), g)
    assert kr.logabsdet() == ld, "the gradient disturbed the kept model"
    ms = kr.gradient_ms()
    assert ms["product_ms"] >= 0.0 and ms["solve_ms"] >= 0.0
    return worst


def check_seeded(KM, lib):
    """the seeded form bit for bit the explicit model_probes form; another seed differs; the defaults are 63 probes, seed 0"""
    kr, _, _ = GP.fit_model(KM, lib, "gauss", 8, 4.0, 1.0, n=192)
    try:
        Z7 = kr.model_probes(63, 7)
        a = kr.log_marginal_likelihood_gradient_coords(probes=63, seed=7, terms=True)
        b = kr.log_marginal_likelihood_gradient_coords(Z=Z7, terms=True)
        assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1]), "seeded and explicit forms differ"
        assert not np.array_equal(kr.log_marginal_likelihood_gradient_coords(probes=63, seed=8), a[0])
        assert np.array_equal(kr.log_marginal_likelihood_gradient_coords(), kr.log_marginal_likelihood_gradient_coords(probes=63, seed=0))
        gc, _ = raw_coords(lib, kr, 63, None, 7)
        assert np.array_equal(gc, a[0])
    finally:
        kr.destroy()


def coords_calls(lib, Kh, n, d, m=3):
    """the new call on the raw handle with pre-filled outputs, explicit and seeded: [(return code, outputs untouched)]"""
    res = []
    for Z in (np.ones((n, m), order="F"), None):
        grad, terms = np.full(d, 123.25), np.full(2 * d + d * m, 123.25)
        rc = lib.SPX_kernel_lml_gradient_coords(Kh, m, None if Z is None else Z.ctypes.data, 5, grad.ctypes.data, terms.ctypes.data)
        res.append((rc, bool(np.all(grad == 123.25) and np.all(terms == 123.25))))
    return res


def check_lifecycle(KM, lib):
    """refusals -- no kept model, a float handle, ANOVA, d = 65, m < 1, wrong shapes -- leave outputs and model alone"""
    n, d = 300, 8
    X, y, _ = GP.model_data(d, n, 20)
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]

    def refused(kr, what, dd=d):
        for rc, untouched in coords_calls(lib, kr.K, n, dd):
            assert rc != 0 and untouched, (what, rc)
        try:
            kr.log_marginal_likelihood_gradient_coords(probes=3)
            raise AssertionError("%s: the Python call answered" % what)
        except RuntimeError:
            pass

    plain = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y)
    refused(plain, "no keep_model")
    plain.destroy()
    kf = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X.astype(np.float32), y.astype(np.float32))
    refused(kf, "float handle")
    kf.destroy()
    ka = KM.KernelRegression(lib, h=h, lam=4.0, kernel="ANOVA", degree=2, argv=args, keep_model=True).fit(X, y)
    lda = ka.logabsdet()
    refused(ka, "ANOVA")
    assert ka.logabsdet() == lda
    ka.destroy()
    X65, y65, _ = GP.model_data(65, n, 20)
    k65 = KM.KernelRegression(lib, h=float(KC.kernel_widths(65)[0]), lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X65, y65)
    ld65 = k65.logabsdet()
    refused(k65, "d = 65", 65)
    assert k65.logabsdet() == ld65 and np.all(np.isfinite(k65.log_marginal_likelihood_gradient(probes=3)))
    k65.destroy()
    kr = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    ld = kr.logabsdet()
    grad, terms = np.full(d, 123.25), np.full(2 * d, 123.25)
    assert lib.SPX_kernel_lml_gradient_coords(kr.K, 0, None, 0, grad.ctypes.data, terms.ctypes.data) != 0
    assert lib.SPX_kernel_lml_gradient_coords(kr.K, -1, None, 0, grad.ctypes.data, terms.ctypes.data) != 0
    assert lib.SPX_kernel_lml_gradient_coords(kr.K, 3, None, 0, None, None) != 0
    assert np.all(grad == 123.25) and np.all(terms == 123.25)
    for bad in (np.ones((n - 1, 3)), np.ones((n + 1, 3)), np.ones((n, 0)), np.ones(n)):
        try:
            kr.log_marginal_likelihood_gradient_coords(Z=bad)
            raise AssertionError("a probe block of shape %s was accepted" % (bad.shape,))
        except ValueError:
            pass
    try:
        kr.log_marginal_likelihood_gradient_coords(probes=0)
        raise AssertionError("probes = 0 was accepted")
    except ValueError:
        pass
    for rc, untouched in coords_calls(lib, kr.K, n, d):
        assert rc == 0 and not untouched
    g1 = kr.log_marginal_likelihood_gradient_coords(probes=5, seed=3)       # without the terms, and without the term buffer
    grad = np.zeros(d)
    assert lib.SPX_kernel_lml_gradient_coords(kr.K, 5, None, 3, grad.ctypes.data, None) == 0 and np.array_equal(grad, g1)
    assert kr.logabsdet() == ld, "the gradient disturbed the kept model"
    assert set(kr.gradient_ms()) == {"product_ms", "solve_ms", "dots_ms"}
    assert lib.SPX_kernel_keep_model(kr.K, 0) == 0
    refused(kr, "after keep_model(false)")
    kr.destroy()


# ---- 4. widths ----------------------------------------------------------------------------------------------------------------------
def check_widths(KM, lib):
    """a model fitted with widths = w on X is bit for bit the plain fit on X / w -- permutation, weights, points, predictions,
    variances -- and its coordinate gradient is dtheta / w; widths = None changes nothing; bad widths are refused"""
    n, d = 300, 8
    X, y, T = GP.model_data(d, n, 20)
    T = T[:40]
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]
    w = 0.5 + 0.25 * np.arange(1, d + 1)
    a = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True, widths=w).fit(X, y)
    b = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X / w, y)
    c = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True, widths=None).fit(X / w, y)
    try:
        assert np.array_equal(a.permutation(), b.permutation()) and np.array_equal(a.weights(), b.weights())
        assert np.array_equal(a.model_points(), b.model_points()) and np.array_equal(a.model_points(), (X / w)[a.permutation() - 1])
        assert np.array_equal(a.decision_function(T), b.decision_function(T / w)) and np.array_equal(a.predict(T), b.predict(T / w))
        assert np.array_equal(a.predict_variance(T), b.predict_variance(T / w))
        assert np.array_equal(c.weights(), b.weights()) and np.array_equal(c.decision_function(T / w), b.decision_function(T / w))
        ga, ta = a.log_marginal_likelihood_gradient_coords(probes=9, seed=2, terms=True)
        gb, tb = b.log_marginal_likelihood_gradient_coords(probes=9, seed=2, terms=True)
        assert np.array_equal(ta["dtheta"], gb) and np.array_equal(gb, tb["dtheta"]) and np.array_equal(ga, gb / w)
        assert not np.array_equal(a.weights(), KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y).weights())
    finally:
        for k in (a, b, c):
            k.destroy()
    for bad in (np.ones((2, d)), np.zeros(d), -np.ones(d), np.full(d, np.nan), []):
        try:
            KM.KernelRegression(lib, widths=bad)
            raise AssertionError("widths %r accepted" % (bad,))
        except ValueError:
            pass
    try:
        KM.KernelRegression(lib, h=h, widths=np.ones(d + 1)).fit(X, y)
        raise AssertionError("widths of the wrong length accepted")
    except ValueError:
        pass
