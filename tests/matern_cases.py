"""Checks of the Matern kernels of smoothness 3/2 and 5/2 (device types 3 and 4) in the device entry points that take
them: the FP64 sums, the exact products, the FP32 prediction and the FP32 product.  Shared by the CPU emulator tests
(tests/test_matern_emu.py) and the GPU tests (tests/test_matern_gpu.py), as tests/gp_cases.py is.

The kernels.  r = |x - y|_2, s = sqrt(2 nu) r / h:
    type 3, Matern32:  k = (1 + s) e^-s             dk/ds = -s e^-s               dk/dh = s^2 e^-s / h
    type 4, Matern52:  k = (1 + s + s^2 / 3) e^-s   dk/ds = -s (1 + s) e^-s / 3   dk/dh = s^2 (1 + s) e^-s / (3 h)
The reference is matern_ref below: long double numpy from the FP64 points.

The bound of one FP64 entry (u = 2^-53), derived as kernel_cases.kernel_entry_bound is.  The code computes q = sum_j (x_j - y_j)^2,
c = 2 nu / h^2, s = sqrt(c q), e = exp(-s), then the polynomial times e.
  q     one rounding of every difference (2 u in its square), one of the square, d - 1 additions:  (d + 2) u relative (all terms are
        positive).  c is two roundings, c q one more:  (d + 5) u in all.
  s     half of that, plus a square root within one unit in the last place (2 u):  rho = ((d + 5) / 2 + 2) u, relative.
  k     a relative rho in s moves k by s |dk/ds| rho.  The exponential within one unit in the last place (2 u), at most four
        roundings in the polynomial (all of its terms positive) and one in the product:  8 u k covers them.
      b = u (((d + 5) / 2 + 2) s |dk/ds| + 8 k) + u |lambda|.
  dk/dh g = s^2 P(s) e^-s / (h or 3 h), P = 1 or 1 + s.  d ln g / d ln s = 2 - s (nu = 3/2), 2 + s / (1 + s) - s (nu = 5/2): at
        most 3 + s in magnitude.  Roundings: s s, 1 + s, two products, 3 h, the division, the exponential (2 u): 8 u.
      b' = u |g| ((3 + s) ((d + 5) / 2 + 2) + 8).
  A pair at distance 0 has q = 0 exactly: s = 0, e = 1, k = 1 and g = 0 exactly, and both bounds say so (b = 8 u for k; the tests
  ask for the exact values on top).
Products and column sums take the forms of gpgrad_cases (sum_r (b'_ir + n u |g_ir|) |B_rc|) and gp_cases with these entry bounds.

The FP32 routes (u24 = 2^-24).  The points are centred, scaled by sqrt(2 nu) / h and rounded once to float, so that the sum of the
squared differences of a pair is u_p = s^2.  Its error du is that of the Gauss exponent of gpmixed_cases.pair_delta on the same
scaled points (dE1 + dE2 in the difference form, dE1 + dE3 <= dE1 + TAU on the matrix cores -- computed by that very function with
these points).  |dk/du_p| = e^-s / 2 (nu = 3/2), (1 + s) e^-s / 6 (nu = 5/2): at most 1/2 and 1/6 everywhere, and decreasing, so
also at the clamped max(u_p - du, 0).  Hence, ABSOLUTE per pair,
      e32 = D du + u24 (2 s |dk/ds| + 12 k),   D = 1/2 or 1/6:
the square root (one unit: relative 2 u24 in s ... counted as 2 s |dk/ds| u24 together with the product s log2 e), exp2 (4 u24 k),
the polynomial and the product (at most 6 u24 k), 2 u24 k of slack.  The product with B adds what gpmixed_cases.product_bound
adds: u24 for B rounded to float and 66 u24 for the FP32 chunk (72 u24 k with the 6 above), the FP64 term, 2^-126 per pair.
Prediction sums (float inputs; reference on the widened floats): sum_r |w_r| (e32_rc + 64 u24 k_rc) + u24 |P_c| + 2^-126 (..), the
form of kpredict_cases with e32 in place of the Gauss term and du from the route rule: min(4 (d + 4) u24 (|x~|^2 + |t~|^2), TAU) on
the matrix cores -- the TAU-based term with D in place of the Gauss factor -- plus (d + 4) u24 u_p for the difference form.
"""
import ctypes

import numpy as np

import gp_cases as GP
import gpmixed_cases as GM
import kernel_cases as KC
import kpredict_cases as KP
from strumpack_amd import hssk as K

LD = np.longdouble
U = KC.U53
U24 = 2.0 ** -24
S = KC.SENTINEL
KT = {"matern32": 3, "matern52": 4}
NAMES = {"matern32": "Matern32", "matern52": "Matern52"}
KERNS = tuple(KT)


def width(d):
    """the Gauss width of kernel_cases: off-diagonal entries of a standard normal cloud in R^8 stay within 0.05 .. 0.92"""
    return float(KC.kernel_widths(d)[0])


def matern_parts(q, ktype, h):
    """long double (s, k, |dk/ds|, dk/dh) from squared distances q"""
    q, h = np.asarray(q, dtype=LD), LD(h)
    s = np.sqrt(LD(3 if ktype == 3 else 5) * q) / h
    e = np.exp(-s)
    if ktype == 3:
        return s, (1 + s) * e, s * e, s * s * e / h
    return s, (1 + s + s * s / 3) * e, s * (1 + s) * e / 3, s * s * (1 + s) * e / (3 * h)


def matern_ref(X, I, J, ktype, h, lam=0.0):
    """(k + lambda on the diagonal, s, |dk/ds|, dk/dh) in long double for the rows I, J of X (n x d)"""
    X = np.asarray(X, dtype=LD)
    I, J = np.asarray(I), np.asarray(J)
    q = np.zeros((len(I), len(J)), dtype=LD)
    for j in range(X.shape[1]):
        q += (X[I, j][:, None] - X[J, j][None, :]) ** 2
    s, k, dks, g = matern_parts(q, ktype, h)
    return k + LD(lam) * (I[:, None] == J[None, :]), s, dks, g


def rho(d):
    return (d + 5) / 2.0 + 2.0


def entry_bound(k, s, dks, d, lam):
    """k: the entry without lambda"""
    return U * (rho(d) * s * dks + 8 * k) + U * abs(lam)


def deriv_bound(g, s, d):
    return U * np.abs(g) * ((3 + s) * rho(d) + 8)


def g_reference(X, ktype, h, deriv, lam):
    """(g, b') over all pairs: the matrix of the exact product and its entry bound"""
    idx = np.arange(len(X))
    k, s, dks, g = matern_ref(X, idx, idx, ktype, h, lam if deriv == 0 else 0.0)
    if deriv == 0:
        k0 = k - LD(lam) * np.eye(len(X), dtype=LD)
        return k, entry_bound(k0, s, dks, X.shape[1], lam)
    return g, deriv_bound(g, s, X.shape[1])


def product_bound(g, bp, B):
    return (bp + len(g) * U * np.abs(g)) @ np.abs(B).astype(LD)


# ---- 1. the formulas themselves -----------------------------------------------------------------------------------------------------
def dense_lml(X, y, ktype, h, lam):
    idx = np.arange(len(X))
    Kd = np.asarray(matern_ref(X, idx, idx, ktype, h, lam)[0], dtype=np.float64)
    return -0.5 * y @ np.linalg.solve(Kd, y) - 0.5 * np.linalg.slogdet(Kd)[1] - 0.5 * len(X) * np.log(2.0 * np.pi)


def check_oracle(kern, d, n=200, lam=4.0, step=1e-5):
    """dk/dh of the table above inside the dense likelihood gradient, against central differences of the dense likelihood (step
    1e-5: truncation and cancellation are both below 1e-8 of the gradients): 1e-5 relative"""
    X, y, _ = GP.model_data(d, n, 2)
    ktype, h = KT[kern], width(d)
    idx = np.arange(n)
    k, _, _, g = matern_ref(X, idx, idx, ktype, h, 0.0)
    Hi = np.linalg.inv(np.asarray(k, dtype=np.float64) + lam * np.eye(n))
    Kp, alpha = np.asarray(g, dtype=np.float64), Hi @ y
    dh, dl = 0.5 * alpha @ Kp @ alpha - 0.5 * np.trace(Hi @ Kp), 0.5 * alpha @ alpha - 0.5 * np.trace(Hi)
    fh = (dense_lml(X, y, ktype, h + step, lam) - dense_lml(X, y, ktype, h - step, lam)) / (2 * step)
    fl = (dense_lml(X, y, ktype, h, lam + step) - dense_lml(X, y, ktype, h, lam - step)) / (2 * step)
    print("oracle %s R^%d: dL/dh %.9g (differences %.9g), dL/dlambda %.9g (differences %.9g)" % (kern, d, dh, fh, dl, fl))
    assert abs(dh - fh) <= 1e-5 * abs(dh), (dh, fh)
    assert abs(dl - fl) <= 1e-5 * abs(dl), (dl, fl)


# ---- 3. hssk_kernel_predict, hssk_kernel_cross, hssk_kernel_predict_cols ------------------------------------------------------------
def check_cross_and_cols(hk, kern, n, m, d, seed=7):
    """gp_cases.check_cross_and_cols for the Matern kernels: every entry of the cross block under entry_bound (a lambda in the spec
    does not reach it; test points that are training points give exactly 1), sentinels around the outputs, the column sums under
    sum_r |W_rc| b_rc + n u sum_r |W_rc k_rc|, two calls bit for bit, and predict_cols with one weight vector in every column bit
    for bit hssk_kernel_predict"""
    rng = np.random.default_rng(seed + d)
    X, T = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    T[-2:] = X[[3, n - 1]]
    W, w = rng.standard_normal((n, m)), rng.standard_normal(n)
    Z = np.vstack([X, T])
    dX, dT = hk.array(X.T), hk.array(T.T)
    ldo, ldw = n + 3, n + 5
    ktype, h = KT[kern], width(d)
    spec = K.KernelSpec(dX.ptr, n, d, ktype, 1, h, 2.0)
    dO = hk.array(np.full((ldo, m + 1), S))
    hk.check(hk.lib.hssk_kernel_cross(hk.ctx, ctypes.byref(spec), dT.ptr, m, dO.ptr, ldo))
    hk.sync()
    got = dO.get()
    assert np.all(got[n:, :] == S) and np.all(got[:, m] == S), "hssk_kernel_cross wrote outside its block"
    k, s, dks, _ = matern_ref(Z, np.arange(n), n + np.arange(m), ktype, h, 0.0)
    b = entry_bound(k, s, dks, d, 0.0)
    err = np.abs(got[:n, :m].astype(LD) - k)
    frac = float((err / b).max())
    assert np.all(err <= b), (kern, n, m, d, frac)
    assert got[3, m - 2] == 1.0 and got[n - 1, m - 1] == 1.0
    hk.check(hk.lib.hssk_kernel_cross(hk.ctx, ctypes.byref(spec), dT.ptr, m, dO.ptr, ldo))
    hk.sync()
    assert np.array_equal(got, dO.get()), "two cross calls differ"
    Wp = np.full((ldw, m), 1e300)
    Wp[:n] = W
    dW, dP = hk.array(Wp), hk.array(np.full((m + 2,), S))
    hk.check(hk.lib.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(spec), dW.ptr, ldw, dT.ptr, m, dP.ptr))
    hk.sync()
    pc = dP.get()
    assert np.all(pc[m:] == S)
    aW = np.abs(W).astype(LD)
    ref, bound = (W.astype(LD) * k).sum(0), (aW * b).sum(0) + n * U * (aW * k).sum(0)
    errc = np.abs(pc[:m].astype(LD) - ref)
    fracc = float((errc / bound).max())
    assert np.all(errc <= bound), (kern, n, m, d, fracc)
    assert float(bound.max()) <= 1e-9 * float(np.abs(ref).max())
    hk.check(hk.lib.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(spec), dW.ptr, ldw, dT.ptr, m, dP.ptr))
    hk.sync()
    assert np.array_equal(pc, dP.get()), "two predict_cols calls differ"
    dW.set(np.vstack([np.tile(w[:, None], (1, m)), np.full((ldw - n, m), 1e300)]))
    dw, dQ = hk.array(w), hk.array(np.full(m + 2, S))
    hk.check(hk.lib.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(spec), dW.ptr, ldw, dT.ptr, m, dP.ptr))
    hk.check(hk.lib.hssk_kernel_predict(hk.ctx, ctypes.byref(spec), dw.ptr, dT.ptr, m, dQ.ptr))
    hk.sync()
    q = dQ.get()
    assert np.all(q[m:] == S) and np.array_equal(dP.get()[:m], q[:m]), kern
    refp = (w.astype(LD)[:, None] * k).sum(0)
    bp = (np.abs(w).astype(LD)[:, None] * (b + n * U * k)).sum(0)
    assert np.all(np.abs(q[:m].astype(LD) - refp) <= bp)
    print("cross / predict_cols %s n=%d m=%d d=%d: largest error / bound %.3f, %.3f" % (kern, n, m, d, frac, fracc))
    for v in (dX, dT, dO, dW, dP, dw, dQ):
        v.free()
    return max(frac, fracc)


# ---- 4. hssk_kernel_matmul ----------------------------------------------------------------------------------------------------------
def matmul(hk, dX, n, d, ktype, h, lam, deriv, B, splits=0, pad=(3, 5)):
    nc = B.shape[1]
    ldb, ldo = n + pad[0], n + pad[1]
    Bp = np.full((ldb, nc), 1e300)
    Bp[:n] = B
    dB, dO = hk.array(Bp), hk.array(np.full((ldo, nc + 1), S))
    spec = K.KernelSpec(dX.ptr, n, d, ktype, 1, h, lam)
    hk.check(hk.lib.hssk_kernel_matmul(hk.ctx, ctypes.byref(spec), deriv, dB.ptr, ldb, nc, dO.ptr, ldo, splits))
    hk.sync()
    got = dO.get()
    dB.free()
    dO.free()
    assert np.all(got[n:, :] == S) and np.all(got[:, nc] == S), "hssk_kernel_matmul wrote outside its block"
    return got[:n, :nc]


# (n, nc, d, kernel, deriv, splits, lambda): every n of {1, 15, 16, 17, 63, 64, 65, 130}, every nc of {1, 16, 17, 64}, every d of
# {1, 8, 64 (whole points in the LDS), 65, 70 (chunks of 32 coordinates)}, both kernels, both values of deriv, the splits forced to
# 1 and 3 at n = 130, lambda != 0 in some
MATMUL_CASES = [
    (1, 1, 1, "matern32", 0, 0, 0.0), (15, 16, 8, "matern52", 1, 0, 0.0), (16, 17, 64, "matern32", 1, 0, 0.0),
    (17, 64, 64, "matern52", 0, 0, 2.5), (63, 1, 65, "matern32", 1, 0, 0.0), (64, 16, 70, "matern52", 1, 0, 0.0),
    (65, 17, 70, "matern32", 0, 0, 0.7), (130, 64, 8, "matern32", 1, 1, 0.0), (130, 64, 8, "matern52", 1, 3, 0.0),
    (130, 17, 1, "matern52", 0, 3, 2.5), (130, 64, 65, "matern32", 0, 3, 0.7), (130, 16, 8, "matern32", 0, 1, 0.0),
    (130, 17, 65, "matern52", 1, 3, 0.0),
]


def check_matmul(hk, n, nc, d, kern, deriv, splits, lam, seed=11):
    rng = np.random.default_rng(seed + n + d)
    X, B = rng.standard_normal((n, d)), rng.standard_normal((n, nc))
    ktype, h = KT[kern], width(d)
    dX = hk.array(X.T)
    got = matmul(hk, dX, n, d, ktype, h, lam, deriv, B, splits)
    g, bp = g_reference(X, ktype, h, deriv, lam)
    ref, E = g @ B.astype(LD), product_bound(g, bp, B)
    err = np.abs(got.astype(LD) - ref)
    frac = float((err / E).max()) if n > 1 or deriv == 0 else 0.0
    print("kernel_matmul %s n=%d nc=%d d=%d deriv=%d splits=%d: largest error / bound %.3f" % (kern, n, nc, d, deriv, splits, frac))
    assert np.all(err <= E), (kern, n, nc, d, deriv, splits, frac)
    if n > 1:
        assert float(E.max()) <= 1e-9 * float(np.abs(ref).max()), "the case proves nothing"
    assert np.array_equal(got, matmul(hk, dX, n, d, ktype, h, lam, deriv, B, splits)), "two calls differ"
    auto = hk.lib.hssk_kernel_matmul_splits(n)
    assert np.array_equal(matmul(hk, dX, n, d, ktype, h, lam, deriv, B, 0), matmul(hk, dX, n, d, ktype, h, lam, deriv, B, auto)), "splits = 0"
    dX.free()
    return frac


def check_matmul_properties(hk, seed=5):
    """duplicate points contribute exactly 0 to the derivative product (no division by the distance) and exactly B to the value
    product; the diagonal of the derivative is exactly 0"""
    rng = np.random.default_rng(seed)
    n = 130
    for kern, ktype in KT.items():
        for d in (8, 70):
            h = width(d)
            X = rng.standard_normal((n, d))
            X[77], X[129] = X[3], X[64]
            dX = hk.array(X.T)
            B = np.zeros((n, 4))
            B[77, 0], B[3, 1], B[129, 2], B[64, 3] = 1.5, -2.0, 3.0, 0.25
            for splits in (1, 3):
                got = matmul(hk, dX, n, d, ktype, h, 0.0, 1, B, splits)
                for col, (i, j) in enumerate([(3, 77), (77, 3), (64, 129), (129, 64)]):
                    assert got[i, col] == 0.0 and got[j, col] == 0.0, (kern, d, splits, i, j)
                assert np.count_nonzero(got) == 4 * (n - 2)
                val = matmul(hk, dX, n, d, ktype, h, 0.0, 0, B, splits)
                for col, (i, j) in enumerate([(3, 77), (77, 3), (64, 129), (129, 64)]):
                    assert val[i, col] == val[j, col] == B[j, col], (kern, d, splits, i, j)
            dX.free()


# ---- 5. the FP32 routes -------------------------------------------------------------------------------------------------------------
def scaled(X, ktype, h):
    return (X - X.mean(0)) * (np.sqrt(3.0 if ktype == 3 else 5.0) / h)


def pair_error32(X, ktype, h, tau):
    """(e32, may_mf, may_df) of the module docstring for all pairs of the rows of X: gpmixed_cases.pair_delta's du on the Matern
    scaling (its Gauss branch computes sum_j df_j^2 of whatever points it is given: here through a width that makes its scale
    ours), then e32 = D du + u24 (2 s |dk/ds| + 12 k)"""
    n, d = X.shape
    xt = scaled(X, ktype, h)
    x32 = xt.astype(np.float32).astype(np.float64)
    E, dE1 = np.zeros((n, n)), np.zeros((n, n))
    for j in range(d):
        df = np.abs(xt[:, None, j] - xt[None, :, j])
        mj = np.abs(xt[:, None, j]) + np.abs(xt[None, :, j])
        E += df * df
        dE1 += 2.0 * df * U24 * mj + (U24 * mj) ** 2
    dE2 = (d + 3) * U24 * (E + dE1)
    nrm = (x32 * x32).sum(1)
    dE3 = 4.0 * (d + 4) * U24 * (nrm[:, None] + nrm[None, :])
    nt = (n + 63) // 64
    tmax = np.array([nrm[t * 64:(t + 1) * 64].astype(np.float32).max() for t in range(nt)], dtype=np.float64)
    rule = 4.0 * (d + 4) * U24 * (tmax[:, None] + tmax[None, :])
    may_mf, may_df = rule <= tau * (1 + 1e-3), rule >= tau * (1 - 1e-3)
    tile = np.arange(n) // 64
    mf, dfm = may_mf[np.ix_(tile, tile)], may_df[np.ix_(tile, tile)]
    du = dE1 + np.maximum(np.where(mf, dE3, 0.0), np.where(dfm, dE2, 0.0))
    idx = np.arange(n)
    k, s, dks, _ = matern_ref(X, idx, idx, ktype, h, 0.0)
    D = 0.5 if ktype == 3 else 1.0 / 6.0
    e32 = D * du.astype(LD) + U24 * (2 * s * dks + 12 * k)
    e32[idx, idx] = 0.0                              # the pair r == i is selected to be 1
    return k, e32, may_mf, may_df


def product_bound32(k, e32, B, lam, splits):
    n = len(k)
    aB = np.abs(B).astype(LD)
    mag = k @ aB + abs(lam) * aB
    return (e32 + 72 * U24 * k) @ aB + LD(2.0 ** -126) * aB.sum(0)[None, :] + (n / 64.0 + splits + 4) * U * mag


# (n, nc, d, kernel, lambda): every n of {1, 63, 64, 65, 130, 200}, every d of {1, 8, 33, 64}
MATMUL32_CASES = [(1, 1, 1, "matern32", 0.5), (63, 17, 8, "matern52", 2.5), (64, 64, 33, "matern32", 0.7), (65, 1, 64, "matern52", 2.5),
                  (130, 17, 8, "matern32", 0.05), (200, 64, 8, "matern52", 4.0), (200, 17, 33, "matern52", 0.7), (130, 16, 64, "matern32", 0.0),
                  (200, 5, 1, "matern32", 2.5)]


def near_mean_points(rng, n, d, h, ktype):
    """within one width of their mean -- and so close to it that the scaled norms pass the rule of the FP32 product (TAU 2^-17)"""
    lim = GM.TAU / (8.0 * (d + 4) * U24) * 0.9
    X = rng.standard_normal((n, d))
    X *= min(1.0, np.sqrt(lim / (3.0 if ktype == 3 else 5.0)) * h) / np.sqrt((X * X).sum(1).max() + 1e-300) * 0.99
    return X


def check_matmul32(hk, n, nc, d, kern, lam, seed=13):
    """hssk_kernel_matmul_f32 on a point set near its mean (matrix-core tiles > 0, none in the difference form), on the same set
    shifted by 50 widths in one tile's worth of directions (all tiles in the difference form: the rule refuses them) -- both under
    the per-pair bound at the splits 1, 3 and 0, bit for bit repeatable, the route counts adding up"""
    rng = np.random.default_rng(seed + n + 3 * d + nc)
    ktype, h = KT[kern], width(d)
    Xn = near_mean_points(rng, n, d, h, ktype)
    far = Xn.copy()
    far[::2] += 50.0 * h                             # half of the points 50 widths away: every tile's norms are huge
    B = rng.standard_normal((n, nc))
    worst = 0.0
    for tag, X in (("near", Xn), ("shifted", far)):
        P = GM.Prepared(hk, X, ktype, h, lam)
        k, e32, may_mf, may_df = pair_error32(X, ktype, h, GM.TAU)
        ref = k @ B.astype(LD) + LD(lam) * B.astype(LD)
        nt = (n + 63) // 64
        auto = hk.lib.hssk_kernel_matmul_f32_splits(n)
        outs = {}
        for splits in sorted({1, 3, 0}):
            got, st = P.matmul(B, splits, stats=True)
            outs[splits] = got
            eff = auto if splits == 0 else splits
            per = -(-nt // min(eff, nt))
            used = -(-nt // per)
            E = product_bound32(k, e32, B, lam, used)
            err = np.abs(got.astype(LD) - ref)
            frac = float((err / E).max())
            worst = max(worst, frac)
            print("kernel_matmul_f32 %s %s n=%d nc=%d d=%d splits=%d: largest error / bound %.3f, tiles mfma %d diff %d"
                  % (kern, tag, n, nc, d, splits, frac, st[0], st[1]))
            assert np.all(np.isfinite(got)) and np.all(err <= E), (kern, tag, n, nc, d, splits, frac)
            assert st[0] + st[1] == nt * nt and st[2] == used, (st, nt, used)
            if tag == "near":
                assert st[0] == nt * nt and st[1] == 0, (tag, st)
                assert float(E.max()) <= 1e-3 * float(np.abs(ref).max())
            elif n > 1:
                assert st[0] == 0 and st[1] == nt * nt, (tag, st)
            assert np.array_equal(got, P.matmul(B, splits)), "two calls differ"
        assert np.array_equal(outs[0], P.matmul(B, auto)), "splits = 0"
        P.free()
    return worst


def check_matmul32_properties(hk, seed=37):
    """near-duplicates x and x + 1e-7 spread over different tiles: on the matrix cores cancellation makes u negative there, and the
    results are finite and inside the bound (the clamp); the pair r == i is exactly 1: one-hot columns give 1 + lambda on the
    diagonal; a column does not depend on the other columns"""
    rng = np.random.default_rng(seed)
    n, d, lam = 200, 8, 0.5
    for kern, ktype in KT.items():
        h = width(d)
        X = near_mean_points(rng, n, d, h, ktype)
        for a, b in ((3, 70), (10, 140), (65, 199), (20, 21)):
            X[b] = X[a] + 1e-7
        P = GM.Prepared(hk, X, ktype, h, lam)
        k, e32, _, _ = pair_error32(X, ktype, h, GM.TAU)
        B = np.zeros((n, 8))
        for c, i in enumerate((3, 70, 10, 140, 65, 199, 20, 0)):
            B[i, c] = 1.0
        got, st = P.matmul(B, 1, stats=True)
        assert st[0] > 0 and np.all(np.isfinite(got)), st
        ref = k @ B.astype(LD) + LD(lam) * B.astype(LD)
        assert np.all(np.abs(got.astype(LD) - ref) <= product_bound32(k, e32, B, lam, 1)), kern
        for c, i in enumerate((3, 70, 10, 140, 65, 199, 20, 0)):
            assert got[i, c] == 1.0 + lam, (kern, i, got[i, c])
        Bf = rng.standard_normal((n, 17))
        full = P.matmul(Bf, 3)
        for c in (0, 9, 16):
            assert np.array_equal(full[:, c], P.matmul(Bf[:, c:c + 1], 3)[:, 0]), "a column depends on the other columns"
        P.free()


def predict_reference32(X, T, w, ktype, h, diff_only):
    """FP64 value P (m) and bound B (m) for float32 inputs (module docstring)"""
    X64, T64, w64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (X, T, w))
    n, d = X64.shape
    Z = np.vstack([X64, T64])
    k, s, dks, _ = matern_ref(Z, np.arange(n), n + np.arange(len(T64)), ktype, h, 0.0)
    nu2 = 3.0 if ktype == 3 else 5.0
    mu = X64.mean(0)
    nx, ntt = ((X64 - mu) ** 2).sum(1) * nu2 / h ** 2, ((T64 - mu) ** 2).sum(1) * nu2 / h ** 2
    du = (d + 4) * U24 * np.asarray(s * s, dtype=np.float64)
    if not diff_only:
        du = du + np.minimum(4 * (d + 4) * U24 * (nx[:, None] + ntt[None, :]), KP.TAU)
    D = 0.5 if ktype == 3 else 1.0 / 6.0
    e32 = D * du.astype(LD) + U24 * (2 * s * dks + 12 * k)
    aw = np.abs(w64).astype(LD)
    P = np.asarray(w64.astype(LD) @ k, dtype=np.float64)
    B = np.asarray(aw @ (e32 + 64 * U24 * k), dtype=np.float64)
    return P, B + U24 * np.abs(P) + 2.0 ** -126 * (float(aw.sum()) + 1)


# (n, m, d): every n of {1, 63, 64, 65, 130, 200}, every d of {1, 8, 33, 64}, and 70 for hssk_matern_predict_f32_wide
PREDICT32_CASES = [(1, 70, 1), (63, 64, 8), (64, 65, 33), (65, 1, 64), (130, 70, 8), (200, 130, 33), (200, 70, 64), (130, 70, 70)]


def check_predict32(hk, kern, n, m, d, seed=100):
    """hssk_matern_predict_f32 (d <= 64) / _wide (d = 70) under the bound: points within one width of their mean (matrix-core
    tiles > 0 up to 64 coordinates), the same points shifted apart by 50 widths (all tiles in the difference form), near-duplicate
    training and test points on the matrix cores (finite, inside the bound); two calls bit for bit"""
    r = np.random.default_rng(seed + n + d)
    ktype, h = KT[kern], width(d)
    X = (r.standard_normal((n, d)) / np.sqrt(d) * 0.5 * h).astype(np.float32)       # |x - mean| about half a width
    T = (r.standard_normal((m, d)) / np.sqrt(d) * 0.5 * h).astype(np.float32)
    T[-1] = X[0] + np.float32(1e-7)
    if n > 1:
        X[-1] = X[0] + np.float32(1e-7)
    w = r.standard_normal(n).astype(np.float32)
    worst = 0.0
    sets = [("near", X, T)]
    Xs, Ts = X.copy(), T.copy()
    Xs[::2] += np.float32(50.0 * h)
    Ts[1::2] -= np.float32(50.0 * h)
    sets.append(("shifted", Xs, Ts))
    for tag, Xa, Ta in sets:
        out, st = hk.kernel_predict_f32(Xa, w, Ta, ktype, h, stats=True)
        out2 = hk.kernel_predict_f32(Xa, w, Ta, ktype, h)
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), out2.view(np.uint32)), "two runs differ"
        P, B = predict_reference32(Xa, Ta, w, ktype, h, d > 64)
        err = np.abs(out.astype(np.float64) - P)
        frac = float((err / B).max())
        worst = max(worst, frac)
        print("matern_predict_f32 %s %s n=%d m=%d d=%d: largest error / bound %.3f, tiles mfma %d diff %d, splits %d"
              % (kern, tag, n, m, d, frac, st[0], st[1], st[2]))
        assert np.all(np.isfinite(out)) and np.all(err <= B), (kern, tag, n, m, d, frac)
        assert st[0] + st[1] == (-(-n // 64)) * (-(-m // 64)) and st[2] == KP.splits_expected(n, m), st
        if tag == "near":
            assert (st[0] > 0 and st[1] == 0) if d <= 64 else st[0] == 0, (tag, st)
            if n > 1:
                assert float(np.median(B)) <= 1e-2 * float(np.median(np.abs(P))), "the case proves nothing"
        else:
            assert st[0] == 0 and st[1] > 0, (tag, st)
    return worst


def check_predict32_refusals(hk):
    """twice_nu outside {3, 5} and the wrong dimension range are refused with the output untouched; the entry points of the three
    kernels of the reference go on refusing the type codes 3, 4 and 5"""
    X, T, w = KP.points(1, 64, 10, 4)
    dX, dT, dw = hk.array(X.ravel()), hk.array(T.ravel()), hk.array(w)
    fill = np.full(10, np.float32(S))
    dp = hk.array(fill)
    f, g = hk.lib.hssk_matern_predict_f32, hk.lib.hssk_matern_predict_f32_wide
    assert f(hk.ctx, dX.ptr, 64, 4, 3, 1.0, dw.ptr, dT.ptr, 10, dp.ptr, None) == 0
    hk.sync()
    assert not np.array_equal(dp.get(), fill)
    dp.set(fill)
    for nu2 in (0, 1, 2, 4, 6, -3):
        assert f(hk.ctx, dX.ptr, 64, 4, nu2, 1.0, dw.ptr, dT.ptr, 10, dp.ptr, None) != 0 and "twice_nu" in hk.error()
        assert g(hk.ctx, dX.ptr, 4, 70, nu2, 1.0, dw.ptr, dT.ptr, 3, dp.ptr, None) != 0 and "twice_nu" in hk.error()
    assert f(hk.ctx, dX.ptr, 3, 65, 5, 1.0, dw.ptr, dT.ptr, 3, dp.ptr, None) != 0 and "dimension" in hk.error()
    assert g(hk.ctx, dX.ptr, 64, 4, 5, 1.0, dw.ptr, dT.ptr, 10, dp.ptr, None) != 0 and "dimension" in hk.error()
    assert f(hk.ctx, dX.ptr, 64, 4, 5, 0.0, dw.ptr, dT.ptr, 10, dp.ptr, None) != 0 and "width" in hk.error()
    for kt in (3, 4, 5):
        assert hk.lib.hssk_kernel_predict_f32(hk.ctx, dX.ptr, 64, 4, kt, 1, 1.0, dw.ptr, dT.ptr, 10, dp.ptr, None) != 0 and "type" in hk.error()
    hk.sync()
    assert np.array_equal(dp.get(), fill), "a refused call wrote its output"
    for v in (dX, dT, dw, dp):
        v.free()


# ---- 9. refusals and lifecycle ------------------------------------------------------------------------------------------------------
def check_refusals(hk):
    """a type of 5 is refused everywhere, the types 3 and 4 by the construction kernels (hssk_kernel_eval_vbatched,
    hssk_gram_gen_vbatched), all with the outputs untouched; ANOVA messages still say ANOVA"""
    n, d, nc = 40, 8, 5
    rng = np.random.default_rng(1)
    dX, dB = hk.array(rng.standard_normal((d, n))), hk.array(rng.standard_normal((n, nc)))
    fill = np.full((n + 1, n), S)
    dO = hk.array(fill)
    bad = K.KernelSpec(dX.ptr, n, d, 5, 1, 1.3, 0.0)
    anova = K.KernelSpec(dX.ptr, n, d, 2, 2, 1.3, 0.0)
    L = hk.lib
    desc = (K.KevalDesc * 1)(K.KevalDesc(None, None, dO.ptr, 8, 8, n + 1, 0, 0))
    assert L.hssk_kernel_eval_vbatched(hk.ctx, ctypes.byref(bad), desc, 1) != 0 and "type" in hk.error()
    assert L.hssk_gram_gen_supported(ctypes.byref(bad), 16) == 0
    gd = (K.GramGenDesc * 1)(K.GramGenDesc(None, 0, None, 20, 8, 8, dO.ptr, n + 1))
    assert L.hssk_gram_gen_vbatched(hk.ctx, ctypes.byref(bad), gd, 1) == 2
    for kt in (3, 4):
        mat = K.KernelSpec(dX.ptr, n, d, kt, 1, 1.3, 0.0)
        assert L.hssk_kernel_eval_vbatched(hk.ctx, ctypes.byref(mat), desc, 1) == 2 and "Matern" in hk.error()
        assert L.hssk_gram_gen_supported(ctypes.byref(mat), 16) == 0
        assert L.hssk_gram_gen_vbatched(hk.ctx, ctypes.byref(mat), gd, 1) == 2
    assert L.hssk_kernel_cross(hk.ctx, ctypes.byref(bad), dX.ptr, 8, dO.ptr, n + 1) != 0
    assert L.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(bad), dB.ptr, n, dX.ptr, 4, dO.ptr) != 0
    assert L.hssk_kernel_predict(hk.ctx, ctypes.byref(bad), dB.ptr, dX.ptr, 4, dO.ptr) != 0
    for deriv in (0, 1):
        assert L.hssk_kernel_matmul(hk.ctx, ctypes.byref(bad), deriv, dB.ptr, n, nc, dO.ptr, n + 1, 0) != 0 and "type" in hk.error()
        assert L.hssk_kernel_matmul(hk.ctx, ctypes.byref(anova), deriv, dB.ptr, n, nc, dO.ptr, n + 1, 0) == 2 and "ANOVA" in hk.error()
    nb = L.hssk_kernel_matmul_f32_prep_bytes(n, d)
    prep = hk.array(np.full(nb, 0xA5, dtype=np.uint8))
    assert L.hssk_kernel_matmul_f32_prep(hk.ctx, ctypes.byref(bad), prep.ptr, nb) != 0
    assert L.hssk_kernel_matmul_f32_prep(hk.ctx, ctypes.byref(anova), prep.ptr, nb) == 2 and "ANOVA" in hk.error()
    assert L.hssk_kernel_matmul_f32(hk.ctx, ctypes.byref(bad), prep.ptr, dB.ptr, n, nc, dO.ptr, n + 1, 0, None) != 0
    assert L.hssk_kernel_matmul_f32(hk.ctx, ctypes.byref(anova), prep.ptr, dB.ptr, n, nc, dO.ptr, n + 1, 0, None) == 2 and "ANOVA" in hk.error()
    hk.sync()
    assert np.array_equal(dO.get(), fill) and np.all(prep.get() == 0xA5), "a refused call wrote its output"
    for v in (dX, dB, dO, prep):
        v.free()
