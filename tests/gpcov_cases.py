"""Checks of the joint predictive covariance of a kept kernel ridge regression fit: hssk_kernel_cross_split,
hssk_kernel_cross_matmul, Kernel<double>::predict_covariance / predict_covariance_exact / covariance_ms with their C and Python
forms, and KernelRegression.sample_posterior.  Shared by the CPU emulator tests (tests/test_gpcov_emu.py) and the GPU tests
(tests/test_gpcov_gpu.py), as tests/gp_cases.py is.

hssk_kernel_cross_split.  An entry depends on its pair alone and the pair arithmetic is the one piece of code of
hssk_kernel_cross: the block is compared with that of hssk_kernel_cross BIT FOR BIT, for every split count.  No bound is involved.

hssk_kernel_cross_matmul, out(a, c) = sum_r k(t_a, x_r) B(r, c).  The reference is long double numpy (kernel_cases.kernel_ref for
Gauss and Laplace, matern_cases.matern_ref for the two Matern kernels) with the entry bounds b of those modules
(kernel_entry_bound, matern_cases.entry_bound; lambda = 0).  The roundings of the kernel as written (u = 2^-53):
  * an evaluated entry k^ is within b of k; its product with B(r, c) and the addition to the accumulator are ONE rounding: the FP64
    matrix core fuses them (v_mfma_f64_16x16x4_f64 is four chained fused multiply-adds per accumulator), so the accumulator of an
    entry is rounded once per training point of its split: n roundings over all splits (a padded point adds an exact zero);
  * the split partials are added in split order: splits - 1 roundings;
  * nothing else (no scaling, no lambda): n + splits - 1 roundings, each relative to a partial sum that is at most
    sum_r |k_ra B(r, c)| to first order.
Asserted is the form of the issue, which leaves five roundings of room:
    B_ac = sum_r |B(r, c)| b_ra + (n + splits + 4) u sum_r |k_ra B(r, c)|,
splits the count the call really takes (at most one per stage of 16 training points).  A case only proves something while the
reference is large against the bound: every case asserts, per output column, max_a |ref_ac| >= 1e3 max_a B_ac.

The joint covariance.  Hd is the dense form of the matrix the handle writes (gp_cases.dense_model: unsymmetric), X the handle's
cluster-ordered points, k_a = k(X, t_a) in long double with entry bounds b_a, z_b = Hd^-1 k_b by numpy, and
    Q_ab = k_a^T z_b,    C_ref = Ktt - (Q + Q^T) / 2.
The library computes k^_b = k_b + e_b, |e_rb| <= b_rb, solves z^_b = Hd^-1 k^_b + delta_b with ||delta_b|| <= 1e-12 cond_2 ||z_b||
(gp_cases.EPS_F), evaluates the row k^_a = k_a + e_a again inside the product and adds over r in stages and splits.  To first order
    Q^_ab - Q_ab = k_a^T delta_b + e_a^T z_b + k_a^T Hd^-1 e_b + (rounding of the sum),
    bound_ab = 1e-12 cond_2 ||k_a|| ||z_b|| + sum_r |z_rb| b_ra + ||Hd^-1||_2 ||k_a|| ||b_b|| + (n + ceil(n / 16)) u sum_r |k_ra z_rb|,
the last term being the count above, n + splits - 1 roundings, with the most splits there can be: one per stage of 16 training
points, splits <= ceil(n / 16), whatever hssk_kernel_cross_matmul_splits(n, m) chooses.  The entry of C gets (bound_ab + bound_ba) / 2 plus
the entry bound of k(t_a, t_b); the halving, the sum Q_ab + Q_ba and the subtraction are three more roundings of numbers of
magnitude at most 1 + |Q|, 4 u (1 + |Q_ab|), added to the bound.  A case only proves something while the bound is small against the
covariances' own scale: every case asserts bound_ab <= 1e-3 sqrt(C_ref,aa C_ref,bb) for all pairs.

The diagonal against predict_variance: both are within their own bounds of the same reference value (Q_cc = k_c^T z_c), so they
differ by at most the sum of the two bounds (gp_cases.variance_reference gives that of predict_variance).

exact = True: the same with the dense exact A = K + lambda I in place of Hd; a column whose reported final relative residual is
resid_b has ||z^_b - z_b|| <= ||A^-1||_2 resid_b ||k_b||, which adds resid_b ||A^-1||_2 ||k_b|| ||k_a|| to bound_ab.

sample_posterior is numpy on the library's covariance: recomputed in the test from the same seed, equal to 1e-12 relative (the
two evaluate the same expressions; the room is for a BLAS that orders a product differently in a second call)."""
import ctypes

import numpy as np

import gp_cases as GP
import gpgrad_cases as GG
import kernel_cases as KC
import matern_cases as MC
from strumpack_amd import hssk as K

LD = np.longdouble
U = KC.U53
S = KC.SENTINEL
TYPES = {"gauss": 0, "laplace": 1, "matern32": 3, "matern52": 4}
STAGE = 16     # training points per stage of hssk_kernel_cross_matmul
TILE = 64      # training points per tile of hssk_kernel_cross_split


def width(ktype, d):
    return MC.width(d) if ktype >= 3 else float(KC.kernel_widths(d)[ktype])


def cross_ref(X, T, ktype, h):
    """(k, b): k(t_a, x_r) as an m x n long double matrix and the bound of one evaluated entry"""
    n, m, d = len(X), len(T), X.shape[1]
    Z = np.vstack([X, T])
    if ktype >= 3:
        k, s, dks, _ = MC.matern_ref(Z, n + np.arange(m), np.arange(n), ktype, h)
        return k, MC.entry_bound(k, s, dks, d, 0.0)
    k, a, A = KC.kernel_ref(Z, n + np.arange(m), np.arange(n), ktype, h, 0.0)
    return k, KC.kernel_entry_bound(a, A, ktype, d, 0.0)


# ---- 1. hssk_kernel_cross_split ------------------------------------------------------------------------------------------------------
# (n, m, d): the corners n = 1, m = 1, d = 65; ragged and full tiles of both point sets; one coordinate, whole points in the LDS (8,
# 64), the first dimension that passes in chunks of 32 and a ragged last chunk (65, 100); eleven training tiles at n = 700
CROSS_SHAPES = ((1, 1, 65), (63, 64, 1), (64, 65, 8), (65, 130, 64), (65, 1, 65), (700, 130, 8), (700, 65, 100), (1, 130, 8), (700, 1, 64))
CROSS_KINDS = dict(GP.KINDS, matern32=(3, 1), matern52=(4, 1))


def cross_call(hk, f, spec, dT, n, m, *splits):
    ldo = n + 3
    dO = hk.array(np.full((ldo, m + 1), S))
    hk.check(f(hk.ctx, ctypes.byref(spec), dT.ptr, m, dO.ptr, ldo, *splits))
    hk.sync()
    got = dO.get()
    dO.free()
    assert np.all(got[n:, :] == S) and np.all(got[:, m] == S), "the cross block wrote outside its block"
    return got[:n, :m]


def check_cross_split(hk, n, m, d, seed=7):
    """all five types: the block of hssk_kernel_cross_split bit for bit that of hssk_kernel_cross for splits 0, 1, 3 and one more than
    there are 64-point tiles of n; ldo = n + 3 with sentinels in the padding rows and in column m"""
    rng = np.random.default_rng(seed + n + d)
    X, T = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    T[-1] = X[n // 2]
    dX, dT = hk.array(X.T), hk.array(T.T)
    tiles = (n + TILE - 1) // TILE
    auto = hk.lib.hssk_kernel_cross_splits(n, m)
    assert 1 <= auto <= tiles, (auto, tiles)
    for name, (ktype, p) in CROSS_KINDS.items():
        if ktype == 2 and p > d:
            continue
        h = width(ktype if ktype != 2 else 0, d)
        spec = K.KernelSpec(dX.ptr, n, d, ktype, p, h, 2.0)
        ref = cross_call(hk, hk.lib.hssk_kernel_cross, spec, dT, n, m)
        assert np.all(ref > 0.0) or ktype == 2
        for splits in (0, 1, 3, tiles + 1):
            got = cross_call(hk, hk.lib.hssk_kernel_cross_split, spec, dT, n, m, splits)
            assert np.array_equal(got, ref), (name, n, m, d, splits, float(np.abs(got - ref).max()))
    for v in (dX, dT):
        v.free()


def check_cross_split_refusals(hk):
    n, m, d = 70, 5, 3
    rng = np.random.default_rng(2)
    dX, dT = hk.array(rng.standard_normal((d, n))), hk.array(rng.standard_normal((d, m)))
    fill = np.full((n, m), S)
    dO = hk.array(fill)
    f = hk.lib.hssk_kernel_cross_split
    ok = K.KernelSpec(dX.ptr, n, d, 0, 1, 1.3, 0.0)
    empty = K.KernelSpec(dX.ptr, 0, d, 0, 1, 1.3, 0.0)
    bad = K.KernelSpec(dX.ptr, n, d, 2, 9, 1.3, 0.0)
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dO.ptr, n - 1, 0) != 0            # ldo < n
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dO.ptr, n, -1) != 0
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, -1, dO.ptr, n, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), None, m, dO.ptr, n, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, None, n, 0) != 0
    assert f(hk.ctx, None, dT.ptr, m, dO.ptr, n, 0) != 0
    assert f(hk.ctx, ctypes.byref(bad), dT.ptr, m, dO.ptr, n, 0) != 0                # ANOVA degree above 8
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, 0, None, n, 0) == 0                   # nothing to do
    assert f(hk.ctx, ctypes.byref(empty), dT.ptr, m, dO.ptr, 0, 0) == 0
    hk.sync()
    assert np.array_equal(dO.get(), fill), "a refused call wrote its output"
    assert hk.lib.hssk_kernel_cross_splits(0, 5) == 1 and hk.lib.hssk_kernel_cross_splits(5, 0) == 1
    for v in (dX, dT, dO):
        v.free()


# ---- 2. hssk_kernel_cross_matmul -----------------------------------------------------------------------------------------------------
def stages(n):
    return (n + STAGE - 1) // STAGE


def splits_taken(hk, n, m, splits):
    """the count the call really takes: whole stages per split, none empty (km_split_plan)"""
    s = min(splits if splits > 0 else hk.lib.hssk_kernel_cross_matmul_splits(n, m), stages(n))
    per = -(-stages(n) // s) * STAGE
    return -(-n // per)


def cross_matmul(hk, dX, n, d, ktype, h, dT, m, B, splits=0, lam=0.0):
    """one call on a padded B (ldb = n + 3) into a pre-filled padded output (ldo = m + 5): the m x nc result after the sentinels"""
    nc = B.shape[1]
    ldb, ldo = n + 3, m + 5
    Bp = np.full((ldb, nc), 1e300)
    Bp[:n] = B
    dB, dO = hk.array(Bp), hk.array(np.full((ldo, nc + 1), S))
    spec = K.KernelSpec(dX.ptr, n, d, ktype, 1, h, lam)
    hk.check(hk.lib.hssk_kernel_cross_matmul(hk.ctx, ctypes.byref(spec), dT.ptr, m, dB.ptr, ldb, nc, dO.ptr, ldo, splits))
    hk.sync()
    got = dO.get()
    dB.free()
    dO.free()
    assert np.all(got[m:, :] == S) and np.all(got[:, nc] == S), "hssk_kernel_cross_matmul wrote outside its block"
    return got[:m, :nc]


def product_bound(k, b, B, n, splits):
    """B_ac of the module docstring"""
    aB = np.abs(B).astype(LD)
    return b @ aB + (n + splits + 4) * U * (np.abs(k) @ aB)


# (n, m, nc, d, kernel, splits; -1: one split per stage, ceil(n / 16)).  Every n of {1, 15, 16, 17, 64, 65, 700, 1100}, every m of
# {1, 63, 64, 65, 130}, every nc of {1, 16, 17, 64}, every d of {1, 8, 64 (whole points in the LDS), 65, 100 (chunks of 32
# coordinates, ragged last chunk)}, the four kernels, the splits 0, 1, 2, 3 and ceil(n / 16)
CROSS_MATMUL_CASES = [
    (1, 1, 1, 1, "gauss", 0),
    (15, 63, 16, 8, "laplace", 1),
    (16, 64, 17, 64, "matern32", 2),
    (17, 65, 64, 65, "matern52", 3),
    (64, 130, 1, 100, "gauss", -1),
    (65, 1, 16, 8, "laplace", -1),
    (65, 130, 17, 1, "matern32", 0),
    (700, 130, 64, 8, "gauss", 0),
    (700, 65, 17, 65, "laplace", 3),
    (700, 64, 64, 64, "matern52", 1),
    (1100, 64, 64, 8, "gauss", -1),
    (1100, 63, 16, 1, "laplace", 2),
    (1100, 130, 17, 100, "matern32", 0),
    (1100, 65, 1, 8, "matern52", 3),
]


def check_cross_matmul(hk, n, m, nc, d, kern, splits, seed=11):
    """the product against the long double reference under B_ac; the reference large against the bound; padded operands with
    sentinels; two calls bit for bit; splits = 0 bit for bit the forced hssk_kernel_cross_matmul_splits(n, m)"""
    rng = np.random.default_rng(seed + n + d + m)
    X, T, B = rng.standard_normal((n, d)), rng.standard_normal((m, d)), rng.standard_normal((n, nc))
    ktype = TYPES[kern]
    h = width(ktype, d)
    if splits < 0:
        splits = stages(n)
    dX, dT = hk.array(X.T), hk.array(T.T)
    got = cross_matmul(hk, dX, n, d, ktype, h, dT, m, B, splits, lam=2.0)        # (a lambda in the spec must not reach the product)
    k, b = cross_ref(X, T, ktype, h)
    ref = k @ B.astype(LD)
    E = product_bound(k, b, B, n, splits_taken(hk, n, m, splits))
    err = np.abs(got.astype(LD) - ref)
    frac = float((err / E).max())
    print("kernel_cross_matmul %s n=%d m=%d nc=%d d=%d splits=%d: largest error / bound %.3f, smallest column max|ref| / max bound %.3g"
          % (kern, n, m, nc, d, splits, frac, float((np.abs(ref).max(0) / E.max(0)).min())))
    assert np.all(np.abs(ref).max(0) >= 1e3 * E.max(0)), "the case proves nothing"
    assert np.all(err <= E), (kern, n, m, nc, d, splits, frac)
    assert np.array_equal(got, cross_matmul(hk, dX, n, d, ktype, h, dT, m, B, splits)), "two calls differ"
    auto = hk.lib.hssk_kernel_cross_matmul_splits(n, m)
    assert 1 <= auto <= stages(n)
    assert np.array_equal(cross_matmul(hk, dX, n, d, ktype, h, dT, m, B, 0), cross_matmul(hk, dX, n, d, ktype, h, dT, m, B, auto)), "splits = 0"
    for v in (dX, dT):
        v.free()
    return frac


def check_cross_matmul_properties(hk, seed=5):
    """n = 1 with a test point equal to the training point: k = 1 exactly, the entry is B(0, c) itself; T = X: the product of
    hssk_kernel_matmul(deriv = 0, lambda = 0) within the sum of the two bounds"""
    rng = np.random.default_rng(seed)
    d, nc = 8, 17
    for kern, ktype in TYPES.items():
        h = width(ktype, d)
        X = rng.standard_normal((1, d))
        T = rng.standard_normal((5, d))
        T[3] = X[0]
        B = rng.standard_normal((1, nc))
        dX, dT = hk.array(X.T), hk.array(T.T)
        got = cross_matmul(hk, dX, 1, d, ktype, h, dT, 5, B)
        assert np.array_equal(got[3], B[0]), (kern, got[3], B[0])
        assert not np.array_equal(got[2], B[0])
        for v in (dX, dT):
            v.free()
    n = 130
    for kern, ktype in GG.KT.items():
        h = width(ktype, d)
        X, B = rng.standard_normal((n, d)), rng.standard_normal((n, nc))
        dX = hk.array(X.T)
        for splits in (1, 3):
            a = cross_matmul(hk, dX, n, d, ktype, h, dX, n, B, splits)
            sq = GG.matmul(hk, dX, n, d, ktype, h, 0.0, 0, B, splits)
            g, bp = GG.g_reference(X, ktype, h, d, 0, 0.0)
            k, b = cross_ref(X, X, ktype, h)
            tol = GG.product_bound(g, bp, B) + product_bound(k, b, B, n, splits)
            assert np.all(np.abs(a.astype(LD) - sq.astype(LD)) <= tol), (kern, splits)
        dX.free()


def check_cross_matmul_refusals(hk):
    n, m, d, nc = 40, 7, 8, 5
    rng = np.random.default_rng(1)
    dX, dT, dB = hk.array(rng.standard_normal((d, n))), hk.array(rng.standard_normal((d, m))), hk.array(rng.standard_normal((n, 65)))
    fill = np.full((m + 2, 66), S)
    dO = hk.array(fill)
    f = hk.lib.hssk_kernel_cross_matmul
    ok = K.KernelSpec(dX.ptr, n, d, 0, 1, 1.3, 0.0)
    anova = K.KernelSpec(dX.ptr, n, d, 2, 2, 1.3, 0.0)
    empty = K.KernelSpec(dX.ptr, 0, d, 0, 1, 1.3, 0.0)
    ldo = m + 2
    assert f(hk.ctx, ctypes.byref(anova), dT.ptr, m, dB.ptr, n, nc, dO.ptr, ldo, 0) == 2 and "ANOVA" in hk.error()
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dB.ptr, n, 0, dO.ptr, ldo, 0) != 0             # nc < 1
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dB.ptr, n, 65, dO.ptr, ldo, 0) != 0            # nc > 64
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dB.ptr, n - 1, nc, dO.ptr, ldo, 0) != 0        # ldb < n
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dB.ptr, n, nc, dO.ptr, m - 1, 0) != 0          # ldo < m
    assert f(hk.ctx, ctypes.byref(ok), None, m, dB.ptr, n, nc, dO.ptr, ldo, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, None, n, nc, dO.ptr, ldo, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dB.ptr, n, nc, None, ldo, 0) != 0
    assert f(hk.ctx, None, dT.ptr, m, dB.ptr, n, nc, dO.ptr, ldo, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, m, dB.ptr, n, nc, dO.ptr, ldo, -1) != 0
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, -1, dB.ptr, n, nc, dO.ptr, ldo, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), dT.ptr, 0, None, n, nc, None, ldo, 0) == 0                # m = 0: nothing to do
    hk.sync()
    assert np.array_equal(dO.get(), fill), "a refused call wrote its output"
    assert hk.lib.hssk_kernel_cross_matmul_splits(0, 5) == 1 and hk.lib.hssk_kernel_cross_matmul_splits(5, 0) == 1
    # n = 0 and m > 0: an empty sum, the block is zeroed and nothing else
    assert f(hk.ctx, ctypes.byref(empty), dT.ptr, m, None, 0, nc, dO.ptr, ldo, 0) == 0
    hk.sync()
    got = dO.get()
    assert np.all(got[:m, :nc] == 0.0) and np.all(got[m:, :] == S) and np.all(got[:, nc:] == S)
    # more splits than stages: every split at least one stage
    B = rng.standard_normal((n, nc))
    a = cross_matmul(hk, dX, n, d, 0, 1.3, dT, m, B, 50)
    assert np.array_equal(a, cross_matmul(hk, dX, n, d, 0, 1.3, dT, m, B, 3))
    for v in (dX, dT, dB, dO):
        v.free()


# ---- 3. the kept model ---------------------------------------------------------------------------------------------------------------
MODEL_CASES = [c for c in GP.MODEL_CASES if c[0] in GG.KT]
COUNTS_CASE = ("gauss", 8, 4.0, 1.0)          # also answers for 1, 64 and 65 test points
M_COV = 70                                     # a full chunk of 64 and a rest of 6


def covariance_reference(Hm, sv, X, T, kind, resid=None):
    """(C_ref, bound of an entry of C, bound_ab of Q) of the module docstring for the matrix Hm (dense, singular values sv)"""
    ktype, p, h = kind
    n, d = X.shape
    m = len(T)
    k, b = cross_ref(X, T, ktype, h)                   # m x n
    kt, b = np.asarray(k.T, dtype=np.float64), np.asarray(b.T, dtype=np.float64)      # n x m: column a is k_a
    idx = np.arange(m)
    tt, a, A = KC.kernel_ref(T, idx, idx, ktype, h, 0.0)
    bt = np.asarray(KC.kernel_entry_bound(a, A, ktype, d, 0.0), dtype=np.float64)
    z = np.linalg.solve(Hm, kt)
    Q = kt.T @ z
    cond, inv = sv[0] / sv[-1], 1.0 / sv[-1]
    nk, nz, nb = np.linalg.norm(kt, axis=0), np.linalg.norm(z, axis=0), np.linalg.norm(b, axis=0)
    bq = (GP.EPS_F * cond * np.outer(nk, nz) + b.T @ np.abs(z) + inv * np.outer(nk, nb)
          + (n + -(-n // STAGE)) * U * (np.abs(kt).T @ np.abs(z)))
    if resid is not None:
        bq = bq + inv * np.outer(nk, nk * np.asarray(resid))
    Cref = np.asarray(tt, dtype=np.float64) - 0.5 * (Q + Q.T)
    bound = 0.5 * (bq + bq.T) + bt + 4.0 * U * (1.0 + np.abs(Q))
    return Cref, bound, bq


def check_covariance(C, Cref, bound, bq, tag):
    m = len(Cref)
    assert C.shape == (m, m), (tag, C.shape)
    assert np.array_equal(C, C.T), tag + ": the covariance is not exactly symmetric"
    dg = np.diag(Cref)
    assert np.all(dg > 0.0), (tag, dg.min())
    scale = np.sqrt(np.outer(dg, dg))
    err = np.abs(C - Cref)
    ratio = float((err / bound).max()) if m else 0.0
    print("covariance %s m=%d: variances in [%.3g, %.3g], largest bound / scale %.3g, largest error %.3g, largest error / bound %.3g"
          % (tag, m, dg.min(), dg.max(), float((bq / scale).max()), err.max(), ratio))
    assert np.all(bq <= 1e-3 * scale), (tag, float((bq / scale).max()))          # the case proves something
    assert np.all(err <= bound), (tag, ratio)
    return ratio


def check_model(KM, lib, kern, d, lam, hscale, path):
    """one fit with keep_model: the covariance of 70 test points (a chunk of 64 and one of 6) against the dense form of the kept
    matrix; exactly symmetric; the diagonal against predict_variance; predict_variance the same bits before and after; the
    COUNTS_CASE also for 1, 64 and 65 test points"""
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    tag = "%s R^%d lambda=%g h=%.3g" % (kern, d, lam, kind[2])
    try:
        Hd, sv, _ = GP.dense_model(kr, path)
        assert not np.array_equal(Hd, Hd.T)                                       # (the reference keeps the unsymmetric matrix)
        X = kr.model_points()
        n = len(X)
        worst = 0.0
        for m in (M_COV,) + ((1, 64, 65) if (kern, d, lam, hscale) == COUNTS_CASE else ()):
            Tm = np.ascontiguousarray(T[-m:])
            before = kr.predict_variance(Tm)
            C = kr.predict_covariance(Tm)
            after = kr.predict_variance(Tm)
            assert np.array_equal(before, after), "predict_covariance changed what predict_variance returns"
            Cref, bound, bq = covariance_reference(Hd, sv, X, Tm, kind)
            worst = max(worst, check_covariance(C, Cref, bound, bq, tag))
            vref, vbound = GP.variance_reference(kr, Hd, sv, Tm, kind)
            assert np.all(np.abs(np.diag(C) - before) <= np.diag(bound) + vbound), tag
            assert np.array_equal(C, kr.predict_covariance(Tm)), "two covariance calls differ"
            ms = kr.covariance_ms()
            assert set(ms) == {"cross_ms", "solve_ms", "product_ms"} and all(v >= 0.0 for v in ms.values())
        assert kr.predict_covariance(T[:0]).shape == (0, 0)
    finally:
        kr.destroy()
    return worst


def dense_exact(X, kind, lam):
    idx = np.arange(len(X))
    return KC.kernel_np(X, idx, idx, kind[0], kind[2], lam)


def check_exact(KM, lib, kern="gauss", d=8, lam=4.0, hscale=1.0, m=M_COV, f32=True):
    """exact=True against the dense exact K + lambda I with the same bound, plus resid_b ||A^-1|| ||k_b|| ||k_a|| for the reported
    final relative residual of column b; f32: also with inner="f32" """
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    T = np.ascontiguousarray(T[-m:])
    try:
        X = kr.model_points()
        Km = dense_exact(X, kind, lam)
        sv = np.linalg.svd(Km, compute_uv=False)
        worst = 0.0
        for inner in (None, "f32") if f32 else (None,):
            C, info = kr.predict_covariance(T, exact=True, info=True, inner=inner)
            assert info["converged"] and len(info["residual"]) == m, info
            assert info["solves"] >= 2                                            # (one first solve per chunk at the least)
            assert (info["products32"] > 0) == (inner == "f32")
            Cref, bound, bq = covariance_reference(Km, sv, X, T, kind, info["residual"])
            worst = max(worst, check_covariance(C, Cref, bound, bq, "exact %s R^%d inner=%s" % (kern, d, inner)))
        assert kr.krylov_inner()[0] == "f64"                                      # (the mode of one call does not stay)
        assert not np.array_equal(C, kr.predict_covariance(T))
    finally:
        kr.destroy()
    return worst


def check_widths(KM, lib, path, kern="gauss", d=8, lam=4.0):
    """a fit with widths = w: the covariance is that of the plain fit on X / w at T / w within both calls' bounds (the covariance
    needs no scaling back), and that one is within the bound of its reference"""
    X, y, T = GP.model_data(d)
    T = T[-M_COV:]
    ktype, p = GP.KINDS[kern]
    h = width(ktype, d)
    w = np.linspace(0.5, 2.0, d)
    a = KM.KernelRegression(lib, h=h, lam=lam, kernel=GP.KERNEL_NAMES[kern], argv=GP.FIT_ARGS, keep_model=True, widths=w).fit(X, y)
    b = KM.KernelRegression(lib, h=h, lam=lam, kernel=GP.KERNEL_NAMES[kern], argv=GP.FIT_ARGS, keep_model=True).fit(X / w, y)
    try:
        Ca, Cb = a.predict_covariance(T), b.predict_covariance(T / w)
        Hd, sv, _ = GP.dense_model(b, path)
        Cref, bound, bq = covariance_reference(Hd, sv, b.model_points(), T / w, (ktype, p, h))
        check_covariance(Cb, Cref, bound, bq, "widths %s R^%d" % (kern, d))
        assert np.all(np.abs(Ca - Cb) <= 2.0 * bound)
    finally:
        a.destroy()
        b.destroy()


def check_set_lambda(KM, lib, path, kern="gauss", d=8, lam1=4.0, lam2=1.5, hscale=1.0):
    """after set_lambda the covariance follows the new factorisation: checked against the rewritten Hd"""
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam1, hscale)
    T = np.ascontiguousarray(T[-M_COV:])
    try:
        C1 = kr.predict_covariance(T)
        Hd1, _, _ = GP.dense_model(kr, path)
        kr.set_lambda(lam2)
        Hd2, sv2, _ = GP.dense_model(kr, path)
        assert np.array_equal(Hd2, Hd1 + (lam2 - lam1) * np.eye(len(Hd1)))
        C2 = kr.predict_covariance(T)
        Cref, bound, bq = covariance_reference(Hd2, sv2, kr.model_points(), T, kind)
        check_covariance(C2, Cref, bound, bq, "%s R^%d lambda %g -> %g" % (kern, d, lam1, lam2))
        assert np.abs(C1 - Cref).max() > bound.max()                      # (the old covariance is another matrix)
    finally:
        kr.destroy()


def check_sample_posterior(KM, lib, kern="gauss", d=8, lam=4.0, m=M_COV, nsamples=5):
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam)
    T = np.ascontiguousarray(T[-m:])
    try:
        got = kr.sample_posterior(T, nsamples, seed=7)
        assert got.shape == (nsamples, m)
        Z = np.random.Generator(np.random.Philox(7)).standard_normal((nsamples, m))
        ref = kr.decision_function(T) + Z @ np.linalg.cholesky(kr.predict_covariance(T)).T
        assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref).max()), float(np.abs(got - ref).max())
        assert np.array_equal(got, kr.sample_posterior(T, nsamples, seed=7)), "the same seed gave other draws"
        assert not np.array_equal(got, kr.sample_posterior(T, nsamples, seed=8))
        ge = kr.sample_posterior(T, 2, seed=7, exact=True, jitter=1e-9, rtol=1e-9)
        assert ge.shape == (2, m) and np.all(np.isfinite(ge))
        # k(t, t) = 1 and no variance above 1 by more than its bound: C - I is negative semidefinite up to rounding
        try:
            kr.sample_posterior(T, nsamples, jitter=-1.0)
        except ValueError as e:
            assert "eigenvalue" in str(e) and "exact=True" in str(e) and "jitter" in str(e), str(e)
        else:
            raise AssertionError("jitter = -1 did not raise")
    finally:
        kr.destroy()


def check_refusals(KM, lib):
    """no kept model, an ANOVA fit, a float handle, a handle before its fit, a wrong test dimension, bad arguments: each refuses
    with the outputs untouched (the C++ members: tests/cpp/test_gpcov_kernel.cpp)"""
    n, d, m = 300, 8, 5
    X, y, T = GP.model_data(d, n, m)
    T = np.ascontiguousarray(T)
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]

    def raw(Kh):
        """[(name, return code, outputs untouched)] of the three C calls"""
        res = []
        c = np.full((m, m), S)
        res.append(("covariance", lib.SPX_kernel_predict_covariance_double(Kh, m, T.ctypes.data, c.ctypes.data, m), bool(np.all(c == S))))
        c = np.full((m, m), S)
        res.append(("exact", lib.SPX_kernel_predict_covariance_exact_double(Kh, m, T.ctypes.data, c.ctypes.data, m, 1e-8, 100, 30, None),
                    bool(np.all(c == S))))
        ms = np.full(3, S)
        res.append(("ms", lib.SPX_kernel_covariance_ms(Kh, ms.ctypes.data), bool(np.all(ms == S))))
        return res

    def raises(f):
        try:
            f()
        except (RuntimeError, ValueError):
            return True
        return False
    kf = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X.astype(np.float32), y.astype(np.float32))
    for name, rc, untouched in raw(kf.K):
        assert rc != 0 and untouched, ("float handle", name, rc)
    assert raises(lambda: kf.predict_covariance(T)) and raises(lambda: kf.sample_posterior(T, 2))
    kf.destroy()
    ka = KM.KernelRegression(lib, h=h, lam=4.0, kernel="ANOVA", degree=2, argv=args, keep_model=True).fit(X, y)
    for name, rc, untouched in raw(ka.K):
        assert rc != 0 and untouched, ("ANOVA", name, rc)
    assert raises(lambda: ka.predict_covariance(T)) and raises(lambda: ka.predict_covariance(T, exact=True)) and raises(ka.covariance_ms)
    ka.destroy()
    kp = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y)           # no kept model
    for name, rc, untouched in raw(kp.K):
        assert rc != 0 and untouched, ("no kept model", name, rc)
    assert raises(lambda: kp.predict_covariance(T)) and raises(lambda: kp.predict_covariance(T, exact=True))
    kp.destroy()
    Xc = np.ascontiguousarray(X)
    Kh = lib.STRUMPACK_create_kernel_double(n, d, Xc.ctypes.data, h, 4.0, 1, 0)
    assert Kh and lib.SPX_kernel_keep_model(Kh, 1) == 0
    for name, rc, untouched in raw(Kh):
        assert rc != 0 and untouched, ("before the fit", name, rc)
    lib.STRUMPACK_destroy_kernel_double(Kh)
    kk = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    c = np.full((m, m), S)
    for rtol, maxit, restart in ((0.0, 100, 30), (float("nan"), 100, 30), (1e-8, 0, 30), (1e-8, 100, 0)):
        assert lib.SPX_kernel_predict_covariance_exact_double(kk.K, m, T.ctypes.data, c.ctypes.data, m, rtol, maxit, restart, None) != 0
    assert lib.SPX_kernel_predict_covariance_double(kk.K, -1, T.ctypes.data, c.ctypes.data, m) != 0
    assert lib.SPX_kernel_predict_covariance_double(kk.K, m, None, c.ctypes.data, m) != 0
    assert lib.SPX_kernel_predict_covariance_double(kk.K, m, T.ctypes.data, None, m) != 0
    assert lib.SPX_kernel_predict_covariance_double(kk.K, m, T.ctypes.data, c.ctypes.data, m - 1) != 0          # ldc < m
    assert np.all(c == S)
    assert raises(lambda: kk.predict_covariance(T[:, :d - 1])) and raises(lambda: kk.predict_covariance(np.zeros((m, d + 1))))
    assert raises(lambda: kk.predict_covariance(T, exact=True, rtol=0.0))
    # a padded output: ldc = m + 2, the rows from m on untouched
    cp = np.full((m, m + 2), S)                                                  # (column-major m + 2 x m, seen transposed)
    assert lib.SPX_kernel_predict_covariance_double(kk.K, m, T.ctypes.data, cp.ctypes.data, m + 2) == 0
    assert np.all(cp[:, m:] == S) and np.array_equal(cp[:, :m].T, kk.predict_covariance(T))
    ms = np.zeros(3)
    assert lib.SPX_kernel_covariance_ms(kk.K, ms.ctypes.data) == 0 and lib.SPX_kernel_covariance_ms(kk.K, None) != 0
    kk.destroy()
