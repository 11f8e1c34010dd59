"""Checks of the log-determinant of a factored HSS matrix (hssk_logabsdet_vbatched, DeviceHSS::logabsdet,
SPX_d_struct_logabsdet), shared by the CPU emulator tests (tests/test_gp_emu.py) and the GPU tests (tests/test_gp_gpu.py).

The oracle is independent of every kernel: the generators the matrix itself writes (HSSMatrix::write), read back and expanded
with numpy (tests/hss_generators.py: read(path).dense()).  That is the compressed matrix exactly, whatever the compression
tolerance, so numpy.linalg.slogdet of it is what the ULV factors must reproduce to rounding.

Tolerance of the log-determinant.  The ULV factors are those of H + dH with ||dH|| / ||H|| <= eps_f, eps_f = 1e-12 being the
constant the project accepts for the forward error of the ULV solve (hss_cases.check_against_generators: fe <= 1e-12 cond).
To first order log|det(H + dH)| - log|det H| = tr(H^-1 dH), and |tr(H^-1 dH)| <= n ||H^-1|| ||dH|| <= n cond_2(H) eps_f.
Hence   |got - slogdet(Hd)[1]| <= 1e-12 n cond_2(Hd),   cond_2 from the singular values of Hd in the test.

Tolerance of the partial sums of hssk_logabsdet_vbatched.  A partial is a sum of n logarithms, each within one unit in the last
place (2^-52 relative), added in some fixed order: (n - 1) 2^-53 relative to the sum of the magnitudes.  The diagonals of the test
are in [2, 10], all logarithms positive, so against a reference computed in long double the error is at most n 2^-52 relative to
the partial itself.  The total is the partials added in index order: that is an exact statement about IEEE additions and is
checked bit for bit.

The kept model of kernel ridge regression (Kernel<double>::keep_model).  Hd is again the dense form of the matrix the handle
writes (SPX_kernel_model_write), X the handle's cluster-ordered points, kt = k(X, t_c) from kernel_cases.kernel_ref in long
double with its entry bounds b (kernel_cases.kernel_entry_bound, lambda = 0), z = Hd^-1 kt by numpy, and the reference variance
    ref_c = k(t_c, t_c) - kt_c^T z_c.
The library computes kt^ = kt + e with |e_r| <= b_r, solves z^ = Hd^-1 kt^ + delta with ||delta|| <= 1e-12 cond_2(Hd) ||z|| (the
forward error the project accepts for the ULV solve) and adds z^_r kt^_r over r.  To first order
    kt^^T z^ - kt^T z = kt^T delta + e^T z + kt^T Hd^-1 e,
    |kt^T delta|    <= 1e-12 cond_2(Hd) ||kt_c|| ||z_c||                                      (forward-error term)
    |e^T z|         <= sum_r |z_rc| b_rc
    |kt^T Hd^-1 e|  <= sum_r |z_rc| b_rc for a symmetric Hd, <= ||Hd^-1||_2 ||kt_c|| ||b_c|| in general
so that   bound_c = 1e-12 cond_2 ||kt_c|| ||z_c|| + 2 sum_r |z_rc| b_rc + ||Hd^-1||_2 ||kt_c|| ||b_c||.
(The rounding of the n-term sum, n 2^-53 sum_r |z_r k_r| <= n 2^-53 ||z|| ||kt||, is below the forward-error term: n 2^-53 < 1e-12.)
A case only proves something while this bound is small against the variances themselves: every case asserts
bound <= 1e-3 min_c ref_c.

Log marginal likelihood: -1/2 y^T alpha - 1/2 log|det Hd| - n/2 log(2 pi) with the handle's labels and weights; the tolerance is
half the log-determinant's plus 1e-12 cond_2 |y^T alpha|."""
import ctypes
import os

import numpy as np

import hss_cases as HC
import hss_generators as G
import kernel_cases as KC
from oracle import hss_oracle as O
from strumpack_amd import capi
from strumpack_amd import hssk as K

EPS_F = 1e-12          # forward-error constant of the ULV solve (hss_cases.py, check_against_generators)
SCALE = 3.7            # no triangle has a diagonal near 1: a node left out of the sum shows


# ---- hssk_logabsdet_vbatched on its own ----------------------------------------------------------------------------------------
def check_logabsdet_kernel(hk, sizes=(1, 63, 64, 65, 300), seed=3):
    """random upper triangles with lda > n: every partial against numpy, the total bit for bit the partials added in index order,
    two calls bit-identical, count = 0 gives 0.0, a zero pivot gives -inf"""
    rng = np.random.default_rng(seed)
    blocks, refs, worst = [], [], 0.0
    for k, n in enumerate(sizes):
        lda = n + 1 + (k % 3)
        A = np.asfortranarray(np.triu(rng.standard_normal((lda, n))))
        dg = rng.uniform(2.0, 10.0, n) * rng.choice([-1.0, 1.0], n)
        A[np.arange(n), np.arange(n)] = dg
        A[n:, :] = 1e300                       # (rows past the triangle are never read)
        blocks.append((hk.array(A), n, lda))
        refs.append(float(np.sum(np.log(np.abs(dg).astype(np.longdouble)))))
    part, total = hk.logabsdet(blocks)
    for n, got, ref in zip(sizes, part, refs):
        err = abs(got - ref) / abs(ref)
        worst = max(worst, err / (n * 2.0 ** -52))
        print("logabsdet kernel: n = %d partial %.17g reference %.17g relative error %.3g (bound %.3g)" % (n, got, ref, err, n * 2.0 ** -52))
        assert err <= n * 2.0 ** -52, (n, got, ref)
    s = 0.0
    for v in part:
        s += float(v)
    assert total == s, (total, s)
    part2, total2 = hk.logabsdet(blocks)
    assert np.array_equal(part, part2) and total == total2
    # count = 0
    p0, t0 = hk.logabsdet([])
    assert len(p0) == 0 and t0 == 0.0 and not np.signbit(t0)
    # IEEE values: a zero pivot is -inf, for the partial and for the total
    Z = np.asfortranarray(np.diag([3.0, 0.0, 5.0]))
    dz = hk.array(Z)
    pz, tz = hk.logabsdet([blocks[2], (dz, 3, 3), blocks[0]])
    assert pz[1] == -np.inf and tz == -np.inf and pz[0] == part[2] and pz[2] == part[0]
    for a, _, _ in blocks:
        a.free()
    dz.free()
    return worst


# ---- the structured API ---------------------------------------------------------------------------------------------------------
def tree_of(info):
    """(children, height) per node from the pre-order table of SPX_d_struct_node_info (6 ints: offset, rows, U rows, U rank, V rank,
    leaf)"""
    nn = len(info)
    kids, height = [None] * nn, [0] * nn

    def walk(i):
        if info[i][5]:
            return i + 1
        c0 = i + 1
        c1 = walk(c0)
        end = walk(c1)
        kids[i] = (c0, c1)
        height[i] = 1 + max(height[c0], height[c1])
        return end
    assert walk(0) == nn
    return kids, height


def logdet_operand(kind, n):
    if kind == "toeplitz":
        return np.asfortranarray(SCALE * O.toeplitz(n))
    if kind == "unsym":
        return np.asfortranarray(SCALE * HC.toeplitz_unsym(n))
    if kind == "full_rank":
        # nothing to compress: every off-diagonal block has full rank, the nodes below the root keep all their rows (m == r)
        rng = np.random.default_rng(41)
        return np.asfortranarray(rng.standard_normal((n, n)) + SCALE * np.sqrt(n) * np.eye(n))
    raise ValueError(kind)


def reference_logdet(H, path):
    """(log|det|, sign, n cond_2 1e-12, dense form) of the compressed matrix from its own generators (a shift is part of them:
    it has been added to the leaves' diagonal blocks)"""
    H.write(path)
    Hd = G.read(path).dense()
    os.remove(path)
    sv = np.linalg.svd(Hd, compute_uv=False)
    sign, ld = np.linalg.slogdet(Hd)
    return ld, sign, EPS_F * Hd.shape[0] * (sv[0] / sv[-1]), Hd


def raw_logabsdet(L, H, sentinel=123.25):
    """the C call itself: (return code, *out) with *out pre-filled"""
    out = ctypes.c_double(sentinel)
    rc = L.SPX_d_struct_logabsdet(H.h, ctypes.byref(out))
    return rc, out.value


# name: (n, leaf size).  The tree halves a node while it has more rows than the leaf size, so it is balanced unless the two halves of
# some node straddle the leaf size (65 -> 32 | 33 at leaf size 32), and a leaf has at most `leaf size` rows: n = 200 at leaf size
# 64 has three levels, n = 1100 at 32 is balanced, n = 900 at 300 has 225-row leaves.  Two levels, siblings of different height
# and leaves above 256 rows therefore have cases of their own (n = 100, 1040, 600) whose node tables show them.
STRUCTURES = {
    "single_node": (40, 64),                       # the root's LU only
    "two_levels": (100, 64),                       # root + two leaves
    "three_levels": (200, 64),                     # leaves, one inner level below the root, root
    "fused_inner_levels": (700, 32),               # check_ulv_node's shape: inner levels through hssk_ulv_node_vbatched
    "seven_levels": (1100, 32),
    "siblings_of_different_height": (1040, 32),    # 65 -> 32 | 33: the 33-row half splits again
    "leaves_of_225_rows": (900, 300),              # the split kernel at its largest tile variant (m in (208, 256])
    "leaves_above_256_rows": (600, 300),           # 300-row leaves: row gathers + product + blocked QR
    "nothing_to_eliminate": (64, 16),              # m == r at every node below the root
}


LOGDET_CASES = ["single_node", "two_levels", "three_levels", "fused_inner_levels", "seven_levels", "siblings_of_different_height",
                "leaves_of_225_rows", "leaves_above_256_rows"]


def check_logdet(L, name, kind, path, shifts=()):
    """One matrix: the structure the case is there for (from node_info and the launch counters), logabsdet against
    slogdet of the generators under 1e-12 n cond_2, two calls bit-identical.  shifts: each is applied on top (shift + factor), with
    the error return checked in between.  Returns the worst error / bound ratio."""
    n, leaf = STRUCTURES[name]
    A = logdet_operand("full_rank" if name == "nothing_to_eliminate" else kind, n)
    c = dict(rel_tol=1e-6, abs_tol=1e-12, leaf_size=leaf, d0=32, dd=16, algorithm="stable")
    H = HC.build(L, A, c)
    assert H.is_compressed()
    info = H.node_info()
    kids, height = tree_of(info)
    inner = [i for i in range(len(info)) if kids[i]]
    leaf_rows = sorted(set(int(info[i][1]) for i in range(len(info)) if info[i][5]))
    if name == "single_node":
        assert len(info) == 1 and info[0][5] == 1
    elif name == "two_levels":
        assert H.levels() == 2 and len(info) == 3
    elif name == "three_levels":
        assert H.levels() == 3 and len(info) == 7
    elif name == "fused_inner_levels":
        assert H.levels() >= 4
    elif name == "seven_levels":
        assert H.levels() == 7 and len(info) == 127
    elif name == "siblings_of_different_height":
        assert any(height[kids[i][0]] != height[kids[i][1]] for i in inner), height
    elif name == "leaves_of_225_rows":
        assert leaf_rows == [225], leaf_rows
    elif name == "leaves_above_256_rows":
        assert leaf_rows == [300], leaf_rows
    elif name == "nothing_to_eliminate":
        assert len(info) > 1 and all(info[i][2] == info[i][3] and info[i][2] > 0 for i in range(1, len(info))), info
    # before factor(): the error, *out untouched
    rc, v = raw_logabsdet(L, H)
    assert rc != 0 and v == 123.25
    c0 = HC.sweep_counters(L)
    H.factor()
    d = HC._delta(L, c0)
    if name in ("fused_inner_levels", "seven_levels", "siblings_of_different_height"):
        assert d["ulv_node_launches"] > 0 or HC.env_flag("NO_ULV_NODE"), d
    if name not in ("single_node", "nothing_to_eliminate"):
        assert any(info[i][2] > info[i][3] for i in range(1, len(info)))      # some node eliminates
    worst, sigma = 0.0, 0.0
    for step in (None,) + tuple(shifts):
        if step is not None:
            H.shift(step)
            sigma += step
            rc, v = raw_logabsdet(L, H)                 # the shift invalidated the factors
            assert rc != 0 and v == 123.25, (rc, v)
            H.factor()
        ref, sign, bound, Hd = reference_logdet(H, path)
        got = H.logabsdet()
        again = H.logabsdet()
        assert got == again, (got, again)
        rc, v = raw_logabsdet(L, H)
        assert rc == 0 and v == got
        ratio = abs(got - ref) / bound
        worst = max(worst, ratio)
        print("logabsdet %s/%s n = %d shift %+.2f: got %.15g reference %.15g (sign %+d) |error| %.3g bound %.3g"
              % (name, kind, n, sigma, got, ref, int(sign), abs(got - ref), bound))
        assert abs(got - ref) <= bound, (name, kind, sigma, got, ref, bound)
        if step is not None and step <= -5.0:
            # the matrix is indefinite here: only the absolute value of the determinant is what the triangles carry
            ev = np.linalg.eigvals(Hd).real
            assert (ev < 0).any() and (ev > 0).any()
    H.destroy()
    return worst


def check_logdet_errors(L):
    """the calls that must refuse, with *out untouched: a partial factorization, a BLR matrix; and factor() after either makes
    the call work again"""
    n = 200
    A = logdet_operand("toeplitz", n)
    c = dict(rel_tol=1e-6, abs_tol=1e-12, leaf_size=32, d0=32, dd=16, algorithm="stable")
    H = HC.build(L, A, c)
    H.partial_factor()
    rc, v = raw_logabsdet(L, H)
    assert rc != 0 and v == 123.25
    try:
        H.logabsdet()
        raise AssertionError("logabsdet accepted the factors of partial_factor")
    except RuntimeError:
        pass
    H.factor()
    rc, v = raw_logabsdet(L, H)
    assert rc == 0 and np.isfinite(v) and v != 123.25
    H.destroy()
    o = capi.StructuredMatrix.options(L, rel_tol=1e-6, abs_tol=1e-12, leaf_size=32, type=capi.SP_TYPE_BLR)
    B = capi.StructuredMatrix.from_dense_and_factor(L, A, o)
    rc, v = raw_logabsdet(L, B)
    assert rc != 0 and v == 123.25
    B.destroy()


# ---- hssk_kernel_cross / hssk_kernel_predict_cols on their own ------------------------------------------------------------------
# (n, m, d): three training tiles of 64, the last one of two points, against chunks of 64, 64 and 2 test points; one coordinate, the
# largest dimension whose points stay whole in the LDS, the first that passes in chunks of 32, and a ragged last chunk
CROSS_SHAPES = ((130, 130, 1), (130, 130, 8), (130, 65, 64), (130, 65, 65), (70, 130, 70))
KINDS = {"gauss": (0, 1), "laplace": (1, 1), "anova": (2, 2)}


def check_cross_and_cols(hk, n, m, d, seed=7):
    """both kernels against kernel_ref in long double: every entry of the cross block under kernel_entry_bound (lambda = 0), the
    rows n .. ldo - 1 of the pre-filled output back bit for bit; the column sums under sum_r |W_rc| b_rc + n 2^-53 sum_r |W_rc k_rc|;
    and the column sums of hssk_kernel_predict_cols with every column equal to w are bit for bit those of hssk_kernel_predict (the
    same pairs in the same order)"""
    rng = np.random.default_rng(seed + d)
    X, T = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    T[-2:] = X[[3, n - 1]]                                   # the last two test points are training points
    W, w = rng.standard_normal((n, m)), rng.standard_normal(n)
    Z = np.vstack([X, T])
    dX, dT = hk.array(X.T), hk.array(T.T)
    ldo, ldw = n + 3, n + 5
    worst = 0.0
    for name, (ktype, p) in KINDS.items():
        if ktype == 2 and p > d:
            continue
        h = float(KC.kernel_widths(d)[ktype])
        spec = K.KernelSpec(dX.ptr, n, d, ktype, p, h, 2.0)      # (a lambda in the spec must not reach the block)
        fill = np.full((ldo, m + 1), KC.SENTINEL)
        dO = hk.array(fill)
        hk.check(hk.lib.hssk_kernel_cross(hk.ctx, ctypes.byref(spec), dT.ptr, m, dO.ptr, ldo))
        hk.sync()
        got = dO.get()
        assert np.all(got[n:, :] == KC.SENTINEL) and np.all(got[:, m] == KC.SENTINEL), "hssk_kernel_cross wrote outside its block"
        k, a, A = KC.kernel_ref(Z, np.arange(n), n + np.arange(m), ktype, h, 0.0, p)
        b = KC.kernel_entry_bound(a, A, ktype, d, 0.0, p)
        err = np.abs(got[:n, :m].astype(np.longdouble) - k)
        frac = float((err / b).max())
        print("kernel_cross %s n=%d m=%d d=%d: largest error / bound %.3f" % (name, n, m, d, frac))
        assert np.all(err <= b), (name, n, m, d, frac)
        Wp = np.full((ldw, m), 1e300)
        Wp[:n] = W
        dW, dP = hk.array(Wp), hk.array(np.full((m + 2,), KC.SENTINEL))
        hk.check(hk.lib.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(spec), dW.ptr, ldw, dT.ptr, m, dP.ptr))
        hk.sync()
        pc = dP.get()
        assert np.all(pc[m:] == KC.SENTINEL)
        aW = np.abs(W).astype(np.longdouble)
        ref = (W.astype(np.longdouble) * k).sum(0)
        bound = (aW * b).sum(0) + n * KC.U53 * (aW * np.abs(k)).sum(0)
        errc = np.abs(pc[:m].astype(np.longdouble) - ref)
        fracc = float((errc / bound).max())
        print("kernel_predict_cols %s n=%d m=%d d=%d: largest error / bound %.3f" % (name, n, m, d, fracc))
        assert np.all(errc <= bound), (name, n, m, d, fracc)
        # one weight vector in every column: the prediction sum itself
        dW.set(np.vstack([np.tile(w[:, None], (1, m)), np.full((ldw - n, m), 1e300)]))
        dw, dQ = hk.array(w), hk.array(np.zeros(m))
        hk.check(hk.lib.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(spec), dW.ptr, ldw, dT.ptr, m, dP.ptr))
        hk.check(hk.lib.hssk_kernel_predict(hk.ctx, ctypes.byref(spec), dw.ptr, dT.ptr, m, dQ.ptr))
        hk.sync()
        assert np.array_equal(dP.get()[:m], dQ.get()), name
        worst = max(worst, frac, fracc)
        for v in (dO, dW, dP, dw, dQ):
            v.free()
    # nothing to do, and the refusals
    spec = K.KernelSpec(dX.ptr, n, d, 0, 1, 1.0, 0.0)
    assert hk.lib.hssk_kernel_cross(hk.ctx, ctypes.byref(spec), dT.ptr, 0, None, n) == 0
    assert hk.lib.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(spec), None, n, dT.ptr, 0, None) == 0
    dO = hk.empty((n, m))
    assert hk.lib.hssk_kernel_cross(hk.ctx, ctypes.byref(spec), dT.ptr, m, dO.ptr, n - 1) != 0       # ldo < n
    assert hk.lib.hssk_kernel_predict_cols(hk.ctx, ctypes.byref(spec), dO.ptr, n - 1, dT.ptr, m, dO.ptr) != 0
    bad = K.KernelSpec(dX.ptr, n, d, 2, 9, 1.0, 0.0)
    assert hk.lib.hssk_kernel_cross(hk.ctx, ctypes.byref(bad), dT.ptr, m, dO.ptr, n) != 0            # ANOVA degree above 8
    for v in (dX, dT, dO):
        v.free()
    return worst


# ---- the kept model ------------------------------------------------------------------------------------------------------------
N_MODEL, M_TEST = 700, 130
FIT_ARGS = ["--hss_leaf_size", "128"]
KERNEL_NAMES = {"gauss": "rbf", "laplace": "Laplace", "anova": "ANOVA"}
# (kernel, d, lambda, factor on the width of kernel_cases.kernel_widths): Gauss and Laplace in R^1, R^8 and R^70, ANOVA of degree 2
# in R^8, each at two values of lambda -- 4 and 0.05 at the plain width wherever the case then proves something (module docstring:
# bound <= 1e-3 of the smallest reference variance).  The fit runs at the default compression tolerance (1e-2), and where the
# kernel matrix is large against lambda the matrix that comes out of it is no longer positive definite next to the test points:
# its reference variances are negative (Gauss R^1: -0.35 at lambda = 0.05, -0.0097 at 4; Gauss R^8 at 0.05: -0.40; ANOVA: -4.1 and
# -0.38).  Those cases take a narrower kernel and / or a larger lambda, chosen from the reference side alone (numpy on the
# written matrix): smallest reference variance 0.030 / 0.039 (Gauss R^1), 0.024 (Gauss R^8), 0.82 / 0.37 (ANOVA).
MODEL_CASES = ([("gauss", 1, 4.0, 0.25), ("gauss", 1, 16.0, 1.0), ("gauss", 8, 4.0, 1.0), ("gauss", 8, 0.05, 0.5),
                ("gauss", 70, 4.0, 1.0), ("gauss", 70, 0.05, 1.0)]
               + [("laplace", d, lam, 1.0) for d in (1, 8, 70) for lam in (4.0, 0.05)]
               + [("anova", 8, 4.0, 0.25), ("anova", 8, 16.0, 0.5)])


def model_data(d, n=N_MODEL, m=M_TEST, seed=17):
    rng = np.random.default_rng(seed + d)
    X = rng.standard_normal((n, d))
    y = np.where(X[:, 0] + 0.3 * rng.standard_normal(n) > 0, 1.0, -1.0)
    T = rng.standard_normal((m, d))
    T[-2:] = X[[5, n - 7]]                                    # the last two test points are training points
    return X, y, T


def fit_model(KM, lib, kern, d, lam, hscale=1.0, keep=True, n=N_MODEL):
    X, y, T = model_data(d, n)
    ktype, p = KINDS[kern]
    h = float(KC.kernel_widths(d)[ktype]) * hscale
    kr = KM.KernelRegression(lib, h=h, lam=lam, kernel=KERNEL_NAMES[kern], degree=p, argv=FIT_ARGS, keep_model=keep).fit(X, y)
    return kr, T, (ktype, p, h)


def dense_model(kr, path):
    """Hd, its singular values and its generators from the file the handle writes"""
    kr.write_model(path)
    R = G.read(path)
    os.remove(path)
    Hd = R.dense()
    return Hd, np.linalg.svd(Hd, compute_uv=False), R


def variance_reference(kr, Hd, sv, T, kind):
    """(reference variances, bounds) of the module docstring for the test points T"""
    ktype, p, h = kind
    X = kr.model_points()
    n, d = X.shape
    m = T.shape[0]
    Z = np.vstack([X, T])
    kt, a, A = KC.kernel_ref(Z, np.arange(n), n + np.arange(m), ktype, h, 0.0, p)
    b = np.asarray(KC.kernel_entry_bound(a, A, ktype, d, 0.0, p), dtype=np.float64)
    ktt = np.array([KC.kernel_ref(T[c:c + 1], [0], [0], ktype, h, 0.0, p)[0][0, 0] for c in range(m)], dtype=np.float64)
    kt = np.asarray(kt, dtype=np.float64)
    z = np.linalg.solve(Hd, kt)
    ref = ktt - (kt * z).sum(0)
    cond, inv = sv[0] / sv[-1], 1.0 / sv[-1]
    nk, nz, nb = np.linalg.norm(kt, axis=0), np.linalg.norm(z, axis=0), np.linalg.norm(b, axis=0)
    bound = EPS_F * cond * nk * nz + 2.0 * (np.abs(z) * b).sum(0) + inv * nk * nb
    return ref, bound


def check_variance(kr, Hd, sv, T, kind, tag):
    ref, bound = variance_reference(kr, Hd, sv, T, kind)
    got = kr.predict_variance(T)
    err = np.abs(got - ref)
    ratio = float((err / bound).max())
    print("variance %s m=%d: variances in [%.3g, %.3g], largest bound %.3g, largest error %.3g, largest error / bound %.3g"
          % (tag, len(T), ref.min(), ref.max(), bound.max(), err.max(), ratio))
    assert bound.max() <= 1e-3 * ref.min(), (tag, bound.max(), ref.min())        # the case proves something
    assert np.all(err <= bound), (tag, ratio)
    assert np.array_equal(got, kr.predict_variance(T)), "two variance calls differ"
    return ratio


def check_logdet_and_lml(kr, Hd, sv, tag):
    n = Hd.shape[0]
    cond = sv[0] / sv[-1]
    sign, ld = np.linalg.slogdet(Hd)
    tol = EPS_F * n * cond
    got = kr.logabsdet()
    print("model %s: logabsdet %.15g reference %.15g |error| %.3g bound %.3g (cond %.3g)" % (tag, got, ld, abs(got - ld), tol, cond))
    assert abs(got - ld) <= tol, (tag, got, ld, tol)
    assert got == kr.logabsdet()
    y, w = kr.model_labels().astype(np.longdouble), kr.weights().astype(np.longdouble)
    ya = float((y * w).sum())
    ref = -0.5 * ya - 0.5 * ld - 0.5 * n * np.log(2.0 * np.pi)
    tol_l = 0.5 * tol + EPS_F * cond * abs(ya)
    lml = kr.log_marginal_likelihood()
    print("model %s: log marginal likelihood %.15g reference %.15g |error| %.3g bound %.3g" % (tag, lml, ref, abs(lml - ref), tol_l))
    assert abs(lml - ref) <= tol_l, (tag, lml, ref, tol_l)
    return max(abs(got - ld) / tol, abs(lml - ref) / tol_l)


def check_model(KM, lib, kern, d, lam, hscale, path, extra_m=()):
    """one fit with keep_model: log-determinant, log marginal likelihood and the variance of the 130 test points (chunks of 64, 64
    and 2) against the dense form of the kept matrix; extra_m: further test point counts on the same fit"""
    kr, T, kind = fit_model(KM, lib, kern, d, lam, hscale)
    tag = "%s R^%d lambda=%g h=%.3g" % (kern, d, lam, kind[2])
    try:
        Hd, sv, _ = dense_model(kr, path)
        worst = check_logdet_and_lml(kr, Hd, sv, tag)
        worst = max(worst, check_variance(kr, Hd, sv, T, kind, tag))
        for m in extra_m:
            worst = max(worst, check_variance(kr, Hd, sv, T[-m:], kind, tag))
    finally:
        kr.destroy()
    return worst


def check_set_lambda(KM, lib, kern, d, lam1, lam2, hscale, path):
    """a fit at lam1, then set_lambda(lam2): the written matrix is Hd1 + (lam2 - lam1) I with the ranks unchanged, the new weights
    solve it to the project's backward error, logabsdet / likelihood / variance follow it under their bounds, and predict uses
    the new weights.  Recorded, not asserted: the distance of the weights from a fresh fit at lam2."""
    kr, T, kind = fit_model(KM, lib, kern, d, lam1, hscale)
    tag = "%s R^%d lambda %g -> %g" % (kern, d, lam1, lam2)
    try:
        Hd1, _, R1 = dense_model(kr, path)
        w1, p1 = kr.weights(), kr.decision_function(T)
        kr.set_lambda(lam2)
        Hd2, sv2, R2 = dense_model(kr, path)
        assert [(a.rU, a.rV) for a in R1.nodes] == [(a.rU, a.rV) for a in R2.nodes]
        assert np.array_equal(Hd2, Hd1 + (lam2 - lam1) * np.eye(len(Hd1)))
        y, w2 = kr.model_labels(), kr.weights()
        F = np.linalg.norm
        e = F(Hd2 @ w2 - y) / (sv2[0] * F(w2) + F(y))
        print("set_lambda %s: backward error of the new weights %.3g" % (tag, e))
        assert e <= HC.GEN_TOL, (tag, e)
        assert not np.array_equal(w1, w2)
        check_logdet_and_lml(kr, Hd2, sv2, tag)
        check_variance(kr, Hd2, sv2, T, kind, tag)
        # predict with the new weights: the long double sum under the bound of kernel_cases.case_kernel_predict
        ktype, p, h = kind
        X = kr.model_points()
        n = len(X)
        k, a, A = KC.kernel_ref(np.vstack([X, T]), np.arange(n), n + np.arange(len(T)), ktype, h, 0.0, p)
        aw = np.abs(w2).astype(np.longdouble)
        ref = w2.astype(np.longdouble) @ k
        bound = aw @ KC.kernel_entry_bound(a, A, ktype, d, 0.0, p) + n * KC.U53 * (aw @ np.abs(k))
        p2 = kr.decision_function(T)
        assert np.all(np.abs(p2.astype(np.longdouble) - ref) <= bound) and not np.array_equal(p1, p2)
    finally:
        kr.destroy()
    fresh, _, _ = fit_model(KM, lib, kern, d, lam2, hscale, keep=False)
    wf = fresh.weights()
    fresh.destroy()
    print("set_lambda %s: ||w - w_fresh|| / ||w_fresh|| = %.3g (not asserted: two compressions of two matrices)" % (tag, F(w2 - wf) / F(wf)))


def model_calls(lib, Kh, T, path):
    """every model call on the raw handle: [(name, return code, output untouched)]"""
    out, res = ctypes.c_double(123.25), []
    res.append(("logabsdet", lib.SPX_kernel_logabsdet(Kh, ctypes.byref(out)), out.value == 123.25))
    res.append(("log_marginal_likelihood", lib.SPX_kernel_log_marginal_likelihood(Kh, ctypes.byref(out)), out.value == 123.25))
    var = np.full(len(T), 123.25)
    res.append(("predict_variance", lib.SPX_kernel_predict_variance_double(Kh, len(T), T.ctypes.data, var.ctypes.data), bool(np.all(var == 123.25))))
    res.append(("model_set_lambda", lib.SPX_kernel_model_set_lambda(Kh, 1.0), True))
    res.append(("model_write", lib.SPX_kernel_model_write(Kh, str(path).encode()), not os.path.exists(path)))
    return res


def check_model_lifecycle(KM, lib, path):
    """the refusals (no keep_model, a float handle, before the first fit), a second fit, keep_model(false), destroy with a live
    model, and: keeping the model changes nothing in what the fit returns"""
    n, d = 300, 8
    X, y, T = model_data(d, n, 20)
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]
    plain = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y)
    for name, rc, untouched in model_calls(lib, plain.K, T, path):
        assert rc != 0 and untouched, ("no keep_model", name, rc)
    wp, pp = plain.weights(), plain.decision_function(T)
    # a float handle: keep_model itself refuses, and so does every call
    kf = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X.astype(np.float32), y.astype(np.float32))
    assert lib.SPX_kernel_keep_model(kf.K, 1) != 0
    for name, rc, untouched in model_calls(lib, kf.K, T, path):
        assert rc != 0 and untouched, ("float handle", name, rc)
    kf.destroy()
    # before the first fit
    Xc = np.ascontiguousarray(X)
    Kh = lib.STRUMPACK_create_kernel_double(n, d, Xc.ctypes.data, h, 4.0, 1, 0)
    assert Kh and lib.SPX_kernel_keep_model(Kh, 1) == 0
    for name, rc, untouched in model_calls(lib, Kh, T, path):
        assert rc != 0 and untouched, ("before the fit", name, rc)
    lib.STRUMPACK_destroy_kernel_double(Kh)
    # the same fit with the model kept: weights and predictions bit for bit
    kept = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    assert np.array_equal(wp, kept.weights()) and np.array_equal(pp, kept.decision_function(T))
    assert np.array_equal(plain.permutation(), kept.permutation())
    plain.destroy()
    ld1 = kept.logabsdet()
    # a second fit on the same handle replaces the model: the negated labels, through the new permutation
    y1 = kept.model_labels()
    a = [b"kernel"] + [x.encode() for x in args]
    y2 = np.ascontiguousarray(-y1)
    lib.STRUMPACK_kernel_fit_HSS_double(kept.K, y2.ctypes.data, len(a), (ctypes.c_char_p * len(a))(*a))
    assert np.array_equal(kept.model_labels(), (-y1)[kept.permutation() - 1])
    assert np.isfinite(kept.log_marginal_likelihood()) and abs(kept.logabsdet() - ld1) <= 1e-2 * abs(ld1)
    assert np.all(np.isfinite(kept.predict_variance(T)))
    # keep_model(false) releases the model: its chunks go back to the pool, the calls refuse, the weights stay
    lib.SPX_device_pool_cached_bytes.restype = ctypes.c_longlong
    c0 = lib.SPX_device_pool_cached_bytes()
    w = kept.weights()
    assert lib.SPX_kernel_keep_model(kept.K, 0) == 0
    c1 = lib.SPX_device_pool_cached_bytes()
    assert c1 >= c0 + n * d * 8, (c0, c1)
    for name, rc, untouched in model_calls(lib, kept.K, T, path):
        assert rc != 0 and untouched, ("after keep_model(false)", name, rc)
    assert np.array_equal(w, kept.weights())
    kept.destroy()
    # destroy with a live model
    live = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    assert np.isfinite(live.logabsdet())
    live.destroy()
