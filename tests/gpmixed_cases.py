"""Checks of the mixed-precision exact solves: hssk_kernel_matmul_f32 on its own and Kernel<double>::model_refine / model_solve /
predict_variance_exact with krylov_inner(FP32), in their C and Python forms.  Shared by the CPU emulator tests
(tests/test_gpmixed_emu.py) and the GPU tests (tests/test_gpmixed_gpu.py), as tests/gpsolve_cases.py is.

u = 2^-24 (FP32), U = 2^-53 (FP64); references are in long double from the FP64 points.

A. The product.  out(i, c) = sum_r k32(x_i, x_r) B(r, c) + lambda B(i, c).  delta_ir, the relative error of k32_ir against the long
double kernel value k_ir, is computed PER PAIR from the points:
  points    x~ = (x - mean) s is rounded once to float: coordinate j of the pair's difference df_j is off by at most u m_j, m_j =
            |x~_ij| + |x~_rj| (a shift of the mean moves no difference).  The base-2 exponent E = sum_j df_j^2 (Gauss), sum_j |df_j|
            (Laplace) is off by   dE1 = sum_j (2 |df_j| u m_j + u^2 m_j^2)   (Gauss),   sum_j u m_j   (Laplace).
  exponent  difference form: one rounding of the difference, one or two of the square, d additions:   dE2 = (d + 3) u (E + dE1).
            matrix-core form (Gauss tiles the rule admits): the two norms are rounded (u each) and the d + 2 products are added in
            FP32 with partial sums of at most 2 (|x~_i|^2 + |x~_r|^2):   dE3 = 4 (d + 4) u (|x~_i|^2 + |x~_r|^2)   -- the kernel's
            own rule with the pair's norms; per tile it is at most HSSK_KMATMUL_F32_TAU.  Which form a pair of tiles takes is
            decided as the kernel decides it, from the tile maxima of the rounded norms; within 1e-3 of the threshold the larger
            of the two terms is taken.
  exp2      4 u (two units in the last place);   B   u (rounded once to float);   chunk   the product and at most 64 FP32
            additions on the matrix cores: 66 u of the chunk's sum of magnitudes.
  delta_ir = expm1(ln 2 (dE1 + dE2 or dE3)) (1 + 1e-4) + 72 u; the diagonal pair is selected to be 1: 72 u.  A kernel value below
  the smallest normal float may come out as 0: 2^-126 |B| per pair is added.
  FP64      the chunk sums are added in FP64, the split partials by hssk_sum_slabs, lambda B is one product and one addition:
            (n / 64 + splits + 4) U (sum_r |k_ir| |B_rc| + |lambda B_ic|).
  |out - ref| <= sum_r delta_ir |k_ir| |B_rc| + 2^-126 sum_r |B_rc| + the FP64 term, entry by entry.

B. The solver.  gmres_mixed_reference is gpsolve_cases.gmres_reference with the three rules of DESIGN.md 8f: the operator inside a
cycle is the dense kernel matrix rounded to float32 applied to the float32-rounded vector (products and sums of those in
float64, lambda z in float64), a cycle is left at max(rtol ||b||, inner_rtol ||r||), and a true residual that does not decrease
switches the rest of the call to the float64 operator.  Iteration counts: in FP64 the allowance is + 2 (an estimate that crosses
rtol one step apart in the two arithmetics, and the cycle that confirms it).  In mixed mode EVERY cycle ends at a threshold the
estimate crosses, so the one-step difference can occur once per cycle of the twin, in either direction, and the confirming
cycle adds its step:   twin - cycles(twin) - 1 <= its <= twin + cycles(twin) + 1.   (Gauss R^1, the hardest fit, sits on the upper
edge on the emulator: 34 steps in 3 cycles against the twin's 31 in 2 -- the true residual behind the last estimate lies on the
other side of rtol ||b|| in the two arithmetics; 33 on the GPU.)  The lower side catches a code path that leaves its cycles much
too early and still reports convergence.  Residual and forward-error bounds are those of gpsolve_cases, rtol unchanged:
convergence is declared on the FP64 residual alone."""
import ctypes

import numpy as np
import scipy.linalg as sla

import gp_cases as GP
import gpgrad_cases as GG
import gpsolve_cases as GS
import kernel_cases as KC
from strumpack_amd import hssk as K

LD = np.longdouble
U24 = 2.0 ** -24
U = KC.U53
S = KC.SENTINEL
TAU = 2.0 ** -17          # HSSK_KMATMUL_F32_TAU (include/hssk.h)
KT = GG.KT
L2E = 1.4426950408889634
TILE = 64


# ---- A. hssk_kernel_matmul_f32 on its own -----------------------------------------------------------------------------------------
def scaled_points(X, ktype, h):
    """the centred and scaled points in float64 (what the prep rounds to float)"""
    s = L2E / h if ktype == 1 else np.sqrt(L2E) / (h * np.sqrt(2.0))
    return (X - X.mean(0)) * s


def pair_delta(X, ktype, h):
    """(delta, tiles that may take the matrix cores, tiles that may take the difference form): delta_ir of the module docstring
    for every pair, computed coordinate by coordinate from the points"""
    n, d = X.shape
    xt = scaled_points(X, ktype, h)
    x32 = xt.astype(np.float32).astype(np.float64)
    E, dE1 = np.zeros((n, n)), np.zeros((n, n))
    for j in range(d):
        df = np.abs(xt[:, None, j] - xt[None, :, j])
        m = np.abs(xt[:, None, j]) + np.abs(xt[None, :, j])
        if ktype == 0:
            E += df * df
            dE1 += 2.0 * df * U24 * m + (U24 * m) ** 2
        else:
            E += df
            dE1 += U24 * m
    dE2 = (d + 3) * U24 * (E + dE1)
    nrm = (x32 * x32).sum(1)
    dE3 = 4.0 * (d + 4) * U24 * (nrm[:, None] + nrm[None, :])
    nt = (n + TILE - 1) // TILE
    tmax = np.array([nrm[t * TILE:(t + 1) * TILE].astype(np.float32).max() for t in range(nt)], dtype=np.float64)
    rule = 4.0 * (d + 4) * U24 * (tmax[:, None] + tmax[None, :])
    may_mf = (rule <= TAU * (1 + 1e-3)) & (ktype == 0)
    may_df = (rule >= TAU * (1 - 1e-3)) | (ktype != 0)
    tile = np.arange(n) // TILE
    mf, dfm = may_mf[np.ix_(tile, tile)], may_df[np.ix_(tile, tile)]
    dE = dE1 + np.maximum(np.where(mf, dE3, 0.0), np.where(dfm, dE2, 0.0))
    delta = np.expm1(np.log(2.0) * dE) * (1 + 1e-4) + 72 * U24
    delta[np.arange(n), np.arange(n)] = 72 * U24
    return delta, may_mf, may_df


def product_bound(k, delta, B, lam, splits):
    """the bound of the module docstring for out = k B + lambda B (k: long double, without lambda)"""
    n = len(k)
    aB = np.abs(B).astype(LD)
    mag = np.abs(k) @ aB + abs(lam) * aB
    return (delta.astype(LD) * np.abs(k)) @ aB + LD(2.0 ** -126) * aB.sum(0)[None, :] + (n / 64.0 + splits + 4) * U * mag


class Prepared:
    """device points with their prepared float form"""

    def __init__(self, hk, X, ktype, h, lam):
        self.hk, (self.n, self.d), self.ktype, self.h, self.lam = hk, X.shape, ktype, h, lam
        self.dX = hk.array(np.ascontiguousarray(X).T)
        self.spec = K.KernelSpec(self.dX.ptr, self.n, self.d, ktype, 1, h, lam)
        self.bytes = hk.lib.hssk_kernel_matmul_f32_prep_bytes(self.n, self.d)
        assert self.bytes > 0
        self.prep = hk.array(np.zeros(self.bytes + 64, dtype=np.uint8))
        self.prep.set(np.full(self.bytes + 64, 0xA5, dtype=np.uint8))
        hk.check(hk.lib.hssk_kernel_matmul_f32_prep(hk.ctx, ctypes.byref(self.spec), self.prep.ptr, self.bytes))
        hk.sync()
        assert np.all(self.prep.get()[self.bytes:] == 0xA5), "the prep wrote past its size"

    def matmul(self, B, splits=0, pad=(3, 5), stats=False):
        """one call on a padded B into a pre-filled padded output: the n x nc result after checking the sentinels around both"""
        hk, n = self.hk, self.n
        nc = B.shape[1]
        ldb, ldo = n + pad[0], n + pad[1]
        Bp = np.full((ldb, nc + 1), 1e300)
        Bp[:n, :nc] = B
        dB, dO = hk.array(Bp), hk.array(np.full((ldo, nc + 1), S))
        st = np.full(4, -1, dtype=np.int64)
        hk.check(hk.lib.hssk_kernel_matmul_f32(hk.ctx, ctypes.byref(self.spec), self.prep.ptr, dB.ptr, ldb, nc, dO.ptr, ldo, splits,
                                               st.ctypes.data if stats else None))
        hk.sync()
        got, Ba = dO.get(), dB.get()
        dB.free()
        dO.free()
        assert np.all(got[n:, :] == S) and np.all(got[:, nc] == S), "hssk_kernel_matmul_f32 wrote outside its block"
        assert np.array_equal(Ba, Bp), "hssk_kernel_matmul_f32 wrote into B"
        return (got[:n, :nc], st) if stats else got[:n, :nc]

    def free(self):
        self.dX.free()
        self.prep.free()


def max_splits(n):
    return (n + TILE - 1) // TILE


# (n, nc, d, kernel, spread of the points, lambda): every n of {1, 63, 64, 65, 200, 1000}, every nc of {1, 17, 64}, every d of
# {1, 8, 31, 64}, both kernels.  Spread 1: a standard normal cloud (at kernel_widths its scaled norms are above the matrix-core rule:
# difference form); spread 0.2: every Gauss tile on the matrix cores.  Every case runs with the splits forced to 1, 3, the maximum
# (one per 64 training points) and 0.
MATMUL_CASES = [
    (1, 1, 1, "gauss", 0.2, 0.5),
    (63, 17, 8, "gauss", 0.2, 2.5),
    (64, 64, 31, "gauss", 0.2, 0.7),
    (65, 1, 64, "gauss", 0.2, 2.5),
    (200, 17, 64, "gauss", 1.0, 0.05),
    (200, 64, 8, "gauss", 0.2, 4.0),
    (1000, 64, 8, "gauss", 0.2, 0.7),
    (1000, 17, 1, "gauss", 1.0, 2.5),
    (1000, 17, 64, "gauss", 0.2, 0.7),
    (1000, 1, 31, "gauss", 0.2, 0.05),
    (200, 64, 31, "gauss", 1.0, 2.5),
    (1, 64, 8, "laplace", 1.0, 2.5),
    (63, 1, 31, "laplace", 1.0, 0.7),
    (64, 17, 1, "laplace", 1.0, 0.05),
    (65, 64, 64, "laplace", 1.0, 4.0),
    (200, 1, 8, "laplace", 1.0, 0.5),
    (1000, 17, 31, "laplace", 0.2, 2.5),
]


def reference(X, ktype, h):
    idx = np.arange(len(X))
    return KC.kernel_ref(X, idx, idx, ktype, h, 0.0)[0]


def check_matmul(hk, n, nc, d, kern, spread, lam, seed=13):
    """random B against the long double product under the per-pair bound, at every split count; two calls bit for bit; splits = 0
    bit for bit the forced hssk_kernel_matmul_f32_splits(n); the route counts add up to the pairs of tiles"""
    rng = np.random.default_rng(seed + n + 3 * d + nc)
    X, B = spread * rng.standard_normal((n, d)), rng.standard_normal((n, nc))
    ktype = KT[kern]
    h = float(KC.kernel_widths(d)[ktype])
    P = Prepared(hk, X, ktype, h, lam)
    k = reference(X, ktype, h)
    delta, may_mf, may_df = pair_delta(X, ktype, h)
    ref = k @ B.astype(LD) + LD(lam) * B.astype(LD)
    worst, nt = 0.0, max_splits(n)
    auto = hk.lib.hssk_kernel_matmul_f32_splits(n)
    assert 1 <= auto <= nt
    outs = {}
    for splits in sorted({1, 3, nt, 0}):
        got, st = P.matmul(B, splits, stats=True)
        outs[splits] = got
        eff = auto if splits == 0 else splits
        per = -(-nt // min(eff, nt))
        used = -(-nt // per)
        E = product_bound(k, delta, B, lam, used)
        err = np.abs(got.astype(LD) - ref)
        frac = float((err / E).max())
        worst = max(worst, frac)
        print("kernel_matmul_f32 %s n=%d nc=%d d=%d spread=%g splits=%d: largest error / bound %.3f, tiles mfma %d diff %d"
              % (kern, n, nc, d, spread, splits, frac, st[0], st[1]))
        assert np.all(err <= E), (kern, n, nc, d, splits, frac)
        assert st[0] + st[1] == nt * nt and st[2] == used, (st, nt, used)
        assert int(may_mf.sum()) >= st[0] >= int((~may_df).sum()) and int(may_df.sum()) >= st[1] >= int((~may_mf).sum()), (st, may_mf, may_df)
        if ktype == 1:
            assert st[0] == 0, "a Laplace tile on the matrix cores"
        assert np.array_equal(got, P.matmul(B, splits)), "two calls differ"
    assert np.array_equal(outs[0], P.matmul(B, auto)), "splits = 0"
    P.free()
    return worst


def border_rows(n, splits):
    """up to 64 row indices: the first and the last point, both sides of every stage (= chunk) border of 64 and of the split
    borders, then evenly spread ones"""
    nt = max_splits(n)
    per = -(-nt // min(splits, nt)) * TILE
    pick = {0, n - 1}
    for b in list(range(TILE, n, TILE)) + list(range(per, n, per)):
        pick.update({b - 1, b})
    pick = sorted(p for p in pick if 0 <= p < n)
    if len(pick) > 64:
        pick = pick[:32] + pick[-32:]
    fill = [int(v) for v in np.linspace(0, n - 1, 64)]
    for v in fill:
        if len(pick) >= min(64, n):
            break
        if v not in pick:
            pick.append(v)
    return sorted(pick)


ONEHOT_CASES = [(200, 8, "gauss", 0.2, 3), (200, 8, "gauss", 1.0, 3), (200, 8, "laplace", 1.0, 3), (1000, 8, "gauss", 0.2, 3),
                (65, 31, "laplace", 1.0, 1), (1000, 1, "gauss", 1.0, 16)]


def check_onehot(hk, n, d, kern, spread, splits, seed=29):
    """B = e_r for up to 64 values of r: column c must be column r_c of the kernel matrix entry by entry within delta_ir k_ir --
    a skipped, doubled or misplaced pair shows"""
    rng = np.random.default_rng(seed + n + d)
    X = spread * rng.standard_normal((n, d))
    ktype = KT[kern]
    h = float(KC.kernel_widths(d)[ktype])
    lam = 0.75
    P = Prepared(hk, X, ktype, h, lam)
    k = reference(X, ktype, h)
    delta, _, _ = pair_delta(X, ktype, h)
    rows = border_rows(n, splits)
    B = np.zeros((n, len(rows)))
    B[rows, np.arange(len(rows))] = 1.0
    got = P.matmul(B, splits)
    worst = 0.0
    for c, r in enumerate(rows):
        want = k[:, r].copy()
        want[r] += LD(lam)
        tol = delta[:, r] * np.abs(k[:, r]) + 2.0 ** -126 + 8 * U * np.abs(want)
        err = np.abs(got[:, c].astype(LD) - want)
        assert np.all(err <= tol), (kern, n, d, r, int(np.argmax(err / tol)), float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
    print("kernel_matmul_f32 one-hot %s n=%d d=%d spread=%g splits=%d: %d columns, largest error / bound %.3f" % (kern, n, d, spread, splits, len(rows), worst))
    P.free()
    return worst


def two_route_points(rng, n, d, h):
    """a tight cloud around the origin and a distant cluster at the end: some pairs of tiles take each route"""
    X = 0.1 * h * rng.standard_normal((n, d))
    far = max(8, n // 20)
    X[-far:] += 3.0 * h / np.sqrt(d) * np.sign(rng.standard_normal(d))
    return X


def check_both_routes(hk, n=200, d=8, nc=17, seed=31):
    rng = np.random.default_rng(seed)
    for kern, ktype in KT.items():
        h = float(KC.kernel_widths(d)[ktype])
        X, B = two_route_points(rng, n, d, h), rng.standard_normal((n, nc))
        lam = 1.5
        P = Prepared(hk, X, ktype, h, lam)
        k = reference(X, ktype, h)
        delta, may_mf, may_df = pair_delta(X, ktype, h)
        got, st = P.matmul(B, 0, stats=True)
        err = np.abs(got.astype(LD) - (k @ B.astype(LD) + LD(lam) * B.astype(LD)))
        E = product_bound(k, delta, B, lam, st[2])
        print("kernel_matmul_f32 two routes %s: tiles mfma %d diff %d, largest error / bound %.3f" % (kern, st[0], st[1], float((err / E).max())))
        assert np.all(err <= E), kern
        if ktype == 0:
            assert st[0] > 0 and st[1] > 0, ("both routes expected", st)
            assert st[0] == int(may_mf.sum()) and st[1] == int(may_df.sum()), (st, may_mf, may_df)
        else:
            assert st[0] == 0 and st[1] == max_splits(n) ** 2, ("Laplace is difference form only", st)
        P.free()


def check_diagonal(hk, seed=37):
    """B = I at n = 64: out(i, i) == 1 + lambda exactly, on both routes and for both kernels"""
    n, d, lam = 64, 8, 2.5
    rng = np.random.default_rng(seed)
    for kern, ktype in KT.items():
        for spread in (0.2, 1.0):
            h = float(KC.kernel_widths(d)[ktype])
            P = Prepared(hk, spread * rng.standard_normal((n, d)), ktype, h, lam)
            got = P.matmul(np.eye(n), 0)
            assert np.all(np.diag(got) == 1.0 + lam), (kern, spread, np.diag(got))
            P.free()


def check_columns(hk, seed=41):
    """a zero column gives exact zeros; columns scaled by 2^40 and 2^-40 give the scaled results of the unscaled call bit for bit;
    column c is the same bits alone and among 64"""
    n, d = 200, 8
    rng = np.random.default_rng(seed)
    for kern, ktype, spread in (("gauss", 0, 0.2), ("gauss", 0, 1.0), ("laplace", 1, 1.0)):
        h = float(KC.kernel_widths(d)[ktype])
        P = Prepared(hk, spread * rng.standard_normal((n, d)), ktype, h, 0.7)
        B = rng.standard_normal((n, 64))
        base = P.matmul(B, 3)
        B2 = B.copy()
        B2[:, 5] = 0.0
        B2[:, 6] *= 2.0 ** 40
        B2[:, 7] *= 2.0 ** -40
        B2[:, 63] *= 2.0 ** 40
        got = P.matmul(B2, 3)
        assert np.all(got[:, 5] == 0.0), "a zero column"
        assert np.array_equal(got[:, 6], base[:, 6] * 2.0 ** 40) and np.array_equal(got[:, 63], base[:, 63] * 2.0 ** 40), "a column scaled by 2^40"
        assert np.array_equal(got[:, 7], base[:, 7] * 2.0 ** -40), "a column scaled by 2^-40"
        keep = [c for c in range(64) if c not in (5, 6, 7, 63)]
        assert np.array_equal(got[:, keep], base[:, keep]), "a column depends on its neighbours"
        for c in (0, 17, 31, 32, 63):
            assert np.array_equal(P.matmul(B[:, c:c + 1], 3)[:, 0], base[:, c]), ("column %d alone" % c)
        assert np.array_equal(P.matmul(B[:, :33], 3), base[:, :33]), "33 columns"
        P.free()


def check_refusals(hk):
    """ANOVA, d = 65, nc = 0 / 65, leading dimensions below n, null pointers: non-zero, message, outputs keep the sentinel"""
    n, d, nc = 40, 8, 5
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, d))
    P = Prepared(hk, X, 0, 1.3, 0.5)
    dB = hk.array(rng.standard_normal((n, 65)))
    fill = np.full((n, 66), S)
    dO = hk.array(fill)
    f, fp = hk.lib.hssk_kernel_matmul_f32, hk.lib.hssk_kernel_matmul_f32_prep
    ok = P.spec
    anova = K.KernelSpec(P.dX.ptr, n, d, 2, 2, 1.3, 0.0)
    dX65 = hk.array(rng.standard_normal((65, n)))
    wide = K.KernelSpec(dX65.ptr, n, 65, 0, 1, 1.3, 0.0)
    pbefore = P.prep.get()
    assert f(hk.ctx, ctypes.byref(anova), P.prep.ptr, dB.ptr, n, nc, dO.ptr, n, 0, None) == 2 and "ANOVA" in hk.error()
    assert f(hk.ctx, ctypes.byref(wide), P.prep.ptr, dB.ptr, n, nc, dO.ptr, n, 0, None) == 2 and "64" in hk.error()
    assert fp(hk.ctx, ctypes.byref(anova), P.prep.ptr, P.bytes) == 2 and fp(hk.ctx, ctypes.byref(wide), P.prep.ptr, P.bytes) == 2
    assert hk.lib.hssk_kernel_matmul_f32_prep_bytes(n, 65) < 0 and hk.lib.hssk_kernel_matmul_f32_prep_bytes(n, 0) < 0
    assert fp(hk.ctx, ctypes.byref(ok), P.prep.ptr, P.bytes - 1) != 0 and fp(hk.ctx, ctypes.byref(ok), None, P.bytes) != 0
    for rc in (f(hk.ctx, ctypes.byref(ok), P.prep.ptr, dB.ptr, n, 0, dO.ptr, n, 0, None),
               f(hk.ctx, ctypes.byref(ok), P.prep.ptr, dB.ptr, n, 65, dO.ptr, n, 0, None),
               f(hk.ctx, ctypes.byref(ok), P.prep.ptr, dB.ptr, n - 1, nc, dO.ptr, n, 0, None),
               f(hk.ctx, ctypes.byref(ok), P.prep.ptr, dB.ptr, n, nc, dO.ptr, n - 1, 0, None),
               f(hk.ctx, ctypes.byref(ok), None, dB.ptr, n, nc, dO.ptr, n, 0, None),
               f(hk.ctx, ctypes.byref(ok), P.prep.ptr, None, n, nc, dO.ptr, n, 0, None),
               f(hk.ctx, ctypes.byref(ok), P.prep.ptr, dB.ptr, n, nc, None, n, 0, None),
               f(hk.ctx, None, P.prep.ptr, dB.ptr, n, nc, dO.ptr, n, 0, None),
               f(None, ctypes.byref(ok), P.prep.ptr, dB.ptr, n, nc, dO.ptr, n, 0, None),
               f(hk.ctx, ctypes.byref(ok), P.prep.ptr, dB.ptr, n, nc, dB.ptr, n, 0, None),
               f(hk.ctx, ctypes.byref(ok), P.prep.ptr, dB.ptr, n, nc, dO.ptr, n, -1, None)):
        assert rc != 0 and hk.error()
    hk.sync()
    assert np.array_equal(dO.get(), fill), "a refused call wrote its output"
    assert np.array_equal(P.prep.get(), pbefore), "a refused prep wrote"
    # more splits than stages: every split one stage
    B = rng.standard_normal((n, nc))
    assert np.array_equal(P.matmul(B, 50), P.matmul(B, 1))
    for v in (dB, dO, dX65):
        v.free()
    P.free()


# ---- B. the solver ----------------------------------------------------------------------------------------------------------------
RTOL = 1e-8
INNER_RTOL = 1e-4


def gmres_mixed_reference(A, A32, lam, msolve, b, x0, rtol, inner_rtol, maxit, restart):
    """gpsolve_cases.gmres_reference with the three rules of the mixed mode (module docstring).  A: the float64 matrix with lambda;
    A32: the kernel matrix without lambda, rounded to float32.  Returns (x, steps, residual history, cycles, fallbacks)."""
    n, m = len(b), min(restart, maxit)
    A32 = A32.astype(np.float64)
    x, bn, steps, hist, cycles, fallbacks, mixed, rprev = x0.copy(), np.linalg.norm(b), 0, [], 0, 0, True, None
    if bn == 0:
        return np.zeros(n), 0, [0.0], 0, 0

    def inner(z):
        if not mixed:
            return A @ z
        return A32 @ z.astype(np.float32).astype(np.float64) + lam * z

    while True:
        r = b - A @ x
        rn = np.linalg.norm(r)
        hist.append(rn / bn)
        if rn <= rtol * bn or steps >= maxit:
            return x, steps, hist, cycles, fallbacks
        if mixed and rprev is not None and not rn < rprev:
            mixed, fallbacks = False, fallbacks + 1
        rprev = rn
        thr = max(rtol * bn, inner_rtol * rn) if mixed else rtol * bn
        cycles += 1
        V = np.zeros((n, m + 1))
        V[:, 0] = r / rn
        R, cs, sn, g, kc = np.zeros((m, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1), 0
        g[0] = rn
        for k in range(m):
            w = inner(msolve(V[:, k]))
            Q = V[:, :k + 1]
            h1 = Q.T @ w
            w = w - Q @ h1
            h2 = Q.T @ w
            w = w - Q @ h2
            below = np.linalg.norm(w)
            V[:, k + 1] = w / below if below > 0 else 0.0
            h = np.append(h1 + h2, below)
            steps += 1
            for i in range(k):
                h[i], h[i + 1] = cs[i] * h[i] + sn[i] * h[i + 1], -sn[i] * h[i] + cs[i] * h[i + 1]
            rr = np.hypot(h[k], h[k + 1])
            if not rr > 0:
                break
            cs[k], sn[k] = h[k] / rr, h[k + 1] / rr
            h[k] = rr
            R[:k + 1, k] = h[:k + 1]
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            kc = k + 1
            if abs(g[k + 1]) <= thr or below == 0 or steps >= maxit:
                break
        if kc == 0:
            return x, steps, hist, cycles, fallbacks
        y = np.linalg.solve(np.triu(R[:kc, :kc]), g[:kc])
        x = x + msolve(V[:, :kc] @ y)


def float_operator(kr, kind):
    """the kernel matrix without lambda from the float32-rounded centred points, rounded to float32: the twin's inner operator"""
    ktype, _, h = kind
    X = kr.model_points()
    x32 = scaled_points(X, ktype, h).astype(np.float32).astype(np.float64)
    df = x32[:, None, :] - x32[None, :, :]
    E = (df * df).sum(-1) if ktype == 0 else np.abs(df).sum(-1)
    return np.exp2(-E).astype(np.float32)


# the kept fits of gpsolve_cases at restart 30 (n = 700), among them Gauss R^1 with ||I - H^-1 A|| = 36
REFINE_CASES = [("gauss", 8, 4.0, 1.0), ("laplace", 8, 0.05, 1.0), ("gauss", 8, 0.05, 0.5), ("gauss", 33, 4.0, 1.0), ("gauss", 1, 0.05, 1.0)]


def check_refine(KM, lib, kern, d, lam, hscale, path, inner_rtol=None):
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    try:
        return check_refined(kr, T, kind, lib, path, "%s R^%d lambda=%g h=%.3g" % (kern, d, lam, kind[2]), inner_rtol)
    finally:
        kr.destroy()


def check_refine_matrix_cores(KM, lib, hk, path, n=GP.N_MODEL, d=8, lam=0.05, spread=0.2):
    """the refine checks on points the matrix-core rule admits (the spread of the product tests): every pair of tiles of the
    fit's own cluster-ordered points is counted on the matrix-core route by the product's statistics before the solver runs"""
    rng = np.random.default_rng(91)
    X, T = spread * rng.standard_normal((n, d)), spread * rng.standard_normal((20, d))
    y = np.where(X[:, 0] + 0.3 * spread * rng.standard_normal(n) > 0, 1.0, -1.0)
    h = float(KC.kernel_widths(d)[0])
    kr = KM.KernelRegression(lib, h=h, lam=lam, kernel="rbf", argv=GP.FIT_ARGS, keep_model=True).fit(X, y)
    try:
        P = Prepared(hk, kr.model_points(), 0, h, lam)
        _, st = P.matmul(kr.model_labels()[:, None], 0, stats=True)
        P.free()
        assert st[0] == max_splits(n) ** 2 and st[1] == 0, ("the fit's points are not on the matrix-core route", st)
        return check_refined(kr, T, (0, 1, h), lib, path, "gauss R^%d spread %g (matrix cores)" % (d, spread), None)
    finally:
        kr.destroy()


def check_refined(kr, T, kind, lib, path, tag, inner_rtol=None):
    Hd, _, _ = GP.dense_model(kr, path)
    y, w0, ld = kr.model_labels(), kr.weights(), kr.logabsdet()
    Kd = GS.exact_matrix(kr, kind)
    lu = sla.lu_factor(Hd)
    msolve = lambda v: sla.lu_solve(lu, v)      # noqa: E731
    irt = INNER_RTOL if inner_rtol is None else inner_rtol
    _, t_its, t_hist, t_cyc, t_fb = gmres_mixed_reference(Kd, float_operator(kr, kind), kr.lam, msolve, y, w0, RTOL, irt, 100, 30)
    _, f_its, f_hist = GS.gmres_reference(Kd, msolve, y, w0, RTOL, 100, 30)
    info = kr.refine(rtol=RTOL, inner="f32", inner_rtol=inner_rtol)
    w = kr.weights()
    r_ld, bound = GS.residual_ld(kr, kind, w, y)
    print("mixed refine %s: %d steps in %d cycles (twin %d in %d, %d fallbacks; FP64 twin %d in %d), %d FP64 + %d FP32 "
          "products, residual %.3g -> %.3g (long double %.3g, bound %.3g)" % (tag, info["iterations"], info["cycles"], t_its, t_cyc, t_fb,
                                                                               f_its, len(f_hist) - 1, info["products"], info["products32"],
                                                                               info["residual0"], info["residual"], r_ld, bound))
    assert kr.krylov_inner() == ("f64", INNER_RTOL), "the per-call mode was not restored"
    assert info["converged"], tag
    assert info["fallbacks"] == 0 and t_fb == 0, (tag, info["fallbacks"], t_fb)
    assert info["products32"] == info["iterations"] == info["its"], (tag, info)
    assert info["products"] == info["cycles"] + 1, (tag, info)
    assert t_its - t_cyc - 1 <= info["iterations"] <= t_its + t_cyc + 1, (tag, info["iterations"], t_its, t_cyc)
    assert abs(info["residual"] - r_ld) <= bound and r_ld <= RTOL + bound, (tag, info["residual"], r_ld, bound)
    sv = np.linalg.svd(Kd, compute_uv=False)
    ae = np.linalg.solve(Kd, y)
    fe, fb = np.linalg.norm(w - ae) / np.linalg.norm(ae), (sv[0] / sv[-1]) * (RTOL + bound + GP.EPS_F)
    assert fe <= fb, (tag, fe, fb)
    GS.prediction_check(kr, kind, T, w)
    assert kr.logabsdet() == ld, "refine changed the log-determinant"
    # the counts through the C call
    st = np.zeros(6)
    assert lib.SPX_kernel_krylov_stats(kr.K, st.ctypes.data) == 0
    assert (st[0], st[1], st[2], st[3]) == (info["products"], info["products32"], 0, info["cycles"]) and st[5] >= 0.0, st
    return kr_counts(info), f_its + len(f_hist)      # (FP64 products of the twin in FP64 mode: steps + cycle starts)


def kr_counts(info):
    return dict(products=info["products"], products32=info["products32"], cycles=info["cycles"], iterations=info["iterations"])


def check_fewer_fp64_products(KM, lib):
    """Gauss R^1 (||I - H^-1 A|| = 36, FP64 GMRES(30) needs 21 steps): the mixed call spends fewer FP64 products than the FP64 call
    from the same fit, and both reach rtol"""
    kr, T, kind = GP.fit_model(KM, lib, "gauss", 1, 0.05, 1.0)
    k2 = GP.fit_model(KM, lib, "gauss", 1, 0.05, 1.0)[0]
    try:
        assert np.array_equal(kr.weights(), k2.weights()), "two fits of the same data differ"
        f64 = k2.refine(rtol=RTOL)
        k2.destroy()
        f32 = kr.refine(rtol=RTOL, inner="f32")
        print("Gauss R^1: FP64 mode %d products (%d steps); mixed %d FP64 + %d FP32 products (%d steps, %d cycles)"
              % (f64["products"], f64["iterations"], f32["products"], f32["products32"], f32["iterations"], f32["cycles"]))
        assert f64["converged"] and f32["converged"] and f64["products32"] == 0 and f64["fallbacks"] == 0
        assert f32["products"] < f64["products"], (f32, f64)
    finally:
        kr.destroy()
        k2.destroy()


def check_solve(KM, lib, path):
    """two blocks (64 + 6 columns, a zero column among them) in mixed mode under gpsolve's bounds; two calls bit for bit; the
    model untouched"""
    kr, T, kind = GP.fit_model(KM, lib, "laplace", 8, 0.05, 1.0)
    try:
        Kd = GS.exact_matrix(kr, kind)
        sv = np.linalg.svd(Kd, compute_uv=False)
        cond = sv[0] / sv[-1]
        y, w0, ld = kr.model_labels(), kr.weights(), kr.logabsdet()
        rng = np.random.default_rng(77)
        n, m = kr.n, 70
        B = np.asfortranarray(rng.standard_normal((n, m)))
        B[:, 0], B[:, 2], B[:, 66] = y, 0.0, 0.0
        kr.set_krylov_inner("f32")
        assert kr.krylov_inner() == ("f32", INNER_RTOL)
        X, info = kr.solve(B, rtol=RTOL)
        assert np.all(np.isfinite(X)) and info["converged"] and len(info["residual"]) == m and info["fallbacks"] == 0
        assert info["products32"] > 0 and info["products"] == info["cycles"] + 2, info
        Xe = np.linalg.solve(Kd, B)
        for c in range(m):
            if not B[:, c].any():
                assert np.all(X[:, c] == 0.0) and info["its"][c] == 0 and info["residual"][c] == 0.0, "the zero column"
                continue
            r_ld, bound = GS.residual_ld(kr, kind, X[:, c], B[:, c])
            assert abs(info["residual"][c] - r_ld) <= bound and r_ld <= RTOL + bound, (c, info["residual"][c], r_ld, bound)
            fe = np.linalg.norm(X[:, c] - Xe[:, c]) / np.linalg.norm(Xe[:, c])
            assert fe <= cond * (RTOL + bound + GP.EPS_F), (c, fe)
        print("mixed solve m=%d: %d steps at most, %d FP64 + %d FP32 products, %d cycles" % (m, info["iterations"], info["products"], info["products32"], info["cycles"]))
        X2, info2 = kr.solve(B, rtol=RTOL)
        assert np.array_equal(X, X2) and np.array_equal(info["its"], info2["its"]), "two mixed solves differ"
        assert np.array_equal(kr.weights(), w0) and kr.logabsdet() == ld, "solve disturbed the model"
        kr.set_krylov_inner("f64")
    finally:
        kr.destroy()


def check_variance(KM, lib, kern, d, lam, hscale, m_test):
    """predict_variance(exact=True, inner="f32") on gpsolve's test points under its bound, rtol unchanged"""
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    T = T[-m_test:]
    try:
        Kd = GS.exact_matrix(kr, kind)
        sv = np.linalg.svd(Kd, compute_uv=False)
        ref, bound = GP.variance_reference(kr, Kd, sv, T, kind)
        ktype, p, h = kind
        X = kr.model_points()
        n = len(X)
        kt = np.asarray(KC.kernel_ref(np.vstack([X, T]), np.arange(n), n + np.arange(len(T)), ktype, h, 0.0, p)[0], dtype=np.float64)
        bound = bound + GS.RTOL * np.linalg.norm(kt, axis=0) ** 2 / sv[-1]
        got, info = kr.predict_variance(T, exact=True, rtol=GS.RTOL, info=True, inner="f32")
        err = np.abs(got - ref)
        print("mixed exact variance %s R^%d: largest error / bound %.3g; %d steps, %d FP64 + %d FP32 products, %d fallbacks"
              % (kern, d, float((err / bound).max()), info["iterations"], info["products"], info["products32"], info["fallbacks"]))
        assert info["converged"] and info["products32"] > 0 and info["fallbacks"] == 0
        assert np.all(err <= bound), float((err / bound).max())
        assert np.array_equal(got, kr.predict_variance(T, exact=True, rtol=GS.RTOL, inner="f32")), "two mixed variance calls differ"
    finally:
        kr.destroy()


def fallback_data(n=300, h=1.0, seed=3):
    """R^1: two clusters centred at +-1e7 h with a spread of a few h.  After centring the float spacing is h / 2 .. h: the rounded
    operator is destroyed, the FP64 one is fine"""
    rng = np.random.default_rng(seed)
    X = np.where(np.arange(n) % 2 == 0, 1.0e7 * h, -1.0e7 * h)[:, None] + 3.0 * h * rng.standard_normal((n, 1))
    y = np.where(rng.standard_normal(n) > 0, 1.0, -1.0)
    return X, y


def check_fallback(KM, lib, path):
    h, lam = 1.0, 0.5
    X, y = fallback_data(h=h)
    kr = KM.KernelRegression(lib, h=h, lam=lam, kernel="rbf", argv=["--hss_leaf_size", "64"], keep_model=True).fit(X, y)
    kind = (0, 1, h)
    try:
        Hd, _, _ = GP.dense_model(kr, path)
        yk, w0 = kr.model_labels(), kr.weights()
        Kd = GS.exact_matrix(kr, kind)
        lu = sla.lu_factor(Hd)
        msolve = lambda v: sla.lu_solve(lu, v)      # noqa: E731
        _, t_its, t_hist, t_cyc, t_fb = gmres_mixed_reference(Kd, float_operator(kr, kind), lam, msolve, yk, w0, RTOL, INNER_RTOL, 100, 30)
        print("fallback twin: residuals at the cycle starts %s, %d fallbacks" % (["%.3g" % v for v in t_hist], t_fb))
        assert len(t_hist) >= 2 and t_hist[1] >= t_hist[0] and t_fb >= 1, "the twin's residual does not rise at the first mixed cycle"
        info = kr.refine(rtol=RTOL, inner="f32")
        w = kr.weights()
        r_ld, bound = GS.residual_ld(kr, kind, w, yk)
        print("fallback: %d fallbacks, %d FP64 + %d FP32 products, residual %.3g -> %.3g (long double %.3g)"
              % (info["fallbacks"], info["products"], info["products32"], info["residual0"], info["residual"], r_ld))
        assert info["fallbacks"] >= 1 and info["converged"], info
        assert abs(info["residual"] - r_ld) <= bound and r_ld <= RTOL + bound, (r_ld, bound)
        sv = np.linalg.svd(Kd, compute_uv=False)
        ae = np.linalg.solve(Kd, yk)
        assert np.linalg.norm(w - ae) / np.linalg.norm(ae) <= (sv[0] / sv[-1]) * (RTOL + bound + GP.EPS_F)
    finally:
        kr.destroy()


def check_precision_setting(KM, lib):
    """precision 0 set explicitly is bitwise never setting it; the setter restores the mode; the mode survives set_lambda and is
    reported by the getter"""
    def fit():
        return GP.fit_model(KM, lib, "gauss", 8, 4.0, 1.0)[0]
    a, b = fit(), fit()
    try:
        assert a.krylov_inner() == ("f64", INNER_RTOL)
        b.set_krylov_inner("f32", 1e-3)
        assert b.krylov_inner() == ("f32", 1e-3)
        b.set_lambda(b.lam)
        assert b.krylov_inner() == ("f32", 1e-3), "set_lambda changed the mode"
        b.set_krylov_inner("f64")
        assert b.krylov_inner() == ("f64", INNER_RTOL)
        ia, ib = a.refine(rtol=RTOL), b.refine(rtol=RTOL)
        assert np.array_equal(a.weights(), b.weights()), "precision 0 differs from the default"
        for key in ("iterations", "products", "solves", "cycles", "residual0", "residual", "products32", "fallbacks"):
            assert ia[key] == ib[key], key
        assert ia["products32"] == 0 and ia["products"] == ia["iterations"] + ia["cycles"] + 1
        rng = np.random.default_rng(5)
        B = rng.standard_normal((a.n, 3))
        assert np.array_equal(a.solve(B)[0], b.solve(B, inner="f64")[0])
        # "f64" forces FP64 for one call on a handle set to FP32; None takes the handle's mode and its inner_rtol
        b.set_lambda(b.lam)
        b.set_krylov_inner("f32", 1e-3)
        forced = b.refine(rtol=RTOL, inner="f64")
        assert forced["products32"] == 0 and forced["products"] == forced["iterations"] + forced["cycles"] + 1, forced
        assert b.krylov_inner() == ("f32", 1e-3), "a per-call override changed the handle"
        b.set_lambda(b.lam)
        own = b.refine(rtol=RTOL)
        assert own["products32"] == own["iterations"] > 0 and b.krylov_inner() == ("f32", 1e-3), own
    finally:
        a.destroy()
        b.destroy()


def mixed_calls(lib, Kh, n, d, m=3):
    return [r for r in GS.solve_calls(lib, Kh, n, d, m) if r[0] != "krylov_ms"]


def check_refusals_and_lifecycle(KM, lib):
    n, d = 300, 8
    X, y, _ = GP.model_data(d, n, 20)
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]
    st = np.full(6, 123.25)
    # a float handle: no mode to set
    kf = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X.astype(np.float32), y.astype(np.float32))
    assert lib.SPX_kernel_set_krylov_inner(kf.K, 1, 0.0) != 0 and lib.SPX_kernel_krylov_inner(kf.K, None, None) != 0
    assert lib.SPX_kernel_krylov_stats(kf.K, st.ctypes.data) != 0 and np.all(st == 123.25)
    kf.destroy()
    # without a kept model: the mode can be set, the calls are refused
    plain = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y)
    assert lib.SPX_kernel_set_krylov_inner(plain.K, 1, 0.0) == 0
    for name, rc, untouched in mixed_calls(lib, plain.K, n, d):
        assert rc != 0 and untouched, ("no keep_model", name, rc)
    assert lib.SPX_kernel_krylov_stats(plain.K, st.ctypes.data) != 0 and np.all(st == 123.25)
    plain.destroy()
    # ANOVA
    ka = KM.KernelRegression(lib, h=h, lam=4.0, kernel="ANOVA", degree=2, argv=args, keep_model=True).fit(X, y)
    lda, wa = ka.logabsdet(), ka.weights()
    assert lib.SPX_kernel_set_krylov_inner(ka.K, 1, 0.0) == 0
    for name, rc, untouched in mixed_calls(lib, ka.K, n, d):
        assert rc != 0 and untouched, ("ANOVA", name, rc)
    assert ka.logabsdet() == lda and np.array_equal(ka.weights(), wa)
    ka.destroy()
    # d = 65: refused in mixed mode, fine in FP64 mode
    X65, y65, _ = GP.model_data(65, n, 20)
    k65 = KM.KernelRegression(lib, h=float(KC.kernel_widths(65)[0]), lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X65, y65)
    ld65, w65 = k65.logabsdet(), k65.weights()
    k65.set_krylov_inner("f32")
    for name, rc, untouched in mixed_calls(lib, k65.K, n, 65):
        assert rc != 0 and untouched, ("d = 65", name, rc)
    assert k65.logabsdet() == ld65 and np.array_equal(k65.weights(), w65), "a refused call disturbed the model"
    try:
        k65.refine(inner="f32")
        raise AssertionError("d = 65 was accepted in mixed mode")
    except RuntimeError:
        pass
    k65.set_krylov_inner("f64")
    assert k65.refine()["converged"], "the FP64 mode has lost a dimension"
    k65.destroy()
    # the setter's own refusals: nothing changes
    kr = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    kr.set_krylov_inner("f32", 1e-3)
    for prec, irt in ((2, 1e-4), (-1, 1e-4), (1, 1.0), (1, 7.0), (0, float("nan")), (1, float("nan")), (1, float("inf"))):
        assert lib.SPX_kernel_set_krylov_inner(kr.K, prec, irt) != 0, (prec, irt)
        assert kr.krylov_inner() == ("f32", 1e-3), (prec, irt)
    for bad in (0.0, 1.0, -1e-4, float("nan")):
        try:
            kr.refine(inner="f32", inner_rtol=bad)
            raise AssertionError("inner_rtol = %r was accepted" % bad)
        except RuntimeError:
            pass
    try:
        kr.refine(inner="f16")
        raise AssertionError("an unknown precision was accepted")
    except ValueError:
        pass
    assert kr.krylov_inner() == ("f32", 1e-3)
    assert lib.SPX_kernel_set_krylov_inner(kr.K, 1, 0.0) == 0 and kr.krylov_inner() == ("f32", INNER_RTOL)      # (<= 0: the default)
    p, r = ctypes.c_int(-5), ctypes.c_double(-5.0)
    assert lib.SPX_kernel_krylov_inner(kr.K, ctypes.byref(p), ctypes.byref(r)) == 0 and p.value == 1 and r.value == INNER_RTOL
    for name, rc, untouched in mixed_calls(lib, kr.K, n, d):
        assert rc == 0 and not untouched, (name, rc)
    assert lib.SPX_kernel_krylov_stats(kr.K, st.ctypes.data) == 0 and st[1] > 0 and st[0] >= 1, st
    kr.destroy()
