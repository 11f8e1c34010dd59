"""Checks of the solves with the EXACT kernel matrix from a kept kernel ridge regression fit: hssk_krylov_start / _orth / _combine,
Kernel<double>::model_refine / model_solve / predict_variance_exact and their C and Python forms.  Shared by the CPU emulator
tests (tests/test_gpsolve_emu.py) and the GPU tests (tests/test_gpsolve_gpu.py), as tests/gpgrad_cases.py is.

u = 2^-53 throughout; references are in long double.

hssk_krylov_orth.  The basis v_0 .. v_k of a column is orthonormal (a QR of random columns: |v_i^T v_j - delta_ij| is a few u), w
is random, n > k + 1.  The kernel computes h1_j = fl(v_j^T w), w' = w - sum_j h1_j v_j, h2_j = fl(v_j^T w'), w'' = w' - sum_j h2_j v_j,
Hout(j) = fl(h1_j + h2_j), Hout(k + 1) = fl(sqrt(fl(w''^T w''))), v_{k+1} = fl(w'' / Hout(k + 1)).
  - An n-term dot product, in any order: |fl(x^T y) - x^T y| <= n u |x|^T |y| <= n u ||x|| ||y||.
  - An update step w - h v is two roundings (one with a fused multiply-add): after the k + 1 steps of a pass every entry is off by at
    most 2 (k + 1) u of the largest magnitude it went through, in norm 2 (k + 1) u ||w|| to first order.
  Reconstruction.  The dot products do not enter: whatever the coefficients are, w'' differs from w - sum_j (h1_j + h2_j) v_j only
  by the update roundings of both passes, 4 (k + 1) u ||w||, the rounding of the k + 1 sums h1_j + h2_j, u sqrt(k + 1) ||w||, and
  Hout(k + 1) v_{k+1} = w'' (1 + delta), |delta| <= u (the error of the norm cancels).  Together at most (5 (k + 1) + 1) u ||w||
  <= 4 (k + 3) n u ||w|| for n >= 2.
  Orthogonality.  v_j^T w'' = (v_j^T w' - h2_j) - sum_{i != j} h2_i v_j^T v_i - (update roundings)^T v_j.  The first term is the error
  of one dot product, n u ||w'||; the h2_i are themselves of the size of the first pass's errors and multiply a few u; the last is
  2 (k + 1) u ||w'||.  Divided by ||w''|| = ||w'|| (1 + O(n u)): (n + 2 k + 2) u (1 + O(n u)) <= 2 (k + 3) n u.
  Norm.  fl(w''^T w'') is within n u of the sum, its root within n u / 2 + u, the division adds u: | ||v_{k+1}|| - 1 | <= (n / 2 + 2) u
  <= 4 n u.
  A w in the span of the basis.  After the first pass what is left is error: the k + 1 dot products, sqrt(k + 1) n u ||w||, the
  updates, 2 (k + 1) u ||w||, and the basis's own (k + 1) (few u) ||w||; the second pass projects and adds its own, smaller ones.
  Below 4 (k + 3) n u ||w||.
So C = 4 covers all four statements (the issue allows at most 8): ORTH_C.

hssk_krylov_start.  r_i = fl(b_i - ax_i) is one rounding; the norm is the root of an n-term sum of squares of the COMPUTED r:
|norms - ||r|| | <= (n / 2 + 2) u ||r||, asserted as (n + 4) u ||r||, r the exact difference; an entry of V0 is r_i (1 + u) / norm
(1 + u): within (n + 6) u |r_i| / ||r|| of the exact quotient.

hssk_krylov_combine.  kcount products and kcount additions in the order of j (and one more addition when accumulating):
|out - ref| <= (kcount + 2) u (sum_j |y_j v_j| + |out_0|) entry by entry.

The solver.  gmres_reference is the same algorithm in float64 numpy on dense matrices: right preconditioning with
np.linalg.solve(Hd, .), Hd the dense form of the matrix the handle writes (gp_cases.dense_model), the operator Kd =
kernel_cases.kernel_np(.., lambda), CGS2, the true residual at the start of every cycle, the same first iterate and the same
stopping tests.  Iteration counts are compared with it (+ 2: an estimate that crosses rtol one step apart in the two
arithmetics, and the cycle that confirms it), never with a constant.  `bound` below is the bound of gpgrad_cases.check_residual:
||E(alpha)||_2 / ||y||_2 with E the product bound of the alpha column -- how far a residual computed with the evaluated kernel
can be from the long double one.  The forward error: alpha - alpha_e = Kd^-1 (r + the reference solve's own residual), so
||alpha - alpha_e|| <= cond_2(Kd) (rtol + bound + EPS_F) ||alpha_e|| (||r|| <= (rtol + bound) ||y|| <= (rtol + bound) ||Kd|| ||alpha_e||).

The exact variance.  ve_c = k(t_c, t_c) - kt_c^T Kd^-1 kt_c.  The bound is gp_cases.variance_reference's with Hd -> Kd, its forward
error term EPS_F cond nk nz replaced by   rtol nk^2 / sigma_min(Kd) + EPS_F cond nk nz:   the solve stops at a residual rtol ||kt||,
which Kd^-1 turns into at most rtol nk / sigma_min in z and the dot product with kt into rtol nk^2 / sigma_min; the second part is
numpy's own solve.

Emulator tier.  The cases are the GPU tier's, with two reductions: the exact variance takes the last 66 of the 130 test points (two
chunks, 64 + 2, the two training points among them) instead of three chunks -- a chunk is some twenty products of 700 x 700 x 64
pairs on the fiber emulator, over a minute for three --, and the C++ driver runs at n = 160 instead of 1000 (N_CPP of the test
modules).  In check_solve the twin runs on every non-zero column of both blocks; its preconditioner is the LU factorisation of Hd
computed once (scipy's lu_factor / lu_solve: the getrf / getrs that np.linalg.solve runs on every call)."""
import numpy as np
import scipy.linalg as sla

import gp_cases as GP
import gpgrad_cases as GG
import kernel_cases as KC

LD = np.longdouble
U = KC.U53
S = KC.SENTINEL
ORTH_C = 4.0
ALL = (1 << 64) - 1


# ---- A. the kernels on their own --------------------------------------------------------------------------------------------------
# (n, nc, k): every n of {1, 63, 64, 65, 257, 1000} (one chunk of 256 rows ragged and full, two chunks with a one-row tail, four
# chunks), every (nc, k) of {1, 17, 64} x {0, 1, 7, 30} at n = 257 and n = 1000
ORTH_CASES = ([(1, 1, 0), (63, 17, 7), (63, 64, 30), (64, 64, 1), (64, 1, 30), (65, 1, 0), (65, 17, 30)]
              + [(n, nc, k) for n in (257, 1000) for nc in (1, 17, 64) for k in (0, 1, 7, 30)])
START_CASES = [(1, 1), (63, 17), (64, 64), (65, 1), (257, 1), (257, 17), (257, 64), (1000, 1), (1000, 17), (1000, 64)]
COMBINE_CASES = [(1, 1, 1), (63, 17, 7), (64, 64, 31), (65, 1, 2), (257, 1, 30), (257, 17, 1), (257, 64, 8), (1000, 1, 1), (1000, 17, 31),
                 (1000, 64, 8)]


def make_basis(rng, n, nc, nb, ldv, extra=1):
    """(ldv, nc, nb + extra) Fortran array: blocks 0 .. nb - 1 hold an orthonormal basis per column in their first n rows,
    everything else the sentinel.  Block j of the device layout is [:, :, j]."""
    V = np.full((ldv, nc, nb + extra), S, order="F")
    for c in range(nc):
        Q, _ = np.linalg.qr(rng.standard_normal((n, nb)))
        V[:n, c, :nb] = Q
    return V


def run_orth(hk, V, n, nc, k, W, active, ldh):
    """one call on copies of V and W: (V after, W after, Hout after), Hout pre-filled with the sentinel and one column wider"""
    dV, dW, dH = hk.array(V), hk.array(W), hk.array(np.full((ldh, nc + 1), S))
    hk.check(hk.lib.hssk_krylov_orth(hk.ctx, dV.ptr, V.shape[0], n, nc, k, dW.ptr, W.shape[0], active, dH.ptr, ldh))
    hk.sync()
    out = dV.get(), dW.get(), dH.get()
    for v in (dV, dW, dH):
        v.free()
    return out


def check_orth(hk, n, nc, k, seed=3):
    rng = np.random.default_rng(seed + 7 * n + nc + 31 * k)
    ldv, ldw, ldh, k1 = n + 3, n + 5, k + 4, k + 1
    assert k1 <= n, "a case needs k + 1 <= n"
    generic = n > k1                     # (n = 1: a basis of one vector, and every w lies in its span)
    V = make_basis(rng, n, nc, k1, ldv, extra=2)
    W = np.full((ldw, nc + 1), S, order="F")
    W[:n, :nc] = rng.standard_normal((n, nc))
    span = -1
    if nc > 2 or not generic:            # one column in the span of its basis, one exactly zero
        span = nc - 1
        W[:n, span] = V[:n, span, :k1] @ rng.standard_normal(k1)
    zero = nc - 2 if nc > 2 else -1
    if zero >= 0:
        W[:n, zero] = 0.0
    Va, Wa, Ha = run_orth(hk, V, n, nc, k, W, ALL, ldh)
    # nothing outside the block: padding rows, the blocks 0 .. k, the block behind k + 1, the columns >= nc
    assert np.array_equal(Va[:, :, :k1], V[:, :, :k1]) and np.all(Va[n:, :, k1] == S) and np.all(Va[:, :, k1 + 1] == S), "V outside block k + 1"
    assert np.all(Wa[n:, :] == S) and np.all(Wa[:, nc] == S), "W outside its block"
    assert np.all(Ha[k + 2:, :] == S) and np.all(Ha[:, nc] == S), "Hout outside its block"
    assert np.all(np.isfinite(Va[:n, :, k1])) and np.all(np.isfinite(Ha[:k + 2, :nc])), "not a number"
    worst = 0.0
    for c in range(nc):
        B, w, h, vn = V[:n, c, :k1].astype(LD), W[:n, c].astype(LD), Ha[:k + 2, c].astype(LD), Va[:n, c, k1].astype(LD)
        wn = float(np.sqrt((w * w).sum()))
        if c == zero:
            assert np.all(Va[:n, c, k1] == 0.0) and np.all(Ha[:k + 2, c] == 0.0), "a zero w"
            continue
        rec = float(np.sqrt(((w - B @ h[:k1] - h[k1] * vn) ** 2).sum()))
        tol = ORTH_C * (k + 3) * n * U
        assert rec <= tol * wn, ("reconstruction", n, nc, k, c, rec / wn, tol)
        worst = max(worst, rec / wn / tol)
        if c == span:
            assert float(h[k1]) <= tol * wn, ("a w in the span", n, nc, k, float(h[k1]) / wn, tol)
            continue
        orth = float(np.abs(B.T @ vn).max())
        nrm = abs(float(np.sqrt((vn * vn).sum())) - 1.0)
        assert orth <= tol, ("orthogonality", n, nc, k, c, orth, tol)
        assert nrm <= ORTH_C * n * U, ("norm", n, nc, k, c, nrm)
        worst = max(worst, orth / tol, nrm / (ORTH_C * n * U))
        # W is left holding the vector that was normalised
        assert np.all(np.abs(Wa[:n, c].astype(LD) - h[k1] * vn) <= 4 * U * np.abs(Wa[:n, c])), "W after the call"
    print("krylov_orth n=%d nc=%d k=%d: largest error / bound %.3g" % (n, nc, k, worst))
    # two calls bit for bit
    Vb, Wb, Hb = run_orth(hk, V, n, nc, k, W, ALL, ldh)
    assert np.array_equal(Va, Vb) and np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb), "two calls differ"
    # inactive columns: zeros in block k + 1 and in Hout, their W untouched; the active ones the same bits as before
    for mask in sorted({1, 1 << (nc - 1), 0x5555555555555555 & ((1 << nc) - 1), 0}):
        Vc, Wc, Hc = run_orth(hk, V, n, nc, k, W, mask, ldh)
        for c in range(nc):
            if (mask >> c) & 1:
                assert np.array_equal(Vc[:, c, k1], Va[:, c, k1]) and np.array_equal(Hc[:, c], Ha[:, c]) and np.array_equal(Wc[:, c], Wa[:, c]), \
                    "a column depends on its neighbours"
            else:
                assert np.all(Vc[:n, c, k1] == 0.0) and np.all(Hc[:k + 2, c] == 0.0) and np.array_equal(Wc[:, c], W[:, c]), "an inactive column"
        assert np.array_equal(Vc[:, :, :k1], V[:, :, :k1]) and np.all(Vc[n:, :, k1] == S) and np.all(Vc[:, :, k1 + 1] == S)
        assert np.all(Hc[k + 2:, :] == S) and np.all(Hc[:, nc] == S) and np.all(Wc[:, nc] == S)
    return worst


def check_start(hk, n, nc, seed=5):
    rng = np.random.default_rng(seed + n + nc)
    ldb, lda, ldv = n + 2, n + 7, n + 3
    B, AX = np.full((ldb, nc), 1e300, order="F"), np.full((lda, nc), 1e300, order="F")
    B[:n], AX[:n] = rng.standard_normal((n, nc)), rng.standard_normal((n, nc))
    if nc > 1:
        AX[:n, nc - 1] = B[:n, nc - 1]                       # a residual that is exactly zero
    dB, dA = hk.array(B), hk.array(AX)
    dV, dN = hk.array(np.full((ldv, nc + 1), S)), hk.array(np.full(nc + 2, S))
    f = hk.lib.hssk_krylov_start
    hk.check(f(hk.ctx, dB.ptr, ldb, dA.ptr, lda, n, nc, dV.ptr, ldv, dN.ptr))
    hk.sync()
    V0, nr = dV.get(), dN.get()
    assert np.all(V0[n:, :] == S) and np.all(V0[:, nc] == S) and np.all(nr[nc:] == S), "hssk_krylov_start wrote outside its block"
    r = B[:n].astype(LD) - AX[:n].astype(LD)
    rn = np.sqrt((r * r).sum(0))
    worst = 0.0
    for c in range(nc):
        if rn[c] == 0:
            assert nr[c] == 0.0 and np.all(V0[:n, c] == 0.0), "a zero residual"
            continue
        e1 = abs(LD(nr[c]) - rn[c]) / ((n + 4) * U * rn[c])
        e2 = (np.abs(V0[:n, c].astype(LD) - r[:, c] / rn[c]) - (n + 6) * U * np.abs(r[:, c]) / rn[c]).max()
        assert e1 <= 1.0 and e2 <= 0.0, (n, nc, c, float(e1), float(e2))
        worst = max(worst, float(e1))
    print("krylov_start n=%d nc=%d: largest norm error / bound %.3g" % (n, nc, worst))
    hk.check(f(hk.ctx, dB.ptr, ldb, dA.ptr, lda, n, nc, dV.ptr, ldv, dN.ptr))
    hk.sync()
    assert np.array_equal(V0, dV.get()) and np.array_equal(nr, dN.get()), "two calls differ"
    for v in (dB, dA, dV, dN):
        v.free()
    return worst


def check_combine(hk, n, nc, kcount, seed=9):
    rng = np.random.default_rng(seed + n + nc + kcount)
    ldv, ldy, ldo = n + 3, kcount + 2, n + 4
    V = np.full((ldv, nc, kcount + 1), 1e300, order="F")
    V[:n, :, :kcount] = rng.standard_normal((n, nc, kcount))
    Y = np.full((ldy, nc), 1e300, order="F")
    Y[:kcount] = rng.standard_normal((kcount, nc))
    O0 = np.full((ldo, nc + 1), S, order="F")
    O0[:n, :nc] = rng.standard_normal((n, nc))
    dV, dY = hk.array(V), hk.array(Y)
    f = hk.lib.hssk_krylov_combine
    prod = V[:n, :, :kcount].astype(LD) * Y[:kcount].T.astype(LD)[None, :, :]
    ref, mag = prod.sum(-1), np.abs(prod).sum(-1)
    for acc in (0, 1):
        for kc in (kcount, 0):
            dO = hk.array(O0)
            hk.check(f(hk.ctx, dV.ptr, ldv, n, nc, kc, dY.ptr, ldy, dO.ptr, ldo, acc))
            hk.sync()
            got = dO.get()
            assert np.all(got[n:, :] == S) and np.all(got[:, nc] == S), "hssk_krylov_combine wrote outside its block"
            if kc == 0:   # zeroed, or not touched
                assert np.array_equal(got[:n, :nc], O0[:n, :nc] if acc else np.zeros((n, nc))), ("kcount = 0", acc)
            else:
                want = ref + (O0[:n, :nc].astype(LD) if acc else 0)
                tol = (kcount + 2) * U * (mag + (np.abs(O0[:n, :nc]) if acc else 0))
                assert np.all(np.abs(got[:n, :nc].astype(LD) - want) <= tol), (n, nc, kcount, acc)
                hk.check(f(hk.ctx, dV.ptr, ldv, n, nc, kc, dY.ptr, ldy, dO.set(O0).ptr, ldo, acc))
                hk.sync()
                assert np.array_equal(got, dO.get()), "two calls differ"
            dO.free()
    for v in (dV, dY):
        v.free()


def check_krylov_refusals(hk):
    """more than 64 columns, a leading dimension below n, a null pointer, a negative k: non-zero, every output untouched;
    n = 0 and nc = 0: nothing to do"""
    n, nc, k = 40, 5, 2
    rng = np.random.default_rng(1)
    V0 = np.full((n, 66, k + 2), S, order="F")
    V0[:, :nc, :k + 1] = rng.standard_normal((n, nc, k + 1))
    W0, H0, N0 = np.full((n, 66), 1.5, order="F"), np.full((k + 2, 66), S), np.full(66, S)
    dV, dW, dH, dN, dB = hk.array(V0), hk.array(W0), hk.array(H0), hk.array(N0), hk.array(rng.standard_normal((n, 66)))
    st, orth, comb = hk.lib.hssk_krylov_start, hk.lib.hssk_krylov_orth, hk.lib.hssk_krylov_combine
    c = hk.ctx
    for rc in (st(c, dB.ptr, n, dB.ptr, n, n, 65, dV.ptr, n, dN.ptr), st(c, dB.ptr, n - 1, dB.ptr, n, n, nc, dV.ptr, n, dN.ptr),
               st(c, dB.ptr, n, dB.ptr, n - 1, n, nc, dV.ptr, n, dN.ptr), st(c, dB.ptr, n, dB.ptr, n, n, nc, dV.ptr, n - 1, dN.ptr),
               st(c, None, n, dB.ptr, n, n, nc, dV.ptr, n, dN.ptr), st(c, dB.ptr, n, None, n, n, nc, dV.ptr, n, dN.ptr),
               st(c, dB.ptr, n, dB.ptr, n, n, nc, None, n, dN.ptr), st(c, dB.ptr, n, dB.ptr, n, n, nc, dV.ptr, n, None),
               st(None, dB.ptr, n, dB.ptr, n, n, nc, dV.ptr, n, dN.ptr), st(c, dB.ptr, n, dB.ptr, n, -1, nc, dV.ptr, n, dN.ptr),
               orth(c, dV.ptr, n, n, 65, k, dW.ptr, n, ALL, dH.ptr, k + 2), orth(c, dV.ptr, n - 1, n, nc, k, dW.ptr, n, ALL, dH.ptr, k + 2),
               orth(c, dV.ptr, n, n, nc, k, dW.ptr, n - 1, ALL, dH.ptr, k + 2), orth(c, dV.ptr, n, n, nc, -1, dW.ptr, n, ALL, dH.ptr, k + 2),
               orth(c, dV.ptr, n, n, nc, k, dW.ptr, n, ALL, dH.ptr, k + 1), orth(c, None, n, n, nc, k, dW.ptr, n, ALL, dH.ptr, k + 2),
               orth(c, dV.ptr, n, n, nc, k, None, n, ALL, dH.ptr, k + 2), orth(c, dV.ptr, n, n, nc, k, dW.ptr, n, ALL, None, k + 2),
               orth(None, dV.ptr, n, n, nc, k, dW.ptr, n, ALL, dH.ptr, k + 2),
               comb(c, dV.ptr, n, n, 65, k, dH.ptr, k + 2, dW.ptr, n, 0), comb(c, dV.ptr, n - 1, n, nc, k, dH.ptr, k + 2, dW.ptr, n, 0),
               comb(c, dV.ptr, n, n, nc, k, dH.ptr, k + 2, dW.ptr, n - 1, 1), comb(c, dV.ptr, n, n, nc, -1, dH.ptr, k + 2, dW.ptr, n, 0),
               comb(c, dV.ptr, n, n, nc, k, dH.ptr, k - 1, dW.ptr, n, 0), comb(c, None, n, n, nc, k, dH.ptr, k + 2, dW.ptr, n, 0),
               comb(c, dV.ptr, n, n, nc, k, None, k + 2, dW.ptr, n, 1), comb(c, dV.ptr, n, n, nc, k, dH.ptr, k + 2, None, n, 0),
               comb(c, dV.ptr, n, n, nc, k, dH.ptr, k + 2, dV.ptr, n, 0), comb(None, dV.ptr, n, n, nc, k, dH.ptr, k + 2, dW.ptr, n, 0)):
        assert rc != 0
    # nothing to do
    assert st(c, None, 0, None, 0, 0, nc, None, 0, None) == 0 and st(c, None, n, None, n, n, 0, None, n, None) == 0
    assert orth(c, None, 0, 0, nc, k, None, 0, ALL, None, k + 2) == 0 and orth(c, None, n, n, 0, k, None, n, ALL, None, k + 2) == 0
    assert comb(c, None, 0, 0, nc, k, None, k, None, 0, 0) == 0 and comb(c, None, n, n, 0, k, None, k, None, n, 1) == 0
    hk.sync()
    assert np.array_equal(dV.get(), V0) and np.array_equal(dW.get(), W0) and np.array_equal(dH.get(), H0) and np.array_equal(dN.get(), N0), \
        "a refused call wrote an output"
    for v in (dV, dW, dH, dN, dB):
        v.free()


# ---- B. the solver against a numpy twin -------------------------------------------------------------------------------------------
def gmres_reference(A, msolve, b, x0, rtol, maxit, restart):
    """right-preconditioned restarted GMRES with CGS2 in float64, one column: the algorithm of Kernel<double>::krylov_block.
    Returns (x, steps, relative residuals at the starts of the cycles)."""
    n, m = len(b), min(restart, maxit)
    x, bn, steps, hist = x0.copy(), np.linalg.norm(b), 0, []
    if bn == 0:
        return np.zeros(n), 0, [0.0]
    while True:
        r = b - A @ x
        rn = np.linalg.norm(r)
        hist.append(rn / bn)
        if rn <= rtol * bn or steps >= maxit:
            return x, steps, hist
        V = np.zeros((n, m + 1))
        V[:, 0] = r / rn
        R, cs, sn, g, kc = np.zeros((m, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1), 0
        g[0] = rn
        for k in range(m):
            w = A @ msolve(V[:, k])
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
            if abs(g[k + 1]) <= rtol * bn or below == 0 or steps >= maxit:
                break
        if kc == 0:
            return x, steps, hist
        y = np.linalg.solve(np.triu(R[:kc, :kc]), g[:kc])
        x = x + msolve(V[:, :kc] @ y)


def exact_matrix(kr, kind):
    X = kr.model_points()
    idx = np.arange(len(X))
    return KC.kernel_np(X, idx, idx, kind[0], kind[2], kr.lam)


_REF = {}


def residual_ld(kr, kind, x, b):
    """(long double relative residual of x, the bound of gpgrad_cases.check_residual for it); the long double kernel matrix of a
    handle is computed once per lambda"""
    X = kr.model_points()
    n, d = X.shape
    key = (kind, kr.lam, hash(X.tobytes()))
    if _REF.get("key") != key:
        _REF.clear()
        _REF["key"], _REF["gb"] = key, GG.g_reference(X, kind[0], kind[2], d, 0, kr.lam)
    g, bp = _REF["gb"]
    x, b = x.astype(LD), b.astype(LD)
    bb = float(np.sqrt((b ** 2).sum()))
    if bb == 0:
        return 0.0, 0.0
    return (float(np.sqrt(((b - g @ x) ** 2).sum())) / bb, float(np.sqrt((GG.product_bound(g, bp, x[:, None]) ** 2).sum())) / bb)


def prediction_check(kr, kind, T, w):
    """decision_function(T) is the prediction sum with the weights w under the bound of gp_cases.check_set_lambda"""
    ktype, p, h = kind
    X = kr.model_points()
    n, d = X.shape
    k, a, A = KC.kernel_ref(np.vstack([X, T]), np.arange(n), n + np.arange(len(T)), ktype, h, 0.0, p)
    aw = np.abs(w).astype(LD)
    bound = aw @ KC.kernel_entry_bound(a, A, ktype, d, 0.0, p) + n * U * (aw @ np.abs(k))
    assert np.all(np.abs(kr.decision_function(T).astype(LD) - w.astype(LD) @ k) <= bound), "predict does not use the new weights"


REFINE_CASES = [("gauss", 8, 4.0, 1.0, 30), ("laplace", 8, 0.05, 1.0, 30), ("gauss", 8, 0.05, 0.5, 30), ("gauss", 33, 4.0, 1.0, 30),
                ("laplace", 8, 0.05, 1.0, 5), ("gauss", 1, 0.05, 1.0, 30), ("gauss", 1, 0.05, 1.0, 10)]
RTOL = 1e-10


def check_refined(kr, kind, Hd, T, rtol, maxit, restart, tag):
    """one refine call on a kept model whose weights are the compressed ones: every statement of the issue's list"""
    y, w0, ld = kr.model_labels(), kr.weights(), kr.logabsdet()
    before = kr.fit_residual()
    print("refine %s: fit_residual before %.3g" % (tag, before))
    assert before >= 1e3 * rtol, (tag, before)
    Kd = exact_matrix(kr, kind)
    _, ref_its, _ = gmres_reference(Kd, lambda v: np.linalg.solve(Hd, v), y, w0, rtol, maxit, restart)
    info = kr.refine(rtol=rtol, maxit=maxit, restart=restart)
    w = kr.weights()
    r_ld, bound = residual_ld(kr, kind, w, y)
    print("refine %s restart %d: %d steps (twin %d), %d products, %d solves, %d cycles, residual %.3g -> %.3g (long double %.3g, bound %.3g)"
          % (tag, restart, info["iterations"], ref_its, info["products"], info["solves"], info["cycles"], info["residual0"],
             info["residual"], r_ld, bound))
    assert info["converged"], tag
    assert info["iterations"] <= ref_its + 2, (tag, info["iterations"], ref_its)
    assert info["iterations"] == info["its"] and info["products"] == info["iterations"] + info["cycles"] + 1
    assert abs(info["residual0"] - before) <= 2 * bound + 1e-12 * before
    assert abs(info["residual"] - r_ld) <= bound, (tag, info["residual"], r_ld, bound)
    assert r_ld <= rtol + bound, (tag, r_ld, bound)
    GG.check_residual(kr, kind, tag, visible=False)                 # fit_residual() is that value now
    sv = np.linalg.svd(Kd, compute_uv=False)
    ae = np.linalg.solve(Kd, y)
    fe, fb = np.linalg.norm(w - ae) / np.linalg.norm(ae), (sv[0] / sv[-1]) * (rtol + bound + GP.EPS_F)
    print("refine %s: forward error %.3g bound %.3g" % (tag, fe, fb))
    assert fe <= fb, (tag, fe, fb)
    prediction_check(kr, kind, T, w)
    assert kr.logabsdet() == ld, "refine changed the log-determinant"
    lml = kr.log_marginal_likelihood()
    ref = -0.5 * float((y.astype(LD) * w.astype(LD)).sum()) - 0.5 * ld - 0.5 * len(y) * np.log(2.0 * np.pi)
    assert abs(lml - ref) <= 1e-13 * (abs(ref) + abs(ld)), "the likelihood does not use the new weights"
    again = kr.refine(rtol=rtol, maxit=maxit, restart=restart)
    assert again["converged"] and again["iterations"] == 0 and again["products"] == 1 and again["cycles"] == 0, again
    assert np.array_equal(kr.weights(), w)
    ms = kr.krylov_ms()
    assert set(ms) == {"product_ms", "solve_ms", "krylov_ms"}
    return info


def check_refine(KM, lib, kern, d, lam, hscale, restart, path):
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    try:
        Hd, _, _ = GP.dense_model(kr, path)
        check_refined(kr, kind, Hd, T, RTOL, 100, restart, "%s R^%d lambda=%g h=%.3g" % (kern, d, lam, kind[2]))
    finally:
        kr.destroy()


def check_no_convergence(KM, lib):
    """Gauss R^1 at restart 5 stagnates (the twin is at 5.5e-3 after 200 steps): 40 steps, not converged, no error, a true residual
    that is not above the first one, the weights the last iterate"""
    kr, T, kind = GP.fit_model(KM, lib, "gauss", 1, 0.05, 1.0)
    try:
        y, w0 = kr.model_labels(), kr.weights()
        buf = np.full(10, 123.25)
        rc = lib.SPX_kernel_model_refine(kr.K, RTOL, 40, 5, buf.ctypes.data)
        assert rc == 0 and buf[0] == 0.0 and buf[1] == 40 and buf[9] == 40 and buf[7] == 1, buf
        w = kr.weights()
        assert not np.array_equal(w, w0)
        r_ld, bound = residual_ld(kr, kind, w, y)
        print("no convergence: residual %.3g -> %.3g (long double %.3g, bound %.3g), %d products, %d cycles" % (buf[5], buf[6], r_ld, bound, buf[2], buf[4]))
        assert abs(buf[8] - r_ld) <= bound and buf[6] == buf[8] and buf[8] <= buf[5] and r_ld > RTOL
        assert buf[2] == 40 + buf[4] + 1 and buf[4] == 8
        GG.check_residual(kr, kind, "after 40 steps", visible=True)
        prediction_check(kr, kind, T, w)
    finally:
        kr.destroy()


def check_solve(KM, lib, path):
    """m = 3 (the labels, a random column, an exactly zero column) and m = 70 (blocks of 64 + 6) on one kept fit"""
    kr, T, kind = GP.fit_model(KM, lib, "laplace", 8, 0.05, 1.0)
    try:
        Hd, _, _ = GP.dense_model(kr, path)
        Kd = exact_matrix(kr, kind)
        sv = np.linalg.svd(Kd, compute_uv=False)
        cond = sv[0] / sv[-1]
        y, w0, ld = kr.model_labels(), kr.weights(), kr.logabsdet()
        rng = np.random.default_rng(77)
        n = kr.n
        lu = sla.lu_factor(Hd)
        msolve = lambda v: sla.lu_solve(lu, v)      # noqa: E731
        for m in (3, 70):
            B = np.asfortranarray(rng.standard_normal((n, m)))
            if m == 3:
                B[:, 0], B[:, 2] = y, 0.0
            X, info = kr.solve(B, rtol=RTOL)
            assert np.all(np.isfinite(X)) and info["converged"] and len(info["residual"]) == m and len(info["its"]) == m
            Xe = np.linalg.solve(Kd, B)
            twin = 0
            for c in range(m):
                if not B[:, c].any():
                    assert np.all(X[:, c] == 0.0) and info["its"][c] == 0 and info["residual"][c] == 0.0, "the zero column"
                    continue
                r_ld, bound = residual_ld(kr, kind, X[:, c], B[:, c])
                assert abs(info["residual"][c] - r_ld) <= bound and r_ld <= RTOL + bound, (m, c, info["residual"][c], r_ld, bound)
                fe = np.linalg.norm(X[:, c] - Xe[:, c]) / np.linalg.norm(Xe[:, c])
                assert fe <= cond * (RTOL + bound + GP.EPS_F), (m, c, fe)
                _, its, _ = gmres_reference(Kd, msolve, B[:, c], msolve(B[:, c]), RTOL, 100, 30)      # (the twin on that column alone)
                assert info["its"][c] <= its + 2, (m, c, info["its"][c], its)
                twin = max(twin, its)
            print("solve m=%d: %d steps at most (twin %d), %d products, %d solves, %d cycles"
                  % (m, info["iterations"], twin, info["products"], info["solves"], info["cycles"]))
            assert info["iterations"] == info["its"].max()
        x1, i1 = kr.solve(y, rtol=RTOL)                  # a vector in, a vector out
        assert x1.shape == (n,) and i1["converged"]
        assert np.array_equal(kr.weights(), w0) and kr.logabsdet() == ld, "solve disturbed the model"
        for bad in (np.ones((n - 1, 2)), np.ones(n + 1)):
            try:
                kr.solve(bad)
                raise AssertionError("a block of %s rows was accepted" % (bad.shape,))
            except ValueError:
                pass
    finally:
        kr.destroy()


def check_after_set_lambda(KM, lib, path):
    """Gauss R^8, lambda 4 -> 0.05 at half the width: refine, set_lambda (the compressed weights and their residual are back),
    refine for the new lambda against a Kd with the new lambda"""
    kr, T, kind = GP.fit_model(KM, lib, "gauss", 8, 4.0, 0.5)
    try:
        first = kr.refine(rtol=RTOL)
        assert first["converged"]
        kr.set_lambda(0.05)
        Hd, _, _ = GP.dense_model(kr, path)
        y, w = kr.model_labels(), kr.weights()
        F = np.linalg.norm
        assert F(Hd @ w - y) <= 1e-10 * (np.linalg.norm(Hd, 2) * F(w) + F(y)), "the weights after set_lambda are not the compressed solve"
        check_refined(kr, kind, Hd, T, RTOL, 100, 30, "gauss R^8 lambda 4 -> 0.05")      # (asserts the visible residual first)
    finally:
        kr.destroy()


def solve_calls(lib, Kh, n, d, m=3, rtol=1e-8, maxit=100, restart=30):
    """the four new calls on the raw handle with pre-filled outputs: [(name, return code, outputs untouched)]"""
    res = []
    info = np.full(8 + 2 * m, 123.25)
    rc = lib.SPX_kernel_model_refine(Kh, rtol, maxit, restart, info.ctypes.data)
    res.append(("model_refine", rc, bool(np.all(info == 123.25))))
    B, X = np.ones((n, m), order="F"), np.full((n, m), 123.25, order="F")
    rc = lib.SPX_kernel_model_solve(Kh, m, B.ctypes.data, n, X.ctypes.data, n, rtol, maxit, restart, info.ctypes.data)
    res.append(("model_solve", rc, bool(np.all(X == 123.25) and np.all(info == 123.25))))
    T, var = np.ones((m, d)), np.full(m, 123.25)
    rc = lib.SPX_kernel_predict_variance_exact_double(Kh, m, T.ctypes.data, var.ctypes.data, rtol, maxit, restart, info.ctypes.data)
    res.append(("predict_variance_exact", rc, bool(np.all(var == 123.25) and np.all(info == 123.25))))
    ms = np.full(3, 123.25)
    res.append(("krylov_ms", lib.SPX_kernel_krylov_ms(Kh, ms.ctypes.data), bool(np.all(ms == 123.25))))
    return res


def check_solve_lifecycle(KM, lib):
    n, d = 300, 8
    X, y, _ = GP.model_data(d, n, 20)
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]
    plain = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y)
    for name, rc, untouched in solve_calls(lib, plain.K, n, d):
        assert rc != 0 and untouched, ("no keep_model", name, rc)
    for call in (plain.refine, lambda: plain.solve(np.ones(n)), lambda: plain.predict_variance(X[:3], exact=True), plain.krylov_ms):
        try:
            call()
            raise AssertionError("a handle without a kept model answered")
        except RuntimeError:
            pass
    plain.destroy()
    kf = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X.astype(np.float32), y.astype(np.float32))
    for name, rc, untouched in solve_calls(lib, kf.K, n, d):
        assert rc != 0 and untouched, ("float handle", name, rc)
    kf.destroy()
    ka = KM.KernelRegression(lib, h=h, lam=4.0, kernel="ANOVA", degree=2, argv=args, keep_model=True).fit(X, y)
    lda, wa = ka.logabsdet(), ka.weights()
    for name, rc, untouched in solve_calls(lib, ka.K, n, d):
        assert rc != 0 and untouched, ("ANOVA", name, rc)
    assert ka.logabsdet() == lda and np.array_equal(ka.weights(), wa)
    ka.destroy()
    kr = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    ld, w = kr.logabsdet(), kr.weights()
    for bad in (dict(rtol=0.0), dict(rtol=-1e-8), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(maxit=0), dict(restart=0),
                dict(maxit=-3), dict(restart=-1)):
        for name, rc, untouched in solve_calls(lib, kr.K, n, d, **bad):
            if name != "krylov_ms":      # (the one call of the four that takes none of rtol / maxit / restart)
                assert rc != 0 and untouched, (bad, name, rc)
        for call in (lambda: kr.refine(**bad), lambda: kr.solve(np.ones(n), **bad), lambda: kr.predict_variance(X[:3], exact=True, **bad)):
            try:
                call()
                raise AssertionError("%s was accepted" % (bad,))
            except RuntimeError:
                pass
    info = np.full(14, 123.25)
    B, Xo = np.ones((n, 3), order="F"), np.full((n, 3), 123.25, order="F")
    assert lib.SPX_kernel_model_solve(kr.K, 3, B.ctypes.data, n - 1, Xo.ctypes.data, n, 1e-8, 100, 30, info.ctypes.data) != 0
    assert lib.SPX_kernel_model_solve(kr.K, 3, B.ctypes.data, n, Xo.ctypes.data, n - 1, 1e-8, 100, 30, info.ctypes.data) != 0
    assert lib.SPX_kernel_model_solve(kr.K, 3, None, n, Xo.ctypes.data, n, 1e-8, 100, 30, info.ctypes.data) != 0
    assert lib.SPX_kernel_model_solve(kr.K, -1, B.ctypes.data, n, Xo.ctypes.data, n, 1e-8, 100, 30, info.ctypes.data) != 0
    assert np.all(Xo == 123.25) and np.all(info == 123.25)
    assert kr.logabsdet() == ld and np.array_equal(kr.weights(), w), "a refused call disturbed the model"
    for name, rc, untouched in solve_calls(lib, kr.K, n, d):
        assert rc == 0 and not untouched, (name, rc)
    assert lib.SPX_kernel_model_refine(kr.K, 1e-8, 100, 30, None) == 0          # info may be NULL
    assert kr.logabsdet() == ld
    assert lib.SPX_kernel_keep_model(kr.K, 0) == 0
    for name, rc, untouched in solve_calls(lib, kr.K, n, d):
        assert rc != 0 and untouched, ("after keep_model(false)", name, rc)
    kr.destroy()


# ---- C. the exact variance --------------------------------------------------------------------------------------------------------
VARIANCE_CASES = [("gauss", 1, 0.05, 1.0), ("laplace", 8, 0.05, 1.0), ("gauss", 8, 0.05, 0.5)]


def check_variance_exact(KM, lib, kern, d, lam, hscale, m_test=GP.M_TEST):
    """m_test: the last m_test of the 130 test points of gp_cases.model_data (the GPU tier: all of them, three chunks)"""
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    T = T[-m_test:]
    tag = "%s R^%d lambda=%g h=%.3g" % (kern, d, lam, kind[2])
    try:
        Kd = exact_matrix(kr, kind)
        sv = np.linalg.svd(Kd, compute_uv=False)
        ref, bound = GP.variance_reference(kr, Kd, sv, T, kind)
        # (the forward-error term of that bound is EPS_F cond nk nz: add the residual's share)
        ktype, p, h = kind
        X = kr.model_points()
        n = len(X)
        kt = np.asarray(KC.kernel_ref(np.vstack([X, T]), np.arange(n), n + np.arange(len(T)), ktype, h, 0.0, p)[0], dtype=np.float64)
        bound = bound + RTOL * np.linalg.norm(kt, axis=0) ** 2 / sv[-1]
        comp = kr.predict_variance(T)
        assert np.array_equal(comp, kr.predict_variance(T, exact=False))
        got, info = kr.predict_variance(T, exact=True, rtol=RTOL, info=True)
        err = np.abs(got - ref)
        gap = float(np.abs(got - comp).max())
        print("exact variance %s: in [%.3g, %.3g] (compressed in [%.3g, %.3g]), largest error %.3g, largest bound %.3g, gap to the "
              "compressed values %.3g; %d steps, %d products, %d solves" % (tag, ref.min(), ref.max(), comp.min(), comp.max(), err.max(),
                                                                           bound.max(), gap, info["iterations"], info["products"], info["solves"]))
        assert info["converged"] and len(info["its"]) == len(T)
        assert np.all(err <= bound), (tag, float((err / bound).max()))
        assert np.all(got >= -bound), (tag, float(got.min()))
        assert gap >= 1e3 * bound.max(), (tag, gap, bound.max())
        after = kr.predict_variance(T)
        assert np.array_equal(comp, after) and np.array_equal(comp, kr.predict_variance(T, exact=False)), "the compressed variance changed"
        assert np.array_equal(got, kr.predict_variance(T, exact=True, rtol=RTOL)), "two exact variance calls differ"
        assert len(kr.predict_variance(T[:0], exact=True)) == 0
    finally:
        kr.destroy()
