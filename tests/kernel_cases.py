"""Kernel-level parity cases shared by the GPU tests (product library, `-m gpu`) and the CPU tests
(the same kernel sources on the fiber emulator, tests/emu).  Every case drives a hssk_* entry point
of include/hssk.h and compares with numpy/LAPACK (the oracle of each dense primitive)."""
import ctypes as C

import numpy as np
import scipy.linalg as sla

from strumpack_amd import hssk as K
from strumpack_amd import hssk as K_


def rng(seed=0):
    return np.random.default_rng(seed)


def case_gemm_vbatched(hk, shapes, seed=0, even_ld=False):
    r = rng(seed)
    descs, keep, expect = [], [], []
    for (m, n, k, ta, tb, alpha, beta) in shapes:
        A = r.standard_normal((k, m) if ta else (m + (2 if even_ld else 0), k))
        B = r.standard_normal((n, k) if tb else (k, n))
        Cm = r.standard_normal((m + 3, n))  # ldc = m + 3
        dA, dB, dC = hk.array(A), hk.array(B), hk.array(Cm)
        keep += [dA, dB, dC]
        descs.append(K.GemmDesc(dA.ptr, dB.ptr, dC.ptr, m, n, k, max(A.shape[0], 1),
                                max(B.shape[0], 1), m + 3, int(ta), int(tb), alpha, beta))
        ref = Cm.copy()
        opA = A.T if ta else A[:m]
        opB = B.T if tb else B
        ref[:m] = alpha * (opA @ opB) + (beta * Cm[:m] if beta != 0 else 0)
        expect.append(ref)
    hk.batch("hssk_gemm_vbatched", descs)
    hk.sync()
    for (dC, ref, sh) in zip(keep[2::3], expect, shapes):
        got = dC.get()
        scale = max(1.0, np.abs(ref).max())
        assert np.abs(got - ref).max() <= 1e-12 * scale * max(sh[2], 1), f"gemm {sh}"


def case_leaf_update(hk, shapes, seed=12):
    """Fused leaf sample update vs numpy: Sr -= R D^T, Sc -= R D."""
    r = rng(seed)
    descs, keep = [], []
    for (d, m) in shapes:
        R, D = r.standard_normal((d + 2, m)), r.standard_normal((m, m))
        Sr, Sc = r.standard_normal((d + 2, m)), r.standard_normal((d + 2, m))
        dR, dD, dSr, dSc = hk.array(R), hk.array(D), hk.array(Sr), hk.array(Sc)
        keep.append((R, D, Sr, Sc, dSr, dSc, dR, dD, d))
        descs.append(K.LeafUpdateDesc(dR.ptr, dD.ptr, dSr.ptr, dSc.ptr, d, m, d + 2, m, d + 2))
    hk.batch("hssk_leaf_update_vbatched", descs)
    hk.sync()
    for (R, D, Sr, Sc, dSr, dSc, _, _, d) in keep:
        er, ec = Sr.copy(), Sc.copy()
        er[:d] -= R[:d] @ D.T
        ec[:d] -= R[:d] @ D
        assert np.allclose(dSr.get(), er, atol=1e-11) and np.allclose(dSc.get(), ec, atol=1e-11)


def case_dgemm(hk, m, n, k, transB, alpha=1.0, beta=0.0, lda_pad=5, seed=1, ldb_pad=1):
    r = rng(seed)
    A = r.standard_normal((m + lda_pad, k))
    B = r.standard_normal((n + ldb_pad, k)) if transB else r.standard_normal((k + ldb_pad, n))
    Cm = r.standard_normal((m + 2, n))
    dA, dB, dC = hk.array(A), hk.array(B), hk.array(Cm)
    hk.check(hk.lib.hssk_dgemm(hk.ctx, int(transB), m, n, k, alpha, dA.ptr, A.shape[0], dB.ptr,
                               B.shape[0], beta, dC.ptr, Cm.shape[0]))
    hk.sync()
    opB = B[:n].T if transB else B[:k]
    ref = Cm.copy()
    ref[:m] = alpha * (A[:m] @ opB) + (beta * Cm[:m] if beta != 0 else 0)
    got = dC.get()
    assert np.abs(got - ref).max() <= 1e-13 * max(k, 1) * max(1.0, np.abs(ref).max()), \
        f"dgemm m={m} n={n} k={k} transB={transB}"


def case_sjlt(hk, n_out, K, dn, nnz, seed=3):
    """hssk_sjlt_dense / hssk_sjlt_sketch against numpy: S = op(A) R for a random +-1 pattern with nnz entries per
    row (matrix_times_SJLT / matrixT_times_SJLT / SJLT_to_dense, HSS/HSSMatrix.sketch.hpp)."""
    r = rng(seed)
    cols = np.stack([r.permutation(dn)[:nnz] for _ in range(K)], axis=1).astype(np.int64)   # nnz x K, distinct per row
    neg = r.integers(0, 2, size=(nnz, K)).astype(bool)
    nq = 4 if nnz <= 4 else 8
    pat = np.full((K, nq), dn, dtype=np.int64)                # unused entries point at column dn
    pat[:, :nnz] = (cols | (neg.astype(np.int64) << 31)).T
    pat = pat.astype(np.uint32).view(np.int32)
    R = np.zeros((K, dn))
    for q in range(nnz):
        R[np.arange(K), cols[q]] = np.where(neg[q], -1.0, 1.0)
    dpat = hk.array(np.ascontiguousarray(pat).reshape(-1), dtype=np.int32)
    ld = dn + 3
    dRt = hk.array(np.full((ld, K), -7.0))
    hk.check(hk.lib.hssk_sjlt_dense(hk.ctx, dRt.ptr, dn, K, ld, dpat.ptr, nnz))
    hk.sync()
    got = dRt.get()
    assert np.array_equal(got[:dn], R.T) and np.all(got[dn:] == -7.0)
    for trans in (0, 1):
        A = r.standard_normal((n_out + 2, K)) if trans == 0 else r.standard_normal((K + 2, n_out))
        dA = hk.array(A)
        dS = hk.array(np.full((ld, n_out), -3.0))
        hk.check(hk.lib.hssk_sjlt_sketch(hk.ctx, trans, n_out, K, dA.ptr, A.shape[0], dpat.ptr, nnz, dn, dS.ptr, ld))
        hk.sync()
        ref = (A[:n_out] @ R).T if trans == 0 else (A[:K].T @ R).T
        got = dS.get()
        assert np.all(got[dn:] == -3.0)
        assert np.abs(got[:dn] - ref).max() <= 1e-13 * K * max(1.0, np.abs(ref).max()), f"sjlt trans={trans}"


def case_toeplitz_randn(hk, n=70):
    dA = hk.empty((n + 2, n))
    dA.set(np.full((n + 2, n), -7.0))
    for kind in ("T", "U"):
        hk.check(hk.lib.hssk_fill_toeplitz(hk.ctx, dA.ptr, n, n + 2, kind.encode()))
        hk.sync()
        i = np.arange(n)
        ref = 1.0 / (1.0 + np.abs(i[:, None] - i[None, :]))
        if kind == "U":
            ref = np.triu(ref)
        got = dA.get()
        assert np.array_equal(got[:n], ref) and np.all(got[n:] == -7.0)
    rows, cols, ld = 24, 4000, 32
    dP = hk.empty((ld, cols))
    dP.set(np.zeros((ld, cols)))
    hk.check(hk.lib.hssk_randn(hk.ctx, dP.ptr, rows, cols, ld, 0, cols, 42))
    hk.sync()
    P = dP.get()
    assert np.all(P[rows:] == 0)
    x = P[:rows].ravel()
    assert abs(x.mean()) < 0.02 and abs(x.std() - 1) < 0.02 and abs((x ** 3).mean()) < 0.05
    # counter-based: a sub-panel regenerated with a row offset reproduces the same numbers
    dQ = hk.empty((8, cols))
    hk.check(hk.lib.hssk_randn(hk.ctx, dQ.ptr, 8, cols, 8, 16, cols, 42))
    hk.sync()
    assert np.array_equal(dQ.get(), P[16:24])


def case_gathers(hk, seed=3):
    r = rng(seed)
    src = r.standard_normal((37, 50))
    idx = r.permutation(50)[:21].astype(np.int32)
    dS, dI = hk.array(src), hk.array(idx)
    dD = hk.array(np.zeros((40, 21)))
    hk.batch("hssk_gather_cols", [K.ColGatherDesc(dS.ptr, dD.ptr, dI.ptr, 37, 21, 37, 40, 0)])
    hk.sync()
    assert np.array_equal(dD.get()[:37], src[:, idx])
    dD2 = hk.array(np.zeros((37, 50)))
    hk.batch("hssk_gather_cols", [K.ColGatherDesc(dD.ptr, dD2.ptr, dI.ptr, 37, 21, 40, 37, 1)])
    hk.sync()
    ref = np.zeros((37, 50))
    ref[:, idx] = src[:, idx]
    assert np.array_equal(dD2.get(), ref)
    # rows
    ridx = r.permutation(37)[:15].astype(np.int32)
    dR = hk.array(ridx)
    dE = hk.array(np.ones((15, 50)))
    hk.batch("hssk_gather_rows", [K.RowGatherDesc(dS.ptr, dE.ptr, dR.ptr, 15, 50, 37, 15, 0, 1)])
    hk.sync()
    assert np.allclose(dE.get(), 1 + src[ridx])
    dF = hk.array(np.zeros((37, 50)))
    hk.batch("hssk_gather_rows", [K.RowGatherDesc(dE.ptr, dF.ptr, dR.ptr, 15, 50, 15, 37, 1, 0)])
    hk.sync()
    ref = np.zeros((37, 50))
    ref[ridx] = 1 + src[ridx]
    assert np.allclose(dF.get(), ref)
    # elements
    Ii = r.permutation(37)[:9].astype(np.int32)
    Jj = r.permutation(50)[:13].astype(np.int32)
    dIi, dJj = hk.array(Ii), hk.array(Jj)
    dB = hk.array(np.zeros((9, 13)))
    dBt = hk.array(np.zeros((13, 9)))
    dBc = hk.array(np.zeros((10, 12)))
    hk.batch("hssk_gather_elems", [
        K.ElemDesc(dS.ptr, 37, dIi.ptr, dJj.ptr, 0, 0, dB.ptr, 9, 13, 9, 0),
        K.ElemDesc(dS.ptr, 37, dIi.ptr, dJj.ptr, 0, 0, dBt.ptr, 9, 13, 13, 1),
        K.ElemDesc(dS.ptr, 37, None, None, 5, 7, dBc.ptr, 10, 12, 10, 0)])
    hk.sync()
    assert np.array_equal(dB.get(), src[np.ix_(Ii, Jj)])
    assert np.array_equal(dBt.get(), src[np.ix_(Ii, Jj)].T)
    assert np.array_equal(dBc.get(), src[5:15, 7:19])
    # large transposed gathers take the tiled kernel (64 x 32 tiles through the LDS): ragged edges, permuted rows, a window
    big = r.standard_normal((150, 130))
    dG = hk.array(big)
    Ib = r.permutation(150)[:101].astype(np.int32)
    dIb = hk.array(Ib)
    dT1 = hk.array(np.full((75, 101), 7.0))     # ldb 75 > n = 70
    dT2 = hk.array(np.zeros((130, 150)))
    dT3 = hk.array(np.zeros((40, 101)))
    hk.batch("hssk_gather_elems", [
        K.ElemDesc(dG.ptr, 150, dIb.ptr, None, 0, 20, dT1.ptr, 101, 70, 75, 1),
        K.ElemDesc(dG.ptr, 150, None, None, 0, 0, dT2.ptr, 150, 130, 130, 1),
        K.ElemDesc(dG.ptr, 150, dIb.ptr, None, 0, 33, dT3.ptr, 101, 40, 40, 1, 10, 90, 40, 60),
        K.ElemDesc(dS.ptr, 37, dIi.ptr, dJj.ptr, 0, 0, dB.ptr, 9, 13, 9, 0)])
    hk.sync()
    t1 = dT1.get()
    assert np.array_equal(t1[:70], big[Ib][:, 20:90].T) and np.all(t1[70:] == 7.0)
    assert np.array_equal(dT2.get(), big.T)
    ref3 = big[Ib][:, 33:73].copy()
    ref3[(Ib < 10) | (Ib >= 90), :] = 0.
    cols = np.arange(33, 73)
    ref3[:, (cols < 40) | (cols >= 60)] = 0.
    assert np.array_equal(dT3.get(), ref3.T)
    assert np.array_equal(dB.get(), src[np.ix_(Ii, Jj)])
    # transpose
    dT = hk.array(np.zeros((52, 37)))
    hk.batch("hssk_transpose", [K.TransposeDesc(dS.ptr, dT.ptr, 37, 50, 37, 52)])
    hk.sync()
    assert np.array_equal(dT.get()[:50], src.T)
    # sumsq + shift
    dO = hk.array(np.zeros(1))
    hk.batch("hssk_sumsq_vbatched", [K.NormDesc(dS.ptr, 30, 50, 37, dO.ptr)])
    hk.sync()
    assert np.isclose(dO.get()[0], (src[:30] ** 2).sum())
    sq = r.standard_normal((12, 12))
    dQ = hk.array(sq)
    arr = (K.ShiftDesc * 1)(K.ShiftDesc(dQ.ptr, 12, 12))
    hk.check(hk.lib.hssk_shift_diag(hk.ctx, arr, 1, 2.5))
    hk.sync()
    assert np.allclose(dQ.get(), sq + 2.5 * np.eye(12))


def _lowrank(r, d, m, rank, decay=1e-9):
    U = r.standard_normal((d, rank))
    V = r.standard_normal((rank, m))
    s = np.logspace(0, np.log10(decay), rank)
    return (U * s) @ V


def case_id(hk, problems, seed=5, deferred=False):
    """problems: list of (d, m, rtol, atol, max_rank, numerical_rank or None).
    deferred: the panel is read in place from a separate source array (desc.src, left untouched) and X is computed by
    hssk_id_xsolve_vbatched into a compact array after the ranks have been read back (desc.defer_x)."""
    r = rng(seed)
    descs, keep = [], []
    for (d, m, rtol, atol, mr, nr) in problems:
        Wm = r.standard_normal((d, m)) if nr is None else _lowrank(r, d, m, nr)
        ld = d + 2
        Wp = np.zeros((ld, m))
        Wp[:d] = Wm
        dperm, drank, dwork = hk.empty((m,), np.int32), hk.empty((1,), np.int32), hk.empty((3 * m,))
        if deferred:
            lds = d + 5
            Sp = np.full((lds, m), 7.0)
            Sp[:d] = Wm
            dS = hk.array(Sp)
            dW = hk.array(np.zeros((ld, m)))
            keep.append((Wm, dW, dperm, drank))
            keep.append((dwork, dS, Sp))
            descs.append(K.IdDesc(dW.ptr, ld, d, m, rtol, atol, mr, dperm.ptr, drank.ptr, dwork.ptr, dS.ptr, lds, 1))
        else:
            dW = hk.array(Wp)
            keep.append((Wm, dW, dperm, drank))
            keep.append(dwork)
            descs.append(K.IdDesc(dW.ptr, ld, d, m, rtol, atol, mr, dperm.ptr, drank.ptr, dwork.ptr))
    hk.batch("hssk_id_vbatched", descs)
    hk.sync()
    xs = {}
    if deferred:
        dmax, mmax = max(p[0] for p in problems), max(p[1] for p in problems)
        solved = int(hk.lib.hssk_id_solves_inline(dmax, mmax))
        xd = []
        for i, (prob, (Wm, dW, dperm, drank)) in enumerate(zip(problems, keep[0::2])):
            assert np.array_equal(keep[2 * i + 1][1].get(), keep[2 * i + 1][2]), "the source panel was modified"
            rank, m = int(drank.get()[0]), prob[1]
            if rank == 0 or rank == m:
                continue
            dX = hk.array(np.full((rank + 1, m - rank), -3.0))
            xs[i] = dX
            xd.append(K.XsolveDesc(dW.ptr, prob[0] + 2, rank, m, dX.ptr, rank + 1, solved))
        if xd:
            hk.batch("hssk_id_xsolve_vbatched", xd)
            hk.sync()
    for i, (prob, (Wm, dW, dperm, drank)) in enumerate(zip(problems, keep[0::2])):
        d, m, rtol, atol, mr, nr = prob
        rank = int(drank.get()[0])
        perm = dperm.get()
        assert sorted(perm.tolist()) == list(range(m)), "perm is not a permutation"
        # reference: LAPACK QRCP with the same stopping rule (dgeqp3tol.f:225-232)
        R, jp = sla.qr(Wm, mode="r", pivoting=True)
        dg = np.abs(np.diag(R))
        kk = min(d, m)
        rr = kk
        for c in range(kk):
            ratio = dg[c] / dg[0] if dg[0] != 0 else np.nan
            if ratio <= rtol or dg[c] <= atol:
                rr = c
                break
        rr = min(rr, mr)
        assert abs(rank - rr) <= (1 if rr > 0 else 0), f"rank {rank} vs LAPACK {rr} for {prob}"
        if rank == 0:
            continue
        if deferred and i in xs:
            Xf = xs[i].get()
            assert np.all(Xf[rank:] == -3.0)
            X = Xf[:rank]
        else:
            X = dW.get()[:rank, rank:]
        # interpolation property: W[:, perm[rank:]] ~= W[:, perm[:rank]] X
        skel = Wm[:, perm[:rank]]
        rest = Wm[:, perm[rank:]]
        err = np.linalg.norm(rest - skel @ X) / max(np.linalg.norm(Wm), 1e-300)
        # residual is bounded by the first rejected pivot (times a modest growth factor)
        bound = (max(rtol * dg[0], atol, dg[min(rank, kk - 1)]) if rank < kk else 1e-13 * dg[0]) \
            * np.sqrt(m) * 4 / max(np.linalg.norm(Wm), 1e-300)
        assert err <= max(bound, 1e-12), f"ID residual {err} > {bound} for {prob}"
        assert X.size == 0 or np.abs(X).max() < 1e3


def case_gram_pchol_id(hk, problems, seed=41):
    """The ID of tall panels from their Gram matrix: hssk_gram_vbatched over row chunks + hssk_sum_partials give W^T W
    (against numpy), hssk_pchol_id_vbatched the pivots / rank / [R11 R12] of the column-pivoted QR with the reference's
    stopping rule (against LAPACK's QRCP of W itself), hssk_id_xsolve_vbatched the interpolation matrix.
    problems: list of (d, m, rtol, atol, max_rank, numerical_rank or None, chunks).
    The partial products and their sum have a leading dimension of m + 1 and are NaN-filled: row m must stay NaN.  On top of
    the flat tolerance, entrywise |G - G_ref| <= (d + 2) u |W|^T |W| against the np.longdouble product (a sum of d products
    whatever the chunking: a chunk of r rows and the sum of c partials round r + c - 1 <= d + 1 times).  Returns error / bound."""
    r = rng(seed)
    worst = 0.0
    gd, sd, pd, keep = [], [], [], []
    for (d, m, rtol, atol, mr, nr, chunks) in problems:
        Wm = r.standard_normal((d, m)) if nr is None else _lowrank(r, d, m, nr) + 1e-9 * r.standard_normal((d, m))
        ldw = d + 3
        Wp = np.full((ldw, m), 5.0)
        Wp[:d] = Wm
        dW = hk.array(Wp)
        rows = -(-d // chunks)
        nch = -(-d // rows)
        ldg = m + 1
        dP = hk.array(np.full((ldg * m * nch,), np.nan))
        dG = None
        for c in range(nch):
            kr = min(rows, d - c * rows)
            gd.append(K.GramDesc(dW.ptr + 8 * c * rows, ldw, kr, m, dP.ptr + 8 * c * ldg * m, ldg))
        cap = int(hk.lib.hssk_pchol_id_rank_cap(m))
        dperm, drank, dR = hk.empty((m,), np.int32), hk.empty((1,), np.int32), hk.array(np.full((cap, m), -3.0))
        keep.append((Wm, dW, dP, dG, dperm, drank, dR, cap, nch))
    hk.batch("hssk_gram_vbatched", gd)
    hk.sync()
    # the partial products, then their sum into a contiguous m x m matrix per problem
    sums, outs = [], []
    for (prob, kp) in zip(problems, keep):
        d, m = prob[0], prob[1]
        Wm, dW, dP, dG, dperm, drank, dR, cap, nch = kp
        dGc = hk.array(np.full(((m + 1) * m,), np.nan))
        outs.append(dGc)
        sums.append(K.SumDesc(dP.ptr, (m + 1) * m, (m + 1) * m, nch, dGc.ptr))
    hk.batch("hssk_sum_partials", sums)
    hk.sync()
    for (prob, kp, dGc) in zip(problems, keep, outs):
        d, m, rtol, atol, mr, nr, chunks = prob
        Wm, dW, dP, dG, dperm, drank, dR, cap, nch = kp
        assert np.all(np.isnan(dP.get().reshape(m + 1, m * nch, order="F")[m])), "a partial product wrote into its padding row"
        Gp = dGc.get().reshape(m + 1, m, order="F")
        assert np.all(np.isnan(Gp[m])), "padding row of the Gram matrix"
        G = Gp[:m]
        Gref = Wm.T @ Wm
        assert np.allclose(G, Gref, rtol=1e-12, atol=1e-12 * np.abs(Gref).max()), "Gram matrix"
        assert np.array_equal(G, G.T), "both triangles carry the same sums"
        Wl = Wm.astype(np.longdouble)
        err, bound = np.abs(G.astype(np.longdouble) - Wl.T @ Wl), (d + 2) * U53 * (np.abs(Wl).T @ np.abs(Wl))
        frac = float((err / bound).max())
        print("gram d=%d m=%d chunks=%d: largest error / bound %.3f" % (d, m, nch, frac))
        assert np.all(err <= bound), "Gram matrix of %s: %d entries beyond the bound (worst %.3g x)" % (prob, int((err > bound).sum()), frac)
        worst = max(worst, frac)
        pd.append(K.PcholDesc(dGc.ptr, m + 1, m, rtol, atol, mr, dperm.ptr, drank.ptr, dR.ptr, cap))
    hk.batch("hssk_pchol_id_vbatched", pd)
    hk.sync()
    for (prob, kp) in zip(problems, keep):
        d, m, rtol, atol, mr, nr, chunks = prob
        Wm, dW, dP, dG, dperm, drank, dR, cap, nch = kp
        assert np.array_equal(dW.get()[:d], Wm), "the panel was modified"
        rank, perm = int(drank.get()[0]), dperm.get()
        Rq, jp = sla.qr(Wm, mode="r", pivoting=True)
        dg = np.abs(np.diag(Rq))
        rr = min(d, m)
        for c in range(min(d, m)):
            if dg[c] / dg[0] <= rtol or dg[c] <= atol:
                rr = c
                break
        if rr > cap:
            assert rank == -1, "a rank beyond the kernel's rows is reported, not truncated"
            continue
        rr = min(rr, mr)
        assert sorted(perm.tolist()) == list(range(m)), "perm is not a permutation"
        assert abs(rank - rr) <= (1 if rr > 0 else 0), f"rank {rank} vs LAPACK {rr} for {prob}"
        assert np.all(np.diff(perm[rank:]) > 0), "columns behind the skeleton keep their order"
        if rank == 0 or rank == m:
            continue
        R = dR.get()[:rank]
        # R^T R reproduces the Gram matrix on the skeleton rows; R11 upper triangular with the pivots' decreasing diagonal
        assert np.allclose(np.tril(R[:, :rank], -1), 0.)
        dd = np.diag(R[:, :rank])
        assert np.all(dd > 0) and np.all(np.diff(dd) <= 1e-12 * dd[0])
        assert np.allclose(dd, dg[:rank], rtol=1e-6)
        dX = hk.array(np.full((rank + 1, m - rank), -3.0))
        hk.batch("hssk_id_xsolve_vbatched", [K.XsolveDesc(dR.ptr, cap, rank, m, dX.ptr, rank + 1, 0)])
        hk.sync()
        X = dX.get()[:rank]
        err = np.linalg.norm(Wm[:, perm[rank:]] - Wm[:, perm[:rank]] @ X) / np.linalg.norm(Wm)
        bound = max(rtol * dg[0], atol, dg[min(rank, min(d, m) - 1)]) * np.sqrt(m) * 4 / np.linalg.norm(Wm)
        assert err <= max(bound, 1e-7), f"ID residual {err} > {bound} for {prob}"
    return worst


GRAM_GEN_SHAPES = ((333, 70, True), (64, 130, False), (17, 1, True), (500, 195, True), (2, 16, False))


def case_gram_gen(hk, n=700, d=6, seed=43, shapes=GRAM_GEN_SHAPES, widths=(1.7, 2.2)):
    """hssk_gram_gen_vbatched: W^T W of blocks W = K(rows, cols) of a kernel matrix, evaluated while they are multiplied, against
    numpy (index lists and ranges, row counts that are no multiple of the stage, Gauss and Laplace).
    shapes: one batch of (rows, m, index lists or ranges); widths: (Gauss, Laplace).  On top of the flat tolerance, entrywise
    |G - G_ref| <= ((rows + 2) u + 2 eps) |W|^T |W| against the np.longdouble product of the np.longdouble entries, eps the
    largest relative kernel_entry_bound of the block; the padding row m of the NaN-filled output stays NaN.  Returns error / bound."""
    r = rng(seed)
    X = r.standard_normal((n, d))
    dX = hk.array(X.T)
    mmax, worst = max(sh[1] for sh in shapes), 0.0
    for (ktype, h) in ((0, float(widths[0])), (1, float(widths[1]))):
        spec = K.KernelSpec(dX.ptr, n, d, ktype, 1, h, 3.0)
        assert hk.lib.hssk_gram_gen_supported(C.byref(spec), 256) == 1
        probs, descs, keep = [], [], []
        for (rows, m, lists) in shapes:
            ri = r.permutation(n)[:rows].astype(np.int32)
            ci = r.permutation(n)[:m].astype(np.int32)
            r0, c0 = int(r.integers(0, n - rows)), int(r.integers(0, n - m))
            dG = hk.array(np.full((m + 1, m), np.nan))
            if lists:
                dri, dci = hk.array(ri), hk.array(ci)
                keep.append((dri, dci))
                descs.append(K.GramGenDesc(dri.ptr, 0, dci.ptr, 0, rows, m, dG.ptr, m + 1))
                rr, cc = ri, ci
            else:
                descs.append(K.GramGenDesc(None, r0, None, c0, rows, m, dG.ptr, m + 1))
                rr, cc = np.arange(r0, r0 + rows), np.arange(c0, c0 + m)
            probs.append((rr, cc, dG, m))
        arr = (K.GramGenDesc * len(descs))(*descs)
        hk.check(hk.lib.hssk_gram_gen_vbatched(hk.ctx, C.byref(spec), arr, len(descs)))
        hk.sync()
        frac = 0.0
        for (rr, cc, dG, m) in probs:
            W = kernel_np(X, rr, cc, ktype, h, 0.0)
            Gp = dG.get()
            assert np.all(np.isnan(Gp[m])), "gram_gen wrote into the padding row"
            G = Gp[:m]
            assert np.allclose(G, W.T @ W, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(W.T @ W).max())), (ktype, len(rr), m)
            assert np.array_equal(G, G.T)
            Wl, a, _ = kernel_ref(X, rr, cc, ktype, h, 0.0)
            GW = Wl.T @ Wl                                       # (W > 0: |W|^T |W| is the product itself)
            eps = U53 * (8 + (d + 4) * float(a.max()))
            err, bound = np.abs(G.astype(np.longdouble) - GW), ((len(rr) + 2) * U53 + 2 * eps) * GW
            f = float((err / bound).max())
            assert np.all(err <= bound), "gram_gen type %d d %d rows %d m %d (batch up to %d columns): %d entries beyond the bound (worst %.3g x)" % (
                ktype, d, len(rr), m, mmax, int((err > bound).sum()), f)
            frac = max(frac, f)
        print("gram_gen type=%d d=%d mmax=%d: largest error / bound %.3f" % (ktype, d, mmax, frac))
        worst = max(worst, frac)
    spec = K.KernelSpec(dX.ptr, n, d, 2, 2, 1.0, 0.0)
    assert hk.lib.hssk_gram_gen_supported(C.byref(spec), 100) == 0   # (ANOVA: evaluated by hssk_kernel_eval_vbatched)
    return worst


# The Gram kernels are instantiated for 5, 12 and 17 tiles (16 x 16) per wave and dispatched on the widest panel of a batch:
# 5 up to 128 columns, 12 up to 208, 17 up to 256.  A wave that is handed more tiles than its instantiation holds drops them
# without a sign, so every batch below has its widest panel on one side of a boundary.
# hssk_gram_vbatched -- (rows, m, rtol, atol, max_rank, numerical rank, chunks), keyed by the widest panel
GRAM_BATCHES = {
    96: [(300, 40, 1e-3, 1e-12, 1000, 12, 1), (301, 96, 1e-4, 1e-12, 1000, 20, 3), (260, 1, 1e-2, 1e-12, 10, None, 1)],
    128: [(300, 128, 1e-3, 1e-12, 1000, 20, 2), (261, 17, 1e-4, 1e-12, 5, 9, 1)],
    129: [(300, 129, 1e-3, 1e-12, 1000, 20, 2), (270, 5, 1e-2, 1e-10, 1000, None, 1)],
    208: [(420, 208, 1e-3, 1e-12, 1000, 30, 2), (300, 64, 1e-4, 1e-12, 1000, 15, 1)],
    209: [(523, 209, 1e-3, 1e-12, 1000, 30, 3), (300, 17, 1e-4, 1e-12, 1000, 6, 1)],
    256: [(600, 256, 1e-3, 1e-12, 1000, 40, 2), (523, 209, 1e-3, 1e-12, 1000, 30, 3), (300, 17, 1e-4, 1e-12, 1000, 6, 1)],
    70: [(259, 70, 1e-3, 1e-12, 1000, 12, 7), (257, 33, 1e-4, 1e-12, 1000, 9, 128)],      # odd row counts, chunks of 37 and of 2 - 3 rows
}
# hssk_gram_gen_vbatched -- (rows, m, lists), keyed by the widest panel; row counts around the 16 rows of a stage, one row, one
# column next to the widest panel
GRAM_GEN_BATCHES = {
    128: ((1, 128, True), (15, 1, False), (33, 96, True)),
    129: ((16, 129, False), (2, 1, True)),
    208: ((17, 208, True), (500, 1, False)),
    209: ((33, 209, False), (15, 70, True)),
    256: ((500, 256, True), (1, 1, False), (16, 200, False)),
}
GRAM_GEN_DIMS = (1, 15, 16)       # (6 is the dimension of the batches above; the row points are fetched by the threads < 16 d)
GRAM_GEN_ROWS = ((1, 40, True), (2, 129, False), (15, 1, True), (16, 96, False), (17, 209, True), (33, 256, False), (500, 128, True))


def case_gram_gen_batch(hk, mmax):
    return case_gram_gen(hk, seed=400 + mmax, shapes=GRAM_GEN_BATCHES[mmax], widths=kernel_widths(6)[:2])


def case_gram_gen_dims(hk, d):
    w = kernel_widths(d)[:2]
    return max(case_gram_gen(hk, d=d, seed=500 + d, shapes=GRAM_GEN_ROWS, widths=w),
               case_gram_gen(hk, d=d, seed=600 + d, shapes=((33, 128, True), (16, 1, False)), widths=w))


def case_qr(hk, shapes, seed=7):
    r = rng(seed)
    descs, keep = [], []
    for (rows, cols, nq) in shapes:
        A = r.standard_normal((rows, cols))
        dA = hk.array(A)
        dQ = hk.empty((rows, max(nq, 1)))
        drd, dwk = hk.empty((2,)), hk.empty((rows + cols,))
        keep.append((A, dA, dQ, drd, dwk))
        descs.append(K.QrDesc(dA.ptr, rows, rows, cols, dQ.ptr if nq else None, rows, nq, drd.ptr, dwk.ptr))
    hk.batch("hssk_qr_vbatched", descs)
    hk.sync()
    for ((rows, cols, nq), (A, dA, dQ, drd, _)) in zip(shapes, keep):
        k = min(rows, cols)
        Rg = np.triu(dA.get())[:k]
        Rl = sla.qr(A, mode="r")[0][:k]
        # same Householder convention as LAPACK dgeqr2 -> same signs
        assert np.allclose(Rg, Rl, atol=1e-11 * np.abs(Rl).max()), f"R mismatch {rows}x{cols}"
        rd = drd.get()
        assert np.isclose(rd[0], np.abs(np.diag(Rl)).max()) and np.isclose(rd[1], np.abs(np.diag(Rl)).min())
        if nq:
            Q = dQ.get()[:, :nq]
            assert np.allclose(Q.T @ Q, np.eye(nq), atol=1e-12)
            kq = min(nq, k)
            assert np.allclose(Q[:, :kq] @ Rg[:kq, :][:, :cols] if nq >= k else Q @ Rg[:nq], A if nq >= k else Q @ Rg[:nq], atol=1e-11)
            if nq >= k:
                assert np.allclose(Q[:, :k] @ Rg, A, atol=1e-11 * max(1, np.abs(A).max()))


def case_qr_staircase(hk, shapes, seed=27):
    """hssk_qr_desc.stair: an interleaved stack of `fan` upper-triangular m x m factors (row r of triangle t at row
    fan * r + t) -- the TSQR tree's input -- must give the same R as the dense sweep / LAPACK."""
    r = rng(seed)
    descs, keep = [], []
    for (m, fan) in shapes:
        rows = fan * m
        A = np.zeros((rows, m))
        for t in range(fan):
            A[t::fan] = np.triu(r.standard_normal((m, m)))
        dA = hk.array(A)
        drd, dwk = hk.empty((2,)), hk.empty((rows + m,))
        keep.append((A, dA, drd, dwk))
        descs.append(K.QrDesc(dA.ptr, rows, rows, m, None, rows, 0, drd.ptr, dwk.ptr, fan))
    hk.batch("hssk_qr_vbatched", descs)
    hk.sync()
    for ((m, fan), (A, dA, drd, _)) in zip(shapes, keep):
        Rg = np.triu(dA.get())[:m]
        Rl = sla.qr(A, mode="r")[0][:m]
        assert np.allclose(Rg, Rl, atol=1e-11 * np.abs(Rl).max()), f"staircase R mismatch m={m} fan={fan}"
        rd = drd.get()
        assert np.isclose(rd[0], np.abs(np.diag(Rl)).max()) and np.isclose(rd[1], np.abs(np.diag(Rl)).min())


def case_qr_lazy(hk, shapes, seed=17):
    """Factor without Q, then hssk_formq_vbatched from the stored reflectors == Q of the one-call path."""
    r = rng(seed)
    d0, d1, keep = [], [], []
    for (rows, cols, nq) in shapes:
        A = r.standard_normal((rows, cols))
        dA = hk.array(A)
        dQ = hk.empty((rows, nq))
        drd, dwk = hk.empty((2,)), hk.empty((rows + cols,))
        keep.append((A, dA, dQ, drd, dwk))
        d0.append(K.QrDesc(dA.ptr, rows, rows, cols, None, rows, 0, drd.ptr, dwk.ptr))
        d1.append(K.QrDesc(dA.ptr, rows, rows, cols, dQ.ptr, rows, nq, None, dwk.ptr))
    hk.batch("hssk_qr_vbatched", d0)
    hk.batch("hssk_formq_vbatched", d1)
    hk.sync()
    for ((rows, cols, nq), (A, dA, dQ, drd, _)) in zip(shapes, keep):
        Ql, Rl = sla.qr(A, mode="economic")
        # LAPACK convention on both sides -> same signs
        assert np.allclose(dQ.get()[:, :min(nq, cols)], Ql[:, :min(nq, cols)], atol=1e-11), f"lazy Q mismatch {rows}x{cols}"
        rd = drd.get()
        assert np.isclose(rd[0], np.abs(np.diag(Rl)).max()) and np.isclose(rd[1], np.abs(np.diag(Rl)).min())


def case_random_shapes(hk, seed, rounds=3):
    """Seeded random shapes through the kernels of round 3 that choose their form by size: the cooperative ID (129 .. 256 rows,
    up to 512 columns: two / three / four workgroups per panel), products with at most four columns, the one-workgroup LU
    (checked as a factorization: P A = L U, |L| <= 1, LAPACK's pivots unless the matrix is degenerate), blocked triangular
    solves with and without the caller's inverted diagonal blocks."""
    r = rng(seed)
    for it in range(rounds):
        probs = []
        for _ in range(int(r.integers(1, 4))):
            d, m = int(r.integers(129, 257)), int(r.integers(2, 513))
            nr = int(r.integers(1, min(d, m) + 1)) if r.random() < 0.8 else None
            mr = int(r.choice([1000, 1000, int(r.integers(1, 200))]))
            probs.append((d, m, float(10.0 ** r.integers(-12, -2)), 1e-14, mr, nr))
        case_id(hk, probs, seed=seed * 100 + it, deferred=bool(r.random() < 0.3))
        cases = [(int(r.integers(1, 700)), int(r.integers(1, 5)), int(r.integers(1, 1025)), int(r.integers(0, 2)), int(r.integers(0, 2)),
                  float(r.choice([1.0, -1.0, 2.5])), float(r.choice([0.0, 1.0, 0.5]))) for _ in range(6)]
        case_gemm_vbatched(hk, cases, seed=seed * 100 + 50 + it)
        # LU
        n = int(r.integers(129, 513))
        A = r.standard_normal((n, n))
        if it % 3 == 1:
            A *= 10.0 ** r.uniform(-6, 6, size=(n, 1))
        dA, dpiv, dinfo = hk.array(A), hk.empty((n,), np.int32), hk.empty((1,), np.int32)
        hk.batch("hssk_getrf_vbatched", [K.LuDesc(dA.ptr, n, n, dpiv.ptr, dinfo.ptr)])
        hk.sync()
        got, gp = dA.get(), dpiv.get()
        PA = A.copy()
        for i, pi in enumerate(gp):
            PA[[i, pi]] = PA[[pi, i]]
        Lf, Uf = np.tril(got, -1) + np.eye(n), np.triu(got)
        assert np.abs(Lf).max() <= 1.0 + 1e-12 and np.allclose(Lf @ Uf, PA, atol=1e-10 * max(1.0, np.abs(Uf).max())), f"LU n={n}"
        assert np.array_equal(gp, sla.lu_factor(A)[1]), f"LU pivots n={n}"
        # blocked triangular solve, with / without given inverses
        n, nrhs = int(r.integers(128, 513)), int(r.integers(1, 50))
        lower, trans, unit = [(1, 0, 1), (0, 0, 0), (0, 1, 0)][it % 3]
        T = sla.lu_factor(r.standard_normal((n, n)))[0] if unit else r.standard_normal((n, n)) + n * np.eye(n)
        B = r.standard_normal((n, nrhs))
        dT, dB = hk.array(T), hk.array(B)
        dinv = None
        if it % 2:
            dinv = hk.empty((((n + 63) // 64) * 4096,))
            hk.batch("hssk_trtri_diag_vbatched", [K.TrtriDesc(dT.ptr, dinv.ptr, n, n, 2 if lower else 1)])
        hk.batch("hssk_trsm_vbatched", [K.TrsmDesc(dT.ptr, dB.ptr, n, nrhs, n, n, lower, trans, unit, dinv.ptr if dinv is not None else None)])
        hk.sync()
        Tt = np.tril(T) if lower else np.triu(T)
        if unit:
            np.fill_diagonal(Tt, 1.0)
        ref = np.linalg.solve(Tt.T if trans else Tt, B)
        assert np.allclose(dB.get(), ref, atol=1e-10 * max(1.0, np.abs(ref).max())), f"trsm n={n} nrhs={nrhs} form={(lower, trans, unit)}"


def case_laswp(hk, shapes, seed=31):
    """hssk_laswp_vbatched: B <- P B, the row interchanges of a getrf applied in order (shapes: (n, nrhs)); up to 1024 rows
    every row replays the interchanges on its index and the rows move in one pass, above that column by column"""
    r = rng(seed)
    descs, keep = [], []
    for (n, nrhs) in shapes:
        piv = np.array([int(r.integers(k, n)) for k in range(n)], dtype=np.int32)
        if n > 3:
            piv[1] = 1            # an interchange with itself
            piv[2] = n - 1
        ldb = n + 3
        B = r.standard_normal((ldb, nrhs))
        dB, dpiv = hk.array(B), hk.array(piv)
        keep.append((B, piv, dB, dpiv, n))
        descs.append(K.LuSolveDesc(None, dpiv.ptr, dB.ptr, n, nrhs, n, ldb))
    hk.batch("hssk_laswp_vbatched", descs)
    hk.sync()
    for (B, piv, dB, dpiv, n) in keep:
        ref = B.copy()
        for k in range(n):
            if piv[k] != k:
                ref[[k, piv[k]]] = ref[[piv[k], k]]
        assert np.array_equal(dB.get(), ref), f"laswp n={n}"


def case_trsm_lu(hk, seed=9, big_lu=(600, 3), extra_lu=()):
    r = rng(seed)
    descs, keep = [], []
    for (n, nrhs, lower, trans, unit) in [(37, 1, 1, 0, 0), (37, 5, 0, 1, 0), (64, 3, 0, 0, 0),
                                          (65, 2, 1, 1, 0), (20, 9, 1, 0, 1), (1, 1, 1, 0, 0),
                                          (130, 1, 0, 1, 0),
                                          # blocked form (inverted 64 x 64 diagonal blocks + batched GEMMs): unit lower, upper,
                                          # transposed upper; ragged last block; a form that stays with the substitution kernel
                                          (256, 40, 1, 0, 1), (256, 33, 0, 0, 0), (200, 24, 0, 1, 0), (150, 16, 1, 1, 0), (129, 8, 0, 0, 0),
                                          # (up to 512 rows all block steps are one launch, a workgroup per 16 right-hand sides)
                                          (512, 17, 1, 0, 1), (300, 1, 0, 0, 0), (450, 5, 0, 1, 0), (130, 1, 1, 0, 1),
                                          (640, 20, 0, 0, 0)]:
        T = r.standard_normal((n, n)) + n * np.eye(n)
        if unit and n > 64:   # a unit triangle as the solves meet it: the L of an LU with partial pivoting (|L_ij| <= 1)
            T = sla.lu_factor(r.standard_normal((n, n)))[0]
        B = r.standard_normal((n, nrhs))
        dT, dB = hk.array(T), hk.array(B)
        keep.append((T, B, dT, dB, lower, trans, unit))
        descs.append(K.TrsmDesc(dT.ptr, dB.ptr, n, nrhs, n, n, lower, trans, unit))
    hk.batch("hssk_trsm_vbatched", descs)
    hk.sync()
    for (T, B, dT, dB, lower, trans, unit) in keep:
        Tt = np.tril(T) if lower else np.triu(T)
        if unit:
            np.fill_diagonal(Tt, 1.0)
        ref = np.linalg.solve(Tt.T if trans else Tt, B)
        assert np.allclose(dB.get(), ref, atol=1e-11 * max(1.0, np.abs(ref).max())), f"trsm lower={lower} trans={trans} n={T.shape[0]}"
    # 130 .. 512: one workgroup with the panel in LDS (getrf_wg_kernel: ragged last panel, several 64-column passes over
    # the trailing matrix); the last one takes the multi-launch blocked path (n > 512)
    # (up to 192 rows: the whole matrix in the registers of one workgroup, getrf_quad_kernel -- every instantiation's edges)
    for n, nrhs in [(1, 1), (45, 3), (96, 2), (97, 1), (128, 1), (130, 1), (156, 2), (160, 1), (161, 2), (192, 1), (193, 1), (256, 2)] + list(extra_lu) + [big_lu]:
        A = r.standard_normal((n, n))
        B = r.standard_normal((n, nrhs))
        dA, dB = hk.array(A), hk.array(B)
        dpiv, dinfo = hk.empty((n,), np.int32), hk.empty((1,), np.int32)
        hk.batch("hssk_getrf_vbatched", [K.LuDesc(dA.ptr, n, n, dpiv.ptr, dinfo.ptr)])
        hk.batch("hssk_getrs_vbatched", [K.LuSolveDesc(dA.ptr, dpiv.ptr, dB.ptr, n, nrhs, n, n)])
        hk.sync()
        assert dinfo.get()[0] == 0
        lu, piv = sla.lu_factor(A)
        assert np.array_equal(dpiv.get(), piv)
        assert np.allclose(dA.get(), lu, atol=1e-9 if n > 128 else 1e-11)
        assert np.allclose(dB.get(), np.linalg.solve(A, B), atol=1e-8 if n > 128 else 1e-9)
    # equal pivot candidates: entries +-1, +-2 -- the first two elimination steps are exact in floating point (multipliers 1/2
    # and 1, then multiples of 1/2), so their ties are real and the first candidate in the interchanged order must win, as in
    # dgetf2; later steps round (ties there are resolved by the order of the updates, LAPACK's own differs between versions):
    # the factorization is checked as one -- P A = L U, |L| <= 1
    for n in [90, 140, 180, 256] + [e[0] for e in extra_lu]:
        A = r.integers(1, 3, size=(n, n)).astype(float) * r.choice([-1.0, 1.0], size=(n, n))
        dA, dpiv, dinfo = hk.array(A), hk.empty((n,), np.int32), hk.empty((1,), np.int32)
        hk.batch("hssk_getrf_vbatched", [K.LuDesc(dA.ptr, n, n, dpiv.ptr, dinfo.ptr)])
        hk.sync()
        lu, piv = sla.lu_factor(A)
        got, gp = dA.get(), dpiv.get()
        assert np.array_equal(gp[:2], piv[:2]), f"pivots with ties, n={n}"
        PA = A.copy()
        for i, pi in enumerate(gp):
            PA[[i, pi]] = PA[[pi, i]]
        Lf, Uf = np.tril(got, -1) + np.eye(n), np.triu(got)
        assert np.abs(Lf).max() <= 1.0 + 1e-14
        assert np.allclose(Lf @ Uf, PA, atol=1e-10 * np.abs(Uf).max()), f"P A = L U, n={n}"
    for n in [150]:
        A = r.standard_normal((n, n))
        A[:, 40] = 0.0
        dA, dpiv, dinfo = hk.array(A), hk.empty((n,), np.int32), hk.empty((1,), np.int32)
        hk.batch("hssk_getrf_vbatched", [K.LuDesc(dA.ptr, n, n, dpiv.ptr, dinfo.ptr)])
        hk.sync()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lu, piv = sla.lu_factor(A)
        assert dinfo.get()[0] == 41
        assert np.array_equal(dpiv.get(), piv)
        assert np.allclose(dA.get(), lu, atol=1e-9)


# ---- kernel-matrix front end -------------------------------------------------------------------
def kernel_np(X, I, J, ktype, h, lam, p=1):
    """numpy restatement of kernel::Kernel::eval (kernel/Kernel.hpp:122-125, 333-399); X is n x d."""
    xi, xj = X[I][:, None, :], X[J][None, :, :]
    if ktype == 0:
        K = np.exp(-((xi - xj) ** 2).sum(-1) / (2 * h * h))
    elif ktype == 1:
        K = np.exp(-np.abs(xi - xj).sum(-1) / h)
    else:
        t = np.exp(-((xi - xj) ** 2) / (2 * h * h))            # per-dimension factors
        Kss = [(t ** (j + 1)).sum(-1) for j in range(p)]
        Kpp = [np.ones(t.shape[:2])]
        for i in range(1, p + 1):
            Kpp.append(sum((-1) ** (s + 1) * Kpp[i - s] * Kss[s - 1] for s in range(1, i + 1)) / i)
        K = Kpp[p]
    return K + lam * (np.asarray(I)[:, None] == np.asarray(J)[None, :])


U53 = 2.0 ** -53


def kernel_ref(X, I, J, ktype, h, lam, p=1):
    """kernel_np in np.longdouble, with what the error bound of an FP64 evaluation needs.  Returns (k, a, A):
    k  the entry, lambda on the diagonal included;
    a  the exponent's magnitude: |x-y|_2^2 / (2 h^2) (Gauss), |x-y|_1 / h (Laplace), the largest per-coordinate one (ANOVA);
    A  the magnitude the rounding errors are relative to: the kernel value itself (Gauss, Laplace: > 0), for ANOVA the
       recurrence with all signs positive (>= |k|: its alternating sum cancels), as kpredict_cases.reference has it."""
    LD = np.longdouble
    X = np.asarray(X, dtype=LD)
    I, J = np.asarray(I), np.asarray(J)
    h = LD(h)
    k, a, A = (np.zeros((len(I), len(J)), dtype=LD) for _ in range(3))
    step = int(max(1, 2_000_000 // max(1, len(J) * X.shape[1])))   # (rows per pass: the differences stay a few tens of MB)
    for i0 in range(0, len(I), step):
        df = X[I[i0:i0 + step]][:, None, :] - X[J][None, :, :]
        sl = slice(i0, i0 + step)
        if ktype == 0:
            a[sl] = (df ** 2).sum(-1) / (2 * h * h)
            k[sl] = A[sl] = np.exp(-a[sl])
        elif ktype == 1:
            a[sl] = np.abs(df).sum(-1) / h
            k[sl] = A[sl] = np.exp(-a[sl])
        else:
            ai = df ** 2 / (2 * h * h)
            t = np.exp(-ai)
            Kss = [(t ** (j + 1)).sum(-1) for j in range(p)]
            Kpp, App = [np.ones(t.shape[:2], dtype=LD)], [np.ones(t.shape[:2], dtype=LD)]
            for i in range(1, p + 1):
                Kpp.append(sum((-1) ** (s + 1) * Kpp[i - s] * Kss[s - 1] for s in range(1, i + 1)) / i)
                App.append(sum(App[i - s] * Kss[s - 1] for s in range(1, i + 1)) / i)
            a[sl], k[sl], A[sl] = ai.max(-1), Kpp[p], App[p]
    return k + LD(lam) * (I[:, None] == J[None, :]), a, A


def kernel_entry_bound(a, A, ktype, d, lam, p=1):
    """Error bound of one FP64 kernel entry against kernel_ref (u = 2^-53; the bound of kpredict_cases with FP64's u):
      Gauss / Laplace   u (8 + (d + 4) a) k + u |lambda|       the d-term sum and its scaling perturb the exponent a relatively
                                                               by (d + 4) u, i.e. exp(-a) by (d + 4) a u; 8 u for exp and the sum
      ANOVA             u (8 + p (d + 10 + 5 a_max)) A + u |lambda|"""
    rel = (8 + (d + 4) * a) if ktype != 2 else (8 + p * (d + 10 + 5 * a))
    return U53 * rel * A + U53 * abs(lam)


def kernel_widths(d):
    """kernel widths (Gauss, Laplace, ANOVA) that keep the entries of a standard normal cloud in R^d away from 0 and 1"""
    return (0.9 * np.sqrt(d) + 0.4, 0.9 * d, 0.9 * np.sqrt(d) + 0.4)


SENTINEL = -7.25


def case_kernel_eval(hk, n=300, d=8, seed=21, kinds=((0, 1), (1, 1), (2, 1), (2, 3)), widths=None):
    """hssk_kernel_eval_vbatched against kernel_ref under kernel_entry_bound: index lists and ranges, a whole tile, one row
    over three column tiles; the outputs are pre-filled and the rows nr .. ldo - 1 of every column must come back bitwise.
    widths: (Gauss, Laplace, ANOVA) kernel widths, None: 1.3 for all (and the flat tolerance of the first version of this
    case on top of the bound).  Returns the largest error / bound."""
    r = rng(seed)
    X = r.standard_normal((n, d))
    dX = hk.array(X.T)                      # d x n, one point per column
    lam, worst = 3.11, 0.0
    for (ktype, p) in kinds:
        h = 1.3 if widths is None else float(widths[ktype])
        spec = K.KernelSpec(dX.ptr, n, d, ktype, p, h, lam)
        I1, J1 = r.permutation(n)[:70].astype(np.int32), r.permutation(n)[:130].astype(np.int32)
        J1[:5] = I1[:5]                      # a few diagonal hits
        dI, dJ = hk.array(I1), hk.array(J1)
        # (rows, columns, ldo, row list, column list, r0, c0)
        probs = [(70, 130, 73, I1, J1, 0, 0),
                 (65, 40, 65, None, None, 100, 120),       # ranges, overlapping -> diagonal entries
                 (64, 64, 67, None, None, 5, 5),           # exactly one tile, the whole diagonal
                 (1, 129, 3, I1[:1], None, 0, 0)]          # one row, a third column tile of one column
        outs = [hk.array(np.full((ldo, nc), SENTINEL)) for (nr, nc, ldo, *_) in probs]
        descs = [K.KevalDesc(dI.ptr if ri is not None else None, dJ.ptr if ci is not None else None, o.ptr, nr, nc, ldo, r0, c0)
                 for (nr, nc, ldo, ri, ci, r0, c0), o in zip(probs, outs)]
        arr = (K.KevalDesc * len(descs))(*descs)
        hk.check(hk.lib.hssk_kernel_eval_vbatched(hk.ctx, C.byref(spec), arr, len(descs)))
        hk.sync()
        frac = 0.0
        for (nr, nc, ldo, ri, ci, r0, c0), o in zip(probs, outs):
            rr = ri if ri is not None else np.arange(r0, r0 + nr)
            cc = ci if ci is not None else np.arange(c0, c0 + nc)
            got = o.get()
            assert np.array_equal(got[nr:].view(np.uint64), np.full((ldo - nr, nc), SENTINEL).view(np.uint64)), \
                "kernel_eval type %d p %d d %d: wrote into the padding rows of a %d x %d block" % (ktype, p, d, nr, nc)
            k, a, A = kernel_ref(X, rr, cc, ktype, h, lam, p)
            err = np.abs(got[:nr].astype(np.longdouble) - k)
            bound = kernel_entry_bound(a, A, ktype, d, lam, p)
            frac = max(frac, float((err / bound).max()))
            assert np.all(err <= bound), "kernel_eval type %d p %d d %d (%d x %d): %d entries beyond the bound (worst %.3g x)" % (
                ktype, p, d, nr, nc, int((err > bound).sum()), float((err / bound).max()))
            if widths is None:
                assert np.allclose(got[:nr], kernel_np(X, rr, cc, ktype, h, lam, p), rtol=1e-12, atol=1e-14)
        print("kernel_eval type=%d p=%d d=%d n=%d: largest error / bound %.3f" % (ktype, p, d, n, frac))
        worst = max(worst, frac)
    return worst


def anova_degrees(d):
    return sorted({1, min(2, d), min(8, d)})


KERNEL_DIMS = (1, 8, 31, 32, 33, 64)      # one pass of 32 staged coordinates, its edges, two passes, the largest dimension


def case_kernel_eval_dims(hk, d, n=200):
    return case_kernel_eval(hk, n=n, d=d, seed=200 + d, kinds=[(0, 1), (1, 1)] + [(2, p) for p in anova_degrees(d)],
                            widths=kernel_widths(d))


def case_knn(hk, n=500, d=8, k=10, seed=22, lattice=False):
    r = rng(seed)
    # lattice: many points at exactly equal distances (and duplicates): ties are ordered by index
    X = r.integers(0, 3, (n, d)).astype(np.float64) if lattice else r.standard_normal((n, d))
    dX = hk.array(X.T)
    out = hk.empty((k, n), dtype=np.int32)
    hk.check(hk.lib.hssk_knn(hk.ctx, dX.ptr, d, n, k, 0, n // 3, out.ptr))      # two query ranges, as two ranks would
    hk.check(hk.lib.hssk_knn(hk.ctx, dX.ptr, d, n, k, n // 3, n, out.ptr))
    hk.sync()
    got = out.get().T                        # row i = neighbours of point i
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).astype(np.float32)   # the kernel ranks float keys
    np.fill_diagonal(D2, np.inf)
    kk = min(k, n - 1)
    for i in range(n):
        mine = got[i][got[i] >= 0]
        assert len(mine) == kk and len(set(mine.tolist())) == kk and i not in mine
        kth = np.sort(D2[i])[kk - 1]
        assert (D2[i][mine] <= kth).all()     # exactly a set of k nearest
        if lattice:                           # ... and among equal distances the smallest indices
            order = np.lexsort((np.arange(n), D2[i]))
            assert set(mine.tolist()) == set(order[:kk].tolist())


# heap search (n, d, k): the 64- and 32-coordinate instantiations at a dimension that fills them / leaves them nearly empty, d = 1
KNN_HEAP_DIMS = ((150, 64, 10), (150, 33, 10), (150, 1, 10))
# filtered search (n, d, k) with HSSK_KNN_FILTER_MIN=600: both sides of its padded-dimension variants (3|4, 9|10, 17|18) and of
# its limits d <= 29 and k <= 128 (beyond them, and with n <= 4 k, the heap search answers)
KNN_FILTER_EDGES = tuple((700, d, 8) for d in (1, 3, 4, 9, 10, 17, 18, 29, 30)) + ((700, 8, 128), (700, 8, 129), (640, 8, 160))


def case_knn_filter_edges(hk):
    import os
    os.environ["HSSK_KNN_FILTER_MIN"] = "600"
    try:
        for (n, d, k) in KNN_FILTER_EDGES:
            case_knn(hk, n=n, d=d, k=k, seed=700 + d + k)
    finally:
        os.environ.pop("HSSK_KNN_FILTER_MIN")


# (n, d, leaf): the device clustering keeps a centre of 64 and extents of 2 x 64 coordinates per cluster
CLUSTER_DIMS = ((3001, 1, 64), (2500, 2, 100), (2000, 33, 64), (1500, 64, 50), (6000, 17, 128))


def case_clustering_dims(KM, lib, algo):
    """Device clustering against the host form at the dimensions' edges, with the splits of large clusters by several workgroups
    at their default size, never (0) and from 1000 points on: status 0, permutation, points and leaf sizes equal."""
    import os
    r = np.random.default_rng(5)
    for (n, d, leaf) in CLUSTER_DIMS:
        pts = r.standard_normal((n, d))
        Xh, ph, lh = KM.clustering(lib, pts, algo, leaf)
        for wide in (None, "0", "1000"):
            if wide is not None:
                os.environ["HSSK_CLUSTER_WIDE_MIN"] = wide
            try:
                st, Xp, perm, leaves = KM.clustering_device(lib, pts, algo, leaf)
            finally:
                os.environ.pop("HSSK_CLUSTER_WIDE_MIN", None)
            assert st == 0, (algo, n, d, leaf, wide, st)
            assert np.array_equal(perm, ph) and np.array_equal(Xp, Xh) and leaves.tolist() == lh.tolist(), (algo, n, d, leaf, wide)


def gram_blocks_child(lib_expr, tmp_path=None):
    """Every batch of GRAM_BATCHES through hssk_gram_vbatched in a fresh process with HSSK_GRAM_BLOCKS=1 (read once per process):
    the 128 x 128 block kernel for all of them.  lib_expr: python source of the library path in the child.  Returns its output."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import kernel_cases as KC\n"
        "from strumpack_amd import hssk as K\n"
        "%s\n"
        "hk = K.Hssk(path)\n"
        "for mmax, batch in sorted(KC.GRAM_BATCHES.items()):\n"
        "    KC.case_gram_pchol_id(hk, batch, seed=800 + mmax)\n"
        "hk.close(); print('gram blocks ok')\n"
    ) % (here, os.path.dirname(here), lib_expr)
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HSSK_GRAM_BLOCKS="1"), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    assert res.stdout.strip().endswith("gram blocks ok")
    return res.stdout


def front_end_two_forms(lib_expr, kern, dim, deg, clus, n, leaf, tmp_path, rtol=1e-3, lam=2.5):
    """n standard normal points in R^dim through the kernel-matrix front end (device clustering, filtered neighbour search, row
    ID from Gram matrices) and, in a second process, through the forms it replaced (STRUMPACK_AMD_CLUSTER_HOST=1
    HSSK_KNN_FILTER=0 STRUMPACK_AMD_ID_GRAM=0): the same permutation and tree, the points in that order, ULV residual against
    the compressed matrix <= 1e-10.  The error of H b on 32 sampled rows against exact np.longdouble kernel rows is limited by
    the column sample (64 neighbours per point), not by rel_tol, so it is measured for the replaced forms in the same call:
    err_new <= max(2 err_old, 10 rel_tol), the factor 2 for ranks that come out one off.  Both are printed
    (profiles/kernelmat_dims.md has the measured ones).  lib_expr: python source of the library path in the child processes."""
    import os
    import subprocess
    import sys
    kt = {"Gauss": 0, "Laplace": 1, "ANOVA": 2}[kern]
    h = float(kernel_widths(dim)[kt])
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from strumpack_amd import capi, dist as sdist\n"
        "%s\n"
        "L = capi.load(path); n, d = %d, %d\n"
        "X = np.random.default_rng(78).standard_normal((n, d))\n"
        "o = capi.StructuredMatrix.options(L, rel_tol=%g, abs_tol=1e-10, leaf_size=%d, max_rank=50000)\n"
        "H, Xp, perm = sdist.from_kernel(L, X, o, kernel=%r, h=%r, lam=%r, degree=%d, clustering=%r, neighbors=64)\n"
        "b = np.linspace(-1, 1, n); y = H.mult(b)[:, 0]; H.factor(); x = H.solve(b)[:, 0]\n"
        "res = float(np.linalg.norm(H.mult(x)[:, 0] - b) / np.linalg.norm(b))\n"
        "np.savez(sys.argv[1], perm=perm, info=H.node_info(), y=y, Xp=Xp, X=X, res=res, rank=H.rank())\n"
    ) % (here, os.path.dirname(here), lib_expr, n, dim, rtol, leaf, kern, h, lam, deg, clus)
    out = []
    for mode, env in (("new", {}), ("old", {"STRUMPACK_AMD_CLUSTER_HOST": "1", "HSSK_KNN_FILTER": "0", "STRUMPACK_AMD_ID_GRAM": "0"})):
        f = str(tmp_path / ("dims_%s.npz" % mode))
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(np.load(f))
    new, old = out
    assert np.array_equal(new["perm"], old["perm"]), "device clustering differs from the host form"
    assert np.array_equal(new["info"][:, [0, 1, 5]], old["info"][:, [0, 1, 5]]), "tree"
    for z in (new, old):
        assert sorted(z["perm"].tolist()) == list(range(1, n + 1)) and np.array_equal(z["Xp"], z["X"][z["perm"] - 1])
    assert float(new["res"]) <= 1e-10 and float(old["res"]) <= 1e-10, (float(new["res"]), float(old["res"]))
    I = np.random.default_rng(3).integers(0, n, 32)
    KI = kernel_ref(new["Xp"], I, np.arange(n), kt, h, lam, deg)[0]
    ref = KI @ np.linspace(-1, 1, n).astype(np.longdouble)
    en, eo = (float(np.linalg.norm(z["y"][I] - ref) / np.linalg.norm(ref)) for z in (new, old))
    print("front end %s d=%d p=%d n=%d: rank new %d old %d, sampled-row error new %.3e old %.3e, ULV residual new %.1e old %.1e" %
          (kern, dim, deg, n, int(new["rank"]), int(old["rank"]), en, eo, float(new["res"]), float(old["res"])))
    assert en <= max(2 * eo, 10 * rtol), (en, eo)
    return en, eo


def case_kernel_predict(hk, n=257, m=70, d=5, seed=23, kinds=((0, 1), (1, 1), (2, 2)), widths=None):
    """hssk_kernel_predict (FP64) against the np.longdouble sum under
        sum_r |w_r| (kernel_entry_bound of k_rc) + n u sum_r |w_r k_rc|        (n additions of the products, in any order).
    widths: as in case_kernel_eval (None: 0.9, and the flat tolerance of the first version on top).  Returns error / bound."""
    r = rng(seed)
    X, T, w = r.standard_normal((n, d)), r.standard_normal((m, d)), r.standard_normal(n)
    dX, dT, dw = hk.array(X.T), hk.array(T.T), hk.array(w)
    Z = np.vstack([X, T])
    worst = 0.0
    for (ktype, p) in kinds:
        h = 0.9 if widths is None else float(widths[ktype])
        dp = hk.array(np.full((m + 2,), SENTINEL))
        spec = K.KernelSpec(dX.ptr, n, d, ktype, p, h, 2.0)
        hk.check(hk.lib.hssk_kernel_predict(hk.ctx, C.byref(spec), dw.ptr, dT.ptr, m, dp.ptr))
        hk.sync()
        got = dp.get()
        assert np.all(got[m:] == SENTINEL), "kernel_predict wrote behind its m predictions"
        k, a, A = kernel_ref(Z, np.arange(n), n + np.arange(m), ktype, h, 0.0, p)
        aw = np.abs(w).astype(np.longdouble)
        ref = w.astype(np.longdouble) @ k
        bound = aw @ kernel_entry_bound(a, A, ktype, d, 0.0, p) + n * U53 * (aw @ np.abs(k))
        err = np.abs(got[:m].astype(np.longdouble) - ref)
        frac = float((err / bound).max())
        print("kernel_predict type=%d p=%d n=%d m=%d d=%d: largest error / bound %.3f" % (ktype, p, n, m, d, frac))
        assert np.all(err <= bound), "kernel_predict type %d p %d (n, m, d) = %s: %d predictions beyond the bound (worst %.3g x)" % (
            ktype, p, (n, m, d), int((err > bound).sum()), frac)
        if widths is None:
            assert np.allclose(got[:m], w @ kernel_np(Z, np.arange(n), n + np.arange(m), ktype, h, 0.0, p), rtol=1e-11, atol=1e-12)
        worst = max(worst, frac)
    return worst


# (n, m, d): one point, n and m on both sides of the 64 training points / 64 test points of a pass and a workgroup, the LDS row
# stride at its largest dimension, two staging passes' worth of coordinates, and the shape of the first version of the case
PREDICT_SHAPES = ((1, 1, 1), (63, 64, 33), (64, 65, 64), (65, 1, 32), (257, 70, 5))


def case_kernel_predict_dims(hk, n, m, d):
    return case_kernel_predict(hk, n=n, m=m, d=d, seed=300 + d, kinds=((0, 1), (1, 1), (2, min(8, d))), widths=kernel_widths(d))


def case_gather_combine(hk, shapes, seed=31):
    """hssk_gather_combine vs numpy: out = G[:, g] + alpha M[:, m] C^T with two-part sources and index lists.
    shapes: (rows, J, K, ng0, ng1, nm0, nm1, transposed_c, with_g)"""
    r = rng(seed)
    descs, keep, expect = [], [], []
    for (rows, J, K, ng0, ng1, nm0, nm1, ct, with_g) in shapes:
        ldg, ldm, ldo = rows + 3, rows + 1, rows + 2
        G0, G1 = r.standard_normal((ldg, ng0)), r.standard_normal((ldg, max(ng1, 1)))
        M0, M1 = r.standard_normal((ldm, max(nm0, 1))), r.standard_normal((ldm, max(nm1, 1)))
        gidx = r.integers(0, ng0 + ng1, J).astype(np.int32)
        midx = r.integers(0, max(nm0 + nm1, 1), max(K, 1)).astype(np.int32)
        Cm = r.standard_normal((K, J)) if ct else r.standard_normal((J, K))   # C(j, k) = Cm[k, j] / Cm[j, k]
        out0 = r.standard_normal((ldo, J))
        alpha = -1.0 if ct else 0.5
        d = [hk.array(x) for x in (G0, G1, M0, M1)] + [hk.array(gidx), hk.array(midx), hk.array(Cm if Cm.size else np.zeros((1, 1))), hk.array(out0)]
        keep.append(d)
        ldc = max(Cm.shape[0], 1)
        csj, csk = (ldc, 1) if ct else (1, ldc)
        descs.append(K_.CombineDesc(d[0].ptr if with_g else None, d[1].ptr, ldg, ng0, d[4].ptr, d[2].ptr, d[3].ptr, ldm, nm0, d[5].ptr,
                                    d[6].ptr, csj, csk, alpha, d[7].ptr, ldo, rows, J, K))
        Gc = np.hstack([G0, G1[:, :ng1]])[:rows]
        Mc = np.hstack([M0[:, :nm0], M1[:, :nm1]])[:rows] if nm0 + nm1 else np.zeros((rows, 1))
        Cjk = Cm.T if ct else Cm
        ref = out0.copy()
        ref[:rows] = (Gc[:, gidx] if with_g else 0.0) + (alpha * Mc[:, midx[:K]] @ Cjk.T if K else 0.0)
        expect.append(ref)
    hk.batch("hssk_gather_combine", descs)
    hk.sync()
    for d, ref, sh in zip(keep, expect, shapes):
        got = d[7].get()
        assert np.abs(got - ref).max() <= 1e-12 * max(1, sh[2]), f"gather_combine {sh}"


def case_qr_early_exit(hk, shapes, seed=41):
    """hssk_qr_desc.stop_rel / stop_abs: the R-diagonal test stops at the first |R_kk| under the tolerance and reports the
    prefix maximum and that |R_kk| -- the values of the full factorisation at that step.  shapes: (rows, cols, stop_rel)"""
    r = rng(seed)
    descs, keep = [], []
    for (rows, cols, srel) in shapes:
        k = min(rows, cols)
        U, _ = np.linalg.qr(r.standard_normal((rows, k)))
        V, _ = np.linalg.qr(r.standard_normal((cols, k)))
        A = (U * 10.0 ** (-np.arange(k) / 4.0)) @ V.T      # singular values decay by 10 every four
        dA, drd, dwk = hk.array(A), hk.array(np.zeros(2)), hk.empty((rows + cols,))
        keep.append((A, dA, drd, dwk, srel))
        descs.append(K.QrDesc(dA.ptr, rows, rows, cols, None, rows, 0, drd.ptr, dwk.ptr, 0, srel, 0.0))
    hk.batch("hssk_qr_vbatched", descs)
    hk.sync()
    for (A, dA, drd, dwk, srel) in keep:
        dg = np.abs(np.diag(np.linalg.qr(A, mode="r")))
        pm = np.maximum.accumulate(dg)
        hit = np.nonzero(dg < srel * pm)[0]
        rd = drd.get()
        if srel > 0 and len(hit):
            k0 = hit[0]
            assert abs(rd[0] - pm[k0]) <= 1e-12 * pm[k0] and rd[1] <= dg[k0] * (1 + 1e-9) + 1e-300, (rd, pm[k0], dg[k0])
            assert rd[1] < srel * rd[0]
        else:
            assert abs(rd[0] - dg.max()) <= 1e-12 * dg.max() and abs(rd[1] - dg.min()) <= 1e-6 * dg.max()


def case_ulv_split(hk, shapes, seed=51):
    """hssk_ulv_split vs numpy.  shapes: (m, r)"""
    r_ = rng(seed)
    descs, keep = [], []
    for (m, r) in shapes:
        q = m - r
        D = r_.standard_normal((m + 3, m))
        perm = r_.permutation(m).astype(np.int32)
        X = r_.standard_normal((max(r, 1) + 1, max(q, 1)))
        W1 = np.full((max(r, 1) + 2, m), -5.0)
        W0t = np.full((m + 1, max(q, 1)), -6.0)
        d = [hk.array(D), hk.array(perm), hk.array(X), hk.array(W1), hk.array(W0t)]
        keep.append((D, perm, X, d, m, r))
        descs.append(K.UlvSplitDesc(d[0].ptr, m + 3, m, r, d[1].ptr, d[2].ptr, max(r, 1) + 1, d[3].ptr, max(r, 1) + 2, d[4].ptr, m + 1))
    hk.batch("hssk_ulv_split", descs)
    hk.sync()
    for (D, perm, X, d, m, r) in keep:
        q = m - r
        PD = D[:m][perm]
        w1 = PD[:r]
        w0t = PD[r:].T - w1.T @ X[:r, :q]
        g1, g0 = d[3].get(), d[4].get()
        assert np.array_equal(g1[:r], w1) and np.all(g1[r:] == -5.0)
        if q:
            assert np.abs(g0[:m, :q] - w0t).max() <= 1e-12 * max(1.0, np.abs(w0t).max()) * max(r, 1)
        assert np.all(g0[m:] == -6.0)


def case_tpqr(hk, sizes, seed=61):
    """hssk_tpqr_vbatched vs numpy: R of [triu(R1); triu(R2)] in place over R1 (signs of the rows are free: R^T R is compared,
    and the magnitudes of the diagonal)."""
    r = rng(seed)
    descs, keep = [], []
    for m in sizes:
        A1, A2 = r.standard_normal((m + 2, m)), r.standard_normal((m + 5, m))   # below the diagonals: junk that must be ignored
        d1, d2 = hk.array(A1), hk.array(A2)
        keep.append((A1, A2, d1, d2, m))
        descs.append(K.TpqrDesc(d1.ptr, m + 2, d2.ptr, m + 5, m))
    hk.batch("hssk_tpqr_vbatched", descs)
    hk.sync()
    for (A1, A2, d1, d2, m) in keep:
        S = np.vstack([np.triu(A1[:m]), np.triu(A2[:m])])
        Rref = np.linalg.qr(S, mode="r")
        got = d1.get()
        R = np.triu(got[:m])
        assert np.array_equal(np.tril(got[:m], -1), np.tril(A1[:m], -1)) and np.array_equal(got[m:], A1[m:]), "wrote outside the upper triangle"
        assert np.array_equal(d2.get(), A2), "R2 was modified"
        scale = np.abs(Rref).max()
        assert np.abs(R.T @ R - Rref.T @ Rref).max() <= 1e-12 * scale * scale * m
        assert np.abs(np.abs(np.diag(R)) - np.abs(np.diag(Rref))).max() <= 1e-11 * scale


def case_qr_r_only(hk, shapes, seed=71):
    """hssk_qr_desc.r_only: the upper triangle of the factored panel equals the one of the full factorisation; the register
    kernels leave what is below it alone.  shapes: (rows, cols)"""
    r = rng(seed)
    full, ronly, keep = [], [], []
    for (rows, cols) in shapes:
        A = r.standard_normal((rows, cols))
        d1, d2 = hk.array(A), hk.array(A)
        w1, w2 = hk.empty((rows + cols,)), hk.empty((rows + cols,))
        keep.append((A, d1, d2, w1, w2))
        full.append(K.QrDesc(d1.ptr, rows, rows, cols, None, rows, 0, None, w1.ptr, 0, 0.0, 0.0, 0))
        ronly.append(K.QrDesc(d2.ptr, rows, rows, cols, None, rows, 0, None, w2.ptr, 0, 0.0, 0.0, 1))
    hk.batch("hssk_qr_vbatched", full)
    hk.batch("hssk_qr_vbatched", ronly)
    hk.sync()
    for (A, d1, d2, w1, w2) in keep:
        F, R = d1.get(), d2.get()
        assert np.array_equal(np.triu(F), np.triu(R))
        low = np.tril(R, -1)
        assert np.array_equal(low, np.tril(A, -1)) or np.array_equal(low, np.tril(F, -1))   # untouched, or the full write-back


def case_contract_codes(hk):
    """Return code 2 (caller composes the step from other entry points) of the size-limited kernels, and empty work."""
    import ctypes as C_
    d = hk.array(np.zeros((300, 300)))
    i = hk.array(np.arange(300, dtype=np.int32))

    def rc(fn, desc):
        arr = (type(desc) * 1)(desc)
        return getattr(hk.lib, fn)(hk.ctx, arr, 1)
    assert rc("hssk_ulv_split", K.UlvSplitDesc(d.ptr, 300, 257, 10, i.ptr, d.ptr, 10, d.ptr, 10, d.ptr, 257)) == 2
    assert rc("hssk_ulv_split", K.UlvSplitDesc(d.ptr, 300, 0, 0, i.ptr, d.ptr, 1, d.ptr, 1, d.ptr, 1)) == 0
    assert rc("hssk_tpqr_vbatched", K.TpqrDesc(d.ptr, 300, d.ptr, 300, 225)) == 2
    assert rc("hssk_tpqr_vbatched", K.TpqrDesc(d.ptr, 300, d.ptr, 300, 0)) == 0
    # a combine with nothing to write, and one whose product has no operand
    assert rc("hssk_gather_combine", K.CombineDesc(d.ptr, None, 300, 300, None, None, None, 300, 300, None, None, 1, 1, 1.0, d.ptr, 300, 0, 5, 3)) == 0
    assert rc("hssk_gather_combine", K.CombineDesc(d.ptr, None, 300, 300, None, None, None, 300, 300, None, None, 1, 1, 1.0, d.ptr, 300, 4, 5, 3)) == 2
    hk.sync()


def case_expand_image(hk):
    """hssk_expand_image: double-precision real image of float / complex blocks with padded leading dimensions, through the
    byte-oriented upload (hssk_h2d_bytes_async) of a strided host block."""
    rng = np.random.default_rng(11)
    rows, cols, lds, ldd = 37, 9, 41, 83
    for dt, code in ((np.float32, 1), (np.complex64, 2), (np.complex128, 3)):
        host = rng.standard_normal((lds + 2, cols)).astype(dt)
        if code > 1:
            host = (host + 1j * rng.standard_normal(host.shape)).astype(dt)
        host = np.asfortranarray(host)
        w = 2 if code > 1 else 1
        es = np.dtype(dt).itemsize
        src = hk.empty((lds, cols), dt)
        # rows [1, rows + 1) of the host block: pitch (lds + 2) scalars on the host, lds scalars on the device
        hk.check(hk.lib.hssk_h2d_bytes_async(hk.ctx, src.ptr, lds * es, host.ctypes.data + es, (lds + 2) * es, rows * es, cols))
        hk.check(hk.lib.hssk_copy_fence(hk.ctx))
        dst = hk.array(np.full((ldd, w * cols), 5.0))
        hk.check(hk.lib.hssk_expand_image(hk.ctx, dst.ptr, ldd, src.ptr, lds, rows, cols, code))
        hk.sync()
        got = dst.get()
        Z = host[1:rows + 1]
        if code == 1:
            want = Z.astype(np.float64)
        else:
            want = np.zeros((2 * rows, 2 * cols))
            want[0::2, 0::2], want[1::2, 0::2] = Z.real, Z.imag
            want[0::2, 1::2], want[1::2, 1::2] = -Z.imag, Z.real
        assert np.array_equal(got[:w * rows], want)
        assert np.all(got[w * rows:] == 5.0)
        assert hk.lib.hssk_expand_image(hk.ctx, dst.ptr, w * rows - 1, src.ptr, lds, rows, cols, code) == 2
    assert hk.lib.hssk_expand_image(hk.ctx, dst.ptr, ldd, src.ptr, lds, rows, cols, 0) == 2
    assert hk.lib.hssk_expand_image(hk.ctx, dst.ptr, ldd, src.ptr, lds, 0, cols, 1) == 0
    assert hk.lib.hssk_h2d_bytes_async(hk.ctx, src.ptr, 8, host.ctypes.data, 16, 12, 2) == 2


def case_upload_two_threads(hk):
    """Two contexts on two host threads upload strided pageable blocks at the same time: the packing threads behind the
    bounce ring are shared by all contexts of the process and take one job at a time."""
    import threading
    hk2 = K.Hssk(hk.lib._name)
    rows, cols, pad = 1100, 1100, 3          # 9.7 MB per block: above the size that goes to the packing threads
    errs = []

    def work(h, seed):
        try:
            rng = np.random.default_rng(seed)
            dst = h.empty((rows, cols))
            for it in range(4):
                src = np.asfortranarray(rng.standard_normal((rows + pad, cols)))
                h.check(h.lib.hssk_h2d_block_async(h.ctx, dst.ptr, rows, src.ctypes.data + 8, rows + pad, rows, cols))
                h.check(h.lib.hssk_copy_fence(h.ctx))
                h.sync()
                if not np.array_equal(dst.get(), src[1:rows + 1]):
                    errs.append("thread %d, upload %d: wrong data" % (seed, it))
            dst.free()
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))
    th = [threading.Thread(target=work, args=(h, k)) for k, h in enumerate((hk, hk2))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    hk2.close()
    assert not errs, errs


def case_sketch_gen(hk, m, n, k, j0, trans, kind=1, alpha=1.0, beta=0.0, lda_pad=0, seed=2):
    """hssk_sketch_gen (op(B) evaluated inside the kernel from a formula) against hssk_dgemm on the written-out block of the
    same matrix: BITWISE equal (same tiles, K-split and summation order), and equal to numpy to rounding.
    Generated block: op(G)(kk, j) = trans ? G(j0 + j, kk) : G(kk, j0 + j), G = the Toeplitz test matrix."""
    r = rng(seed)
    A = r.standard_normal((m + lda_pad, k))
    C0 = r.standard_normal((m + 2, n))
    g = K.Gen(kind, 0, (C.c_double * 4)(0, 0, 0, 0))
    ii, jj = np.arange(k)[:, None], (j0 + np.arange(n))[None, :]
    G = 1.0 / (1.0 + np.abs(ii - jj))          # G(kk, j0 + j): symmetric unless kind 2
    if kind == 2:
        G = np.where((jj > ii) if trans else (ii > jj), 0.0, G)   # upper triangle: G(i, j) = 0 for i > j
    # the stored block through the library's own fill (also checked against numpy)
    ldb = k + (k & 1)
    dB = hk.array(np.zeros((ldb, n)))
    hk.check(hk.lib.hssk_gen_fill(hk.ctx, C.byref(g), dB.ptr, k, n, ldb, 0, j0, int(trans)))
    hk.sync()
    assert np.array_equal(dB.get()[:k], G), "gen_fill"
    dA, dC1, dC2 = hk.array(A), hk.array(C0), hk.array(C0)
    hk.check(hk.lib.hssk_sketch_gen(hk.ctx, C.byref(g), int(trans), m, n, k, j0, alpha, dA.ptr, A.shape[0], beta, dC1.ptr, C0.shape[0]))
    hk.check(hk.lib.hssk_dgemm(hk.ctx, 0, m, n, k, alpha, dA.ptr, A.shape[0], dB.ptr, ldb, beta, dC2.ptr, C0.shape[0]))
    hk.sync()
    got, dense = dC1.get(), dC2.get()
    ref = C0.copy()
    ref[:m] = alpha * (A[:m] @ G) + (beta * C0[:m] if beta != 0 else 0)
    assert np.abs(got - ref).max() <= 1e-13 * max(k, 1) * max(1.0, np.abs(ref).max()), f"sketch_gen m={m} n={n} k={k}"
    return np.array_equal(got, dense)


def case_gen_elems(hk, seed=4):
    r = rng(seed)
    n = 500
    I = r.permutation(n)[:37].astype(np.int32)
    J = r.permutation(n)[:29].astype(np.int32)
    for kind in (1, 2):
        g = K.Gen(kind, 0, (C.c_double * 4)(0, 0, 0, 0))
        dI, dJ = hk.array(I), hk.array(J)
        dB, dBt, dD = hk.array(np.zeros((40, 29))), hk.array(np.zeros((29, 37))), hk.array(np.zeros((50, 50)))
        descs = [K.ElemDesc(None, 0, dI.ptr, dJ.ptr, 0, 0, dB.ptr, 37, 29, 40, 0, 0, 0, 0, 0),
                 K.ElemDesc(None, 0, dI.ptr, dJ.ptr, 0, 0, dBt.ptr, 37, 29, 29, 1, 0, 0, 0, 0),
                 K.ElemDesc(None, 0, None, None, 100, 120, dD.ptr, 50, 50, 50, 0, 0, 0, 0, 0)]
        arr = (K.ElemDesc * len(descs))(*descs)
        hk.check(hk.lib.hssk_gen_elems(hk.ctx, C.byref(g), arr, len(descs)))
        hk.sync()
        T = 1.0 / (1.0 + np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]))
        if kind == 2:
            T = np.triu(T)
        assert np.array_equal(dB.get()[:37], T[np.ix_(I, J)])
        assert np.array_equal(dBt.get(), T[np.ix_(I, J)].T)
        assert np.array_equal(dD.get(), T[100:150, 120:170])


def case_colsets(hk, universe=5000, seed=81):
    """hssk_colsets vs numpy: sorted unique ids of one or two lists, ids inside [lo, hi) and negative ones dropped; leaf form
    (a k x m block of neighbour ids) and inner form (two sorted sets); empty results; the count word."""
    r = np.random.default_rng(seed)
    cases = []
    ann = r.integers(-1, universe, size=(64 * 300,)).astype(np.int32)          # a leaf of 300 points, 64 neighbours each
    cases.append((ann, None, 1200, 1500))
    a = np.unique(r.integers(0, universe, 4000)).astype(np.int32)
    b = np.unique(r.integers(0, universe, 2500)).astype(np.int32)
    cases.append((a, b, 1000, 1900))
    cases.append((a[:7], b[:1], 0, 0))
    cases.append((np.arange(10, 20, dtype=np.int32), None, 10, 20))           # everything inside: empty
    cases.append((np.array([universe - 1, 0, universe - 1, 31, 32, 33], dtype=np.int32), np.array([0, 63, 64], dtype=np.int32), 5, 6))
    descs, keep = [], []
    for s0, s1, lo, hi in cases:
        d0 = hk.array(s0)
        d1 = hk.array(s1) if s1 is not None else None
        out = hk.array(np.full(len(s0) + (len(s1) if s1 is not None else 0) + 1, -7, dtype=np.int32))
        cnt = hk.array(np.full(1, -3, dtype=np.int32))
        keep.append((d0, d1, out, cnt))
        descs.append(K.ColsetDesc(d0.ptr, d1.ptr if d1 is not None else None, len(s0), len(s1) if s1 is not None else 0, lo, hi, out.ptr, cnt.ptr))
    arr = (K.ColsetDesc * len(descs))(*descs)
    hk.check(hk.lib.hssk_colsets(hk.ctx, arr, len(descs), universe))
    hk.sync()
    for (s0, s1, lo, hi), (d0, d1, out, cnt) in zip(cases, keep):
        allv = np.concatenate([s0, s1]) if s1 is not None else s0
        ref = np.unique(allv[(allv >= 0) & ((allv < lo) | (allv >= hi))])
        c = int(cnt.get()[0])
        got = out.get()
        assert c == len(ref), (c, len(ref))
        assert np.array_equal(got[:c], ref)
        assert np.all(got[c:] == -7)
    # a universe beyond the LDS bitmap is refused, not mis-answered
    assert hk.lib.hssk_colsets(hk.ctx, arr, 1, 40_000_000) == 2

