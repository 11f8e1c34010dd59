"""Checks of the native single-precision sketch shared by the GPU tests (product library) and the CPU tests (the same sources
on the fiber emulator): the kernels hssk_sgemm_sketch / hssk_gather_elems_f32 / hssk_narrow_f32 against numpy, and the
SPX_s_struct_from_dense_device entry against the reference's float fixture, the promoted host path and dense algebra."""
import ctypes as C
import os

import numpy as np

import hss_cases as HC
from strumpack_amd import capi
from strumpack_amd import hssk as K

U32 = 2.0 ** -24
HSSK_DT_F32 = 1


# ---- kernels ------------------------------------------------------------------------------------------------------------
def _fmaf_chain(A32, opB32, cols):
    """plain k-ordered float32 chain over the whole k for the output columns `cols`: float64 product (exact for float32
    factors), one rounding to float32 per step"""
    acc = np.zeros((A32.shape[0], len(cols)), dtype=np.float32)
    a64 = A32.astype(np.float64)
    b64 = opB32[:, cols].astype(np.float64)
    for kk in range(A32.shape[1]):
        acc = (acc.astype(np.float64) + a64[:, kk][:, None] * b64[kk][None, :]).astype(np.float32)
    return acc.astype(np.float64)


def case_sgemm(hk, m, n, k, transB, alpha=1.0, beta=0.0, lda_pad=5, ldb_pad=1, seed=1):
    """hssk_sgemm_sketch against fl32(A) op(B) in float64: the worst-case FP32 bound elementwise, for k >= 1024 the normwise
    error against that of a plain float32 fmaf chain, and bitwise equal results of two calls.  Returns the measured ratio."""
    r = np.random.default_rng(seed)
    A = r.standard_normal((m + lda_pad, k))
    B = r.standard_normal((n + ldb_pad, k) if transB else (k + ldb_pad, n), dtype=np.float32)
    Cm = r.standard_normal((m + 2, n))
    dA, dB = hk.array(A), hk.array(B, dtype=np.float32)
    outs = []
    for _ in range(2):
        dC = hk.array(Cm)
        hk.check(hk.lib.hssk_sgemm_sketch(hk.ctx, int(transB), m, n, k, alpha, dA.ptr, A.shape[0], dB.ptr, B.shape[0],
                                          beta, dC.ptr, Cm.shape[0]))
        hk.sync()
        outs.append(dC.get())
        dC.free()
    dA.free()
    dB.free()
    got = outs[0]
    tag = f"sgemm m={m} n={n} k={k} transB={transB} alpha={alpha} beta={beta} pads=({lda_pad},{ldb_pad})"
    assert np.array_equal(outs[0], outs[1]), tag + ": two calls differ"
    assert np.array_equal(got[m:], Cm[m:]), tag + ": rows beyond m were written"
    A32 = A[:m].astype(np.float32)
    opB = B[:n].T if transB else B[:k]          # k x n view, float32
    a64, aabs = A32.astype(np.float64), np.abs(A32).astype(np.float64)
    worst = 0.0
    ref = np.empty((m, n))
    for c0 in range(0, n, 4096):                # (column blocks: the float64 copies of a large operand stay small)
        b64 = opB[:, c0:c0 + 4096].astype(np.float64)
        rb = alpha * (a64 @ b64) + (beta * Cm[:m, c0:c0 + 4096] if beta != 0 else 0)
        bound = (k + 4) * U32 * abs(alpha) * (aabs @ np.abs(b64)) + 4 * 2.0 ** -53 * np.abs(rb)
        diff = np.abs(got[:m, c0:c0 + 4096] - rb)
        bad = diff > bound
        assert not bad.any(), tag + f": {int(bad.sum())} entries beyond the elementwise FP32 bound, first at {np.argwhere(bad)[0]} (+{c0})"
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, diff / bound, 0.0))))
        ref[:, c0:c0 + 4096] = rb
    ratio = None
    if k >= 1024:
        cols = np.unique(np.linspace(0, n - 1, min(n, 64)).astype(int)) if n < 64 * 2 else \
            np.sort(np.random.default_rng(seed + 7).choice(n, 64, replace=False))
        chain = alpha * _fmaf_chain(A32, opB, cols) + (beta * Cm[:m][:, cols] if beta != 0 else 0)
        nref = np.linalg.norm(ref[:, cols])
        e_kernel = np.linalg.norm(got[:m][:, cols] - ref[:, cols]) / nref
        e_chain = np.linalg.norm(chain - ref[:, cols]) / nref
        ratio = e_kernel / e_chain
        print(f"{tag}: normwise error {e_kernel:.3e}, float32 fmaf chain {e_chain:.3e}, ratio {ratio:.3f}; "
              f"largest fraction of the elementwise bound {worst:.2e}")
        assert e_kernel <= 2 * e_chain, tag + f": normwise error {e_kernel:.3e} is {ratio:.2f} x that of a float32 fmaf chain ({e_chain:.3e})"
    else:
        print(f"{tag}: largest fraction of the elementwise bound {worst:.2e}")
    return ratio


def case_gather_elems_f32(hk, seed=4):
    """hssk_gather_elems_f32 against numpy fancy indexing on a float matrix: index lists, contiguous ranges, transpose and
    ownership windows; exact."""
    r = np.random.default_rng(seed)
    n, lda = 150, 157
    A = r.standard_normal((lda, n)).astype(np.float32)
    dA = hk.array(A, dtype=np.float32)
    keep, descs, expect = [dA], [], []

    def add(I, J, i0, j0, m, nn, transpose, win=(0, 0, 0, 0), pad=3):
        gi = np.asarray(I) if I is not None else np.arange(i0, i0 + m)
        gj = np.asarray(J) if J is not None else np.arange(j0, j0 + nn)
        ref = A[np.ix_(gi, gj)].astype(np.float64)
        rlo, rhi, clo, chi = win
        if rhi > rlo:
            ref[(gi < rlo) | (gi >= rhi), :] = 0.
        if chi > clo:
            ref[:, (gj < clo) | (gj >= chi)] = 0.
        if transpose:
            ref = ref.T.copy()
        ldb = ref.shape[0] + pad
        dB = hk.array(np.full((ldb, ref.shape[1]), -9.0))
        dI = hk.array(gi.astype(np.int32), dtype=np.int32) if I is not None else None
        dJ = hk.array(gj.astype(np.int32), dtype=np.int32) if J is not None else None
        keep.extend([dB, dI, dJ])
        descs.append(K.ElemDesc(dA.ptr, lda, dI.ptr if dI else None, dJ.ptr if dJ else None, i0, j0, dB.ptr, m, nn, ldb,
                                int(transpose), rlo, rhi, clo, chi))
        expect.append((dB, ref))

    I1, J1 = r.permutation(n)[:37], r.permutation(n)[:21]
    add(I1, J1, 0, 0, 37, 21, False)
    add(I1, J1, 0, 0, 37, 21, True)
    add(None, None, 11, 40, 64, 50, False)
    add(None, None, 0, 0, 70, 45, True, pad=0)          # (large enough for a tiled transposed gather)
    add(None, J1, 100, 0, 50, 21, False)
    add(I1, None, 0, 3, 37, 9, False)
    add(I1, J1, 0, 0, 37, 21, False, win=(30, 120, 0, 0))
    add(None, None, 5, 5, 40, 33, True, win=(0, 0, 10, 20))
    add(I1, J1, 0, 0, 37, 21, False, win=(20, 90, 50, 140))
    add(None, None, 149, 149, 1, 1, False)
    hk.batch("hssk_gather_elems_f32", descs)
    hk.sync()
    for q, (dB, ref) in enumerate(expect):
        got = dB.get()
        assert np.array_equal(got[:ref.shape[0]], ref), f"gather_elems_f32 request {q}"
        assert np.all(got[ref.shape[0]:] == -9.0), f"gather_elems_f32 request {q}: rows beyond the block were written"
    for d in keep:
        if d is not None:
            d.free()


def case_narrow_f32(hk, seed=5):
    """hssk_narrow_f32 followed by hssk_expand_image(HSSK_DT_F32) equals src.astype(float32).astype(float64) exactly"""
    r = np.random.default_rng(seed)
    for (rows, cols, lds, ldd, ldx) in [(300, 17, 300, 300, 300), (129, 40, 140, 133, 131), (1, 1, 4, 2, 3), (70, 260, 70, 71, 75)]:
        src = r.standard_normal((lds, cols)) * 10.0 ** r.integers(-30, 30, (lds, cols))
        src[0, 0] = 1.0 + 2.0 ** -30                        # (rounds to 1.0f)
        dS = hk.array(src)
        dF = hk.array(np.full((ldd, cols), -5.0, dtype=np.float32), dtype=np.float32)
        dX = hk.array(np.full((ldx, cols), -7.0))
        hk.check(hk.lib.hssk_narrow_f32(hk.ctx, dF.ptr, ldd, dS.ptr, lds, rows, cols))
        hk.check(hk.lib.hssk_expand_image(hk.ctx, dX.ptr, ldx, dF.ptr, ldd, rows, cols, HSSK_DT_F32))
        hk.sync()
        with np.errstate(over="ignore"):
            want32 = src[:rows].astype(np.float32)
        f, x = dF.get(), dX.get()
        assert np.array_equal(f[:rows], want32) and np.all(f[rows:] == -5.0), (rows, cols)
        assert np.array_equal(x[:rows], want32.astype(np.float64)) and np.all(x[rows:] == -7.0), (rows, cols)
        for d in (dS, dF, dX):
            d.free()


# ---- the C interface -----------------------------------------------------------------------------------------------------
def s_options(L, rel_tol, abs_tol, leaf, max_rank=None):
    o = capi.CSPOptions()
    L.SP_s_struct_default_options(C.byref(o))
    o.type, o.rel_tol, o.abs_tol, o.leaf_size, o.verbose = capi.SP_TYPE_HSS, rel_tol, abs_tol, leaf, 0
    if max_rank is not None:
        o.max_rank = max_rank
    return o


def _err(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b)


def _fixture():
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scz_golden.npz"))
    n, leaf, rtol, _ = G["s_0_meta"]
    return G, int(n), int(leaf), float(rtol)


def check_fixture(L, hk, precision):
    """the reference's float fixture s_0 through the device entry: the assertions and tolerances of hss_cases.check_scz"""
    G, n, leaf, rtol = _fixture()
    A = HC.scz_matrix("s", n)
    B, Yref, Ycref, Xref = G["s_0_B"], G["s_0_Y"], G["s_0_Yc"], G["s_0_X"]
    lda = n + 4                                           # (a leading dimension larger than the row count)
    Ap = np.zeros((lda, n), dtype=np.float32, order="F")
    Ap[:n] = A
    dA = hk.array(Ap, dtype=np.float32)
    H = capi.StructuredMatrixF32.from_dense_device(L, dA.ptr, n, lda, s_options(L, rtol, 1e-10, leaf), None, precision)
    assert H.sketch_route() == precision
    assert H.rows() == n and L.SP_s_struct_cols(H.h) == n and 0 < H.rank() < n // 2
    assert H.memory() > 0 and H.nonzeros() > 0
    st = H.stats()
    assert st["rounds"] >= 1 and st["t_compress"] > 0
    if precision == 1:
        assert st["sketch_kernel_bytes"] >= 2 * 4.0 * n * n
    AB = A.astype(np.float64) @ B
    eps = 3e-6
    Y, Yc, Yt = H.mult(B, "N"), H.mult(B, "C"), H.mult(B, "T")
    ref_err = _err(Yref, AB)
    assert _err(Y, AB) <= max(2 * ref_err, 10 * rtol) + eps
    assert _err(Y, Yref) <= 10 * rtol + eps
    assert _err(Yc, Ycref) <= 10 * rtol + eps
    assert _err(Yt, A.T.astype(np.float64) @ B) <= 10 * rtol + eps
    H.factor()
    X = H.solve(B)
    assert _err(X, Xref) <= 50 * rtol + eps
    assert _err(A.astype(np.float64) @ X, B) <= 50 * rtol + eps
    sig = 0.75
    H.shift(sig)
    H.factor()
    X = H.solve(B)
    assert _err((A.astype(np.float64) + sig * np.eye(n)) @ X, B) <= 50 * rtol + eps
    H.destroy()
    assert H.h is None
    dA.free()


def check_exact_route_vs_host(L, hk):
    """precision 2 against the promoted host path (SP_s_struct_from_dense) on the same matrix and options: the same FP64
    arithmetic on the same widened entries, the same random stream (both draw the engine's seeded Gaussian block)"""
    G, n, leaf, rtol = _fixture()
    A = HC.scz_matrix("s", n)
    B = G["s_0_B"]
    o = s_options(L, rtol, 1e-10, leaf)
    dA = hk.array(A, dtype=np.float32)
    Hd = capi.StructuredMatrixF32.from_dense_device(L, dA.ptr, n, n, o, None, 2)
    Hh = capi.StructuredMatrixF32.from_dense(L, A, o)
    assert Hd.sketch_route() == 2 and Hh.sketch_route() == 0
    assert Hd.rank() == Hh.rank()
    # (both paths draw the engine's seeded Gaussian block: the same random stream.  The handles return floats; equal FP64
    #  results round to equal floats, so the comparison is at the 1e-10 the FP64 arithmetic warrants)
    Yd, Yh = Hd.mult(B).astype(np.float64), Hh.mult(B).astype(np.float64)
    assert _err(Yd, Yh) <= 1e-10, _err(Yd, Yh)
    Hd.factor()
    Hh.factor()
    Xd, Xh = Hd.solve(B).astype(np.float64), Hh.solve(B).astype(np.float64)
    assert _err(Xd, Xh) <= 1e-10, _err(Xd, Xh)
    Hd.destroy()
    Hh.destroy()
    dA.free()


def check_auto_rule(L, hk):
    """n = 700: (700 + 4) 2^-24 = 4.2e-5 lies between rel_tol = 1e-3 (route 1) and 1e-6 (route 2)"""
    n, leaf = 700, 64
    A = HC.scz_matrix("s", n)
    dA = hk.array(A, dtype=np.float32)
    B = np.random.default_rng(2).standard_normal((n, 3)).astype(np.float32)
    AB = A.astype(np.float64) @ B
    for rtol, route in ((1e-3, 1), (1e-6, 2)):
        H = capi.StructuredMatrixF32.from_dense_device(L, dA.ptr, n, n, s_options(L, rtol, 1e-10, leaf), None, 0)
        assert H.sketch_route() == route, (rtol, H.sketch_route())
        e = _err(H.mult(B), AB)
        assert e <= 10 * rtol + 3e-6, (rtol, e)
        H.destroy()
    dA.free()


def check_errors(L, hk):
    """SP_TYPE_BLR, a non-square shape and precision 7 each return 1 and leave *S untouched"""
    n = 96
    dA = hk.array(HC.scz_matrix("s", n), dtype=np.float32)
    o = s_options(L, 1e-3, 1e-10, 32)
    sentinel = 0x1234
    for (rows, cols, typ, prec) in ((n, n, capi.SP_TYPE_BLR, 1), (n, n - 1, capi.SP_TYPE_HSS, 1), (n, n, capi.SP_TYPE_HSS, 7)):
        o.type = typ
        h = C.c_void_p(sentinel)
        assert L.SPX_s_struct_from_dense_device(C.byref(h), rows, cols, dA.ptr, n, C.byref(o), None, prec) == 1
        assert h.value == sentinel
    o.type = capi.SP_TYPE_HSS
    h = C.c_void_p()
    assert L.SPX_s_struct_from_dense_device(C.byref(h), n, n, dA.ptr, n, C.byref(o), None, 1) == 0
    L.SP_s_struct_destroy(C.byref(h))
    dA.free()


def check_tree_pass(L, hk, n=1024, leaf=32):
    """a float compress whose ranks fit the single-launch tree pass uses it (hssk_elem_src.use_gen == 2) and does not fall back;
    the double path takes the same pass at this size"""
    A = HC.scz_matrix("s", n)
    o = s_options(L, 1e-4, 1e-10, leaf)
    dA64 = hk.array(A.astype(np.float64))
    l0, f0 = L.SPX_tree_pass_launches(), L.SPX_tree_pass_fallbacks()
    Hd = capi.StructuredMatrix.from_dense_device(L, dA64.ptr, n, n, o, None)
    l1, f1 = L.SPX_tree_pass_launches(), L.SPX_tree_pass_fallbacks()
    assert l1 > l0 and f1 == f0, "the double path does not take the single-launch pass at this size"
    rank64 = Hd.rank()
    Hd.destroy()
    dA64.free()
    dA = hk.array(A, dtype=np.float32)
    for prec in (1, 2):
        H = capi.StructuredMatrixF32.from_dense_device(L, dA.ptr, n, n, o, None, prec)
        l2, f2 = L.SPX_tree_pass_launches(), L.SPX_tree_pass_fallbacks()
        assert l2 > l1 and f2 == f1, (prec, l1, l2, f1, f2)
        assert abs(H.rank() - rank64) <= 2
        l1 = l2
        H.destroy()
    dA.free()


def toeplitz_inf_norm(n):
    """largest absolute row sum of A(i, j) = 1 / (1 + |i - j|)"""
    h = np.concatenate([[0.0], np.cumsum(1.0 / (1.0 + np.arange(1, n)))])    # h[q] = sum_{d=1..q} 1 / (1 + d)
    i = np.arange(n)
    return float(np.max(1.0 + h[i] + h[n - 1 - i]))


def device_toeplitz_f32(hk, n, panel=2048):
    """the float Toeplitz operand in HBM, made from hssk_fill_toeplitz_block panels through hssk_narrow_f32"""
    dA = hk.empty((n, n), dtype=np.float32)
    dP = hk.empty((n, panel))
    for c0 in range(0, n, panel):
        nc = min(panel, n - c0)
        hk.check(hk.lib.hssk_fill_toeplitz_block(hk.ctx, dP.ptr, n, nc, n, 0, c0, b"T"))
        hk.check(hk.lib.hssk_narrow_f32(hk.ctx, dA.at(0, c0), n, dP.ptr, n, n, nc))
    hk.sync()
    dP.free()
    return dA


def check_full_size(L, hk, n=32768, rel_tol=1e-4, precision=1):
    """N = 32768 float Toeplitz in HBM, the options and bars of test_hss_gpu.test_sjlt_sketch_full_size; the residual bar
    adds what the three roundings to float at the SP_s_ boundary (X out, Y out, b in) can add at most:
    |Y - b| <= 1.01 2^-24 (|A|_inf |X| + 2 |b|) + 1e-12 |b|   (|A|_inf bounds |A|_2: A is symmetric; 1.01 covers
    |H| <= (1 + 10 rtol) |A|)"""
    dA = device_toeplitz_f32(hk, n)
    o = s_options(L, rel_tol, 1e-8, 256, max_rank=50000)
    H = capi.StructuredMatrixF32.from_dense_device(L, dA.ptr, n, n, o, None, precision)
    rank = H.rank()
    print(f"full size n={n} rel_tol={rel_tol} precision={precision}: rank {rank}")
    assert H.sketch_route() == precision
    assert 26 <= rank <= 40, rank
    st = H.stats()
    if precision == 1:
        assert st["sketch_kernel_bytes"] >= 2 * 4.0 * n * n
    rng = np.random.default_rng(0)
    cols = rng.integers(0, n, 16)
    E = np.zeros((n, 16), dtype=np.float32)
    E[cols, np.arange(16)] = 1.0
    i = np.arange(n)
    Acols = 1.0 / (1.0 + np.abs(i[:, None] - cols[None, :]))
    err = np.linalg.norm(H.mult(E).astype(np.float64) - Acols) / np.linalg.norm(Acols)
    print(f"  16 columns against the exact ones: {err:.3e}")
    assert err < 2e-4, err
    H.factor()
    b = rng.standard_normal((n, 2)).astype(np.float32)
    X = H.solve(b)
    Y = H.mult(X)
    b64, X64 = b.astype(np.float64), X.astype(np.float64)
    res = np.linalg.norm(Y.astype(np.float64) - b64)
    bar = 1.01 * U32 * (toeplitz_inf_norm(n) * np.linalg.norm(X64) + 2 * np.linalg.norm(b64)) + 1e-12 * np.linalg.norm(b64)
    print(f"  residual {res:.3e}, bar {bar:.3e}")
    assert res <= bar, (res, bar)
    H.destroy()
    dA.free()
    return rank
