#!/usr/bin/env python
"""Fixture of kernel ridge regression beyond R^64, produced by the REFERENCE itself (oracle/_ref, built by oracle/ref/Makefile)
in the pattern of make_golden_kernel.py -- run in the build container only:

    LD_LIBRARY_PATH=/usr/lib/x86_64-linux-gnu:/opt/conda/lib MKL_THREADING_LAYER=GNU python tests/golden/make_golden_kernel_highdim.py

One Gauss case: n = 1500 points in R^100 (seeded: a few Gaussian clusters whose spread lives in a 3-dimensional subspace,
tests/highdim_cases.clustered_points, rounded to float so that the fixture holds them exactly), h = sqrt(d), lambda = 1,
leaves of 128, 2-means clustering, 64 approximate neighbours.
Outputs: tests/golden/kernel_highdim_golden.json (+ .npz: the points, labels, test points, and the reference's permutation,
weights and predictions).

The order of the points.  The reference's Kernel::permute() (kernel/Kernel.hpp, data_.lapmr(perm_, true)) applies the POINT
permutation to the d FEATURE rows of the training set: xLAPMR follows the cycles of perm[0:d] through the entries that are <= d.
At d = 8 and n >= 400 that almost never moves a row (tests/kernel_golden.py treats the cases where it does); at d = 100 and
n = 1500 each of the first 100 entries is <= 100 with probability 1/15, so some rows nearly always move.  The reference's kernel
matrix is invariant under that, but its randomized neighbour search projects the coordinates on random directions and is not:
it then runs on other numbers than a search on the caller's points, finds other lists, and the column samples, ranks and
weights follow.  That is a property of the reference's data handling, not of
the search, so the fixture takes the points in an order in which the quirk is dormant: points among the first d of the input that the
clustering puts among its first d are exchanged with later ones until none is left.  This file asserts that the reference's
stored points then ARE the caller's points in cluster order, and that the product's host search on them equals the
reference's lists bit for bit; it also records, for the record, how many feature rows the unmodified order moves.

rel_tol = 1e-4: the device-neighbour test compares weights fitted on ANOTHER column sample (exact instead of approximate
neighbours) under the allowance 2e-2 of tests/test_kernel_gpu.py; two samples agree to about the compression tolerance times the
condition number of K + lambda I (here ~ 1e2 .. 1e3), which 1e-4 keeps an order of magnitude inside that allowance and 1e-2 does not.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import ref_lib as R  # noqa: E402
import highdim_cases as HD  # noqa: E402

L = R.lib()
vp = C.c_void_p
L.ref_kernel_regression.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_double, C.c_double, C.c_int,
                                    C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, vp, vp, vp]
L.ref_kernel_hss_create.restype = vp
L.ref_kernel_hss_create.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
L.ref_kernel_hss_destroy.argtypes = [vp]
L.ref_kernel_hss_info.argtypes = [vp, vp]
L.ref_kernel_hss_node_info.argtypes = [vp, vp, C.c_int]
L.ref_kernel_hss_data.argtypes = [vp, vp, vp]
L.ref_clustering.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int]
L.ref_ann.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp]

N, M, D, LEAF, ANN, RTOL, LAM, CLUSTERING = 1500, 100, 100, 128, 64, 1e-4, 1.0, 1
H = float(np.float32(np.sqrt(D)))


def cluster_perm(X):
    a = np.ascontiguousarray(X).copy()
    perm, ls = np.zeros(N, np.int32), np.zeros(4096, np.int32)
    L.ref_clustering(N, D, a.ctypes.data, CLUSTERING, LEAF, perm.ctypes.data, ls.ctypes.data, 4096)
    return perm


def moved(perm):
    """positions among the first d whose entry xLAPMR would follow: 1-based entries <= d that are no fixed points"""
    return [i for i in range(D) if perm[i] <= D and perm[i] != i + 1]


X, y, T = HD.clustered_points(2100, N, M, D)
X, T = X.astype(np.float32).astype(np.float64), T.astype(np.float32).astype(np.float64)
r = np.random.default_rng(7)
perm = cluster_perm(X)
moved_unmodified = len(moved(perm))


def ref_ann(P, k=ANN):
    P = np.ascontiguousarray(P)
    ids, sc = np.zeros((N, k), np.uint32), np.zeros((N, k))
    L.ref_ann(N, D, P.ctypes.data, 5, k, ids.ctypes.data, sc.ctypes.data)
    return ids


def ref_stored_points(X):
    """the points the reference's kernel holds after HSSMatrix(Kernel&, opts), and its permutation"""
    X = np.ascontiguousarray(X)
    Hh = L.ref_kernel_hss_create(N, D, X.ctypes.data, 0, H, LAM, 1, 1e-2, 1e-8, LEAF, 50000, CLUSTERING, ANN, 5)
    data, rperm = np.zeros_like(X), np.zeros(N, np.int32)
    L.ref_kernel_hss_data(Hh, data.ctypes.data, rperm.ctypes.data)
    L.ref_kernel_hss_destroy(Hh)
    return data, rperm


# the cause, shown on the unmodified order with the reference's own routines: its stored points are the caller's points in
# cluster order with feature columns exchanged, and its search finds other lists on them than on the caller's points
if moved_unmodified:
    data0, perm0 = ref_stored_points(X)
    mine0 = X[perm0 - 1]
    assert not np.array_equal(data0, mine0) and np.array_equal(np.sort(data0, axis=1), np.sort(mine0, axis=1))
    a0, b0 = ref_ann(data0), ref_ann(mine0)
    print("unmodified order: %d feature rows moved; %d of %d neighbour lists of the reference's search differ between its stored "
          "points and the caller's points" % (moved_unmodified, int((np.sort(a0, 1) != np.sort(b0, 1)).any(1).sum()), N), flush=True)
for rounds in range(1000):
    bad = moved(perm)
    if not bad:
        break
    for i in bad:                                   # exchange the early input point with a late one
        a, b = perm[i] - 1, int(r.integers(D, N))
        X[[a, b]], y[[a, b]] = X[[b, a]], y[[b, a]]
    perm = cluster_perm(X)
assert not moved(perm), "no order found in which the feature rows stay"
print("feature rows the unmodified order moves:", moved_unmodified, "; exchanges rounds:", rounds, flush=True)

X, y, T = np.ascontiguousarray(X), np.ascontiguousarray(y), np.ascontiguousarray(T)
w, pr = np.zeros(N), np.zeros(M)
info = (C.c_longlong * 4)()
L.ref_kernel_regression(N, D, X.ctypes.data, y.ctypes.data, M, T.ctypes.data, 0, H, LAM, 1, RTOL, 1e-8, LEAF, CLUSTERING, ANN,
                        w.ctypes.data, pr.ctypes.data, C.addressof(info))
Hh = L.ref_kernel_hss_create(N, D, X.ctypes.data, 0, H, LAM, 1, RTOL, 1e-8, LEAF, 50000, CLUSTERING, ANN, 5)
hi = (C.c_longlong * 4)()
L.ref_kernel_hss_info(Hh, hi)
ni = np.zeros((1 << 14, 6), np.int32)
cnt = L.ref_kernel_hss_node_info(Hh, ni.ctypes.data, 1 << 14)
data, rperm = np.zeros_like(X), np.zeros(N, np.int32)
L.ref_kernel_hss_data(Hh, data.ctypes.data, rperm.ctypes.data)
L.ref_kernel_hss_destroy(Hh)
assert np.array_equal(rperm, perm)
assert np.array_equal(data, X[rperm - 1]), "the reference moved feature rows after all"

# the reference's first-round lists on its stored points against the product's host search on the caller's points in cluster order
annl = ref_ann(data)
try:
    from strumpack_amd import kernel as KM
    import emu_lib
    mine = KM.approximate_neighbors(KM.load(emu_lib.build()), X[rperm - 1], ANN, 5)
    print("host search on the caller's points == the reference's lists:", np.array_equal(mine, annl.astype(np.int32)), flush=True)
except Exception as e:      # the emulator library is a convenience here, not a requirement of the fixture
    print("product search not compared:", e)

out = dict(n=N, m=M, d=D, ktype=0, h=H, lam=LAM, p=1, rel_tol=RTOL, leaf=LEAF, clustering=CLUSTERING, ann=ANN,
           compressed=int(hi[0]), levels=int(hi[1]), rank=int(hi[2]), memory=int(hi[3]), nodes=ni[:cnt].tolist(),
           feature_rows_moved_by_the_unmodified_order=moved_unmodified)
json.dump(out, open(os.path.join(HERE, "kernel_highdim_golden.json"), "w"), indent=0)
np.savez_compressed(os.path.join(HERE, "kernel_highdim_golden.npz"), X=X.astype(np.float32), y=y.astype(np.int8),
                    T=T.astype(np.float32), perm=rperm, weights=w, prediction=pr)
print("rank", hi[2], "levels", hi[1], "compressed", hi[0], "memory MB", hi[3] / 1e6)
