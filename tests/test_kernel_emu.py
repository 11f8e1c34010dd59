"""Kernel-matrix front end on the CPU: the product's host code (clustering, tree, orchestration)
and kernel sources (emulated) against fixtures made by the reference, and the numpy oracle against the same."""
import numpy as np
import pytest

import emu_lib
import kernel_golden as KG
from oracle import hss_oracle as O
from strumpack_amd import kernel as KM


@pytest.fixture(scope="module")
def lib():
    return KM.load(emu_lib.build())


@pytest.mark.parametrize("algo", ["2means", "kdtree", "cobble", "natural"])
def test_clustering_matches_reference(lib, algo):
    J, Z = KG.golden()
    X = KG.susy()[0]
    for tag, pts in (("full", X), ("sub1000", X[:1000])):
        g = J["clustering_%s_%s" % (tag, algo)]
        Xp, perm, leaves = KM.clustering(lib, pts, algo, g["leaf"])
        assert np.array_equal(perm, Z["perm_%s_%s" % (tag, algo)])
        assert leaves.tolist() == g["leaves"]
        assert np.array_equal(Xp, pts[perm - 1])


def _serial_tree(X, leaf, split):
    """Serial restatement of binary_tree_clustering's recursion (host/Clustering.hpp: recurse + group_zero_first) with numpy
    splits: returns the 1-based permutation and the leaf sizes."""
    n = len(X)
    perm = np.arange(1, n + 1)
    leaves = []

    def rec(lo, hi):
        m = hi - lo
        if m < leaf:
            leaves.append(m)
            return
        lab = split(X[perm[lo:hi] - 1])
        n0 = int((lab == 0).sum())
        # group_zero_first: the j-th zero-labelled point is swapped into slot j
        loc = perm[lo:hi].copy()
        labc = lab.copy()
        ct = cj = 0
        for _ in range(n0):
            while labc[cj] != 0:
                cj += 1
            if cj != ct:
                loc[[cj, ct]] = loc[[ct, cj]]
                labc[cj] = labc[ct]
                labc[ct] = 0
            cj += 1
            ct += 1
        perm[lo:hi] = loc
        if n0 == 0 or n0 == m:
            leaves.append(m)
            return
        rec(lo, lo + n0)
        rec(lo + n0, hi)

    rec(0, n)
    return perm, leaves


def _median_labels(key):
    n = len(key)
    # std::nth_element leaves an implementation-defined arrangement, but WHICH elements fall below the median position is
    # determined when the keys are distinct
    order = np.argsort(key, kind="stable")
    lab = np.zeros(n, dtype=np.int64)
    lab[order[n // 2:]] = 1
    return lab


def _split_cobble(P):
    cen = np.zeros(P.shape[1])
    for j in range(P.shape[1]):
        cen[j] = np.add.accumulate(P[:, j])[-1] / len(P)       # (left-to-right sum, as the host code)
    first = int(np.argmax(np.sqrt(((P - cen) ** 2).sum(1))))
    return _median_labels(np.sqrt(((P - P[first]) ** 2).sum(1)))


def _split_kd(P):
    ext = P.max(0) - P.min(0)
    return _median_labels(P[:, int(np.argmax(ext))])


@pytest.mark.parametrize("algo,split", [("cobble", _split_cobble), ("kdtree", _split_kd)])
def test_clustering_large_set_on_host_threads(lib, algo, split):
    """70 000 points: the halves of the top splits run on host threads and the passes of the first levels in pieces
    (Clustering.hpp: recurse / for_pieces); the tree must be the serial one.  Leaf sets are compared (the order inside the
    halves of a median split is nth_element's)."""
    r = np.random.default_rng(11)
    X = r.random((70000, 5))
    Xp, perm, leaves = KM.clustering(lib, X, algo, 600)
    assert np.array_equal(Xp, X[perm - 1]) and sorted(perm.tolist()) == list(range(1, 70001))
    rperm, rleaves = _serial_tree(X, 600, split)
    assert leaves.tolist() == rleaves
    off = 0
    for m in rleaves:
        assert set(perm[off:off + m].tolist()) == set(rperm[off:off + m].tolist())
        off += m


@pytest.mark.parametrize("algo", ["cobble", "kdtree"])
def test_clustering_device_form(lib, algo):
    """The median-split partitioners on the device (kernels/hssk_cluster.hip, one launch per tree level): the reference's
    permutation on its own fixture, the host form's on random points; point sets whose answer hangs on ties (a lattice, all
    points equal) or on a long chain of displacements are handed back untouched (status != 0)."""
    J, Z = KG.golden()
    X = KG.susy()[0]
    for tag, pts in (("full", X), ("sub1000", X[:1000])):
        g = J["clustering_%s_%s" % (tag, algo)]
        st, Xp, perm, leaves = KM.clustering_device(lib, pts, algo, g["leaf"])
        if st == 0:   # (the fixture's own data has duplicated values in some coordinates: kd may stand back)
            assert np.array_equal(perm, Z["perm_%s_%s" % (tag, algo)])
            assert leaves.tolist() == g["leaves"]
            assert np.array_equal(Xp, pts[perm - 1])
        else:
            assert algo == "kdtree"
    r = np.random.default_rng(17)
    for pts, leaf in ((r.random((9000, 6)), 100), (r.standard_normal((5000, 3)) * 40 - 7, 64), (r.random((257, 2)), 9)):
        st, Xp, perm, leaves = KM.clustering_device(lib, pts, algo, leaf)
        Xh, ph, lh = KM.clustering(lib, pts, algo, leaf)
        assert st == 0 and np.array_equal(perm, ph) and np.array_equal(Xp, Xh) and leaves.tolist() == lh.tolist()
    # large clusters are split by several workgroups (a launch per step: hssk_cluster.hip, cluster_wide_kernel) -- here from
    # 3000 points on, so that two levels take that form
    import os
    os.environ["HSSK_CLUSTER_WIDE_MIN"] = "3000"
    try:
        for pts, leaf in ((r.random((13001, 5)), 200), (r.standard_normal((9000, 3)) * 40 - 7, 64)):
            st, Xp, perm, leaves = KM.clustering_device(lib, pts, algo, leaf)
            Xh, ph, lh = KM.clustering(lib, pts, algo, leaf)
            assert st == 0 and np.array_equal(perm, ph) and np.array_equal(Xp, Xh) and leaves.tolist() == lh.tolist()
        lat = r.integers(0, 3, (8000, 4)).astype(float)
        st, Xp, perm, leaves = KM.clustering_device(lib, lat, algo, 100)
        assert st > 0 and np.array_equal(Xp, lat)
    finally:
        os.environ.pop("HSSK_CLUSTER_WIDE_MIN")
    # ties: the device form stands back and moves nothing
    for pts in (r.integers(0, 3, (3000, 4)).astype(float), np.ones((500, 3))):
        st, Xp, perm, leaves = KM.clustering_device(lib, pts, algo, 100)
        assert st > 0 and np.array_equal(Xp, pts) and not perm.any()
    # the swap sequence: keys ascending (nothing moves), descending (every point of the upper half moves once), and one large
    # key in front of ascending ones (its point is displaced n / 2 times: beyond what the device follows)
    key = np.sort(r.random(2000))
    for k, expect in ((key, 0), (key[::-1].copy(), 0), (np.concatenate([[2.0], key[:-1]]), 5)):
        pts = np.stack([k, 1e-3 * r.random(2000)], axis=1)
        if algo == "cobble":   # distances from the farthest point order like the first coordinate when that point is the smallest key
            pts = pts.copy()
            pts[:, 0] = 1.0 - pts[:, 0] if expect != 5 else pts[:, 0]
            pts = np.vstack([pts, [[-50.0, 0.0]]]) if expect != 5 else pts
        st, Xp, perm, leaves = KM.clustering_device(lib, pts, algo, 1500)
        if algo == "kdtree":
            assert st == expect
        if st == 0:
            Xh, ph, lh = KM.clustering(lib, pts, algo, 1500)
            assert np.array_equal(perm, ph) and np.array_equal(Xp, Xh)


@pytest.mark.parametrize("algo", ["cobble", "kdtree"])
def test_clustering_device_form_dims(lib, algo):
    """d = 1, 2, 17, 33 and 64 (the kernels keep 64 centre and 128 extent coordinates per cluster), every form of the wide split"""
    import kernel_cases as KC
    KC.case_clustering_dims(KM, lib, algo)


@pytest.mark.parametrize("algo", ["cobble", "kdtree", "pca"])
def test_median_split_fast_selection_is_the_reference_selection(algo):
    """The median splits select on a copy of the keys and make the reference's nth_element call only when equal keys straddle
    the median position (Clustering.hpp: median_labels); with STRUMPACK_AMD_CLUSTER_EXACT_SELECT=1 they always make it.  Same
    permutations either way, on random points and on a lattice with many duplicated points (a subprocess per mode: the switch
    is read once)."""
    import os
    import subprocess
    import sys
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import emu_lib; from strumpack_amd import kernel as KM\n"
        "lib = KM.load(emu_lib.build()); r = np.random.default_rng(5)\n"
        "out = []\n"
        "for X in (r.random((20000, 6)), r.integers(0, 3, (9000, 4)).astype(float), np.repeat(r.random((700, 3)), 9, axis=0)):\n"
        "    Xp, perm, leaves = KM.clustering(lib, X, %r, 100)\n"
        "    out.append(perm.tolist()); out.append(leaves.tolist())\n"
        "import hashlib, json; print(hashlib.sha256(json.dumps(out).encode()).hexdigest())\n"
    ) % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))), algo)
    digests = []
    for mode in ("0", "1"):
        env = dict(os.environ, STRUMPACK_AMD_CLUSTER_EXACT_SELECT=mode)
        res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        digests.append(res.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1]


def test_pca_clustering_matches_reference_up_to_mirroring(lib):
    """The principal direction comes from LAPACK syevx in the reference: its sign is implementation-defined, so a split
    may come out mirrored; the two halves (as point sets) and the leaf sizes must agree."""
    J, Z = KG.golden()
    X = KG.susy()[0]
    for tag, pts in (("full", X), ("sub1000", X[:1000])):
        g = J["clustering_%s_pca" % tag]
        Xp, perm, leaves = KM.clustering(lib, pts, "pca", g["leaf"])
        ref = Z["perm_%s_pca" % tag]
        n = len(perm)
        assert sorted(leaves.tolist()) == sorted(g["leaves"])
        mine, theirs = set(perm[:n // 2].tolist()), set(ref[:n // 2].tolist())
        assert mine == theirs or mine == set(ref[n - n // 2:].tolist()) or len(mine ^ theirs) <= 2
        assert np.array_equal(Xp, pts[perm - 1])


@pytest.mark.parametrize("tag", ["gauss_1500", "gauss_10k"])
def test_approximate_neighbors_match_reference(lib, tag):
    """The host restatement of the reference's randomized neighbour search (NeighborSearch.hpp) returns the reference's
    lists (same mt19937 stream, same sort calls); ties in a projection may differ by the rounding of a BLAS dot."""
    J, Z = KG.golden()
    g = J["regression_" + tag]
    X = KG.susy()[0][:g["n"]][Z["perm_" + tag] - 1]
    ref = Z["ann_" + tag]
    got = KM.approximate_neighbors(lib, X, ref.shape[1])
    assert (got == ref).mean() > 0.999, (got == ref).mean()


@pytest.mark.parametrize("tag", ["gauss_400", "laplace_400", "anova_400"])
def test_oracle_kernel_compression_matches_reference(tag):
    """numpy restatement of compress_recursive_ann with the reference's neighbour lists == the reference's ranks."""
    J, Z = KG.golden()
    g = J["regression_" + tag]
    X = KG.susy()[0][:g["n"]][Z["perm_" + tag] - 1]
    nodes = np.array(g["nodes"])
    H = O.HSSMatrix.from_kernel(X, O.kernel_function(g["ktype"], g["h"], g["p"]), g["lam"], nodes[:, 1], nodes[:, 5],
                                Z["ann_" + tag].astype(np.int64), O.Options(rel_tol=g["rel_tol"], abs_tol=1e-8, leaf_size=g["leaf"]))
    assert H.is_compressed()
    ranks = np.array([nd.rU for nd in H.nodes])
    assert np.array_equal(ranks, nodes[:, 3]), (ranks, nodes[:, 3])
    # and it is a working solver: weights as the reference's
    H.factor()
    y = KG.susy()[1][:g["n"]][Z["perm_" + tag] - 1]
    w = H.solve(y.reshape(-1, 1)).ravel()
    wr = Z["weights_" + tag]
    assert np.linalg.norm(w - wr) <= 1e-8 * np.linalg.norm(wr)


@pytest.mark.parametrize("tag", ["gauss_400", "laplace_400", "anova_400"])
def test_regression_with_reference_neighbours(lib, tag):
    KG.check_regression(KM, lib, tag, inject=True, acc_tol=0.0, rank_tol=0.0, w_tol=1e-7 if tag == "gauss_400" else 1e-6)


def test_column_sets_on_device_equal_the_host_form():
    """compress_kernel builds the nodes' column sets on the device (hssk_colsets) unless STRUMPACK_AMD_KERNEL_HOST_SETS=1
    asks for the host threads: same sets, hence the same node table (ranks, sizes), permutation and regression weights --
    with the library's own exact neighbours and with injected lists (a subprocess per mode: the switch is read once)."""
    import hashlib  # noqa: F401
    import os
    import subprocess
    import sys
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import emu_lib; from strumpack_amd import kernel as KM\n"
        "lib = KM.load(emu_lib.build()); r = np.random.default_rng(9)\n"
        "X = r.random((900, 4)); y = np.sign(X[:, 0] - 0.5 + 0.1 * r.standard_normal(900))\n"
        "res = []\n"
        "for nb in (None, 'inject'):\n"
        "    m = KM.KernelRegression(lib, h=0.7, lam=2.0, kernel='rbf', argv=['--hss_leaf_size', '64', '--hss_rel_tol', '1e-3', '--hss_approximate_neighbors', '24'])\n"
        "    if nb is None:\n"
        "        m.fit(X, y)\n"
        "    else:\n"
        "        perm = res[1]\n"
        "        Xp = X[np.array(perm) - 1]\n"
        "        D = ((Xp[:, None, :] - Xp[None, :, :]) ** 2).sum(-1); np.fill_diagonal(D, np.inf)\n"
        "        ann = np.argsort(D, axis=1, kind='stable')[:, :24].astype(np.int32)\n"
        "        m.fit(X, y, neighbors=ann)\n"
        "    res += [m.node_info().tolist(), m.permutation().tolist(), np.round(m.weights(), 12).tolist()]\n"
        "    m.destroy()\n"
        "import hashlib, json; print(hashlib.sha256(json.dumps(res).encode()).hexdigest())\n"
    ) % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    digests = []
    for mode in ("0", "1"):
        env = dict(os.environ, STRUMPACK_AMD_KERNEL_HOST_SETS=mode)
        res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
        digests.append(res.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1]

