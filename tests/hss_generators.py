"""Reference for a compressed HSS matrix that does not depend on any kernel: the generators as HSSMatrix::write stores them
(csrc/host/hss_io.cpp: "HSSAMD01" | int n, nnodes | per node in pre-order 13 ints {lo, m, lvl, height, c0, c1, parent, Ustate,
Vstate, rU, rV, mU, mV}, then the blocks D, B01, B10, XU, permU, Ir, XV, permV, Ic, each as (int64 count, payload)), read with
plain numpy, and H, H^T applied by recursion over the tree with explicitly nested bases (the reference's HSSMatrix.apply.hpp):

    H(node) = [ H(c0)                      Ubig(c0) B01 Vbig(c1)^T ]      Ubig(leaf)  = U(leaf)
              [ Ubig(c1) B10 Vbig(c0)^T    H(c1)                   ]      Ubig(node)  = blockdiag(Ubig(c0), Ubig(c1)) U(node)

with the interpolative bases U (mU x rU) of HSSBasisID: U[permU[k], k] = 1 for k < rU, U[permU[rU + j], :] = XU[:, j]^T (V the same
from permV, XV).  A leaf's basis acts on its rows; an inner node's on the children's skeleton coordinates, c0's first.  B01 is
rU(c0) x rV(c1), B10 is rU(c1) x rV(c0).  Exact to float64 rounding whatever the compression tolerance."""
import numpy as np

MAGIC = b"HSSAMD01"
FIELDS = ("lo", "m", "lvl", "height", "c0", "c1", "parent", "Ustate", "Vstate", "rU", "rV", "mU", "mV")
BLOCKS = (("D", "<f8"), ("B01", "<f8"), ("B10", "<f8"), ("XU", "<f8"), ("permU", "<i4"), ("Ir", "<i4"), ("XV", "<f8"),
          ("permV", "<i4"), ("Ic", "<i4"))


class Node:
    def __init__(self, f):
        for k, v in zip(FIELDS, f):
            setattr(self, k, int(v))
        self.raw = {}

    @property
    def leaf(self):
        return self.c0 < 0


class HSS:
    """the generators of one compressed matrix (read() makes it)"""

    def __init__(self, n, nodes):
        self.n, self.nodes = n, nodes
        self._U, self._V = {}, {}

    # ---- bases ---------------------------------------------------------------------------------
    @staticmethod
    def _basis(perm, X, r, m):
        B = np.zeros((m, r))
        B[perm[:r], np.arange(r)] = 1.0
        B[perm[r:], :] = X.T
        return B

    def U(self, i):
        """U of node i (mU x rU), None at the root"""
        if i not in self._U:
            nd = self.nodes[i]
            self._U[i] = self._basis(nd.permU, nd.XU, nd.rU, nd.mU)
        return self._U[i]

    def V(self, i):
        if i not in self._V:
            nd = self.nodes[i]
            self._V[i] = self._basis(nd.permV, nd.XV, nd.rV, nd.mV)
        return self._V[i]

    def big_mul(self, i, Z, which):
        """Ubig(i) @ Z (which 'U') or Vbig(i) @ Z ('V'): blockdiag(big(c0), big(c1)) (basis(i) Z)"""
        nd = self.nodes[i]
        T = (self.U(i) if which == "U" else self.V(i)) @ Z
        if nd.leaf:
            return T
        r0 = self.nodes[nd.c0].rU if which == "U" else self.nodes[nd.c0].rV
        return np.vstack([self.big_mul(nd.c0, T[:r0], which), self.big_mul(nd.c1, T[r0:], which)])

    def big(self, i, which):
        """Ubig(i) / Vbig(i) as an explicit m x r matrix"""
        nd = self.nodes[i]
        Bs = self.U(i) if which == "U" else self.V(i)
        if nd.leaf:
            return Bs
        a, b = self.big(nd.c0, which), self.big(nd.c1, which)
        blk = np.zeros((a.shape[0] + b.shape[0], a.shape[1] + b.shape[1]))
        blk[:a.shape[0], :a.shape[1]] = a
        blk[a.shape[0]:, a.shape[1]:] = b
        return blk @ Bs

    # ---- products ------------------------------------------------------------------------------
    def _apply(self, i, X, T):
        """(op(H(i)) X, Vbig(i)^T X [Ubig(i)^T X for op = transpose]) for the rows X of node i"""
        nd = self.nodes[i]
        inb, outb = ("U", "V") if T else ("V", "U")
        if nd.leaf:
            Y = (nd.D.T if T else nd.D) @ X
            W = None if i == 0 else (self.U(i) if T else self.V(i)).T @ X
            return Y, W
        a = self.nodes[nd.c0]
        Y0, W0 = self._apply(nd.c0, X[:a.m], T)
        Y1, W1 = self._apply(nd.c1, X[a.m:], T)
        # N: H01 = Ubig0 B01 Vbig1^T, H10 = Ubig1 B10 Vbig0^T;  T: (H^T)01 = Vbig0 B10^T Ubig1^T, (H^T)10 = Vbig1 B01^T Ubig0^T
        C01, C10 = (nd.B10.T, nd.B01.T) if T else (nd.B01, nd.B10)
        Y0 = Y0 + self.big_mul(nd.c0, C01 @ W1, outb)
        Y1 = Y1 + self.big_mul(nd.c1, C10 @ W0, outb)
        W = None if i == 0 else (self.U(i) if T else self.V(i)).T @ np.vstack([W0, W1])
        return np.vstack([Y0, Y1]), W

    def apply(self, X, trans="N"):
        X = np.asarray(X, dtype=np.float64).reshape(self.n, -1)
        return self._apply(0, X, trans != "N")[0]

    def _dense(self, i):
        nd = self.nodes[i]
        if nd.leaf:
            return nd.D.copy()
        a, b = nd.c0, nd.c1
        top = np.hstack([self._dense(a), self.big(a, "U") @ nd.B01 @ self.big(b, "V").T])
        bot = np.hstack([self.big(b, "U") @ nd.B10 @ self.big(a, "V").T, self._dense(b)])
        return np.vstack([top, bot])

    def dense(self):
        if self.n > 4096:
            raise ValueError("dense(H): n = %d > 4096" % self.n)
        return self._dense(0)

    def norm2(self, iters=30, seed=0):
        """||H||_2 (n <= 4096: exact; else power iteration on H^T H with the reference apply, from below)"""
        if self.n <= 4096:
            return float(np.linalg.norm(self.dense(), 2))
        x = np.random.default_rng(seed).standard_normal((self.n, 1))
        s = 0.0
        for _ in range(iters):
            x /= np.linalg.norm(x)
            y = self.apply(x)
            s = np.linalg.norm(y)
            x = self.apply(y, "T")
        return float(s)


def _check(ok, what):
    if not ok:
        raise ValueError("HSS file: " + what)


def read(path):
    """the generators of the HSS matrix in the file `path` (written by HSSMatrix::write); every block is checked against the node
    table, and only a fully compressed matrix is accepted"""
    with open(path, "rb") as f:
        buf = f.read()
    _check(buf[:8] == MAGIC, "bad magic")
    n, nn = (int(v) for v in np.frombuffer(buf, "<i4", 2, 8))
    _check(n >= 0 and nn >= 1, "bad header")
    off = 16
    nodes = []
    for _ in range(nn):
        _check(off + 52 <= len(buf), "truncated node table")
        nd = Node(np.frombuffer(buf, "<i4", 13, off))
        off += 52
        for name, dt in BLOCKS:
            _check(off + 8 <= len(buf), "truncated block count")
            cnt = int(np.frombuffer(buf, "<i8", 1, off)[0])
            off += 8
            size = np.dtype(dt).itemsize
            _check(0 <= cnt and off + cnt * size <= len(buf), "block %s: bad count %d" % (name, cnt))
            nd.raw[name] = np.frombuffer(buf, dt, cnt, off).copy()
            off += cnt * size
        nodes.append(nd)
    _check(off == len(buf), "%d bytes behind the last node" % (len(buf) - off))
    # tree: pre-order, children follow their parent, rows tile the parent's
    def walk(i, lo, par):
        _check(i < nn, "node index")
        nd = nodes[i]
        _check(nd.lo == lo and nd.parent == par and nd.m >= 0, "node %d: position in the tree" % i)
        if nd.leaf:
            _check(nd.c1 < 0, "node %d: one child" % i)
            return i + 1
        _check(nd.c0 == i + 1, "node %d: c0 is not the next node" % i)
        nxt = walk(nd.c0, lo, i)
        _check(nd.c1 == nxt, "node %d: c1 is not behind c0's subtree" % i)
        _check(nodes[nd.c0].m + nodes[nd.c1].m == nd.m, "node %d: children's rows" % i)
        return walk(nd.c1, lo + nodes[nd.c0].m, i)
    _check(walk(0, 0, -1) == nn and nodes[0].m == n, "tree does not cover the matrix")
    for i, nd in enumerate(nodes):
        R = nd.raw
        cnt = {k: len(v) for k, v in R.items()}
        if i > 0:
            _check(nd.Ustate == 2 and nd.Vstate == 2, "node %d is not compressed (Ustate %d, Vstate %d)" % (i, nd.Ustate, nd.Vstate))
        if nd.leaf:
            _check(cnt["D"] == nd.m * nd.m and cnt["B01"] == 0 and cnt["B10"] == 0, "leaf %d: block sizes" % i)
            nd.D = R["D"].reshape(nd.m, nd.m, order="F")
            if i > 0:
                _check(nd.mU == nd.m and nd.mV == nd.m, "leaf %d: basis rows" % i)
        else:
            a, b = nodes[nd.c0], nodes[nd.c1]
            _check(cnt["D"] == 0, "inner node %d has a D" % i)
            _check(cnt["B01"] == a.rU * b.rV and cnt["B10"] == b.rU * a.rV, "node %d: coupling block sizes" % i)
            nd.B01 = R["B01"].reshape(a.rU, b.rV, order="F")
            nd.B10 = R["B10"].reshape(b.rU, a.rV, order="F")
            if i > 0:
                _check(nd.mU == a.rU + b.rU and nd.mV == a.rV + b.rV, "node %d: basis rows" % i)
        if i == 0:
            _check(all(cnt[k] == 0 for k in ("XU", "permU", "Ir", "XV", "permV", "Ic")), "the root has a basis")
            continue
        _check(0 <= nd.rU <= nd.mU and 0 <= nd.rV <= nd.mV, "node %d: ranks" % i)
        _check(cnt["XU"] == nd.rU * (nd.mU - nd.rU) and cnt["permU"] == nd.mU and cnt["Ir"] == nd.rU, "node %d: U sizes" % i)
        _check(cnt["XV"] == nd.rV * (nd.mV - nd.rV) and cnt["permV"] == nd.mV and cnt["Ic"] == nd.rV, "node %d: V sizes" % i)
        for p in ("permU", "permV"):
            _check(np.array_equal(np.sort(R[p]), np.arange(len(R[p]))), "node %d: %s is not a permutation" % (i, p))
        for s in ("Ir", "Ic"):
            _check(np.all((R[s] >= 0) & (R[s] < n)), "node %d: %s out of range" % (i, s))
        nd.permU, nd.permV = R["permU"], R["permV"]
        nd.XU = R["XU"].reshape(nd.rU, nd.mU - nd.rU, order="F")
        nd.XV = R["XV"].reshape(nd.rV, nd.mV - nd.rV, order="F")
    return HSS(n, nodes)


def write(H, path):
    """the same file back (every field as read): read -> write -> read must be lossless, byte for byte"""
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(np.array([H.n, len(H.nodes)], "<i4").tobytes())
        for nd in H.nodes:
            f.write(np.array([getattr(nd, k) for k in FIELDS], "<i4").tobytes())
            for name, dt in BLOCKS:
                v = np.ascontiguousarray(nd.raw[name], dtype=dt)
                f.write(np.array([len(v)], "<i8").tobytes())
                f.write(v.tobytes())
