"""What the kept model of kernel ridge regression costs next to the fit it comes from (profiles/gp_variance.md).

One process, the bench's kernel workload: N points uniform in [0, 1)^8, Gauss kernel h = 1.3, lambda = 3.11, cobble clustering,
leaf 128, rel_tol 1e-2, 64 neighbours.  Needs the GPU (the product library; no fallback).

  fit            STRUMPACK_kernel_fit_HSS_double with keep_model: host clock around the call, and its own stage split
                 (compress / factor / solve, SPX_kernel_fit_info)
  logabsdet      SPX_kernel_logabsdet: host clock around the call (it ends in a device synchronise: one launch pair and an
                 8-byte copy), minimum and median of --reps calls, next to the factorization of the same run
  set_lambda     SPX_kernel_model_set_lambda (shift + factor + solve), alternating between two values, next to the fit
  variance       SPX_kernel_predict_variance_double of --m test points: host clock, and the device-clock split into cross-kernel
                 blocks, solves and column sums (events around the launches of each chunk of 64), per chunk
  solve64        the 64-right-hand-side solve the engine reaches on its own: SPX_d_struct_solve_device on a device buffer of
                 random right-hand sides, the same matrix built through SPX_d_struct_from_kernel, host clock around calls that
                 end in a synchronise (first call, then the minimum of the replayed ones)

    python tools/gp_bench.py --n 100000 --m 4096 --out gp_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(ts), "median_ms": float(np.median(ts)), "first_ms": ts[0], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--leaf", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "gp_bench.py measures on the GPU"
    from strumpack_amd import _loader, capi, dist as sdist
    from strumpack_amd import hssk as K
    from strumpack_amd import kernel as KM
    lib = KM.load(_loader.lib_path())
    L = capi.load(_loader.lib_path())
    rng = np.random.default_rng(2025)
    X = rng.random((a.n, 8))
    y = np.sign((X - 0.5) @ rng.standard_normal(8))
    T = rng.random((a.m, 8))
    h, lam, lam2 = 1.3, 3.11, 1.0
    argv = ["--hss_leaf_size", str(a.leaf), "--hss_rel_tol", "1e-2", "--hss_abs_tol", "1e-8", "--hss_approximate_neighbors", "64"]
    res = {"n": a.n, "m": a.m, "leaf": a.leaf, "h": h, "lambda": lam}
    kr = KM.KernelRegression(lib, h=h, lam=lam, kernel="rbf", argv=argv, keep_model=True)
    fits = []
    for _ in range(3):                              # (the first fit of a process loads code objects and fills the device pool)
        t0 = time.perf_counter()
        kr.fit(X, y)
        fits.append((time.perf_counter() - t0) * 1e3)
    info = kr.info()
    res["fit"] = {"host_ms": fits, "compress_ms": info["compress_us"] / 1e3, "factor_ms": info["factor_us"] / 1e3,
                  "solve_ms": info["solve_us"] / 1e3, "rank": info["rank"], "levels": info["levels"]}
    res["logabsdet"] = dict(clock(kr.logabsdet, 2 * a.reps), value=kr.logabsdet())
    res["log_marginal_likelihood"] = kr.log_marginal_likelihood()
    flip = [lam2, lam]
    res["set_lambda"] = clock(lambda: kr.set_lambda(flip[0]) and flip.reverse(), a.reps)
    if kr.lam != lam:
        kr.set_lambda(lam)
    var = None
    walls, splits = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        var = kr.predict_variance(T)
        walls.append((time.perf_counter() - t0) * 1e3)
        splits.append(kr.variance_ms())
    chunks = (a.m + 63) // 64
    best = splits[int(np.argmin(walls))]
    res["variance"] = {"host_ms": walls, "chunks": chunks, "device_ms": splits,
                       "per_chunk_ms": {k: v / chunks for k, v in best.items()},
                       "min": float(var.min()), "max": float(var.max()), "negative": int((var < 0).sum())}
    kr.destroy()
    # the engine's own 64-right-hand-side solve on the same matrix
    opts = capi.StructuredMatrix.options(L, rel_tol=1e-2, abs_tol=1e-8, leaf_size=a.leaf, max_rank=50000)
    H, Xp, perm = sdist.from_kernel(L, X, opts, kernel="Gauss", h=h, lam=lam, clustering="cobble", neighbors=64)
    H.factor()
    hk = K.Hssk(_loader.lib_path())
    dB = hk.array(rng.standard_normal((a.n, 64)))
    res["solve64"] = clock(lambda: H.solve_device(dB.ptr, 64), a.reps)
    res["factor_ms_struct"] = H.stats()["t_factor"] * 1e3
    dB.free()
    H.destroy()
    hk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
