"""What the per-coordinate length-scale gradient (ARD) costs, and which group size hssk_kernel_matmul_coord should default to
(profiles/gp_ard.md).

One process, the workload of tools/gp_bench.py: N points uniform in [0, 1)^8, Gauss kernel h = 1.3, lambda = 3.11, cobble
clustering, leaf 128, rel_tol 1e-2, 64 neighbours.  Needs the GPU (the product library; no fallback).

  launches     one hssk_kernel_matmul_coord launch with 64 columns for every built nj, beside hssk_kernel_matmul(deriv = 1) with the
               same columns: device events, the variants alternating inside every repetition, one untimed round first.  The
               deriv = 1 product is what one coordinate per launch would cost; the criterion for the shipped default group is
               time(nj) / nj < time(deriv = 1) in this run.
  resources    registers and scratch per variant from the compiler's report (--resources: a JSON written by --resources-only,
               which compiles the two kernel files with -Rpass-analysis=kernel-resource-usage and needs no GPU), the dynamic LDS
               from the kernels' own layout, and the workgroups per compute unit both allow (the compiler's waves per SIMD, 160 KB)
  gradient     SPX_kernel_lml_gradient_coords with 63 probes on the bench fit: host clock, and the device-event split
               (SPX_kernel_gradient_ms); beside SPX_kernel_lml_gradient with the same probes

    python tools/gp_ard_bench.py --resources-only res.json
    python tools/gp_ard_bench.py --n 100000 --resources res.json --out gp_ard_bench.json --md profiles/gp_ard.md
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MFMA_TFLOPS = 78.6          # gfx950 FP64 matrix peak (strumpack_amd/csrc/kernels/hssk_dgemm.hip)
LDS_PER_CU = 160 * 1024
D = 8


def lds_bytes(nj, d):
    """dynamic LDS of kmatmul_coord_kernel<., nj> (nj = 0: kmatmul_kernel, whole points): stage buffers of g and B, the row points and
    two stages of training points (hssk_kmatmul_coord.hip: kmc_lds_doubles)"""
    return 8 * ((2 * max(nj, 1) + 2) * 64 * 17 + 64 * (d | 1) + 2 * 16 * (d | 1))


def compile_resources():
    """{variant: {vgpr, agpr, scratch, spill, waves}} for Gauss: "deriv1" and "nj<k>", from the compiler's remarks"""
    src = os.path.join(ROOT, "strumpack_amd", "csrc")
    out = {}
    for fname in ("hssk_kmatmul.hip", "hssk_kmatmul_coord.hip"):
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
               "-I" + os.path.join(src, "hip"), "-I" + os.path.join(src, "kernels"), "-I" + os.path.join(src, "host"),
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(src, "kernels", fname), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        name = None
        for line in text.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                f = m.group(1)
                name = None
                if "kmatmul_kernelILi0ELi1ELb0E" in f:
                    name = "deriv1"
                k = re.search(r"kmatmul_coord_kernelILi0ELi(\d+)E", f)
                if k:
                    name = "nj" + k.group(1)
                if name:
                    out[name] = {}
                continue
            if name is None:
                continue
            for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("spill", r"VGPRs Spill: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m:
                    out[name][key] = int(m.group(1))
    return out


def launches(path, n, reps):
    from strumpack_amd import hssk as K
    hk = K.Hssk(path)
    L = hk.lib
    L.hssk_watch_start.argtypes = L.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    L.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.hssk_watch_read_ms.restype = C.c_double
    top, nc = L.hssk_kernel_matmul_coord_max(), 64
    assert top <= 6, "one stopwatch per variant"
    dX = hk.array(np.random.default_rng(1).random((D, n)))
    spec = K.KernelSpec(dX.ptr, n, D, 0, 1, 1.3, 0.0)
    dW, dO = hk.empty((n, nc)), hk.empty((n * nc * top,))
    hk.check(L.hssk_randn(hk.ctx, dW.ptr, n, nc, n, 0, nc, 9))
    per_rep = {v: [] for v in range(top + 1)}
    for rep in range(reps + 1):                     # (round 0 untimed: code objects, the LDS attribute)
        for v in range(top + 1):                    # v = 0: the deriv = 1 product; v >= 1: nj = v
            L.hssk_watch_start(hk.ctx, v)
            if v == 0:
                hk.check(L.hssk_kernel_matmul(hk.ctx, C.byref(spec), 1, dW.ptr, n, nc, dO.ptr, n, 0))
            else:
                hk.check(L.hssk_kernel_matmul_coord(hk.ctx, C.byref(spec), 0, v, dW.ptr, n, nc, dO.ptr, n, n * nc, 0))
            L.hssk_watch_stop(hk.ctx, v)
        for v in range(top + 1):
            ms = L.hssk_watch_read_ms(hk.ctx, v, None)
            if rep:
                per_rep[v].append(ms)
    # the values: the coordinates of one launch of nj = top add up to h times the deriv = 1 product only over all eight, so
    # compare coordinate 0 of every nj bit for bit instead
    ref = None
    same = True
    for v in range(1, top + 1):
        hk.check(L.hssk_kernel_matmul_coord(hk.ctx, C.byref(spec), 0, v, dW.ptr, n, nc, dO.ptr, n, n * nc, 0))
        hk.sync()
        first = dO.get()[:n * nc].copy()
        same = same and (ref is None or np.array_equal(ref, first))
        ref = first if ref is None else ref
    for a in (dX, dW, dO):
        a.free()
    default = L.hssk_kernel_matmul_coord_group()
    splits = L.hssk_kernel_matmul_splits(n)
    hk.close()
    rows = [dict(variant="deriv1" if v == 0 else "nj%d" % v, nj=max(v, 1), ms=per_rep[v], min_ms=min(per_rep[v]), median_ms=float(np.median(per_rep[v])))
            for v in range(top + 1)]
    return dict(rows=rows, default_group=default, splits=splits, coordinate0_bitwise_equal=bool(same), nc=nc)


def gradients(lib_path, n, leaf, reps):
    from strumpack_amd import kernel as KM
    lib = KM.load(lib_path)
    rng = np.random.default_rng(2025)
    X = rng.random((n, D))
    y = np.sign((X - 0.5) @ rng.standard_normal(D))
    argv = ["--hss_leaf_size", str(leaf), "--hss_rel_tol", "1e-2", "--hss_abs_tol", "1e-8", "--hss_approximate_neighbors", "64"]
    kr = KM.KernelRegression(lib, h=1.3, lam=3.11, kernel="rbf", argv=argv, keep_model=True)
    fits = []
    for _ in range(3):                              # (the first fit of a process loads code objects and fills the device pool)
        t0 = time.perf_counter()
        kr.fit(X, y)
        fits.append((time.perf_counter() - t0) * 1e3)
    out = {"fit_ms": fits}
    for name, call in (("coords", lambda: kr.log_marginal_likelihood_gradient_coords(probes=63, seed=1, terms=True)),
                       ("h", lambda: kr.log_marginal_likelihood_gradient(probes=63, seed=1, terms=True))):
        walls, splits, val = [], [], None
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            val = call()
            walls.append((time.perf_counter() - t0) * 1e3)
            splits.append(kr.gradient_ms())
        out[name] = {"host_ms": walls[1:], "device_ms": splits[1 + int(np.argmin(walls[1:]))]}
        if name == "coords":
            t = val[1]
            out[name].update(dtheta=val[0].tolist(), quad=t["quad"].tolist(), trace=t["trace"].tolist(),
                             trace_se=(t["tc"].std(axis=1, ddof=1) / np.sqrt(t["tc"].shape[1])).tolist())
        else:
            out[name].update(dh=val[0], h_dh=1.3 * val[0])
    kr.destroy()
    return out


def markdown(r):
    n, rows, res = r["n"], r["launches"]["rows"], r.get("resources") or {}
    base = rows[0]["min_ms"]
    L = ["# Per-coordinate length-scale gradients (ARD) from the kept fit", "",
         "Tool: `tools/gp_ard_bench.py` (one process; the workload of `tools/gp_bench.py`: N = %d points uniform in [0, 1)^8, Gauss, h = 1.3," % n,
         "lambda = 3.11, cobble, leaf %d, rel_tol 1e-2, 64 neighbours).  Kernel times are device events around single launches with 64" % r["leaf"],
         "columns, the variants alternating inside each of %d repetitions after one untimed round (grid: %d row tiles x %d split);"
         % (len(rows[0]["ms"]), (n + 63) // 64, r["launches"]["splits"]),
         "the gradient times are host clocks around calls that end in a device synchronise.", "",
         "## One launch: `hssk_kernel_matmul_coord` for every built nj beside `hssk_kernel_matmul(deriv = 1)`", "",
         "| variant | min ms | median ms | per coordinate (min) | against deriv = 1 | TFLOP/s on the matrix cores | VGPR + AGPR | scratch | dynamic LDS | workgroups / CU (registers, LDS) |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        v = res.get(row["variant"])
        lds = lds_bytes(0 if row["variant"] == "deriv1" else row["nj"], D)
        if v:
            regs = "%d + %d" % (v["vgpr"], v["agpr"])
            occ = "%d (%d, %d)" % (min(v["waves"], LDS_PER_CU // lds), v["waves"], LDS_PER_CU // lds)
            scr = "%d B, %d spilled" % (v["scratch"], v["spill"])
        else:
            regs = occ = scr = "not recorded"
        per = row["min_ms"] / row["nj"]
        L.append("| %s | %.2f | %.2f | %.2f ms | %.2f x | %.1f | %s | %s | %.1f KB | %s |"
                 % (row["variant"], row["min_ms"], row["median_ms"], per, per / base, 2.0 * n * n * 64 * row["nj"] / (row["min_ms"] * 1e-3) / 1e12,
                    regs, scr, lds / 1024.0, occ))
    dflt = r["launches"]["default_group"]
    drow = rows[dflt]
    best = min(rows[1:], key=lambda q: q["min_ms"] / q["nj"])
    ok = drow["min_ms"] / drow["nj"] < base
    L += ["",
          "The deriv = 1 product is what one coordinate per launch would cost (the same pass over the pairs, one matrix).  Criterion",
          "for the shipped default group: its time per coordinate below the deriv = 1 product of this run.", "",
          "- Shipped default `hssk_kernel_matmul_coord_group()` = %d: %.2f ms per coordinate against %.2f ms: criterion %s."
          % (dflt, drow["min_ms"] / drow["nj"], base, "MET" if ok else "NOT MET"),
          "- Cheapest per coordinate in this run: nj = %d at %.2f ms." % (best["nj"], best["min_ms"] / best["nj"]),
          "- Coordinate 0 bit for bit the same from every nj: %s." % ("yes" if r["launches"]["coordinate0_bitwise_equal"] else "NO"),
          "- FP64 matrix roof %.1f TFLOP/s: the flops counted are the 2 n^2 64 nj of the products alone, not the n^2 exponentials and" % FP64_MFMA_TFLOPS,
          "  8 n^2 coordinate differences that every variant evaluates once per launch on the vector units.", ""]
    g = r.get("gradient")
    if g:
        c, h = g["coords"], g["h"]
        cd, hd = c["device_ms"], h["device_ms"]
        launches_per_block = (D + dflt - 1) // dflt
        L += ["## The whole gradient, 63 probes (one block of 64 columns with alpha)", "",
              "| call | host ms (min of %d) | products | solves | column dots |" % len(c["host_ms"]), "|---|---|---|---|---|",
              "| `SPX_kernel_lml_gradient_coords` (8 coordinates in %d launches of at most %d) | %.1f | %.2f ms | %.3f ms | %.3f ms |"
              % (launches_per_block, dflt, min(c["host_ms"]), cd["product_ms"], cd["solve_ms"], cd["dots_ms"]),
              "| `SPX_kernel_lml_gradient` (dL/dh, dL/dlambda) | %.1f | %.2f ms | %.3f ms | %.3f ms |"
              % (min(h["host_ms"]), hd["product_ms"], hd["solve_ms"], hd["dots_ms"]),
              "",
              "Fit with `keep_model` (host clock, third fit): %.1f ms.  Eight coordinates cost %.2f x the gradient in h; eight deriv = 1"
              % (g["fit_ms"][-1], min(c["host_ms"]) / min(h["host_ms"])),
              "launches would cost %.1f ms of products alone." % (8 * base), "",
              "dL/dtheta_j = " + ", ".join("%.5g" % v for v in c["dtheta"]) + ";",
              "standard errors of the trace means: " + ", ".join("%.2g" % v for v in c["trace_se"]) + ".",
              "sum_j dL/dtheta_j = %.6g, h dL/dh of the existing gradient with the same probes = %.6g." % (sum(c["dtheta"]), h["h_dh"]),
              "These are gradients of the exact-kernel likelihood evaluated with the inverse of the matrix compressed at rel_tol 1e-2",
              "(DESIGN 8d, 8i).", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--leaf", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None, help="JSON of --resources-only; without it the kernel files are compiled here")
    ap.add_argument("--resources-only", default=None, metavar="JSON", help="write the compiler's resource report and stop (no GPU needed)")
    ap.add_argument("--no-gradient", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if a.resources_only:
        with open(a.resources_only, "w") as f:
            json.dump(compile_resources(), f)
        return
    import torch
    assert torch.cuda.is_available(), "gp_ard_bench.py measures on the GPU"
    from strumpack_amd import _loader
    path = _loader.lib_path()
    if a.resources:
        with open(a.resources) as f:
            resources = json.load(f)
    else:
        resources = compile_resources()
    res = {"n": a.n, "leaf": a.leaf, "resources": resources}
    res["launches"] = launches(path, a.n, a.reps)
    if not a.no_gradient:
        res["gradient"] = gradients(path, a.n, a.leaf, max(2, a.reps // 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
