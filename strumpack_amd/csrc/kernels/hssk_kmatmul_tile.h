// The tile of the exact kernel-matrix products: shared by hssk_kmatmul.hip (the kernel and its derivative in h) and
// hssk_kmatmul_coord.hip (the per-coordinate derivatives), so that both split the training points into the same stages.
#pragma once

namespace {

constexpr int KM_T = 256;      // threads: four waves
constexpr int KM_R = 64;       // output rows per workgroup
constexpr int KM_K = 16;       // training points per stage
constexpr int KM_KP = KM_K + 1;
constexpr int KM_DMAX = 64;    // most coordinates a whole point keeps in the LDS
constexpr long long KM_GRID = 512;   // workgroups hssk_kernel_matmul_splits aims at (two per compute unit of an MI355X)

}  // namespace
