// The FP64 pair arithmetic of kernel ridge regression, shared by the prediction sum (hssk_kernel_predict, hssk_kernelmat.hip) and
// by the cross-kernel block and the column-weighted sum of the predictive variance (hssk_kernel_cross,
// hssk_kernel_predict_cols, hssk_gp.hip).  A workgroup is one wave: lane = test point c, the training points pass through the LDS
// 64 (beyond 64 coordinates: RT) at a time and every lane meets them in training order.  What a lane does with the value
// k(x_r, t_c) of a pair is the kernel's MODE:
//   PR_SUM    sum += w[r] k             (one weight vector, staged with the training tile)          -> pred[c]
//   PR_COLS   sum += W(r, c) k          (a weight column per test point, read from global memory)   -> pred[c]
//   PR_CROSS  out(r, c) = k             (no sum)
// The value itself -- the order of the coordinates, the exponentials, Newton's identities of the ANOVA kernel -- is one piece of
// code for the three, and the sums of PR_SUM and PR_COLS take the pairs of a test point in the same order.
// SPLIT (PR_CROSS only, hssk_kernel_cross_split): the grid has a second dimension over ranges of whole 64-point tiles of the
// training points (pr_split_per); an entry depends on its pair alone, so the block is bit for bit that of the one-dimensional grid.
#pragma once
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_matern.h"

namespace {

constexpr int PR_T = 64;
constexpr int PR_DMAX = 64;   // most coordinates a whole point keeps in the LDS (kernel_predict_kernel)
constexpr int PR_DC = 32;     // coordinates per pass beyond that (kernel_predict_wide_kernel)
constexpr int PR_SUM = 0, PR_COLS = 1, PR_CROSS = 2;
// static LDS of the two kernels (checked against the device's limit by the entry points that launch them)
constexpr size_t PR_LDS_POINT = sizeof(double) * (2 * PR_T * (PR_DMAX + 1) + PR_T);
constexpr size_t PR_LDS_WIDE = sizeof(double) * (PR_T * (PR_DC + 1) + 32 * PR_DC + 32);

// training points per split of a SPLIT grid of s ranges: whole tiles of PR_T (a multiple of every RT of the wide kernel)
__host__ __device__ inline long long pr_split_per(long long n, long long s) {
  const long long tiles = (n + PR_T - 1) / PR_T;
  return ((tiles + s - 1) / s) * PR_T;
}

// prediction[c] = sum_r w[r] k(x_r, t_c)   (no lambda: train and test points are different sets)
// MAT: the Matern kernels (types 3 and 4) -- the Gauss distance loop with the finish of hssk_matern.h; an instantiation of its
// own, so that the code of the other three kernels is what it was
template <int MODE, bool MAT = false, bool SPLIT = false>
__global__ __launch_bounds__(PR_T) void kernel_predict_kernel(hssk_kernel_spec ks, const double* __restrict__ w, size_t ldw,
                                                              const double* __restrict__ T, int m,
                                                              double* __restrict__ pred, size_t ldo) {
  HSSK_SHARED double xt[PR_T * (PR_DMAX + 1)];
  HSSK_SHARED double xr[PR_T * (PR_DMAX + 1)];
  HSSK_SHARED double wr[PR_T];
  const int tid = threadIdx.x, c = blockIdx.x * PR_T + tid, d = ks.d;
  const bool live = c < m;
  for (int j = 0; j < d; j++) xt[tid * (PR_DMAX + 1) + j] = live ? T[(size_t)c * d + j] : 0.;
  double sum = 0.;
  const long long rb = SPLIT ? (long long)blockIdx.y * pr_split_per(ks.n, gridDim.y) : 0;
  const long long re = SPLIT ? min(ks.n, rb + pr_split_per(ks.n, gridDim.y)) : ks.n;
  for (long long r0 = rb; r0 < re; r0 += PR_T) {
    __syncthreads();
    for (int e = tid; e < PR_T * d; e += PR_T) {
      const int pt = e / d, j = e % d;
      xr[pt * (PR_DMAX + 1) + j] = r0 + pt < ks.n ? ks.X[(size_t)(r0 + pt) * d + j] : 0.;
    }
    if (MODE == PR_SUM) wr[tid] = r0 + tid < ks.n ? w[r0 + tid] : 0.;
    __syncthreads();
    const int rend = (int)min((long long)PR_T, re - r0);
    for (int r = 0; r < rend; r++) {
      double v;
      if (MAT) {
        double acc = 0.;
        for (int i = 0; i < d; i++) {
          const double df = xr[r * (PR_DMAX + 1) + i] - xt[tid * (PR_DMAX + 1) + i];
          acc += df * df;
        }
        v = hssk_matern_rt(ks.type, acc, hssk_matern_c(ks.type, ks.h), ks.h);
      } else if (ks.type == 2) {
        double Kss[8], Kpp[9];
        for (int j = 0; j < ks.p; j++) Kss[j] = 0.;
        for (int i = 0; i < d; i++) {
          const double df = xr[r * (PR_DMAX + 1) + i] - xt[tid * (PR_DMAX + 1) + i];
          const double tmp = exp(-(df * df) / (2. * ks.h * ks.h));
          double pw = tmp;
          for (int j = 0; j < ks.p; j++) { Kss[j] += pw; pw *= tmp; }
        }
        Kpp[0] = 1.;
        for (int i = 1; i <= ks.p; i++) {
          double s = 0.;
          for (int q = 1; q <= i; q++) s += ((q & 1) ? 1. : -1.) * Kpp[i - q] * Kss[q - 1];
          Kpp[i] = s / i;
        }
        v = Kpp[ks.p];
      } else {
        double acc = 0.;
        for (int i = 0; i < d; i++) {
          const double df = xr[r * (PR_DMAX + 1) + i] - xt[tid * (PR_DMAX + 1) + i];
          acc += ks.type == 0 ? df * df : fabs(df);
        }
        v = exp(acc * (ks.type == 0 ? -1. / (2. * ks.h * ks.h) : -1. / ks.h));
      }
      if (MODE == PR_SUM) sum += wr[r] * v;
      else if (MODE == PR_COLS) sum += (live ? w[(size_t)c * ldw + r0 + r] : 0.) * v;
      else if (live) pred[(size_t)c * ldo + r0 + r] = v;
    }
  }
  if (MODE != PR_CROSS && live) pred[c] = sum;
}

// e_E = (1 / E) sum_q (-1)^(q + 1) e_(E - q) s_q for E = 1 .. p, the sums in kernel_predict_kernel's order (every index a
// constant: the arrays stay in registers)
template <int E>
__device__ inline void anova_newton(const double (&S)[8], double (&K)[9], int p, double& v) {
  anova_newton<E - 1>(S, K, p, v);
  if (E <= p) {
    double s = 0.;
#pragma unroll
    for (int q = 1; q <= E; q++) s += ((q & 1) ? 1. : -1.) * K[E - q] * S[q - 1];
    K[E] = s / E;
    v = K[E];
  }
}
template <>
__device__ inline void anova_newton<0>(const double (&)[8], double (&K)[9], int, double&) { K[0] = 1.; }

// The same sum beyond PR_DMAX coordinates: whole points no longer fit the LDS, so a tile of RT training points meets the
// workgroup's 64 test points in passes of PR_DC coordinates.  What a pair has accumulated -- the distance (Gauss, Laplace) or the
// p power sums of its per-coordinate exponentials (ANOVA) -- carries across the passes in registers; RT is what the registers
// hold (32 distances, 8 x 8 power sums; the Matern kernels, TYPE 3 and 4, carry the Gauss distance).  Per pair the coordinates are met in order and the pairs of a test point in training
// order, as in kernel_predict_kernel: the same arithmetic, the same error bound.  The test points' pass is staged again for
// every training tile (one staged value per RT differences).
template <int TYPE, int RT, int MODE, bool SPLIT = false>
__global__ __launch_bounds__(PR_T) void kernel_predict_wide_kernel(hssk_kernel_spec ks, const double* __restrict__ w, size_t ldw,
                                                                   const double* __restrict__ T, int m, double* __restrict__ pred,
                                                                   size_t ldo) {
  constexpr int NS = TYPE == 2 ? 8 : 1;   // sums a pair carries
  HSSK_SHARED double xt[PR_T * (PR_DC + 1)];   // [test point][coordinate of the pass]
  HSSK_SHARED double xr[RT * PR_DC];           // [training point][coordinate of the pass]: read as broadcasts
  HSSK_SHARED double wr[RT];
  const int tid = threadIdx.x, cb = blockIdx.x * PR_T, c = cb + tid, d = ks.d, P = ks.p;
  const double h2 = 2. * ks.h * ks.h;
  double sum = 0.;
  const long long rb = SPLIT ? (long long)blockIdx.y * pr_split_per(ks.n, gridDim.y) : 0;
  const long long re = SPLIT ? min(ks.n, rb + pr_split_per(ks.n, gridDim.y)) : ks.n;
  for (long long r0 = rb; r0 < re; r0 += RT) {
    double acc[RT][NS];
#pragma unroll
    for (int r = 0; r < RT; r++)
#pragma unroll
      for (int q = 0; q < NS; q++) acc[r][q] = 0.;
    for (int d0 = 0; d0 < d; d0 += PR_DC) {
      const int dc = min(PR_DC, d - d0);
      __syncthreads();
      // (test points past m and training points past n read the last one; their results are dropped)
      for (int e = tid; e < PR_T * dc; e += PR_T) {
        const int pt = e / dc, j = e % dc;
        xt[pt * (PR_DC + 1) + j] = hssk_gload(T, (size_t)min(cb + pt, m - 1) * d + d0 + j);
      }
      for (int e = tid; e < RT * dc; e += PR_T) {
        const int pt = e / dc, j = e % dc;
        xr[pt * PR_DC + j] = hssk_gload(ks.X, (size_t)min(r0 + pt, ks.n - 1) * d + d0 + j);
      }
      if (MODE == PR_SUM && d0 == 0 && tid < RT) wr[tid] = r0 + tid < ks.n ? w[r0 + tid] : 0.;
      __syncthreads();
      for (int j = 0; j < dc; j++) {
        const double t = xt[tid * (PR_DC + 1) + j];
#pragma unroll
        for (int r = 0; r < RT; r++) {
          const double df = xr[r * PR_DC + j] - t;
          if (TYPE == 2) {
            const double tmp = exp(-(df * df) / h2);
            double pw = tmp;
#pragma unroll
            for (int q = 0; q < NS; q++)
              if (q < P) { acc[r][q] += pw; pw *= tmp; }
          } else {
            acc[r][0] += TYPE == 1 ? fabs(df) : df * df;
          }
        }
      }
    }
    const int rend = (int)min((long long)RT, re - r0);
#pragma unroll
    for (int r = 0; r < RT; r++)
      if (r < rend) {
        double v = 0.;
        if (TYPE == 2) {
          double S[8], Kpp[9];
#pragma unroll
          for (int q = 0; q < 8; q++) S[q] = acc[r][q < NS ? q : 0];
          anova_newton<8>(S, Kpp, P, v);
        } else if (TYPE == 3 || TYPE == 4) {
          v = hssk_matern<TYPE == 3 ? 3 : 4, 0>(acc[r][0], hssk_matern_c(TYPE, ks.h), ks.h);
        } else {
          v = exp(acc[r][0] * (TYPE == 0 ? -1. / h2 : -1. / ks.h));
        }
        if (MODE == PR_SUM) sum += wr[r] * v;
        else if (MODE == PR_COLS) sum += (c < m ? w[(size_t)c * ldw + r0 + r] : 0.) * v;
        else if (c < m) pred[(size_t)c * ldo + r0 + r] = v;
      }
  }
  if (MODE != PR_CROSS && c < m) pred[c] = sum;
}

inline void check_spec(const hssk_kernel_spec& ks) {
  if (ks.type < 0 || ks.type > 4)
    throw std::invalid_argument("hssk kernel: type must be 0 (Gauss), 1 (Laplace), 2 (ANOVA), 3 (Matern32) or 4 (Matern52)");
  if (ks.d <= 0 || ks.n < 0 || !ks.X) throw std::invalid_argument("hssk kernel: bad point set");
  if (ks.type == 2 && (ks.p < 1 || ks.p > 8 || ks.p > ks.d)) throw std::invalid_argument("hssk kernel: ANOVA degree must be in [1, min(8, d)]");
}

}  // namespace
