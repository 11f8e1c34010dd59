// The products of the per-coordinate derivatives of the EXACT kernel matrix with a block of up to 64 vectors, the matrices
// never stored (hssk_kernel_matmul_coord): what the gradient of the log marginal likelihood in one length scale per coordinate
// needs beside the kept ULV factors (Kernel<double>::log_marginal_likelihood_gradient_coords).
//
//   out_j(i, c) = sum_r k(x_i, x_r) D_j(x_i, x_r) B(r, c),    j = j0 .. j0 + nj - 1
//   D_j = (x_j - y_j)^2 / h^2 (Gauss),  |x_j - y_j| / h (Laplace):    sum_j k D_j = h dk/dh
//
// kmatmul_kernel (hssk_kmatmul.hip) with NJ matrices in flight: the same tile of 64 rows, the same stages of 16 training points
// (hssk_kmatmul_tile.h), the same transposed v_mfma_f64_16x16x4_f64 product, the same double buffering with one barrier per
// stage, the same padding (a point past the end reads the last valid one and its entries are SELECTED to be 0), the same split
// partials added in split order.  What is shared among the NJ coordinates of a launch is everything that is expensive per
// pair: the distance over all d coordinates, its exponential, the stage of B and its fragment reads.  What each coordinate
// keeps of its own: a stage buffer of g_j (two of them, [64][17] doubles each) and four hssk_d4 accumulators (32 registers).
//
// An entry.  k^ = exp(fl(acc scale)) exactly as kmatmul_kernel evaluates it (the coordinates in order), then per coordinate
//   g_j = fl(fl(k^ fl(df_j df_j)) c),  c = fl(1 / fl(h h))    (Gauss)
//   g_j = fl(fl(k^ |df_j|) c),         c = fl(1 / h)          (Laplace)
// with df_j = fl(x_ij - x_rj) taken again from the LDS: products only, nothing a compiler may contract, so that the value of a
// coordinate does not depend on NJ or on the group that computed it.  i == r (and any duplicated point) has df_j = 0 and gives
// exactly 0; no lambda appears anywhere.
//
// Whole points only (d <= KM_DMAX and the footprint within the device's LDS), Gauss and Laplace only.  No atomics: two calls
// agree bit for bit, and splits = 0 is bit for bit the forced count hssk_kernel_matmul_splits(n).
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_kpair.h"
#include "hssk_kmatmul_split.h"
#include "hssk_kmatmul_tile.h"

namespace {

constexpr int KMC_MAX = 4;       // most coordinates per launch (instantiated: 1 .. KMC_MAX)
constexpr int KMC_GROUP = 3;     // what a caller with no preference takes: the cheapest per coordinate measured (profiles/gp_ard.md)

// doubles of dynamic LDS: two stages of g per coordinate | two stages of B | row points [64][dp] | training points 2 x [16][dp]
inline size_t kmc_lds_doubles(int nj, int dp) {
  return (size_t)(2 * nj + 2) * KM_R * KM_KP + (size_t)KM_R * dp + 2 * (size_t)KM_K * dp;
}

template <int TYPE, int NJ>
__global__ __launch_bounds__(KM_T) void kmatmul_coord_kernel(hssk_kernel_spec ks, int j0, const double* __restrict__ B, size_t ldb, int nc,
                                                             double* __restrict__ out, size_t ldo, size_t cstride, size_t slab,
                                                             long long per) {
  HSSK_DYN_SHARED(double, km_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = hssk_uniform(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
  const int d = ks.d, dp = d | 1;
  const long long n = ks.n, i0 = (long long)blockIdx.x * KM_R;
  const long long rb = (long long)blockIdx.y * per, re = min(n, rb + per);
  constexpr int ST = KM_R * KM_KP;   // doubles of one stage buffer
  double* Gs = km_lds;               // [2][NJ][64][17]
  double* Bs = Gs + 2 * NJ * ST;
  double* Xi = Bs + 2 * ST;
  double* Xr = Xi + KM_R * dp;
  double* o = out + (size_t)blockIdx.y * slab;
  const double scale = TYPE == 0 ? -1. / (2. * ks.h * ks.h) : -1. / ks.h;
  const double cj = TYPE == 0 ? 1. / (ks.h * ks.h) : 1. / ks.h;
  // entries of a stage this thread evaluates / fetches: training point kt against the rows (columns of B) it + 16 q
  const int kt = tid & 15, it = tid >> 4;
  hssk_d4 acc[NJ][4];
#pragma unroll
  for (int jj = 0; jj < NJ; jj++)
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[jj][ct] = hssk_d4{0., 0., 0., 0.};
  double bv[4], xv[4];

  // a stage's training points: the 16 d doubles from point k0 on are contiguous; thread t fetches the elements t + 256 q, one
  // stage ahead through registers (points past the last one read the last one)
  int xpt[4], xj[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { xpt[q] = (tid + KM_T * q) / d; xj[q] = (tid + KM_T * q) % d; }
  auto fetch_points = [&](long long k0) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (tid + KM_T * q < KM_K * d) xv[q] = hssk_gload(ks.X, (size_t)min(k0 + xpt[q], n - 1) * d + xj[q]);
  };
  auto put_points = [&](int pb) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (tid + KM_T * q < KM_K * d) Xr[pb * KM_K * dp + xpt[q] * dp + xj[q]] = xv[q];
  };
  auto fetch_b = [&](long long k0) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int c = it + 16 * q;
      bv[q] = (k0 + kt < re && c < nc) ? B[(size_t)(k0 + kt) + (size_t)c * ldb] : 0.;
    }
  };
  // the entries of stage k0 into the NJ buffers at Sg, one pair at a time (one exponential in flight: the loop is kept rolled,
  // as in kmatmul_kernel).  A training point past the split's end: selected to be 0.
  auto generate = [&](long long k0, int pb, double* Sg) {
    const double* xr = Xr + pb * KM_K * dp + kt * dp;
    const bool live = k0 + kt < re;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
      const double* xi = Xi + (it + 16 * q) * dp;
      double a = 0.;
      for (int j = 0; j < d; j++) {
        const double df = xi[j] - xr[j];
        a += TYPE == 1 ? fabs(df) : df * df;
      }
      const double k = exp(a * scale);
#pragma unroll
      for (int jj = 0; jj < NJ; jj++) {
        const double df = xi[j0 + jj] - xr[j0 + jj];
        const double s = TYPE == 1 ? fabs(df) : df * df;
        const double v = (k * s) * cj;
        Sg[jj * ST + (it + 16 * q) * KM_KP + kt] = live ? v : 0.;
      }
    }
  };

  if (rb < re) {
    for (int e = tid; e < KM_R * d; e += KM_T) {
      const int pt = e / d, j = e % d;
      Xi[pt * dp + j] = hssk_gload(ks.X, (size_t)min(i0 + pt, n - 1) * d + j);
    }
    fetch_points(rb);
    put_points(0);
    __syncthreads();
    if (rb + KM_K < re) fetch_points(rb + KM_K);
    generate(rb, 0, Gs);
    fetch_b(rb);
    int buf = 0;
    for (long long k0 = rb; k0 < re; k0 += KM_K, buf ^= 1) {
      const double* Sg = Gs + buf * NJ * ST;
      double* Sb = Bs + buf * ST;
#pragma unroll
      for (int q = 0; q < 4; q++) Sb[(it + 16 * q) * KM_KP + kt] = bv[q];
      const bool more = k0 + KM_K < re;
      if (more) put_points(buf ^ 1);   // (the points of stage k0 + 16 into the buffer stage k0 - 16's evaluation read last)
      __syncthreads();
      if (more) {
        fetch_b(k0 + KM_K);
        if (k0 + 2 * KM_K < re) fetch_points(k0 + 2 * KM_K);
        generate(k0 + KM_K, buf ^ 1, Gs + (buf ^ 1) * NJ * ST);   // (those buffers were last read before this stage's barrier)
      }
#pragma unroll
      for (int kk = 0; kk < KM_K; kk += 4) {
        // (all four column tiles whatever nc, as in kmatmul_kernel; one read of the B fragments serves the NJ coordinates)
        double bf[4];
#pragma unroll
        for (int ct = 0; ct < 4; ct++) bf[ct] = Sb[(16 * ct + l15) * KM_KP + kk + l4];
#pragma unroll
        for (int jj = 0; jj < NJ; jj++) {
          const double gf = Sg[jj * ST + (16 * wave + l15) * KM_KP + kk + l4];
#pragma unroll
          for (int ct = 0; ct < 4; ct++) acc[jj][ct] = hssk_mfma_f64_16x16x4(bf[ct], gf, acc[jj][ct]);
        }
      }
    }
  }
  // acc[jj][ct][r] = out_{j0 + jj}(row 16 wave + l15, column 16 ct + l4 + 4 r)
  const long long gi = i0 + 16 * wave + l15;
#pragma unroll
  for (int jj = 0; jj < NJ; jj++)
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int c = 16 * ct + l4 + 4 * r;
        if (gi < n && c < nc) hssk_gstore(o, (size_t)jj * cstride + (size_t)gi + (size_t)c * ldo, acc[jj][ct][r]);
      }
}

template <int TYPE, int NJ>
void kmc_launch(hssk_ctx* ctx, const hssk_kernel_spec& ks, int j0, const double* B, size_t ldb, int nc, double* out, size_t ldo,
                size_t cstride, size_t slab, long long per, int splits) {
  const size_t shm = sizeof(double) * kmc_lds_doubles(NJ, ks.d | 1);
  const dim3 grid((unsigned)((ks.n + KM_R - 1) / KM_R), (unsigned)splits);
  hssk_rt::allow_dynamic_lds(kmatmul_coord_kernel<TYPE, NJ>, shm);
  HSSK_LAUNCH((kmatmul_coord_kernel<TYPE, NJ>), grid, dim3(KM_T), shm, ctx->stream, ks, j0, B, ldb, nc, out, ldo, cstride, slab, per);
}

template <int TYPE>
void kmc_dispatch(int nj, hssk_ctx* ctx, const hssk_kernel_spec& ks, int j0, const double* B, size_t ldb, int nc, double* out,
                  size_t ldo, size_t cstride, size_t slab, long long per, int splits) {
  static_assert(KMC_MAX == 4, "one case per instantiated group size");
  switch (nj) {
    case 1: kmc_launch<TYPE, 1>(ctx, ks, j0, B, ldb, nc, out, ldo, cstride, slab, per, splits); break;
    case 2: kmc_launch<TYPE, 2>(ctx, ks, j0, B, ldb, nc, out, ldo, cstride, slab, per, splits); break;
    case 3: kmc_launch<TYPE, 3>(ctx, ks, j0, B, ldb, nc, out, ldo, cstride, slab, per, splits); break;
    default: kmc_launch<TYPE, 4>(ctx, ks, j0, B, ldb, nc, out, ldo, cstride, slab, per, splits); break;
  }
}

}  // namespace

extern "C" int hssk_kernel_matmul_coord_max(void) { return KMC_MAX; }
extern "C" int hssk_kernel_matmul_coord_group(void) { return KMC_GROUP; }

extern "C" int hssk_kernel_matmul_coord(hssk_ctx* ctx, const hssk_kernel_spec* spec, int j0, int nj, const double* B, long long ldb,
                                        int nc, double* out, long long ldo, long long out_stride, int splits) {
  HSSK_API_BEGIN
  if (!ctx || !spec) throw std::invalid_argument("hssk_kernel_matmul_coord: no context or kernel");
  if (nc < 0 || nc > 64) throw std::invalid_argument("hssk_kernel_matmul_coord: between 0 and 64 columns at a time");
  if (j0 < 0 || nj < 1 || nj > KMC_MAX)
    throw std::invalid_argument("hssk_kernel_matmul_coord: coordinates j0 >= 0, between 1 and hssk_kernel_matmul_coord_max() of them");
  if (splits < 0) throw std::invalid_argument("hssk_kernel_matmul_coord: negative split count");
  if (spec->n == 0 || nc == 0) return 0;
  check_spec(*spec);
  if (spec->type != 0 && spec->type != 1) HSSK_UNSUPPORTED("Gauss and Laplace kernels only (no ANOVA, no Matern coordinate derivative)");
  if (spec->d > KM_DMAX) HSSK_UNSUPPORTED("at most 64 coordinates");
  if ((long long)j0 + nj > spec->d) throw std::invalid_argument("hssk_kernel_matmul_coord: coordinates past the dimension");
  if (!B || !out) throw std::invalid_argument("hssk_kernel_matmul_coord: null pointer");
  const long long n = spec->n;
  if (ldb < n || ldo < n) throw std::invalid_argument("hssk_kernel_matmul_coord: leading dimension below the point count");
  const long long block = ldo * (nc - 1) + n;   // doubles from the first to the last entry of one output block
  if (out_stride < block) throw std::invalid_argument("hssk_kernel_matmul_coord: output stride below one n x nc block");
  if (B < out + (size_t)(nj - 1) * out_stride + block && out < B + (size_t)ldb * (nc - 1) + n)
    throw std::invalid_argument("hssk_kernel_matmul_coord: out may not alias B");
  if ((n + KM_R - 1) / KM_R > 0x7fffffffLL) throw std::invalid_argument("hssk_kernel_matmul_coord: too many row tiles for one grid");
  if (sizeof(double) * kmc_lds_doubles(nj, spec->d | 1) > hssk_rt::max_lds_per_workgroup()) {
    hssk_set_error("hssk_kernel_matmul_coord: the stage buffers do not fit the LDS of this device");
    return 2;
  }
  const KmSplit sp = km_split_plan(n, KM_K, splits, hssk_kernel_matmul_splits(n));
  const long long s = sp.s, per = sp.per;
  double* dst = out;
  size_t ldd = (size_t)ldo, slab = 0, cstride = (size_t)out_stride;
  if (s > 1) {   // the slabs of coordinate jj: s of them from dst + jj cstride on
    slab = (size_t)n * nc;
    cstride = slab * (size_t)s;
    dst = ctx->kmm_slabs(sizeof(double) * cstride * (size_t)nj);
    ldd = (size_t)n;
  }
  if (spec->type == 0) kmc_dispatch<0>(nj, ctx, *spec, j0, B, (size_t)ldb, nc, dst, ldd, cstride, slab, per, (int)s);
  else kmc_dispatch<1>(nj, ctx, *spec, j0, B, (size_t)ldb, nc, dst, ldd, cstride, slab, per, (int)s);
  hssk_rt::check_launch();
  if (s > 1)
    for (int jj = 0; jj < nj; jj++)
      if (const int rc = km_reduce_splits(ctx, dst + (size_t)jj * cstride, n, nc, (int)s, out + (size_t)jj * (size_t)out_stride, ldo)) return rc;
  HSSK_API_END
}
