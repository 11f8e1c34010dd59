// The cross-kernel block between test and training points on a grid over BOTH point sets (hssk_kernel_cross_split), and its
// product with a block of up to 64 vectors, the block never stored (hssk_kernel_cross_matmul).  What the joint predictive
// covariance of a Gaussian process needs beside the kept ULV factors (Kernel<double>::predict_covariance).
//
//   hssk_kernel_cross_split    out(r, c) = k(x_r, t_c)                      r < n, c < m
//   hssk_kernel_cross_matmul   out(a, c) = sum_r k(t_a, x_r) B(r, c)        a < m, c < nc <= 64      (no lambda term)
//
// hssk_kernel_cross_split is the kernel of hssk_kpair.h in its mode PR_CROSS with a second grid dimension over ranges of whole
// 64-point tiles of the training points: the pair arithmetic is that one piece of code, an entry depends on its pair alone, and
// the block is bit for bit that of hssk_kernel_cross whatever the split count.
//
// hssk_kernel_cross_matmul.  Tiling: the grid is (tiles of 64 test points = output rows) x (splits of the training points).  A
// workgroup of four waves owns a tile; wave w keeps the 16 rows 16 w .. 16 w + 15 against all 64 columns in four hssk_d4
// accumulators.  The training points of the workgroup's split arrive in stages of 16 (hssk_kmatmul_tile.h: the stages of
// hssk_kernel_matmul).  A stage is a 64 x 16 block of k and the 16 x 64 tile of B, both in the LDS as [64][17] doubles, two
// buffers each.  Every thread evaluates four entries of a stage (one training point against four test points) and fetches four
// entries of B.  The double-buffered pattern of kmatmul_kernel: while v_mfma_f64_16x16x4_f64 multiplies stage s out of buffer
// s & 1, the same wave's vector unit evaluates stage s + 1 into the other buffer and fetches that stage's B entries into
// registers -- one barrier per stage.  The product is taken transposed (A operand: the B tile, B operand: k), so that the 16
// lanes of a result register hold 16 consecutive rows of one output column.
//
// Points.  Up to KM_DMAX coordinates the tile's 64 test points stay in the LDS for the whole kernel and a stage's 16 training
// points are fetched one stage ahead through registers; beyond that -- or where that footprint does not fit the device's LDS --
// both point sets pass through in chunks of KX_DC coordinates and the four distances of a thread accumulate in registers across
// the chunks, the coordinates in order.
//
// Padding.  Test points past m and training points past the split's end read the LAST valid point (never memory out of bounds,
// never an exp of garbage); the k of such a training point is SELECTED to be 0 (not multiplied by 0), its B entries are 0, and the
// rows past m and the columns past nc are not stored.
//
// Order of every sum.  The distance of a pair: the coordinates in order.  An output entry: its training points in order within a
// split -- four per MFMA, the MFMAs of a stage in k order, the stages in order, one accumulator per entry -- and, with more than
// one split, the split partials in split order (hssk_sum_slabs over slabs the context keeps).  No atomics: two calls agree bit
// for bit, and splits = 0 is bit for bit the forced count hssk_kernel_cross_matmul_splits(n, m).
//
// With one tile of test points all parallelism comes from the split: the automatic count aims at KX_GRID workgroups with at
// most KX_SPLITS splits (profiles/gp_covariance.md has the sweep both were chosen from).
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_kpair.h"
#include "hssk_kmatmul_split.h"
#include "hssk_kmatmul_tile.h"

namespace {

constexpr int KX_DC = 32;              // coordinates per pass beyond KM_DMAX
constexpr long long KX_GRID = 768;     // workgroups hssk_kernel_cross_matmul_splits aims at: three per compute unit of an MI355X, what
                                       // the kernel's registers allow -- one full round (1024 measured 14 % slower than 768 and 1536)
constexpr long long KX_SPLITS = 256;   // and the most splits it takes: beyond that the sum of the slabs costs more than the split gains
constexpr long long KC_GRID = 2048;    // one-wave workgroups hssk_kernel_cross_splits aims at (flat from 512 on)

// doubles of dynamic LDS: two stages of k | two stages of B | test points [64][dp] | training points 2 x [16][dp]
inline size_t kx_lds_doubles(int dp) { return 4 * (size_t)KM_R * KM_KP + (size_t)KM_R * dp + 2 * (size_t)KM_K * dp; }
inline int kx_stride(int d, bool wide) { return wide ? KX_DC + 1 : (d | 1); }

template <int TYPE, bool WIDE>
__global__ __launch_bounds__(KM_T) void kcross_matmul_kernel(hssk_kernel_spec ks, const double* __restrict__ T, int m,
                                                             const double* __restrict__ B, size_t ldb, int nc, double* __restrict__ out,
                                                             size_t ldo, size_t slab, long long per) {
  HSSK_DYN_SHARED(double, kx_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = hssk_uniform(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
  const int d = ks.d, dp = WIDE ? KX_DC + 1 : (d | 1);
  const long long n = ks.n;
  const int i0 = (int)blockIdx.x * KM_R;
  const long long rb = (long long)blockIdx.y * per, re = min(n, rb + per);
  double* Gs = kx_lds;
  double* Bs = Gs + 2 * KM_R * KM_KP;
  double* Xi = Bs + 2 * KM_R * KM_KP;
  double* Xr = Xi + KM_R * dp;
  double* o = out + (size_t)blockIdx.y * slab;
  const double scale = TYPE == 0 ? -1. / (2. * ks.h * ks.h) : -1. / ks.h;
  const double mc = hssk_matern_c(TYPE, ks.h);   // (TYPE 3 and 4 only)
  // entries of a stage this thread evaluates / fetches: training point kt against the test points (columns of B) it + 16 q
  const int kt = tid & 15, it = tid >> 4;
  hssk_d4 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ct++) acc[ct] = hssk_d4{0., 0., 0., 0.};
  double bv[4], xv[4];

  // a stage's training points (whole points only): the 16 d doubles from point k0 on are contiguous; thread t fetches the
  // elements t + 256 q, one stage ahead through registers (points past the last one read the last one)
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
  // a distance -> an entry of k, straight into the stage buffer Sg (a training point past the split's end: selected to be 0)
  auto finish = [&](long long k0, int q, double a, double* Sg) {
    double v;
    if (TYPE >= 3) v = hssk_matern<TYPE >= 3 ? TYPE : 3, 0>(a, mc, ks.h);
    else v = exp(a * scale);
    Sg[(it + 16 * q) * KM_KP + kt] = k0 + kt < re ? v : 0.;
  };
  // the entries of stage k0 into Sg.  Whole points: one entry at a time (the loop is kept rolled: one exponential in flight)
  auto generate = [&](long long k0, int pb, double* Sg) {
    if (!WIDE) {
      const double* xr = Xr + pb * KM_K * dp + kt * dp;
#pragma unroll 1
      for (int q = 0; q < 4; q++) {
        const double* xi = Xi + (it + 16 * q) * dp;
        double a = 0.;
        for (int j = 0; j < d; j++) {
          const double df = xi[j] - xr[j];
          a += TYPE == 1 ? fabs(df) : df * df;
        }
        finish(k0, q, a, Sg);
      }
    } else {
      double a[4] = {0., 0., 0., 0.};
      for (int d0 = 0; d0 < d; d0 += KX_DC) {
        const int dc = min(KX_DC, d - d0);
        __syncthreads();   // (the previous pass has been read by every wave)
        for (int e = tid; e < KM_R * dc; e += KM_T) {
          const int pt = e / dc, j = e % dc;
          Xi[pt * dp + j] = hssk_gload(T, (size_t)min(i0 + pt, m - 1) * d + d0 + j);
        }
        for (int e = tid; e < KM_K * dc; e += KM_T) {
          const int pt = e / dc, j = e % dc;
          Xr[pt * dp + j] = hssk_gload(ks.X, (size_t)min(k0 + pt, n - 1) * d + d0 + j);
        }
        __syncthreads();
        for (int j = 0; j < dc; j++) {
          const double t = Xr[kt * dp + j];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const double df = Xi[(it + 16 * q) * dp + j] - t;
            a[q] += TYPE == 1 ? fabs(df) : df * df;
          }
        }
      }
#pragma unroll 1
      for (int q = 0; q < 4; q++) finish(k0, q, q == 0 ? a[0] : q == 1 ? a[1] : q == 2 ? a[2] : a[3], Sg);
    }
  };

  if (rb < re) {
    if (!WIDE) {
      for (int e = tid; e < KM_R * d; e += KM_T) {
        const int pt = e / d, j = e % d;
        Xi[pt * dp + j] = hssk_gload(T, (size_t)min(i0 + pt, m - 1) * d + j);
      }
      fetch_points(rb);
      put_points(0);
      __syncthreads();
      if (rb + KM_K < re) fetch_points(rb + KM_K);
    }
    generate(rb, 0, Gs);
    fetch_b(rb);
    int buf = 0;
    for (long long k0 = rb; k0 < re; k0 += KM_K, buf ^= 1) {
      double* Sg = Gs + buf * KM_R * KM_KP;
      double* Sb = Bs + buf * KM_R * KM_KP;
#pragma unroll
      for (int q = 0; q < 4; q++) Sb[(it + 16 * q) * KM_KP + kt] = bv[q];
      const bool more = k0 + KM_K < re;
      if (!WIDE && more) put_points(buf ^ 1);   // (the points of stage k0 + 16 into the buffer stage k0 - 16's evaluation read last)
      __syncthreads();
      if (more) {
        fetch_b(k0 + KM_K);
        if (!WIDE && k0 + 2 * KM_K < re) fetch_points(k0 + 2 * KM_K);
        generate(k0 + KM_K, buf ^ 1, Gs + (buf ^ 1) * KM_R * KM_KP);   // (that buffer was last read before this stage's barrier)
      }
#pragma unroll
      for (int kk = 0; kk < KM_K; kk += 4) {
        const double gf = Sg[(16 * wave + l15) * KM_KP + kk + l4];
        // (all four column tiles whatever nc: the B entries of the columns past nc are zeros in the LDS)
#pragma unroll
        for (int ct = 0; ct < 4; ct++) acc[ct] = hssk_mfma_f64_16x16x4(Sb[(16 * ct + l15) * KM_KP + kk + l4], gf, acc[ct]);
      }
    }
  }
  // acc[ct][r] = out(row 16 wave + l15, column 16 ct + l4 + 4 r)
  const int gi = i0 + 16 * wave + l15;
#pragma unroll
  for (int ct = 0; ct < 4; ct++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int c = 16 * ct + l4 + 4 * r;
      if (gi < m && c < nc) hssk_gstore(o, (size_t)gi + (size_t)c * ldo, acc[ct][r]);
    }
}

template <int TYPE, bool WIDE>
void kx_launch(hssk_ctx* ctx, const hssk_kernel_spec& ks, const double* T, int m, const double* B, size_t ldb, int nc, double* out, size_t ldo,
               size_t slab, long long per, int splits) {
  const size_t shm = sizeof(double) * kx_lds_doubles(kx_stride(ks.d, WIDE));
  const dim3 grid((unsigned)((m + KM_R - 1) / KM_R), (unsigned)splits);
  hssk_rt::allow_dynamic_lds(kcross_matmul_kernel<TYPE, WIDE>, shm);
  HSSK_LAUNCH((kcross_matmul_kernel<TYPE, WIDE>), grid, dim3(KM_T), shm, ctx->stream, ks, T, m, B, ldb, nc, out, ldo, slab, per);
}
template <int TYPE, class... A>
void kx_dispatch_wide(bool wide, A... a) {
  if (wide) kx_launch<TYPE, true>(a...);
  else kx_launch<TYPE, false>(a...);
}
template <class... A>
void kx_dispatch(int type, bool wide, A... a) {
  switch (type) {
    case 0: kx_dispatch_wide<0>(wide, a...); break;
    case 1: kx_dispatch_wide<1>(wide, a...); break;
    case 3: kx_dispatch_wide<3>(wide, a...); break;
    default: kx_dispatch_wide<4>(wide, a...); break;
  }
}

// the PR_CROSS kernels of hssk_kpair.h on the split grid
void kc_launch(hssk_ctx* ctx, const hssk_kernel_spec* spec, const double* T, int m, double* out, size_t ldo, int splits) {
  const dim3 grid((unsigned)((m + PR_T - 1) / PR_T), (unsigned)splits);
  const double* w = nullptr;
  const size_t ldw = 0;
  const bool wide = spec->d > PR_DMAX;
  if (!wide && spec->type >= 3) HSSK_LAUNCH((kernel_predict_kernel<PR_CROSS, true, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (!wide) HSSK_LAUNCH((kernel_predict_kernel<PR_CROSS, false, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 3) HSSK_LAUNCH((kernel_predict_wide_kernel<3, 32, PR_CROSS, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 4) HSSK_LAUNCH((kernel_predict_wide_kernel<4, 32, PR_CROSS, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 0) HSSK_LAUNCH((kernel_predict_wide_kernel<0, 32, PR_CROSS, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 1) HSSK_LAUNCH((kernel_predict_wide_kernel<1, 32, PR_CROSS, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else HSSK_LAUNCH((kernel_predict_wide_kernel<2, 8, PR_CROSS, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
}

}  // namespace

extern "C" int hssk_kernel_cross_splits(long long n, int m) {
  if (n <= 0 || m <= 0) return 1;
  const long long tn = (n + PR_T - 1) / PR_T, tm = ((long long)m + PR_T - 1) / PR_T;
  return (int)std::max<long long>(1, std::min(std::min<long long>(tn, 65535), (KC_GRID + tm - 1) / tm));
}

extern "C" int hssk_kernel_cross_split(hssk_ctx* ctx, const hssk_kernel_spec* spec, const double* T, int m, double* out, long long ldo,
                                       int splits) {
  HSSK_API_BEGIN
  if (!ctx || !spec) throw std::invalid_argument("hssk_kernel_cross_split: no context or kernel");
  if (m < 0) throw std::invalid_argument("hssk_kernel_cross_split: negative test point count");
  if (ldo < 0) throw std::invalid_argument("hssk_kernel_cross_split: negative leading dimension");
  if (splits < 0) throw std::invalid_argument("hssk_kernel_cross_split: negative split count");
  if (m == 0) return 0;
  check_spec(*spec);
  if (!T || !out) throw std::invalid_argument("hssk_kernel_cross_split: null pointer");
  if (spec->n == 0) return 0;
  if (ldo < spec->n) throw std::invalid_argument("hssk_kernel_cross_split: leading dimension below the training point count");
  if ((spec->d > PR_DMAX ? PR_LDS_WIDE : PR_LDS_POINT) > hssk_rt::max_lds_per_workgroup()) {
    hssk_set_error("hssk_kernel_cross_split: the point tiles do not fit the LDS of this device");
    return 2;
  }
  // whole tiles of PR_T per split, none empty
  const long long tiles = (spec->n + PR_T - 1) / PR_T;
  long long s = std::min<long long>(splits > 0 ? splits : hssk_kernel_cross_splits(spec->n, m), std::min<long long>(tiles, 65535));
  const long long per = pr_split_per(spec->n, s);
  s = (spec->n + per - 1) / per;
  kc_launch(ctx, spec, T, m, out, (size_t)ldo, (int)s);
  hssk_rt::check_launch();
  HSSK_API_END
}

extern "C" int hssk_kernel_cross_matmul_splits(long long n, int m) {
  if (n <= 0 || m <= 0) return 1;
  const long long tiles = ((long long)m + KM_R - 1) / KM_R, stages = (n + KM_K - 1) / KM_K;
  return (int)std::max<long long>(1, std::min(std::min<long long>(stages, KX_SPLITS), (KX_GRID + tiles - 1) / tiles));
}

extern "C" int hssk_kernel_cross_matmul(hssk_ctx* ctx, const hssk_kernel_spec* spec, const double* T, int m, const double* B, long long ldb,
                                        int nc, double* out, long long ldo, int splits) {
  HSSK_API_BEGIN
  if (!ctx || !spec) throw std::invalid_argument("hssk_kernel_cross_matmul: no context or kernel");
  if (m < 0) throw std::invalid_argument("hssk_kernel_cross_matmul: negative test point count");
  if (nc < 1 || nc > 64) throw std::invalid_argument("hssk_kernel_cross_matmul: between 1 and 64 columns at a time");
  if (splits < 0) throw std::invalid_argument("hssk_kernel_cross_matmul: negative split count");
  if (m == 0) return 0;
  check_spec(*spec);
  if (spec->type == 2) HSSK_UNSUPPORTED("Gauss / Laplace / Matern kernels only (no ANOVA product)");
  const long long n = spec->n;
  if (!T || !out || (n > 0 && !B)) throw std::invalid_argument("hssk_kernel_cross_matmul: null pointer");
  if (ldb < n) throw std::invalid_argument("hssk_kernel_cross_matmul: ldb below the training point count");
  if (ldo < m) throw std::invalid_argument("hssk_kernel_cross_matmul: ldo below the test point count");
  if (B == out) throw std::invalid_argument("hssk_kernel_cross_matmul: out may not alias B");
  if (n == 0) {   // an empty sum: zeros
    for (int c = 0; c < nc; c++)
      if (const int rc = hssk_memset_zero(ctx, out + (size_t)c * ldo, (long long)sizeof(double) * m)) return rc;
    return 0;
  }
  const size_t lds = hssk_rt::max_lds_per_workgroup();
  const bool wide = spec->d > KM_DMAX || sizeof(double) * kx_lds_doubles(kx_stride(spec->d, false)) > lds;
  if (wide && sizeof(double) * kx_lds_doubles(kx_stride(spec->d, true)) > lds) {
    hssk_set_error("hssk_kernel_cross_matmul: the stage buffers do not fit the LDS of this device");
    return 2;
  }
  const KmSplit sp = km_split_plan(n, KM_K, splits, hssk_kernel_cross_matmul_splits(n, m));
  const long long s = sp.s, per = sp.per;
  double* dst = out;
  size_t ldd = (size_t)ldo, slab = 0;
  if (s > 1) {
    slab = (size_t)m * nc;
    dst = ctx->kmm_slabs(sizeof(double) * slab * (size_t)s);
    ldd = (size_t)m;
  }
  kx_dispatch(spec->type, wide, ctx, *spec, T, m, B, (size_t)ldb, nc, dst, ldd, slab, per, (int)s);
  hssk_rt::check_launch();
  if (s > 1)
    if (const int rc = km_reduce_splits(ctx, dst, m, nc, (int)s, out, ldo)) return rc;
  HSSK_API_END
}
