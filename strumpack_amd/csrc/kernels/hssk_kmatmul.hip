// The product of the EXACT kernel matrix -- or of its derivative in the width h -- with a block of up to 64 vectors, the matrix
// never stored (hssk_kernel_matmul), and the column dot products that go with it (hssk_coldots).  What the gradient of the log
// marginal likelihood needs beside the kept ULV factors (Kernel<double>::log_marginal_likelihood_gradient).
//
//   out(i, c) = sum_r g(x_i, x_r) B(r, c)      g = k (+ lambda on the diagonal)                         deriv = 0
//                                              g = dk/dh = k a c_h, a the exponent's magnitude,         deriv = 1
//                                                  c_h = 2 / h (Gauss), 1 / h (Laplace)
//                                              the Matern kernels (TYPE 3 and 4): value and derivative are the finish of
//                                                  hssk_matern.h on the Gauss distance
//
// Tiling.  The grid is (tiles of 64 output rows) x (splits of the training points).  A workgroup of four waves owns a tile; wave w
// keeps the 16 rows 16 w .. 16 w + 15 against all 64 columns in four hssk_d4 accumulators (32 registers).  The training points
// of the workgroup's split arrive in stages of 16.  A stage is a 64 x 16 block of g and the 16 x 64 tile of B; both sit in the
// LDS as [64][17] doubles (k contiguous, padded: the fragment reads of a wave touch 16 rows x 4 k), two buffers each.  Every thread
// evaluates four entries of a stage (one training point against four rows: FP64 differences, one exp) and fetches four entries
// of B.  The double-buffered pattern of gram_gen_panel_kernel: while v_mfma_f64_16x16x4_f64 multiplies stage s out of buffer
// s & 1, the same wave's vector unit evaluates stage s + 1 straight into the other buffer (its last readers were the MFMAs of
// stage s - 1, in front of this stage's barrier) and fetches that stage's B entries into registers, which follow at the top of
// the next iteration -- one barrier per stage.  The product is taken transposed (A operand: the B tile, B operand: g), so that
// the 16 lanes of a result register hold 16 consecutive rows of one output column: 128-byte stores.
//
// Points.  Up to KM_DMAX coordinates the tile's 64 row points stay in the LDS for the whole kernel and a stage's 16 training
// points are fetched one stage ahead through registers into one of two small buffers (stride d | 1: consecutive points on
// different banks).  Beyond that -- or where that footprint does not fit the device's LDS -- the coordinates pass through in
// chunks of KM_DC: both point sets are staged per chunk and stage, and the four distances of a thread accumulate in registers
// across the chunks, the coordinates in order (as in kernel_predict_wide_kernel): the same arithmetic, the same error bound.
//
// Padding.  Rows past n and training points past the split's end read the LAST valid point (never memory out of bounds, never
// an exp of garbage); the g of such a training point is then SELECTED to be 0 (not multiplied by 0), its B entries are 0, and
// the rows and the columns past nc are not stored.  They contribute exactly nothing.
//
// Order of every sum.  The distance of a pair: the coordinates in order.  An output entry: its training points in order -- four
// per MFMA, the MFMAs of a stage in k order, the stages in order, one accumulator per entry -- and, with more than one split,
// the split partials in split order (hssk_sum_slabs over slabs the context keeps).  No atomics: two calls agree bit for bit,
// and splits = 0 is bit for bit the forced count hssk_kernel_matmul_splits(n).
//
// hssk_coldots: one workgroup per column; thread t adds the products of the rows t, t + 256, ... in that order, the 64 lane sums
// of a wave are added on the DPP network, the four wave sums in wave order.
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_kpair.h"
#include "hssk_kmatmul_split.h"
#include "hssk_kmatmul_tile.h"

namespace {

constexpr int KM_DC = 32;      // coordinates per pass beyond KM_DMAX

// doubles of dynamic LDS: two stages of g | two stages of B | row points [64][dp] | training points 2 x [16][dp]
inline size_t km_lds_doubles(int dp) { return 4 * (size_t)KM_R * KM_KP + (size_t)KM_R * dp + 2 * (size_t)KM_K * dp; }
inline int km_stride(int d, bool wide) { return wide ? KM_DC + 1 : (d | 1); }

template <int TYPE, int DERIV, bool WIDE>
__global__ __launch_bounds__(KM_T) void kmatmul_kernel(hssk_kernel_spec ks, const double* __restrict__ B, size_t ldb, int nc,
                                                       double* __restrict__ out, size_t ldo, size_t slab, long long per) {
  HSSK_DYN_SHARED(double, km_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = hssk_uniform(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
  const int d = ks.d, dp = WIDE ? KM_DC + 1 : (d | 1);
  const long long n = ks.n, i0 = (long long)blockIdx.x * KM_R;
  const long long rb = (long long)blockIdx.y * per, re = min(n, rb + per);
  double* Gs = km_lds;
  double* Bs = Gs + 2 * KM_R * KM_KP;
  double* Xi = Bs + 2 * KM_R * KM_KP;
  double* Xr = Xi + KM_R * dp;
  double* o = out + (size_t)blockIdx.y * slab;
  const double scale = TYPE == 0 ? -1. / (2. * ks.h * ks.h) : -1. / ks.h;
  const double ch = TYPE == 0 ? 2. / ks.h : 1. / ks.h;
  const double mc = hssk_matern_c(TYPE, ks.h);   // (TYPE 3 and 4 only)
  // entries of a stage this thread evaluates / fetches: training point kt against the rows (columns of B) it + 16 q
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
  // a distance -> an entry of g, straight into the stage buffer Sg (a training point past the split's end: selected to be 0)
  auto finish = [&](long long k0, int q, double a, double* Sg) {
    double v;
    if (TYPE >= 3) {
      v = hssk_matern<TYPE >= 3 ? TYPE : 3, DERIV>(a, mc, ks.h);
    } else {
      const double e = a * scale;
      v = exp(e);
      if (DERIV) v = v * -e * ch;
    }
    if (!DERIV && i0 + it + 16 * q == k0 + kt) v += ks.lambda;
    Sg[(it + 16 * q) * KM_KP + kt] = k0 + kt < re ? v : 0.;
  };
  // the entries of stage k0 into Sg.  Whole points: one entry at a time (one exponential in flight: the loop is kept rolled, so
  // that the registers of four inlined exponentials do not cost a workgroup per compute unit)
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
      for (int d0 = 0; d0 < d; d0 += KM_DC) {
        const int dc = min(KM_DC, d - d0);
        __syncthreads();   // (the previous pass has been read by every wave)
        for (int e = tid; e < KM_R * dc; e += KM_T) {
          const int pt = e / dc, j = e % dc;
          Xi[pt * dp + j] = hssk_gload(ks.X, (size_t)min(i0 + pt, n - 1) * d + d0 + j);
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
        Xi[pt * dp + j] = hssk_gload(ks.X, (size_t)min(i0 + pt, n - 1) * d + j);
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
        // (all four column tiles whatever nc: the B entries of the columns past nc are zeros in the LDS, and MFMAs behind a
        // branch on the tile count cost the kernel 120 registers -- a workgroup per compute unit)
#pragma unroll
        for (int ct = 0; ct < 4; ct++) acc[ct] = hssk_mfma_f64_16x16x4(Sb[(16 * ct + l15) * KM_KP + kk + l4], gf, acc[ct]);
      }
    }
  }
  // acc[ct][r] = out(row 16 wave + l15, column 16 ct + l4 + 4 r)
  const long long gi = i0 + 16 * wave + l15;
#pragma unroll
  for (int ct = 0; ct < 4; ct++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int c = 16 * ct + l4 + 4 * r;
      if (gi < n && c < nc) hssk_gstore(o, (size_t)gi + (size_t)c * ldo, acc[ct][r]);
    }
}

template <int TYPE, int DERIV, bool WIDE>
void km_launch(hssk_ctx* ctx, const hssk_kernel_spec& ks, const double* B, size_t ldb, int nc, double* out, size_t ldo, size_t slab,
               long long per, int splits) {
  const size_t shm = sizeof(double) * km_lds_doubles(km_stride(ks.d, WIDE));
  const dim3 grid((unsigned)((ks.n + KM_R - 1) / KM_R), (unsigned)splits);
  hssk_rt::allow_dynamic_lds(kmatmul_kernel<TYPE, DERIV, WIDE>, shm);
  HSSK_LAUNCH((kmatmul_kernel<TYPE, DERIV, WIDE>), grid, dim3(KM_T), shm, ctx->stream, ks, B, ldb, nc, out, ldo, slab, per);
}

// type -> deriv -> wide: the 16 instances
template <int TYPE, int DERIV, class... A>
void km_dispatch_wide(bool wide, A... a) {
  if (wide) km_launch<TYPE, DERIV, true>(a...);
  else km_launch<TYPE, DERIV, false>(a...);
}
template <int TYPE, class... A>
void km_dispatch_deriv(int deriv, bool wide, A... a) {
  if (deriv) km_dispatch_wide<TYPE, 1>(wide, a...);
  else km_dispatch_wide<TYPE, 0>(wide, a...);
}
template <class... A>
void km_dispatch(int type, int deriv, bool wide, A... a) {
  switch (type) {
    case 0: km_dispatch_deriv<0>(deriv, wide, a...); break;
    case 1: km_dispatch_deriv<1>(deriv, wide, a...); break;
    case 3: km_dispatch_deriv<3>(deriv, wide, a...); break;
    default: km_dispatch_deriv<4>(deriv, wide, a...); break;
  }
}

__global__ __launch_bounds__(KM_T) void coldots_kernel(const double* __restrict__ A, size_t lda, const double* __restrict__ B, size_t ldb,
                                                       long long n, double* __restrict__ out) {
  HSSK_SHARED double part[KM_T / 64];
  const int tid = threadIdx.x;
  const double* a = A + (size_t)blockIdx.x * lda;
  const double* b = B + (size_t)blockIdx.x * ldb;
  double s = 0.;
  for (long long i = tid; i < n; i += KM_T) s += a[i] * b[i];
  s = hssk_wave_sum(s);   // (every lane takes part, also those without a row)
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.;
    for (int w = 0; w < KM_T / 64; w++) t += part[w];
    out[blockIdx.x] = t;
  }
}

}  // namespace

extern "C" int hssk_kernel_matmul_splits(long long n) {
  if (n <= 0) return 1;
  const long long tiles = (n + KM_R - 1) / KM_R, stages = (n + KM_K - 1) / KM_K;
  return (int)std::max<long long>(1, std::min(std::min<long long>(stages, 64), (KM_GRID + tiles - 1) / tiles));
}

extern "C" int hssk_kernel_matmul(hssk_ctx* ctx, const hssk_kernel_spec* spec, int deriv, const double* B, long long ldb, int nc,
                                  double* out, long long ldo, int splits) {
  HSSK_API_BEGIN
  if (!ctx || !spec) throw std::invalid_argument("hssk_kernel_matmul: no context or kernel");
  if (nc < 0 || nc > 64) throw std::invalid_argument("hssk_kernel_matmul: between 0 and 64 columns at a time");
  if (deriv != 0 && deriv != 1) throw std::invalid_argument("hssk_kernel_matmul: deriv is 0 (the kernel) or 1 (its derivative in h)");
  if (splits < 0) throw std::invalid_argument("hssk_kernel_matmul: negative split count");
  if (spec->n == 0 || nc == 0) return 0;
  check_spec(*spec);
  if (spec->type == 2) HSSK_UNSUPPORTED("Gauss / Laplace / Matern kernels only (no ANOVA derivative, no ANOVA product)");
  if (!B || !out) throw std::invalid_argument("hssk_kernel_matmul: null pointer");
  if (ldb < spec->n || ldo < spec->n) throw std::invalid_argument("hssk_kernel_matmul: leading dimension below the point count");
  if (B == out) throw std::invalid_argument("hssk_kernel_matmul: out may not alias B");
  const long long n = spec->n;
  if ((n + KM_R - 1) / KM_R > 0x7fffffffLL) throw std::invalid_argument("hssk_kernel_matmul: too many row tiles for one grid");
  const size_t lds = hssk_rt::max_lds_per_workgroup();
  const bool wide = spec->d > KM_DMAX || sizeof(double) * km_lds_doubles(km_stride(spec->d, false)) > lds;
  if (wide && sizeof(double) * km_lds_doubles(km_stride(spec->d, true)) > lds) {
    hssk_set_error("hssk_kernel_matmul: the stage buffers do not fit the LDS of this device");
    return 2;
  }
  const KmSplit sp = km_split_plan(n, KM_K, splits, hssk_kernel_matmul_splits(n));
  const long long s = sp.s, per = sp.per;
  double* dst = out;
  size_t ldd = (size_t)ldo, slab = 0;
  if (s > 1) {
    slab = (size_t)n * nc;
    dst = ctx->kmm_slabs(sizeof(double) * slab * (size_t)s);
    ldd = (size_t)n;
  }
  km_dispatch(spec->type, deriv, wide, ctx, *spec, B, (size_t)ldb, nc, dst, ldd, slab, per, (int)s);
  hssk_rt::check_launch();
  if (s > 1)
    if (const int rc = km_reduce_splits(ctx, dst, n, nc, (int)s, out, ldo)) return rc;
  HSSK_API_END
}

extern "C" int hssk_coldots(hssk_ctx* ctx, const double* A, long long lda, const double* B, long long ldb, long long n, int nc, double* out) {
  HSSK_API_BEGIN
  if (!ctx) throw std::invalid_argument("hssk_coldots: no context");
  if (n < 0 || nc < 0) throw std::invalid_argument("hssk_coldots: negative size");
  if (nc == 0) return 0;
  if (!out || (n > 0 && (!A || !B))) throw std::invalid_argument("hssk_coldots: null pointer");
  if (lda < n || ldb < n) throw std::invalid_argument("hssk_coldots: leading dimension below the row count");
  HSSK_LAUNCH(coldots_kernel, dim3((unsigned)nc), dim3(KM_T), 0, ctx->stream, A, (size_t)lda, B, (size_t)ldb, n, out);
  hssk_rt::check_launch();
  HSSK_API_END
}
