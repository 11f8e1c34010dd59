// The product of the exact kernel matrix with a block of up to 64 vectors in single precision per pair: the inner operator of the
// mixed-precision exact solves (hssk_kernel_matmul_f32).  FP32 per pair and per chunk of 64 training points on the
// matrix cores, FP64 across chunks and splits, bitwise repeatable.
//
//   out(i, c) = sum_r k32(x_i, x_r) B(r, c) + lambda B(i, c)         B, out: the solver's FP64 blocks
//
// Points (hssk_kernel_matmul_f32_prep, once per call of the solver).  The FP64 points are centred in FP64 (kmf_mean_kernel: the
// mean in a fixed order), scaled by s (Gauss: s^2 = log2(e) / (2 h^2); Laplace: s = log2(e) / h; Matern: s = sqrt(2 nu) / h) and
// rounded ONCE to float.  They
// are kept coordinate by coordinate (row j of Pa is coordinate j of every point, ldn = n rounded up to 64) in the augmented form
// of the prediction kernel: rows 0 .. d-1: -2 x~, row d: |x~|^2 (of the rounded x~, in FP64, rounded once), row d + 1: 1, zeros up
// to the 2 KSM rows the matrix-core route reads; padding points are all zero.  x~ itself is -0.5 times a row: exact.  tmax[t]:
// the largest |x~|^2 of tile t.
//
// Grid: (tiles of 64 rows) x (splits of the training points).  A workgroup of four waves meets its split in stages of 64 training
// points.  A stage is the 64 x 64 block g of kernel values and the 64 x 64 block of B rounded to float, both in the LDS, two
// buffers each.  While v_mfma_f32_32x32x2_f32 multiplies stage s out of buffer s & 1, the same waves evaluate stage s + 1 into
// the other buffer and fetch its B entries into registers -- one barrier per stage, as in hssk_kmatmul.hip.
//
// The kernel values of a stage go one of two routes, the same for the whole workgroup:
//   * matrix cores (Gauss, Matern): wave w takes the 32 training points 32 (w >> 1) .. against the 32 rows 32 (w & 1) ..; the
//     base-2 exponent |x~_r|^2 + |x~_i|^2 - 2 x~_r . x~_i is the accumulator of KSM v_mfma_f32_32x32x2_f32 over K = d + 2 (training
//     points along M, rows along N = the lane), then exp2.  Taken iff 4 (d + 4) 2^-24 (tmax[row tile] + tmax[training tile]), the
//     worst error the norm expansion can cause in an exponent, is at most HSSK_KMATMUL_F32_TAU;
//   * difference form (Laplace, and the Gauss stages the rule refuses): lane = row, wave w takes the training points 16 w ..
//     16 w + 15, whose coordinates arrive through uniform loads; FP32 differences, the coordinates in order, then exp2.
// The pair r == i is SELECTED to be 1 and a training point past the split's end to be 0, whatever was evaluated.
// The Matern kernels (TYPE 3 and 4) take both routes under the same rule and threshold: with their scale the
// accumulator -- of the matrix cores or of the differences -- is u = s^2, and exp2 gives way to hssk_matern_f32(u), whose clamp
// max(u, 0) in front of the square root keeps near-duplicate points, where cancellation makes u negative, finite.
//
// The product is taken transposed (A operand: the B stage, columns along M; B operand: g, rows along N = the lane), wave w owning
// the 32 rows 32 (w & 1) .. against the 32 columns 32 (w >> 1) ..: 32 MFMAs per stage into a cleared FP32 accumulator, which is
// then added to the FP64 running sums in registers: no FP32 sum is longer than 64 training points.  lambda B(i, c) is added in
// FP64 from the unrounded B by the split that holds the diagonal.  With more than one split the partials go to slabs the context
// keeps and are added in split order (hssk_sum_slabs).  No atomics on any result: two calls agree bit for bit, and a column's
// result depends on no other column (the MFMA keeps the columns of its A operand apart).
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_kpair.h"
#include "hssk_kmatmul_split.h"
#include "hssk_matern.h"

#include <cmath>
#include <cstdlib>

namespace {

constexpr int KF_T = 64;        // tile edge: rows per workgroup, training points per stage (= the longest FP32 sum)
constexpr int KF_BP = KF_T + 1; // row stride of the staged B block (k contiguous: the transposing reads spread over the banks)
constexpr int KF_G = 64;        // workgroups of the mean reduction
constexpr int KF_DMAX = 64;
constexpr long long KF_GRID = 1024;   // workgroups hssk_kernel_matmul_f32_splits aims at (two rounds of two per compute unit)

inline int kf_ksm(int d) { return d <= 2 ? 2 : (d <= 8 ? 5 : (d <= 16 ? 9 : (d <= 32 ? 17 : 33))); }
inline size_t kf_align(size_t v) { return (v + 255) & ~size_t(255); }
struct KfLayout {
  long long ldn, nt;
  int kp;
  size_t o_pm, o_pa, o_tm, total;
};
inline KfLayout kf_layout(long long n, int d) {
  KfLayout L;
  L.nt = (n + KF_T - 1) / KF_T;
  L.ldn = L.nt * KF_T;
  L.kp = 2 * kf_ksm(d);
  L.o_pm = 0;
  L.o_pa = kf_align(sizeof(double) * KF_G * (size_t)d);
  L.o_tm = kf_align(L.o_pa + sizeof(float) * (size_t)L.kp * (size_t)L.ldn);
  L.total = kf_align(L.o_tm + sizeof(float) * (size_t)L.nt);
  return L;
}

// partial sums of the coordinates: workgroup g adds the points g, g + G, ... (thread t always meets coordinate t % d)
__global__ __launch_bounds__(256) void kmf_mean_kernel(const double* __restrict__ X, int d, long long n, double* __restrict__ part) {
  HSSK_SHARED double red[256];
  const int tid = threadIdx.x, Tp = (256 / d) * d, ppw = Tp / d;
  double s = 0.;
  if (tid < Tp) {
    const int j = tid % d, pl = tid / d;
    for (long long i = (long long)blockIdx.x * ppw + pl; i < n; i += (long long)KF_G * ppw) s += X[(size_t)i * d + j];
  }
  red[tid] = tid < Tp ? s : 0.;
  __syncthreads();
  if (tid < d) {
    double a = 0.;
    for (int q = tid; q < Tp; q += d) a += red[q];
    part[blockIdx.x * d + tid] = a;
  }
}

// one wave per tile of 64 points: the augmented rows and the tile's largest norm
__global__ __launch_bounds__(64) void kmf_prep_kernel(const double* __restrict__ X, long long n, int d, int KP, double scale,
                                                      const double* __restrict__ part, float* __restrict__ Pa, long long ldn,
                                                      float* __restrict__ tmax) {
  HSSK_SHARED double mean[KF_DMAX];
  const int lane = threadIdx.x;
  if (lane < d) {
    double a = 0.;
    for (int g = 0; g < KF_G; g++) a += part[g * d + lane];
    mean[lane] = a / (double)n;
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * KF_T + lane;
  const bool live = i < n;
  double s2 = 0.;
  for (int j = 0; j < d; j++) {
    const float f = live ? (float)((X[(size_t)i * d + j] - mean[j]) * scale) : 0.f;
    s2 += (double)f * (double)f;
    Pa[(size_t)j * ldn + i] = -2.f * f;
  }
  const float nf = (float)s2;
  Pa[(size_t)d * ldn + i] = nf;
  Pa[(size_t)(d + 1) * ldn + i] = live ? 1.f : 0.f;
  for (int j = d + 2; j < KP; j++) Pa[(size_t)j * ldn + i] = 0.f;
  const float big = (float)hssk_wave_max((double)nf);
  if (lane == 0) tmax[blockIdx.x] = big;
}

struct KfArgs {
  const float *Pa, *tmax;
  const double* B;
  double* out;
  long long n, ldn, per;
  size_t ldb, ldo, slab;
  int d, nc;
  double lambda;
  long long* dstats;
};

template <int TYPE, int KSM>
__global__ __launch_bounds__(256) void kmf_main_kernel(KfArgs a) {
  HSSK_DYN_SHARED(float, kf_lds);
  float* Gs = kf_lds;                        // 2 x [64 training points][64 rows]
  float* Bs = kf_lds + 2 * KF_T * KF_T;      // 2 x [64 columns][65]: k contiguous
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31, wv = hssk_uniform(tid >> 6);
  const int rblk = wv & 1, hblk = wv >> 1, d = a.d, nc = a.nc;
  const int n = (int)a.n, ldn = (int)a.ldn, i0 = (int)blockIdx.x * KF_T;   // (n < 2^31 - 1024: checked by the host)
  const int rb = (int)((long long)blockIdx.y * a.per), re = (int)min(a.n, (long long)rb + a.per);
  const float* __restrict__ Pa = a.Pa;
  const double* __restrict__ B = a.B;
  double* o = a.out + (size_t)blockIdx.y * a.slab;
  // the rows of this wave as the second operand of the exponent MFMAs: x~ | 1 | |x~|^2
  float bq[KSM];
  if (TYPE != 1) {
#pragma unroll
    for (int s = 0; s < KSM; s++) {
      const int c = 2 * s + half;
      const size_t at = (size_t)i0 + 32 * rblk + l32;
      bq[s] = c < d ? -0.5f * Pa[(size_t)c * ldn + at] : (c == d ? Pa[(size_t)(d + 1) * ldn + at] : (c == d + 1 ? Pa[(size_t)d * ldn + at] : 0.f));
    }
  }
  const double tm = TYPE != 1 ? (double)a.tmax[blockIdx.x] : 0.;
  const double rule = 4. * (d + 4) * 5.9604644775390625e-8;   // 4 (d + 4) 2^-24
  long long nmf = 0, ndf = 0;
  double dacc[16];
#pragma unroll
  for (int r = 0; r < 16; r++) dacc[r] = 0.;
  // entries of a B stage this thread fetches: training point kt of the stage, the columns cq + 4 q
  const int kt = tid & 63, cq = tid >> 6;
  float bv[16];
  // (every load unconditional, from a clamped row and column, and the zeros of the rows past the split's end SELECTED
  // afterwards: loads behind a branch each wait for their own latency, sixteen in a row per stage.  A column past nc holds
  // column nc - 1 again: the MFMA keeps the columns of its A operand apart and the columns past nc are never stored, while
  // sixteen loop-invariant lane masks for them would cost 32 scalar registers)
  auto fetch_b = [&](int k0) {
    const double* p = B + min(k0 + kt, re - 1);
    const bool in = k0 + kt < re;
    double t[16];
#pragma unroll
    for (int q = 0; q < 16; q++) t[q] = p[(size_t)min(cq + 4 * q, nc - 1) * a.ldb];
#pragma unroll
    for (int q = 0; q < 16; q++) bv[q] = in ? (float)t[q] : 0.f;
  };
  // the route of stage k0, and on the matrix-core route its training operand: fetched in FRONT of the product MFMAs of the
  // stage before, which cover the latency (up to 16 coordinates; beyond, the registers are worth more than the overlap)
  constexpr bool PRE = KSM <= 9;
  float xa[PRE ? KSM : 1];
  auto route = [&](int k0) {
    const bool mf = TYPE != 1 && rule * (tm + (double)a.tmax[k0 / KF_T]) <= HSSK_KMATMUL_F32_TAU;
    if (PRE && mf) {
#pragma unroll
      for (int s = 0; s < KSM; s++) xa[PRE ? s : 0] = Pa[(size_t)(2 * s + half) * ldn + (size_t)k0 + 32 * hblk + l32];
    }
    return mf;
  };
  // the 64 x 64 kernel values of stage k0 into Sg[training point][row]
  auto generate = [&](int k0, float* Sg, bool mf) {
    if (mf) {
      nmf++;
      hssk_f16v e;
#pragma unroll
      for (int r = 0; r < 16; r++) e[r] = 0.f;
#pragma unroll
      for (int s = 0; s < KSM; s++)
        e = hssk_mfma_f32_32x32x2(PRE ? xa[PRE ? s : 0] : Pa[(size_t)(2 * s + half) * ldn + (size_t)k0 + 32 * hblk + l32], bq[s], e);
      // entry r of a lane: training point 32 hblk + 8 (r / 4) + 4 half + r % 4 of the stage against row 32 rblk + l32 of the tile
      const int row = 32 * rblk + l32;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int kk = 32 * hblk + 8 * (r / 4) + 4 * half + (r % 4);
        float v = TYPE >= 3 ? hssk_matern_f32<TYPE >= 3 ? TYPE : 3>(e[r]) : exp2f(-fmaxf(e[r], 0.f));
        if (k0 + kk == i0 + row) v = 1.f;
        Sg[kk * KF_T + row] = k0 + kk < re ? v : 0.f;
      }
    } else {
      ndf++;
      // lane = row; the wave's 16 training points are the same for every lane: uniform loads
      float acc[16];
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = 0.f;
      const float* xb = Pa + (size_t)k0 + 16 * wv;
      const float* tb = Pa + (size_t)i0 + lane;
#pragma unroll 1
      for (int j = 0; j < d; j++, xb += ldn, tb += ldn) {
        const float t = -0.5f * *tb;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float df = -0.5f * xb[r] - t;
          acc[r] += TYPE == 1 ? fabsf(df) : df * df;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int kk = 16 * wv + r;
        float v = TYPE >= 3 ? hssk_matern_f32<TYPE >= 3 ? TYPE : 3>(acc[r]) : exp2f(-acc[r]);
        if (k0 + kk == i0 + lane) v = 1.f;
        Sg[kk * KF_T + lane] = k0 + kk < re ? v : 0.f;
      }
    }
  };

  if (rb < re) {
    // the pass in front of the first stage only evaluates and fetches (one copy of the evaluation in the code: its registers)
    int buf = 1;
    for (int k0 = rb - KF_T; k0 < re; k0 += KF_T, buf ^= 1) {
      const bool live = k0 >= rb;
      const float* Sg = Gs + buf * KF_T * KF_T;
      float* Sb = Bs + buf * KF_T * KF_BP;
      if (live) {
#pragma unroll
        for (int q = 0; q < 16; q++) Sb[(cq + 4 * q) * KF_BP + kt] = bv[q];
      }
      __syncthreads();
      const bool more = k0 + KF_T < re;
      bool mf = false;
      if (more) {
        fetch_b(k0 + KF_T);
        mf = route(k0 + KF_T);
      }
      const bool prod = live && 32 * hblk < nc;   // (uniform over the wave: with at most 32 columns the waves 2 and 3 only generate)
      hssk_f16v f;
#pragma unroll
      for (int r = 0; r < 16; r++) f[r] = 0.f;
      if (prod) {
        // the operands of 16 MFMAs into registers first: their LDS reads are in flight together, under the MFMAs in front of them
#pragma unroll
        for (int k1 = 0; k1 < KF_T; k1 += 32) {
          float av[16], gv[16];
#pragma unroll
          for (int q = 0; q < 16; q++) {
            av[q] = Sb[(32 * hblk + l32) * KF_BP + k1 + 2 * q + half];
            gv[q] = Sg[(k1 + 2 * q + half) * KF_T + 32 * rblk + l32];
          }
#pragma unroll
          for (int q = 0; q < 16; q++) f = hssk_mfma_f32_32x32x2(av[q], gv[q], f);
        }
      }
      // the next stage is evaluated BEFORE this stage's accumulator is read: the vector unit works under the MFMAs in flight
      if (more) generate(k0 + KF_T, Gs + (buf ^ 1) * KF_T * KF_T, mf);   // (that buffer was last read before this stage's barrier)
      if (prod) {
#pragma unroll
        for (int r = 0; r < 16; r++) dacc[r] += (double)f[r];
      }
    }
  }
  // dacc[r] = out(row 32 rblk + l32, column 32 hblk + 8 (r / 4) + 4 half + r % 4)
  const int gi = i0 + 32 * rblk + l32;
  const bool diag = gi >= rb && gi < re;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int c = 32 * hblk + 8 * (r / 4) + 4 * half + (r % 4);
    if (gi < n && c < nc) {
      double v = dacc[r];
      if (diag) v += a.lambda * B[(size_t)gi + (size_t)c * a.ldb];
      hssk_gstore(o, (size_t)gi + (size_t)c * a.ldo, v);
    }
  }
  if (a.dstats && tid == 0) {
    if (nmf) hssk_gadd_ll(a.dstats, nmf);
    if (ndf) hssk_gadd_ll(a.dstats + 1, ndf);
  }
}

constexpr size_t KF_SHM = sizeof(float) * 2 * ((size_t)KF_T * KF_T + (size_t)KF_T * KF_BP);

template <int TYPE, int KSM>
void kmf_launch(hssk_ctx* ctx, const KfArgs& a, int splits) {
  const dim3 grid((unsigned)((a.n + KF_T - 1) / KF_T), (unsigned)splits);
  hssk_rt::allow_dynamic_lds(kmf_main_kernel<TYPE, KSM>, KF_SHM);
  HSSK_LAUNCH((kmf_main_kernel<TYPE, KSM>), grid, dim3(256), KF_SHM, ctx->stream, a);
}

// the matrix-core depth of the instance: one per kf_ksm value
template <int TYPE>
void kf_dispatch(int ksm, hssk_ctx* ctx, const KfArgs& a, int splits) {
  switch (ksm) {
    case 2: kmf_launch<TYPE, 2>(ctx, a, splits); break;
    case 5: kmf_launch<TYPE, 5>(ctx, a, splits); break;
    case 9: kmf_launch<TYPE, 9>(ctx, a, splits); break;
    case 17: kmf_launch<TYPE, 17>(ctx, a, splits); break;
    default: kmf_launch<TYPE, 33>(ctx, a, splits); break;
  }
}

void kmf_check_spec(const char* who, const hssk_ctx* ctx, const hssk_kernel_spec* spec) {
  if (!ctx || !spec) throw std::invalid_argument(std::string(who) + ": no context or kernel");
  check_spec(*spec);
  if (!(spec->h > 0.)) throw std::invalid_argument(std::string(who) + ": the kernel width must be positive");
  if (spec->n > (1LL << 31) - 1024) throw std::invalid_argument(std::string(who) + ": point count out of range");
}

}  // namespace

extern "C" int hssk_kernel_matmul_f32_splits(long long n) {
  if (n <= 0) return 1;
  const long long tiles = (n + KF_T - 1) / KF_T;
  return (int)std::max<long long>(1, std::min(std::min<long long>(tiles, 64), (KF_GRID + tiles - 1) / tiles));
}

extern "C" long long hssk_kernel_matmul_f32_prep_bytes(long long n, int d) {
  if (n < 0 || d < 1 || d > KF_DMAX) return -1;
  return (long long)kf_layout(n, d).total;
}

extern "C" int hssk_kernel_matmul_f32_prep(hssk_ctx* ctx, const hssk_kernel_spec* spec, void* prep, long long bytes) {
  HSSK_API_BEGIN
  kmf_check_spec("hssk_kernel_matmul_f32_prep", ctx, spec);
  if (spec->type == 2) HSSK_UNSUPPORTED("Gauss / Laplace / Matern kernels only (no ANOVA product)");
  if (spec->d > KF_DMAX) HSSK_UNSUPPORTED("at most 64 coordinates");
  if (spec->n == 0) return 0;
  const KfLayout L = kf_layout(spec->n, spec->d);
  if (!prep) throw std::invalid_argument("hssk_kernel_matmul_f32_prep: null pointer");
  if (bytes < (long long)L.total) throw std::invalid_argument("hssk_kernel_matmul_f32_prep: the buffer is smaller than hssk_kernel_matmul_f32_prep_bytes");
  char* base = (char*)prep;
  const double l2e = 1.4426950408889634;
  const double scale = spec->type >= 3 ? std::sqrt(spec->type == 3 ? 3. : 5.) / spec->h
                                       : (spec->type == 1 ? l2e / spec->h : std::sqrt(l2e) / (spec->h * std::sqrt(2.)));
  HSSK_LAUNCH(kmf_mean_kernel, dim3(KF_G), dim3(256), 0, ctx->stream, spec->X, spec->d, spec->n, (double*)(base + L.o_pm));
  HSSK_LAUNCH(kmf_prep_kernel, dim3((unsigned)L.nt), dim3(64), 0, ctx->stream, spec->X, spec->n, spec->d, L.kp, scale,
              (const double*)(base + L.o_pm), (float*)(base + L.o_pa), L.ldn, (float*)(base + L.o_tm));
  hssk_rt::check_launch();
  HSSK_API_END
}

extern "C" int hssk_kernel_matmul_f32(hssk_ctx* ctx, const hssk_kernel_spec* spec, const void* prep, const double* B, long long ldb, int nc,
                                      double* out, long long ldo, int splits, long long* stats) {
  HSSK_API_BEGIN
  kmf_check_spec("hssk_kernel_matmul_f32", ctx, spec);
  if (spec->type == 2) HSSK_UNSUPPORTED("Gauss / Laplace / Matern kernels only (no ANOVA product)");
  if (spec->d > KF_DMAX) HSSK_UNSUPPORTED("at most 64 coordinates");
  if (nc < 1 || nc > 64) throw std::invalid_argument("hssk_kernel_matmul_f32: between 1 and 64 columns at a time");
  if (splits < 0) throw std::invalid_argument("hssk_kernel_matmul_f32: negative split count");
  if (stats) for (int i = 0; i < 4; i++) stats[i] = 0;
  if (spec->n == 0) return 0;
  if (!prep || !B || !out) throw std::invalid_argument("hssk_kernel_matmul_f32: null pointer");
  if (ldb < spec->n || ldo < spec->n) throw std::invalid_argument("hssk_kernel_matmul_f32: leading dimension below the point count");
  if (B == out) throw std::invalid_argument("hssk_kernel_matmul_f32: out may not alias B");
  if (KF_SHM > hssk_rt::max_lds_per_workgroup()) {
    hssk_set_error("hssk_kernel_matmul_f32: the stage buffers do not fit the LDS of this device");
    return 2;
  }
  const long long n = spec->n;
  const KfLayout L = kf_layout(n, spec->d);
  const KmSplit sp = km_split_plan(n, KF_T, splits, hssk_kernel_matmul_f32_splits(n));
  const long long s = sp.s, per = sp.per;
  // context slabs: 256 bytes of statistics, then the split partials
  const size_t slab = s > 1 ? (size_t)n * nc : 0;
  char* work = (char*)ctx->kmm_slabs(256 + sizeof(double) * slab * (size_t)s);
  KfArgs a;
  a.Pa = (const float*)((const char*)prep + L.o_pa);
  a.tmax = (const float*)((const char*)prep + L.o_tm);
  a.B = B;
  a.out = s > 1 ? (double*)(work + 256) : out;
  a.n = n; a.ldn = L.ldn; a.per = per;
  a.ldb = (size_t)ldb; a.ldo = s > 1 ? (size_t)n : (size_t)ldo; a.slab = slab;
  a.d = spec->d; a.nc = nc;
  a.lambda = spec->lambda;
  a.dstats = stats ? (long long*)work : nullptr;
  if (stats) {
    hssk_rt::memset_async(work, 0, 16, ctx->stream);
    hssk_watch_read_ms(ctx, 0, nullptr);   // (whatever an earlier caller left recorded there is dropped)
    hssk_watch_start(ctx, 0);
  }
  const int ksm = kf_ksm(spec->d);
  if (spec->type == 1) kmf_launch<1, 1>(ctx, a, (int)s);   // (the difference form only: no matrix-core depth)
  else if (spec->type == 3) kf_dispatch<3>(ksm, ctx, a, (int)s);
  else if (spec->type == 4) kf_dispatch<4>(ksm, ctx, a, (int)s);
  else kf_dispatch<0>(ksm, ctx, a, (int)s);
  hssk_rt::check_launch();
  if (s > 1)
    if (const int rc = km_reduce_splits(ctx, (const double*)(work + 256), n, nc, (int)s, out, ldo)) return rc;
  if (stats) {
    hssk_watch_stop(ctx, 0);
    long long hs[2] = {0, 0};
    hssk_rt::d2h(hs, work, 16, ctx->stream);
    hssk_rt::sync(ctx->stream);
    stats[0] = hs[0]; stats[1] = hs[1]; stats[2] = s;
    stats[3] = (long long)std::llround(hssk_watch_read_ms(ctx, 0, nullptr) * 1e3);
  }
  HSSK_API_END
}
