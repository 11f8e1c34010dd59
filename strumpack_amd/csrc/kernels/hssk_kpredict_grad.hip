// The gradient of the prediction sum in the test point (hssk_kernel_predict_grad):
//   G(j, c) = sum_r w_rc dk(x_r, t_c) / dt_cj,     w_rc = w[r] (one weight vector) or W(r, c) (a weight column per test point).
// With delta_j = x_rj - t_cj the derivative of a pair is f delta_j (Laplace: f sign(delta_j), sign(0) = 0), f the pair factor
//   Gauss     k / h^2                          Laplace    k / h
//   Matern32  (3 / h^2) e^-s                   Matern52   (5 / (3 h^2)) (1 + s) e^-s
// No form divides by the distance: a pair of equal points adds exactly 0 to every coordinate, a Laplace pair that agrees in
// coordinate j exactly 0 to that coordinate.  The distance loop, the exponentials and s are those of hssk_kpair.h and
// hssk_matern.h (the coordinates in order, the same functions), and every term is formed from the difference x_rj - t_cj itself.
//
// Grid: (tiles of 64 test points) x (splits of the training points; km_split_plan in stages of KG_T).  A workgroup is four waves
// over the tile's 64 test points, lane = test point.  The training points of its split pass through the LDS KG_T at a time, and
// each tile takes two phases:
//   A  wave q evaluates phi = w f for the tile's training points r = q (mod 4), four pairs at a time, and stores phi[r][lane];
//   B  after a barrier, wave q adds phi[r][lane] delta_j over the tile's training points in training order for the coordinates
//      j = q (mod 4): NJ = ceil(d / 4) <= 16 accumulators per lane, indexed by compile-time constants (NJ is a template
//      parameter; a register array indexed by a run-time coordinate would go to scratch memory).
// So the distance work is split by training points and the gradient work by coordinates.  The next training tile is fetched into
// registers between the phases and stored into the other of two LDS buffers after phase B: two barriers per tile.
//
// Padding: test points past m and training points past the split's end are zero in the LDS; W(r, c) is read for live lanes and
// training points of the split only; phase B stops at the split's last training point; rows d .. ldg - 1 and columns >= m of G are
// never written.  Every LDS index is below the tile constants: rows < KG_T, coordinates < d <= dp, lanes < 64.
//
// Order of every sum: the coordinates of a distance in order, the training points of an entry in order, the split partials in
// split order (hssk_sum_slabs over slabs the context keeps; with one split G is written directly).  No atomics: two calls agree
// bit for bit, and with the same forced split count a column of G does not depend on m, on the other test points or on its
// position.
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_kmatmul_split.h"
#include "hssk_matern.h"

namespace {

constexpr int KG_T = 64;       // tile edge: test points per workgroup, training points per stage
constexpr int KG_W = 4;        // waves per workgroup
constexpr int KG_DMAX = 64;
// The automatic split count (profiles/gp_predict_gradient.md): enough splits for KG_GRID workgroups -- sixteen per compute unit of
// an MI355X, a constant, not a device query: three workgroups of d = 8 share a compute unit, and the rounds of a grid a few
// times that size end evenly -- but no split shorter than KG_MIN_STAGES stages, below which the launch and the reduction of the
// partials cost more than the split saves
constexpr long long KG_GRID = 4096;
constexpr long long KG_MIN_STAGES = 6;

// doubles of dynamic LDS: test tile [64][dp] | two training tiles [64][dp] | phi [64][64] | two weight tiles [64]
inline int kg_stride(int d) { return d | 1; }   // (odd: the lanes' own points lie on different banks)
inline size_t kg_lds_doubles(int dp) { return 3 * (size_t)KG_T * dp + (size_t)KG_T * KG_T + 2 * KG_T; }

// the pair factor from the distance a (Gauss, Matern: squared Euclidean; Laplace: the 1-norm).  Gauss and Laplace: the exponential
// of kernel_predict_kernel (hssk_kpair.h) as it is written there; the Matern kernels: the finish of hssk_matern.h
template <int TYPE>
__device__ inline double kg_factor(double a, double h) {
  if (TYPE == 0) return exp(a * (-1. / (2. * h * h))) * (1. / (h * h));
  if (TYPE == 1) return exp(a * (-1. / h)) * (1. / h);
  return hssk_matern_dt_factor<TYPE >= 3 ? TYPE : 3>(a, hssk_matern_c(TYPE, h));
}

template <int TYPE, int NJ>
__global__ __launch_bounds__(KG_T * KG_W) void kpredict_grad_kernel(hssk_kernel_spec ks, const double* __restrict__ W, size_t ldw,
                                                                  const double* __restrict__ T, int m, double* __restrict__ out,
                                                                  size_t ldo, size_t slab, long long per) {
  HSSK_DYN_SHARED(double, kg_lds);
  const int tid = threadIdx.x, lane = tid & 63, q = hssk_uniform(tid >> 6);
  const int d = ks.d, dp = d | 1, c0 = blockIdx.x * KG_T, c = c0 + lane;
  const long long rb = (long long)blockIdx.y * per, re = min(ks.n, rb + per);
  const bool live = c < m, cols = ldw != 0;
  double* xt = kg_lds;
  double* xr = xt + KG_T * dp;
  double* phi = xr + 2 * KG_T * dp;
  double* wr = phi + KG_T * KG_T;
  const int ne = KG_T * d;   // doubles of a training tile: contiguous in X from its first point on
  for (int e = tid; e < ne; e += KG_T * KG_W) {
    const int pt = e / d, j = e % d;
    xt[pt * dp + j] = c0 + pt < m ? hssk_gload(T, (size_t)(c0 + pt) * d + j) : 0.;
  }
  // a tile through registers: thread t holds the elements t + 256 k (zero past the split's end)
  double xv[NJ], wv = 0.;
  auto fetch = [&](long long r0) {
#pragma unroll
    for (int k = 0; k < NJ; k++) {
      const int e = tid + KG_T * KG_W * k;
      xv[k] = (e < ne && r0 + e / d < re) ? hssk_gload(ks.X, (size_t)r0 * d + e) : 0.;
    }
    if (!cols && tid < KG_T) wv = r0 + tid < re ? hssk_gload(W, (size_t)(r0 + tid)) : 0.;
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int k = 0; k < NJ; k++) {
      const int e = tid + KG_T * KG_W * k;
      if (e < ne) xr[buf * KG_T * dp + (e / d) * dp + e % d] = xv[k];
    }
    if (!cols && tid < KG_T) wr[buf * KG_T + tid] = wv;
  };
  fetch(rb);
  put(0);
  __syncthreads();
  // the wave's coordinates of the lane's test point, and their sums
  double tq[NJ], acc[NJ];
#pragma unroll
  for (int i = 0; i < NJ; i++) {
    const int j = q + KG_W * i;
    tq[i] = j < d ? xt[lane * dp + j] : 0.;
    acc[i] = 0.;
  }
  int buf = 0;
  for (long long r0 = rb; r0 < re; r0 += KG_T, buf ^= 1) {
    const double* xb = xr + buf * KG_T * dp;
    const double* wb = wr + buf * KG_T;
    const int rend = (int)min((long long)KG_T, re - r0);
    // A: phi of the training points q, q + 4, ..., four pairs at a time (rows past the split's end are zero points: their phi is
    // computed and never read)
    // (kept rolled, like the loop of phase B: unrolled, the uniform row addresses of the groups outgrow the scalar registers)
#pragma unroll 1
    for (int g = 0; g < KG_T / (4 * KG_W); g++) {
      double a[4], w[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int r = q + KG_W * (4 * g + u);
        a[u] = 0.;
        w[u] = cols ? ((live && r < rend) ? hssk_gload(W, (size_t)c * ldw + (size_t)(r0 + r)) : 0.) : wb[r];
      }
      for (int i = 0; i < d; i++) {
        const double t = xt[lane * dp + i];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const double df = xb[(q + KG_W * (4 * g + u)) * dp + i] - t;
          a[u] += TYPE == 1 ? fabs(df) : df * df;
        }
      }
#pragma unroll 1
      for (int u = 0; u < 4; u++) phi[(q + KG_W * (4 * g + u)) * KG_T + lane] = w[u] * kg_factor<TYPE>(a[u], ks.h);
    }
    const bool more = r0 + KG_T < re;   // (the same in every thread)
    if (more) fetch(r0 + KG_T);
    __syncthreads();
    // B: the wave's coordinates over the tile's training points in order
#pragma unroll 1
    for (int r = 0; r < rend; r++) {
      const double p = phi[r * KG_T + lane];
#pragma unroll
      for (int i = 0; i < NJ; i++) {
        const int j = q + KG_W * i;
        if (j < d) {
          const double dl = xb[r * dp + j] - tq[i];
          if (TYPE == 1) acc[i] += dl > 0. ? p : (dl < 0. ? -p : 0.);
          else acc[i] += p * dl;
        }
      }
    }
    if (more) put(buf ^ 1);
    __syncthreads();
  }
  if (live) {
    double* o = out + (size_t)blockIdx.y * slab + (size_t)c * ldo;
#pragma unroll
    for (int i = 0; i < NJ; i++) {
      const int j = q + KG_W * i;
      if (j < d) hssk_gstore(o, (size_t)j, acc[i]);
    }
  }
}

// no training points: the empty sum
__global__ __launch_bounds__(256) void kpredict_grad_zero_kernel(int d, int m, double* __restrict__ out, size_t ldo) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < (long long)d * m) out[(size_t)(e / d) * ldo + e % d] = 0.;
}

template <int TYPE, int NJ>
void kg_launch(hssk_ctx* ctx, const hssk_kernel_spec& ks, const double* W, size_t ldw, const double* T, int m, double* out, size_t ldo,
               size_t slab, long long per, int splits) {
  const size_t shm = sizeof(double) * kg_lds_doubles(kg_stride(ks.d));
  const dim3 grid((unsigned)((m + KG_T - 1) / KG_T), (unsigned)splits);
  hssk_rt::allow_dynamic_lds(kpredict_grad_kernel<TYPE, NJ>, shm);
  HSSK_LAUNCH((kpredict_grad_kernel<TYPE, NJ>), grid, dim3(KG_T * KG_W), shm, ctx->stream, ks, W, ldw, T, m, out, ldo, slab, per);
}
// coordinates per wave: the smallest of 1, 2, 4, 8, 16 that holds ceil(d / 4)
template <int TYPE, class... A>
void kg_dispatch_nj(int d, A... a) {
  if (d <= 4) kg_launch<TYPE, 1>(a...);
  else if (d <= 8) kg_launch<TYPE, 2>(a...);
  else if (d <= 16) kg_launch<TYPE, 4>(a...);
  else if (d <= 32) kg_launch<TYPE, 8>(a...);
  else kg_launch<TYPE, 16>(a...);
}
template <class... A>
void kg_dispatch(int type, int d, A... a) {
  switch (type) {
    case 0: kg_dispatch_nj<0>(d, a...); break;
    case 1: kg_dispatch_nj<1>(d, a...); break;
    case 3: kg_dispatch_nj<3>(d, a...); break;
    default: kg_dispatch_nj<4>(d, a...); break;
  }
}

}  // namespace

extern "C" int hssk_kernel_predict_grad_splits(long long n, int m) {
  if (n <= 0 || m <= 0) return 1;
  const long long tiles = ((long long)m + KG_T - 1) / KG_T, stages = (n + KG_T - 1) / KG_T;
  return (int)std::max<long long>(1, std::min(stages / KG_MIN_STAGES, (KG_GRID + tiles - 1) / tiles));
}

extern "C" int hssk_kernel_predict_grad(hssk_ctx* ctx, const hssk_kernel_spec* spec, const double* W, long long ldw, const double* T, int m,
                                        double* G, long long ldg, int splits) {
  HSSK_API_BEGIN
  if (!ctx || !spec) throw std::invalid_argument("hssk_kernel_predict_grad: no context or kernel");
  if (spec->type < 0 || spec->type > 4)
    throw std::invalid_argument("hssk_kernel_predict_grad: type must be 0 (Gauss), 1 (Laplace), 3 (Matern32) or 4 (Matern52)");
  if (spec->d < 1 || spec->n < 0) throw std::invalid_argument("hssk_kernel_predict_grad: bad point set");
  if (m < 0) throw std::invalid_argument("hssk_kernel_predict_grad: negative test point count");
  if (splits < 0) throw std::invalid_argument("hssk_kernel_predict_grad: negative split count");
  if (ldw < 0 || (ldw > 0 && ldw < spec->n))
    throw std::invalid_argument("hssk_kernel_predict_grad: ldw is 0 (one weight vector) or at least the training point count");
  if (ldg < spec->d) throw std::invalid_argument("hssk_kernel_predict_grad: leading dimension of the gradient below the point dimension");
  if (spec->type == 2) HSSK_UNSUPPORTED("Gauss / Laplace / Matern kernels only (no ANOVA derivative)");
  if (spec->d > KG_DMAX) HSSK_UNSUPPORTED("at most 64 coordinates");
  if (m == 0) return 0;
  if (!T || !G || (spec->n > 0 && (!spec->X || !W))) throw std::invalid_argument("hssk_kernel_predict_grad: null pointer");
  const long long n = spec->n;
  const int d = spec->d;
  if (n == 0) {
    const long long nb = ((long long)d * m + 255) / 256;
    HSSK_LAUNCH(kpredict_grad_zero_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d, m, G, (size_t)ldg);
    hssk_rt::check_launch();
    return 0;
  }
  if (sizeof(double) * kg_lds_doubles(kg_stride(d)) > hssk_rt::max_lds_per_workgroup()) {
    hssk_set_error("hssk_kernel_predict_grad: the point tiles do not fit the LDS of this device");
    return 2;
  }
  const KmSplit sp = km_split_plan(n, KG_T, splits, hssk_kernel_predict_grad_splits(n, m));
  const long long s = sp.s, per = sp.per;
  double* dst = G;
  size_t ldd = (size_t)ldg, slab = 0;
  if (s > 1) {   // partials: d x m, leading dimension d
    slab = (size_t)d * m;
    dst = ctx->kmm_slabs(sizeof(double) * slab * (size_t)s);
    ldd = (size_t)d;
  }
  kg_dispatch(spec->type, d, ctx, *spec, W, (size_t)ldw, T, m, dst, ldd, slab, per, (int)s);
  hssk_rt::check_launch();
  if (s > 1)
    if (const int rc = km_reduce_splits(ctx, dst, d, m, (int)s, G, ldg)) return rc;
  HSSK_API_END
}
