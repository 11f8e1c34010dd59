// The vector kernels of a block Krylov iteration that runs up to 64 right-hand sides in lockstep (Kernel<double>::model_refine /
// model_solve / predict_variance_exact): the start of a cycle (hssk_krylov_start), one orthogonalisation step by
// classical Gram-Schmidt applied twice (hssk_krylov_orth) and linear combinations of the basis (hssk_krylov_combine).
//
// Layout.  A basis is a sequence of blocks; block j is an n x nc column-major matrix with leading dimension ldv at
// V + j ldv nc, so that every block can be handed to hssk_kernel_matmul or to a device solve as it is.  Column c of the blocks is
// the basis of right-hand side c: the columns never mix, and what a column receives does not depend on its neighbours.
//
// Grid.  Every kernel runs (row chunks of 256) x (columns): one row per thread, a workgroup of four waves per chunk and column --
// 391 x 64 workgroups at n = 1e5, nc = 64, and 391 for a column alone.  A step of the orthogonalisation is four launches and
// three hssk_sum_slabs:
//   1. dots:     P(s, c, j) = sum over the rows of chunk s of V_j(:, c) w(:, c),  j <= k;       h1 = sum_s P(s)
//   2. update 1: w -= sum_j h1(j) V_j  (j ascending), stored; the dots again on the new w;      h2 = sum_s P(s)
//   3. update 2: w -= sum_j h2(j) V_j, stored; Q(s, c) = sum over the chunk of w^2;             ss = sum_s Q(s)
//   4. finish:   V_{k+1} = w / sqrt(ss) (zeros when the norm is 0), Hout(j) = h1(j) + h2(j), Hout(k + 1) = sqrt(ss).
// hssk_krylov_start is "r = b - ax, Q(s, c)", the sum over s, and the same finish; hssk_krylov_combine is one launch.
//
// Order of every sum.  A dot product or a sum of squares over a chunk: one product per thread (one row per thread, nothing to
// add there), the 64 lanes of a wave by hssk_wave_sum, the four waves in wave order by one thread; the chunks in chunk order by
// hssk_sum_slabs (a second pass over partials the context keeps).  The updates and hssk_krylov_combine add their terms in the
// order of the blocks, j = 0, 1, ...  No atomics anywhere: two calls agree bit for bit.
//
// What is written.  Rows n .. ld - 1 and columns >= nc of no operand are touched.  hssk_krylov_orth overwrites the ACTIVE
// columns of W with the orthogonalised, not yet normalised vector; an inactive column (its bit of `active` clear) leaves its W
// alone and receives zeros in block k + 1 and in Hout.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; none of the kernels spills or uses scratch,
// eight waves per SIMD everywhere):
//   kr_dots_kernel      22 VGPRs  42 SGPRs  2048 B LDS      kr_update_kernel<1>  24 VGPRs  50 SGPRs  2048 B LDS
//   kr_update_kernel<2> 22 VGPRs  50 SGPRs  2048 B LDS      kr_resid_kernel      10 VGPRs  23 SGPRs  2048 B LDS
//   kr_finish_kernel    16 VGPRs  26 SGPRs     0 B LDS      kr_combine_kernel    22 VGPRs  50 SGPRs     0 B LDS
#include "hssk_device.h"
#include "hssk_internal.h"

namespace {

constexpr int KR_T = 256;       // threads of a workgroup = rows of a chunk
constexpr int KR_W = KR_T / 64;
constexpr int KR_J = 64;        // dot products a workgroup hands over per barrier

// P[j] = sum over this workgroup's rows of V_j(row) w, j < k1: per wave on the DPP network, the waves in wave order.  Vc: column c
// of block 0; every thread of the workgroup calls (a thread without a row: in == false, w == 0).
__device__ __forceinline__ void kr_block_dots(const double* __restrict__ Vc, size_t vstride, size_t row, bool in, double w, int k1,
                                              double* __restrict__ P, double (*part)[KR_J]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j0 = 0; j0 < k1; j0 += KR_J) {
    const int jt = min(KR_J, k1 - j0);
    for (int j = 0; j < jt; j += 4) {
      double p[4];
#pragma unroll
      for (int u = 0; u < 4; u++) p[u] = (in && j + u < jt) ? hssk_gload(Vc, (size_t)(j0 + j + u) * vstride + row) * w : 0.;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double s = hssk_wave_sum(p[u]);   // (every lane takes part)
        if (lane == 0 && j + u < jt) part[wave][j + u] = s;
      }
    }
    __syncthreads();
    if (tid < jt) {
      double t = 0.;
      for (int q = 0; q < KR_W; q++) t += part[q][tid];
      P[j0 + tid] = t;
    }
    __syncthreads();
  }
}

// Q[0] = sum over this workgroup's rows of v^2, in the same order
__device__ __forceinline__ void kr_block_sumsq(double v, double* __restrict__ Q, double (*part)[KR_J]) {
  const int tid = threadIdx.x;
  const double s = hssk_wave_sum(v * v);
  if ((tid & 63) == 0) part[tid >> 6][0] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.;
    for (int q = 0; q < KR_W; q++) t += part[q][0];
    Q[0] = t;
  }
}

__global__ __launch_bounds__(KR_T) void kr_dots_kernel(const double* __restrict__ V, size_t ldv, size_t vstride, long long n, int nc, int k1,
                                                       const double* __restrict__ W, size_t ldw, unsigned long long active,
                                                       double* __restrict__ P) {
  HSSK_SHARED double part[KR_W][KR_J];
  const int tid = threadIdx.x, c = blockIdx.y;
  double* Pc = P + ((size_t)blockIdx.x * nc + c) * k1;
  if (!((active >> c) & 1ULL)) {   // (uniform over the workgroup)
    for (int j = tid; j < k1; j += KR_T) Pc[j] = 0.;
    return;
  }
  const long long row = (long long)blockIdx.x * KR_T + tid;
  const bool in = row < n;
  const double w = in ? hssk_gload(W, (size_t)c * ldw + row) : 0.;
  kr_block_dots(V + (size_t)c * ldv, vstride, (size_t)row, in, w, k1, Pc, part);
}

// w -= sum_j H(j, c) V_j(:, c) on the rows of the chunk, stored; PASS 1: the dots of the new w into P, PASS 2: its sum of squares
// into Q
template <int PASS>
__global__ __launch_bounds__(KR_T) void kr_update_kernel(const double* __restrict__ V, size_t ldv, size_t vstride, long long n, int nc, int k1,
                                                         double* __restrict__ W, size_t ldw, unsigned long long active,
                                                         const double* __restrict__ H, double* __restrict__ P) {
  HSSK_SHARED double part[KR_W][KR_J];
  const int tid = threadIdx.x, c = blockIdx.y;
  double* Pc = PASS == 1 ? P + ((size_t)blockIdx.x * nc + c) * k1 : P + (size_t)blockIdx.x * nc + c;
  if (!((active >> c) & 1ULL)) {
    if (PASS == 1) for (int j = tid; j < k1; j += KR_T) Pc[j] = 0.;
    else if (tid == 0) Pc[0] = 0.;
    return;
  }
  const long long row = (long long)blockIdx.x * KR_T + tid;
  const bool in = row < n;
  const double* Vc = V + (size_t)c * ldv;
  const double* hc = H + (size_t)c * k1;
  double w = 0.;
  if (in) {
    w = hssk_gload(W, (size_t)c * ldw + row);
#pragma unroll 4
    for (int j = 0; j < k1; j++) w -= hc[j] * hssk_gload(Vc, (size_t)j * vstride + row);
    hssk_gstore(W, (size_t)c * ldw + row, w);
  }
  if (PASS == 1) kr_block_dots(Vc, vstride, (size_t)row, in, w, k1, Pc, part);
  else kr_block_sumsq(w, Pc, part);
}

// R = B - AX on the rows of the chunk, stored; its sum of squares into Q
__global__ __launch_bounds__(KR_T) void kr_resid_kernel(const double* __restrict__ B, size_t ldb, const double* __restrict__ AX, size_t ldax,
                                                        long long n, int nc, double* __restrict__ R, size_t ldr, double* __restrict__ Q) {
  HSSK_SHARED double part[KR_W][KR_J];
  const int c = blockIdx.y;
  const long long row = (long long)blockIdx.x * KR_T + threadIdx.x;
  double r = 0.;
  if (row < n) {
    r = hssk_gload(B, (size_t)c * ldb + row) - hssk_gload(AX, (size_t)c * ldax + row);
    hssk_gstore(R, (size_t)c * ldr + row, r);
  }
  kr_block_sumsq(r, Q + (size_t)blockIdx.x * nc + c, part);
}

// dst(:, c) = src(:, c) / sqrt(ss[c]) (zeros for an inactive column and where the norm is not positive; dst may be src); the
// first chunk's workgroup writes Hout(j, c) = h1(j, c) + h2(j, c), j < k1, and Hout(k1, c) = the norm
__global__ __launch_bounds__(KR_T) void kr_finish_kernel(const double* src, size_t lds, long long n, int k1, unsigned long long active,
                                                         const double* __restrict__ ss, const double* __restrict__ h1,
                                                         const double* __restrict__ h2, double* dst, size_t ldd, double* __restrict__ Hout,
                                                         size_t ldh) {
  const int tid = threadIdx.x, c = blockIdx.y;
  const bool act = (active >> c) & 1ULL;
  const double nrm = act ? sqrt(ss[c]) : 0.;
  const long long row = (long long)blockIdx.x * KR_T + tid;
  if (row < n) {
    double v = 0.;
    if (nrm > 0.) v = hssk_gload(src, (size_t)c * lds + row) / nrm;
    hssk_gstore(dst, (size_t)c * ldd + row, v);
  }
  if (blockIdx.x == 0) {
    for (int j = tid; j < k1; j += KR_T) Hout[(size_t)c * ldh + j] = act ? h1[(size_t)c * k1 + j] + h2[(size_t)c * k1 + j] : 0.;
    if (tid == 0) Hout[(size_t)c * ldh + k1] = nrm;
  }
}

// out(:, c) (+)= sum_{j < kcount} Y(j, c) V_j(:, c), the terms added in the order of j
__global__ __launch_bounds__(KR_T) void kr_combine_kernel(const double* __restrict__ V, size_t ldv, size_t vstride, long long n, int kcount,
                                                          const double* __restrict__ Y, size_t ldy, double* __restrict__ out, size_t ldo,
                                                          int accumulate) {
  const int c = blockIdx.y;
  const long long row = (long long)blockIdx.x * KR_T + threadIdx.x;
  if (row >= n) return;
  const double* Vc = V + (size_t)c * ldv;
  const double* yc = Y + (size_t)c * ldy;
  double acc = 0.;
#pragma unroll 4
  for (int j = 0; j < kcount; j++) acc += yc[j] * hssk_gload(Vc, (size_t)j * vstride + row);
  if (accumulate) acc += hssk_gload(out, (size_t)c * ldo + row);
  hssk_gstore(out, (size_t)c * ldo + row, acc);
}

long long kr_chunks(long long n) { return (n + KR_T - 1) / KR_T; }

void kr_check_shape(const char* who, hssk_ctx* ctx, long long n, int nc) {
  if (!ctx) throw std::invalid_argument(std::string(who) + ": no context");
  if (n < 0 || nc < 0) throw std::invalid_argument(std::string(who) + ": negative size");
  if (nc > 64) throw std::invalid_argument(std::string(who) + ": at most 64 columns at a time");
  if (kr_chunks(n) > 0x7fffffffLL) throw std::invalid_argument(std::string(who) + ": too many row chunks for one grid");
}

}  // namespace

extern "C" int hssk_krylov_start(hssk_ctx* ctx, const double* B, long long ldb, const double* AX, long long ldax, long long n, int nc,
                                 double* V0, long long ldv, double* norms) {
  HSSK_API_BEGIN
  kr_check_shape("hssk_krylov_start", ctx, n, nc);
  if (n == 0 || nc == 0) return 0;
  if (!B || !AX || !V0 || !norms) throw std::invalid_argument("hssk_krylov_start: null pointer");
  if (ldb < n || ldax < n || ldv < n) throw std::invalid_argument("hssk_krylov_start: leading dimension below the row count");
  const long long S = kr_chunks(n);
  double* ws = ctx->kry_work(sizeof(double) * ((size_t)nc + (size_t)S * nc));
  double *ss = ws, *Q = ws + nc;
  const dim3 grid((unsigned)S, (unsigned)nc);
  HSSK_LAUNCH(kr_resid_kernel, grid, dim3(KR_T), 0, ctx->stream, B, (size_t)ldb, AX, (size_t)ldax, n, nc, V0, (size_t)ldv, Q);
  hssk_rt::check_launch();
  if (const int rc = hssk_sum_slabs(ctx, Q, nc, nc, (int)S, ss)) return rc;
  HSSK_LAUNCH(kr_finish_kernel, grid, dim3(KR_T), 0, ctx->stream, (const double*)V0, (size_t)ldv, n, 0, ~0ULL, (const double*)ss,
              (const double*)nullptr, (const double*)nullptr, V0, (size_t)ldv, norms, (size_t)1);
  hssk_rt::check_launch();
  HSSK_API_END
}

extern "C" int hssk_krylov_orth(hssk_ctx* ctx, double* V, long long ldv, long long n, int nc, int k, double* W, long long ldw,
                                unsigned long long active, double* Hout, long long ldh) {
  HSSK_API_BEGIN
  kr_check_shape("hssk_krylov_orth", ctx, n, nc);
  if (k < 0) throw std::invalid_argument("hssk_krylov_orth: negative step");
  if (n == 0 || nc == 0) return 0;
  if (!V || !W || !Hout) throw std::invalid_argument("hssk_krylov_orth: null pointer");
  if (ldv < n || ldw < n) throw std::invalid_argument("hssk_krylov_orth: leading dimension below the row count");
  if (ldh < (long long)k + 2) throw std::invalid_argument("hssk_krylov_orth: Hout needs k + 2 rows");
  const long long S = kr_chunks(n);
  const int k1 = k + 1;
  const size_t nh = (size_t)nc * k1, np = (size_t)S * nh;
  double* ws = ctx->kry_work(sizeof(double) * (2 * nh + (size_t)nc + np + (size_t)S * nc));
  double *h1 = ws, *h2 = h1 + nh, *ss = h2 + nh, *P = ss + nc, *Q = P + np;
  const size_t vstride = (size_t)ldv * nc;
  double* Vn = V + (size_t)k1 * vstride;
  const dim3 grid((unsigned)S, (unsigned)nc);
  HSSK_LAUNCH(kr_dots_kernel, grid, dim3(KR_T), 0, ctx->stream, (const double*)V, (size_t)ldv, vstride, n, nc, k1, (const double*)W, (size_t)ldw, active, P);
  hssk_rt::check_launch();
  if (const int rc = hssk_sum_slabs(ctx, P, (long long)nh, (long long)nh, (int)S, h1)) return rc;
  HSSK_LAUNCH(kr_update_kernel<1>, grid, dim3(KR_T), 0, ctx->stream, (const double*)V, (size_t)ldv, vstride, n, nc, k1, W, (size_t)ldw, active,
              (const double*)h1, P);
  hssk_rt::check_launch();
  if (const int rc = hssk_sum_slabs(ctx, P, (long long)nh, (long long)nh, (int)S, h2)) return rc;
  HSSK_LAUNCH(kr_update_kernel<2>, grid, dim3(KR_T), 0, ctx->stream, (const double*)V, (size_t)ldv, vstride, n, nc, k1, W, (size_t)ldw, active,
              (const double*)h2, Q);
  hssk_rt::check_launch();
  if (const int rc = hssk_sum_slabs(ctx, Q, nc, nc, (int)S, ss)) return rc;
  HSSK_LAUNCH(kr_finish_kernel, grid, dim3(KR_T), 0, ctx->stream, (const double*)W, (size_t)ldw, n, k1, active, (const double*)ss,
              (const double*)h1, (const double*)h2, Vn, (size_t)ldv, Hout, (size_t)ldh);
  hssk_rt::check_launch();
  HSSK_API_END
}

extern "C" int hssk_krylov_combine(hssk_ctx* ctx, const double* V, long long ldv, long long n, int nc, int kcount, const double* Y,
                                   long long ldy, double* out, long long ldo, int accumulate) {
  HSSK_API_BEGIN
  kr_check_shape("hssk_krylov_combine", ctx, n, nc);
  if (kcount < 0) throw std::invalid_argument("hssk_krylov_combine: negative block count");
  if (n == 0 || nc == 0) return 0;
  if (!out || (kcount > 0 && (!V || !Y))) throw std::invalid_argument("hssk_krylov_combine: null pointer");
  if (ldo < n || (kcount > 0 && ldv < n)) throw std::invalid_argument("hssk_krylov_combine: leading dimension below the row count");
  if (ldy < kcount) throw std::invalid_argument("hssk_krylov_combine: Y needs kcount rows");
  if (kcount > 0 && (const double*)out == V) throw std::invalid_argument("hssk_krylov_combine: out may not alias the basis");
  if (kcount == 0 && accumulate) return 0;   // (nothing to add: out is not touched)
  HSSK_LAUNCH(kr_combine_kernel, dim3((unsigned)kr_chunks(n), (unsigned)nc), dim3(KR_T), 0, ctx->stream, V, (size_t)ldv,
              (size_t)ldv * nc, n, kcount, Y, (size_t)ldy, out, (size_t)ldo, accumulate);
  hssk_rt::check_launch();
  HSSK_API_END
}
