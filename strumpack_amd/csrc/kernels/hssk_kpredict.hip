// Single-precision prediction of kernel ridge regression: pred[c] = sum_r w[r] k(x_r, t_c) from float points and float weights
// in HBM (hssk_kernel_predict_f32).  FP32 per pair, FP64 across pairs, bitwise repeatable.
//
// Grid: test tiles of 64 points x splits of the training set.  A workgroup is four waves that share the 64 test points; wave w
// takes the training tiles 4 c + w (64 points each) of the chunks c of its split.  Every (training tile, test tile) pair goes one
// of two routes, the same for the whole wave:
//   * matrix cores (Gauss, Matern): the base-2 exponent |x~|^2 + |t~|^2 - 2 x~.t~ of 32 x 32 pairs is the accumulator of
//     v_mfma_f32_32x32x2_f32 over K = d + 2 coordinates (x~ = s (x - mean), s^2 = log2(e) / (2 h^2); the two norms are extra
//     coordinates; training points along M, test points along N = the lane).  Taken iff the worst relative error the norm
//     expansion can cause in a term, 4 (d + 4) 2^-24 (max |x~|^2 + max |t~|^2), is at most HSSK_KPREDICT_TAU;
//   * difference form (Laplace, ANOVA, and the Gauss tiles the rule refuses): FP32 differences of the caller's floats on the
//     VALU, a lane per test point, the training coordinates through uniform loads.
// Either way a lane multiplies 16 kernel values by their weights, adds them in FP32 and adds that one number to an FP64 running
// sum: no FP32 sum is longer than 16 terms.  The four waves' sums are added in wave order, the splits' sums by a second launch
// in split order, rounded once to float.  The split count depends on (n, m) alone, so the order of every sum is fixed.
//
// The Matern kernels (types 3 and 4) take both routes with the points scaled by sqrt(2 nu) / h instead: the
// accumulator of the matrix cores -- or, in the difference form, the FP32 distance times 2 nu / h^2 -- is u = s^2, and the value is
// hssk_matern_f32(u) = polynomial(s) exp2(-s log2 e), s = sqrt(max(u, 0)).  The route rule and its threshold are the Gauss ones,
// read on these scaled points: |dk/du| <= 1/2, so an error in u costs a term no more than it costs a Gauss term.
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_matern.h"

#include <cmath>
#include <cstdlib>

namespace {

constexpr int KP_T = 64;    // tile edge: training points per wave step, test points per workgroup
constexpr int KP_W = 4;     // waves per workgroup
constexpr int KP_G = 64;    // workgroups of the mean reduction
constexpr int KP_DMAX = 64;
constexpr int KP_WGS = 2048;   // workgroups the grid aims at (eight per compute unit of an MI355X; a constant, not a device query)

struct KpArgs {
  const float *X, *T, *Xa, *Ta, *wpad, *xmax, *tmax;
  long long n;
  int m, d, type, p, ldn, ldm, chunks, splits, force_diff;
  float s2;   // Gauss / ANOVA: log2(e) / (2 h^2); Laplace: log2(e) / h; Matern: 2 nu / h^2
  double* partial;
  long long* dstats;
};

// partial sums of the training coordinates in FP64: workgroup g adds the points g, g + G, ... (thread t always meets coordinate t % d)
__global__ __launch_bounds__(256) void kp_mean_kernel(const float* __restrict__ X, int d, long long n, double* __restrict__ part) {
  HSSK_SHARED double red[256];
  const int tid = threadIdx.x, Tp = (256 / d) * d, ppw = Tp / d;
  double s = 0.;
  if (tid < Tp) {
    const int j = tid % d, pl = tid / d;
    for (long long i = (long long)blockIdx.x * ppw + pl; i < n; i += (long long)KP_G * ppw) s += (double)X[(size_t)i * d + j];
  }
  red[tid] = tid < Tp ? s : 0.;
  __syncthreads();
  if (tid < d) {
    double a = 0.;
    for (int q = tid; q < Tp; q += d) a += red[q];
    part[blockIdx.x * d + tid] = a;
  }
}

// The augmented operands, one wave per tile of 64 points (tiles 0 .. tx-1: training, the rest: test).  Row k of Xa / Ta is
// coordinate k of every point: training  -2 x~ | |x~|^2 | 1 | 0 ..,  test  t~ | 1 | |t~|^2 | 0 ..  (norms of the ROUNDED x~, in
// FP64, rounded once); padding points are all zero and carry weight zero.  tilemax: the largest norm of the tile.
__global__ __launch_bounds__(64) void kp_prep_kernel(const float* __restrict__ X, long long n, const float* __restrict__ T, int m, int d, int KP,
                                                     double scale, const double* __restrict__ part, const float* __restrict__ w,
                                                     float* __restrict__ Xa, int ldn, float* __restrict__ Ta, int ldm,
                                                     float* __restrict__ wpad, float* __restrict__ xmax, float* __restrict__ tmax, int tx) {
  HSSK_SHARED double mean[KP_DMAX];
  const int lane = threadIdx.x;
  if (lane < d) {
    double a = 0.;
    for (int g = 0; g < KP_G; g++) a += part[g * d + lane];
    mean[lane] = a / (double)n;
  }
  __syncthreads();
  const bool train = (int)blockIdx.x < tx;
  const int tile = train ? blockIdx.x : blockIdx.x - tx;
  const long long i = (long long)tile * KP_T + lane, cnt = train ? n : (long long)m;
  const float* P = train ? X : T;
  float* O = train ? Xa : Ta;
  const size_t ld = train ? ldn : ldm;
  const bool live = i < cnt;
  double s2 = 0.;
  for (int j = 0; j < d; j++) {
    const float f = live ? (float)(((double)P[(size_t)i * d + j] - mean[j]) * scale) : 0.f;
    s2 += (double)f * (double)f;
    O[(size_t)j * ld + i] = train ? -2.f * f : f;
  }
  const float nf = (float)s2, one = live ? 1.f : 0.f;
  O[(size_t)d * ld + i] = train ? nf : one;
  O[(size_t)(d + 1) * ld + i] = train ? one : nf;
  for (int j = d + 2; j < KP; j++) O[(size_t)j * ld + i] = 0.f;
  if (train) wpad[i] = live ? w[i] : 0.f;
  const float big = (float)hssk_wave_max((double)nf);
  if (lane == 0) (train ? xmax : tmax)[tile] = big;
}

// e_E = (1 / E) sum_q (-1)^(q + 1) e_(E - q) s_q for E = 1 .. p (every index a constant: the arrays stay in registers)
template <int E>
__device__ inline void kp_newton(const float (&S)[8], float (&K)[9], int p, float& v) {
  kp_newton<E - 1>(S, K, p, v);
  if (E <= p) {
    float s = 0.f;
#pragma unroll
    for (int q = 1; q <= E; q++) s += ((q & 1) ? 1.f : -1.f) * K[E - q] * S[q - 1];
    K[E] = s / (float)E;
    v = K[E];
  }
}
template <>
__device__ inline void kp_newton<0>(const float (&)[8], float (&K)[9], int, float&) { K[0] = 1.f; }

// 16 training points (rows of xb, d floats each) against the lane's test point: sum_i w[i] k(x_i, t) in FP32.  FULL: all 16 exist;
// otherwise the rows beyond `top` read row `top` (their weights are zero)
template <int TYPE, bool FULL>
__device__ inline float kp_diff16(const KpArgs& a, const float* tl, const float* xb, const float* wb, int top, int lane) {
  const int d = a.d;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  for (int j = 0; j < d; j++) {
    const float t = tl[j * KP_T + lane];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float df = xb[(FULL ? i : min(i, top)) * d + j] - t;
      acc[i] += TYPE == 1 ? fabsf(df) : df * df;
    }
  }
  float s16 = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) s16 += wb[i] * (TYPE >= 3 ? hssk_matern_f32<TYPE >= 3 ? TYPE : 3>(acc[i] * a.s2) : exp2f(-(acc[i] * a.s2)));
  return s16;
}

// ---- difference form of one tile: 64 training points from r0 on against the wave's 64 test points (lane = test point, its
// coordinates in tl[j * 64 + lane]); returns the lane's sum over the tile, every 16 terms added in FP32 and then to the FP64 sum
template <int TYPE>
__device__ inline double kp_diff_tile(const KpArgs& a, const float* tl, long long r0, int lane) {
  const int d = a.d;
  const long long last = a.n - 1;
  double dd = 0.;
  if (TYPE == 2) {
    float s16 = 0.f;
    for (int i = 0; i < KP_T; i++) {
      const long long rr = r0 + i;
      if (rr > last) break;
      const float* xp = a.X + (size_t)rr * d;
      float Kss[8];
#pragma unroll
      for (int q = 0; q < 8; q++) Kss[q] = 0.f;
      for (int j = 0; j < d; j++) {
        const float df = xp[j] - tl[j * KP_T + lane];
        const float tmp = exp2f(-(df * df * a.s2));
        float pw = tmp;
#pragma unroll
        for (int q = 0; q < 8; q++)
          if (q < a.p) { Kss[q] += pw; pw *= tmp; }
      }
      // Newton's identities, degree by degree; the value of degree p is kept
      float Kpp[9] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v = 0.f;
      kp_newton<8>(Kss, Kpp, a.p, v);
      s16 += a.wpad[rr] * v;
      if ((i & 15) == 15) { dd += (double)s16; s16 = 0.f; }
    }
    return dd + (double)s16;
  }
  for (int i0 = 0; i0 < KP_T; i0 += 16) {
    const long long rb = r0 + i0;
    if (rb > last) break;
    const float* xb = a.X + (size_t)rb * d;
    dd += rb + 15 <= last ? (double)kp_diff16<TYPE, true>(a, tl, xb, a.wpad + rb, 15, lane)
                          : (double)kp_diff16<TYPE, false>(a, tl, xb, a.wpad + rb, (int)(last - rb), lane);
  }
  return dd;
}

// KSM k-steps of two coordinates: 2 KSM >= d + 2 rows of Xa / Ta.  MT: 0 for the three kernels of the reference (the type is
// read from the arguments), 3 / 4 for the Matern kernels, which get instantiations of their own
template <int KSM, int MT>
__global__ __launch_bounds__(256) void kp_main_kernel(KpArgs a) {
  HSSK_DYN_SHARED(float, kp_lds);
  double* red = (double*)kp_lds;              // [KP_W * 64]: the waves' sums
  float* tl = kp_lds + 2 * KP_W * KP_T;       // [d * 64]: the test tile as the caller gave it (difference form)
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31, wv = hssk_uniform(tid >> 6);
  const int tt = blockIdx.x, sp = blockIdx.y, d = a.d, c0 = tt * KP_T;
  for (int e = tid; e < KP_T * d; e += 256) {
    const int pt = e / d, j = e % d;
    tl[j * KP_T + pt] = a.T[(size_t)min(c0 + pt, a.m - 1) * d + j];
  }
  __syncthreads();
  float bq[2][KSM];
#pragma unroll
  for (int g = 0; g < 2; g++)
#pragma unroll
    for (int s = 0; s < KSM; s++) bq[g][s] = (MT || a.type == 0) ? a.Ta[(size_t)(2 * s + half) * a.ldm + c0 + 32 * g + l32] : 0.f;
  const double tm = (MT || a.type == 0) ? (double)a.tmax[tt] : 0.;
  const double rule = 4. * (d + 4) * 5.9604644775390625e-8;   // 4 (d + 4) 2^-24
  const long long ch0 = (long long)sp * a.chunks / a.splits, ch1 = (long long)(sp + 1) * a.chunks / a.splits;
  double dm0 = 0., dm1 = 0., dd = 0.;
  long long nmf = 0, ndf = 0;
  for (long long ch = ch0; ch < ch1; ch++) {
    const long long r0 = (ch * KP_W + wv) * KP_T;
    if (r0 >= a.n) continue;   // (a tile of padding only)
    const bool mf = (MT || a.type == 0) && !a.force_diff && rule * ((double)a.xmax[r0 / KP_T] + tm) <= HSSK_KPREDICT_TAU;
    if (mf) {
      nmf++;
#pragma unroll
      for (int blk = 0; blk < 2; blk++) {
        const size_t rb = (size_t)r0 + 32 * blk;
        hssk_f16v acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < KSM; s++) {
          const float x = a.Xa[(size_t)(2 * s + half) * a.ldn + rb + l32];
          acc0 = hssk_mfma_f32_32x32x2(x, bq[0][s], acc0);
          acc1 = hssk_mfma_f32_32x32x2(x, bq[1][s], acc1);
        }
        // entry r of a lane is training row 8 (r / 4) + 4 half + r % 4 of the block
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const hssk_f4 wq = *(const hssk_f4*)(a.wpad + rb + 8 * q + 4 * half);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            s0 += wq[i] * (MT ? hssk_matern_f32<MT ? MT : 3>(acc0[4 * q + i]) : exp2f(-fmaxf(acc0[4 * q + i], 0.f)));
            s1 += wq[i] * (MT ? hssk_matern_f32<MT ? MT : 3>(acc1[4 * q + i]) : exp2f(-fmaxf(acc1[4 * q + i], 0.f)));
          }
        }
        dm0 += (double)s0;
        dm1 += (double)s1;
      }
    } else {
      ndf++;
      if (MT) dd += kp_diff_tile<MT>(a, tl, r0, lane);
      else dd += a.type == 0 ? kp_diff_tile<0>(a, tl, r0, lane) : (a.type == 1 ? kp_diff_tile<1>(a, tl, r0, lane) : kp_diff_tile<2>(a, tl, r0, lane));
    }
  }
  // the two lane halves of a matrix-core column, then the routes: lane l = test point l = column l32 of group half
  const double m0 = dm0 + hssk_shfl_xor(dm0, 32), m1 = dm1 + hssk_shfl_xor(dm1, 32);
  red[wv * KP_T + lane] = (half ? m1 : m0) + dd;
  __syncthreads();
  if (wv == 0) a.partial[(size_t)sp * a.ldm + c0 + lane] = ((red[lane] + red[KP_T + lane]) + red[2 * KP_T + lane]) + red[3 * KP_T + lane];
  if (lane == 0) {
    if (nmf) hssk_gadd_ll(a.dstats, nmf);
    if (ndf) hssk_gadd_ll(a.dstats + 1, ndf);
  }
}

// ---- beyond KP_DMAX coordinates (hssk_kernel_predict_f32_wide) ----------------------------------------------------------------
// The difference form only, with the grid, the sums and their order of kp_main_kernel.  A test tile of R^784 is 200 KB, so
// the coordinates pass through the LDS KPW_DC at a time: the 64 test points' (shared by the four waves) and, per wave, those of
// the RS training points it meets in a sweep over the coordinates, read back as broadcasts.  (Through uniform loads, as in
// kp_diff16, RS row addresses and their values outgrow the scalar registers once the coordinate loop is the outer one.)  What the
// pairs of a lane have accumulated stays in registers across the passes: the distance (Gauss, Laplace: RS = 32) or the p power
// sums (ANOVA: RS = 16).  Per pair the coordinates are added in order in FP32, exactly the sum of the difference form above: the
// bound of DESIGN.md 8b holds as it is written in d, no term is added.  Training rows past the last one read the last one and
// carry the weight zero (wpad), so every wave of a workgroup meets every barrier.
constexpr int KPW_DC = 64;            // coordinates per pass
constexpr int KPW_LD = KP_T + 1;      // row stride of the staged test pass (the transposing stores spread over the banks)

__global__ __launch_bounds__(256) void kp_wpad_kernel(const float* __restrict__ w, long long n, int ldn, float* __restrict__ wpad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < ldn) wpad[i] = i < n ? w[i] : 0.f;
}

template <int TYPE, int RS>
__global__ __launch_bounds__(256) void kp_wide_kernel(KpArgs a) {
  constexpr int NS = TYPE == 2 ? 8 : 1;   // sums a pair carries
  HSSK_SHARED double red[KP_W * KP_T];
  HSSK_SHARED float tl[KPW_DC * KPW_LD];       // [coordinate of the pass][test point]
  HSSK_SHARED float xs[KP_W * RS * KPW_DC];    // per wave: [training point of the sweep][coordinate of the pass]
  const int tid = threadIdx.x, lane = tid & 63, wv = hssk_uniform(tid >> 6);
  const int tt = blockIdx.x, sp = blockIdx.y, d = a.d, c0 = tt * KP_T;
  float* xw = xs + wv * RS * KPW_DC;
  const long long last = a.n - 1;
  const long long ch0 = (long long)sp * a.chunks / a.splits, ch1 = (long long)(sp + 1) * a.chunks / a.splits;
  double dd = 0.;
  long long ndf = 0;
  for (long long ch = ch0; ch < ch1; ch++) {
    const long long r0 = (ch * KP_W + wv) * KP_T;
    if (r0 <= last) ndf++;
    for (int i0 = 0; i0 < KP_T; i0 += RS) {
      const long long rb = r0 + i0;
      const bool act = rb <= last;                        // (uniform over the wave; a sweep of padding only stages and waits)
      const int top = act ? (int)min((long long)(RS - 1), last - rb) : 0;
      const float* xb = a.X + (size_t)(act ? rb : 0) * d;
      float acc[RS][NS];
#pragma unroll
      for (int i = 0; i < RS; i++)
#pragma unroll
        for (int q = 0; q < NS; q++) acc[i][q] = 0.f;
      for (int d0 = 0; d0 < d; d0 += KPW_DC) {
        const int dc = min(KPW_DC, d - d0);
        __syncthreads();
        for (int e = tid; e < KP_T * dc; e += 256) {
          const int pt = e / dc, j = e % dc;
          tl[j * KPW_LD + pt] = a.T[(size_t)min(c0 + pt, a.m - 1) * d + d0 + j];
        }
        for (int e = lane; e < RS * dc; e += 64) {
          const int i = e / dc, j = e % dc;
          xw[i * KPW_DC + j] = xb[(size_t)min(i, top) * d + d0 + j];
        }
        __syncthreads();
        if (act)
          for (int j = 0; j < dc; j++) {
            const float t = tl[j * KPW_LD + lane];
#pragma unroll
            for (int i = 0; i < RS; i++) {
              const float df = xw[i * KPW_DC + j] - t;
              if (TYPE == 2) {
                const float tmp = exp2f(-(df * df * a.s2));
                float pw = tmp;
#pragma unroll
                for (int q = 0; q < NS; q++)
                  if (q < a.p) { acc[i][q] += pw; pw *= tmp; }
              } else {
                acc[i][0] += TYPE == 1 ? fabsf(df) : df * df;
              }
            }
          }
      }
      if (act) {
        // every 16 terms added in FP32 and then to the FP64 sum, as in kp_diff_tile
#pragma unroll
        for (int g = 0; g < RS / 16; g++) {
          const float* wb = a.wpad + rb + 16 * g;
          float s16 = 0.f;
#pragma unroll
          for (int i = 0; i < 16; i++) {
            float v = 0.f;
            if (TYPE == 2) {
              float S[8], Kpp[9] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int q = 0; q < 8; q++) S[q] = acc[16 * g + i][q < NS ? q : 0];
              kp_newton<8>(S, Kpp, a.p, v);
            } else if (TYPE >= 3) {
              v = hssk_matern_f32<TYPE >= 3 ? TYPE : 3>(acc[16 * g + i][0] * a.s2);
            } else {
              v = exp2f(-(acc[16 * g + i][0] * a.s2));
            }
            s16 += wb[i] * v;
          }
          dd += (double)s16;
        }
      }
    }
  }
  red[wv * KP_T + lane] = dd;
  __syncthreads();
  if (wv == 0) a.partial[(size_t)sp * a.ldm + c0 + lane] = ((red[lane] + red[KP_T + lane]) + red[2 * KP_T + lane]) + red[3 * KP_T + lane];
  if (lane == 0 && ndf) hssk_gadd_ll(a.dstats + 1, ndf);
}

// the splits in index order, rounded once
__global__ __launch_bounds__(256) void kp_reduce_kernel(const double* __restrict__ partial, int ldm, int splits, int m, float* __restrict__ pred) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  double s = 0.;
  for (int q = 0; q < splits; q++) s += partial[(size_t)q * ldm + c];
  pred[c] = (float)s;
}

__global__ __launch_bounds__(256) void kp_zero_kernel(float* __restrict__ pred, int m) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < m) pred[c] = 0.f;
}

template <int KSM, int MT>
void kp_launch_main_t(hssk_ctx* ctx, const KpArgs& a, int nt, size_t shm) {
  hssk_rt::allow_dynamic_lds(kp_main_kernel<KSM, MT>, shm);
  HSSK_LAUNCH((kp_main_kernel<KSM, MT>), dim3((unsigned)nt, (unsigned)a.splits), dim3(256), shm, ctx->stream, a);
}
template <int KSM>
void kp_launch_main(hssk_ctx* ctx, const KpArgs& a, int nt, size_t shm) {
  if (a.type == 3) kp_launch_main_t<KSM, 3>(ctx, a, nt, shm);
  else if (a.type == 4) kp_launch_main_t<KSM, 4>(ctx, a, nt, shm);
  else kp_launch_main_t<KSM, 0>(ctx, a, nt, shm);
}

// what the difference form multiplies a pair's FP32 distance by, and the scale of the prepared points of the matrix-core route
inline float kp_s2(int type, double h) {
  const double l2e = 1.4426950408889634;
  return (float)(type >= 3 ? hssk_matern_c(type, h) : (type == 1 ? l2e / h : l2e / (2. * h * h)));
}
inline double kp_point_scale(int type, double h) {
  return type >= 3 ? std::sqrt(type == 3 ? 3. : 5.) / h : std::sqrt(1.4426950408889634) / (h * std::sqrt(2.));
}

size_t kp_align(size_t v) { return (v + 255) & ~size_t(255); }

}  // namespace

extern "C" int hssk_kernel_predict_splits(long long n, int m) {
  if (n <= 0 || m <= 0) return 0;
  const long long chunks = (n + KP_W * KP_T - 1) / (KP_W * KP_T), nt = ((long long)m + KP_T - 1) / KP_T;
  const long long want = (KP_WGS + nt - 1) / nt;
  return (int)std::max<long long>(1, std::min(want, chunks));
}

namespace {
// The two public forms of each prediction.  hssk_kernel_predict_f32 / _wide take the three kernels of the reference and go on
// refusing every other type code, as they always have; hssk_matern_predict_f32 / _wide take twice_nu = 3 or 5 and pass the type
// 3 or 4 (`matern`).  `who` names the entry point in the messages.
int kp_predict(const char* who_, bool matern, hssk_ctx* ctx, const float* X, long long n, int d, int type, int p, double h, const float* w,
               const float* T, int m, float* pred, long long* stats) {
  HSSK_API_BEGIN
  const std::string who(who_);
  if (!ctx) throw std::invalid_argument(who + ": no context");
  if (matern ? (type != 3 && type != 4) : (type < 0 || type > 2))
    throw std::invalid_argument(who + (matern ? ": twice_nu must be 3 (Matern32) or 5 (Matern52)" : ": type must be 0 (Gauss), 1 (Laplace) or 2 (ANOVA)"));
  if (d < 1 || d > KP_DMAX) throw std::invalid_argument(who + ": point dimension must be in [1, 64]");
  if (type == 2 && (p < 1 || p > 8 || p > d)) throw std::invalid_argument(who + ": ANOVA degree must be in [1, min(8, d)]");
  if (n < 0 || n > (1LL << 31) - 1024) throw std::invalid_argument(who + ": training point count out of range");
  if (m < 0 || m > (1 << 30)) throw std::invalid_argument(who + ": test point count out of range");
  if (!(h > 0.)) throw std::invalid_argument(who + ": the kernel width must be positive");
  if ((n > 0 && (!X || !w)) || (m > 0 && (!T || !pred))) throw std::invalid_argument(who + ": null pointer");
  if (stats) for (int i = 0; i < 6; i++) stats[i] = 0;
  if (m == 0) return 0;
  if (n == 0) {
    HSSK_LAUNCH(kp_zero_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, pred, m);
    hssk_rt::check_launch();
    return 0;
  }
  const int KSM = d <= 2 ? 2 : (d <= 8 ? 5 : (d <= 16 ? 9 : (d <= 32 ? 17 : 33))), KP = 2 * KSM;
  const int chunks = (int)((n + KP_W * KP_T - 1) / (KP_W * KP_T)), nt = (m + KP_T - 1) / KP_T;
  const int splits = hssk_kernel_predict_splits(n, m), ldn = chunks * KP_W * KP_T, ldm = nt * KP_T, tx = ldn / KP_T;
  const size_t shm = sizeof(double) * KP_W * KP_T + sizeof(float) * KP_T * (size_t)d;
  if (shm > hssk_rt::max_lds_per_workgroup()) { hssk_set_error(who + ": the test tile does not fit the LDS of this device"); return 2; }
  // scratch: statistics | partial means | Xa | Ta | padded weights | tile norms | partial sums
  const size_t o_st = 0, o_pm = 256, o_xa = kp_align(o_pm + sizeof(double) * KP_G * d), o_ta = kp_align(o_xa + sizeof(float) * (size_t)KP * ldn);
  const size_t o_wp = kp_align(o_ta + sizeof(float) * (size_t)KP * ldm), o_xm = kp_align(o_wp + sizeof(float) * (size_t)ldn);
  const size_t o_tm = kp_align(o_xm + sizeof(float) * tx), o_pa = kp_align(o_tm + sizeof(float) * nt);
  const size_t total = o_pa + sizeof(double) * (size_t)splits * ldm;
  char* base = (char*)ctx->scratch(total);
  static const bool force = [] { const char* e = std::getenv("HSSK_KPREDICT_FORCE_DIFF"); return e && e[0] == '1'; }();
  KpArgs a;
  a.X = X; a.T = T; a.Xa = (float*)(base + o_xa); a.Ta = (float*)(base + o_ta); a.wpad = (float*)(base + o_wp);
  a.xmax = (float*)(base + o_xm); a.tmax = (float*)(base + o_tm);
  a.n = n; a.m = m; a.d = d; a.type = type; a.p = type == 2 ? p : 1; a.ldn = ldn; a.ldm = ldm; a.chunks = chunks; a.splits = splits;
  a.force_diff = force ? 1 : 0;
  a.s2 = kp_s2(type, h);
  a.partial = (double*)(base + o_pa);
  a.dstats = (long long*)(base + o_st);
  hssk_rt::memset_async(a.dstats, 0, 16, ctx->stream);
  if (stats) hssk_watch_start(ctx, 4);
  HSSK_LAUNCH(kp_mean_kernel, dim3(KP_G), dim3(256), 0, ctx->stream, X, d, n, (double*)(base + o_pm));
  HSSK_LAUNCH(kp_prep_kernel, dim3((unsigned)(tx + nt)), dim3(64), 0, ctx->stream, X, n, T, m, d, KP, kp_point_scale(type, h),
              (const double*)(base + o_pm), w, (float*)(base + o_xa), ldn, (float*)(base + o_ta), ldm, (float*)(base + o_wp),
              (float*)(base + o_xm), (float*)(base + o_tm), tx);
  if (stats) { hssk_watch_stop(ctx, 4); hssk_watch_start(ctx, 6); }
  if (KSM == 2) kp_launch_main<2>(ctx, a, nt, shm);
  else if (KSM == 5) kp_launch_main<5>(ctx, a, nt, shm);
  else if (KSM == 9) kp_launch_main<9>(ctx, a, nt, shm);
  else if (KSM == 17) kp_launch_main<17>(ctx, a, nt, shm);
  else kp_launch_main<33>(ctx, a, nt, shm);
  if (stats) { hssk_watch_stop(ctx, 6); hssk_watch_start(ctx, 4); }
  HSSK_LAUNCH(kp_reduce_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)a.partial, ldm, splits, m, pred);
  if (stats) hssk_watch_stop(ctx, 4);
  hssk_rt::check_launch();
  if (stats) {
    long long hs[2] = {0, 0};
    hssk_rt::d2h(hs, a.dstats, 16, ctx->stream);
    hssk_rt::sync(ctx->stream);
    const double ms_main = hssk_watch_read_ms(ctx, 6, nullptr), ms_rest = hssk_watch_read_ms(ctx, 4, nullptr);
    stats[0] = hs[0]; stats[1] = hs[1]; stats[2] = splits;
    stats[3] = (long long)std::llround((ms_main + ms_rest) * 1e3);
    stats[4] = (long long)std::llround(ms_main * 1e3);
    stats[5] = (long long)std::llround(ms_rest * 1e3);
  }
  HSSK_API_END
}

int kp_predict_wide(const char* who_, bool matern, hssk_ctx* ctx, const float* X, long long n, int d, int type, int p, double h,
                    const float* w, const float* T, int m, float* pred, long long* stats) {
  HSSK_API_BEGIN
  const std::string who(who_);
  if (!ctx) throw std::invalid_argument(who + ": no context");
  if (matern ? (type != 3 && type != 4) : (type < 0 || type > 2))
    throw std::invalid_argument(who + (matern ? ": twice_nu must be 3 (Matern32) or 5 (Matern52)" : ": type must be 0 (Gauss), 1 (Laplace) or 2 (ANOVA)"));
  if (d <= KP_DMAX) throw std::invalid_argument(who + ": point dimension must be above 64 (hssk_kernel_predict_f32 takes the others)");
  if (type == 2 && (p < 1 || p > 8)) throw std::invalid_argument(who + ": ANOVA degree must be in [1, 8]");
  if (n < 0 || n > (1LL << 31) - 1024) throw std::invalid_argument(who + ": training point count out of range");
  if (m < 0 || m > (1 << 30)) throw std::invalid_argument(who + ": test point count out of range");
  if (!(h > 0.)) throw std::invalid_argument(who + ": the kernel width must be positive");
  if ((n > 0 && (!X || !w)) || (m > 0 && (!T || !pred))) throw std::invalid_argument(who + ": null pointer");
  if (stats) for (int i = 0; i < 6; i++) stats[i] = 0;
  if (m == 0) return 0;
  if (n == 0) {
    HSSK_LAUNCH(kp_zero_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, pred, m);
    hssk_rt::check_launch();
    return 0;
  }
  const int chunks = (int)((n + KP_W * KP_T - 1) / (KP_W * KP_T)), nt = (m + KP_T - 1) / KP_T;
  const int splits = hssk_kernel_predict_splits(n, m), ldn = chunks * KP_W * KP_T, ldm = nt * KP_T;
  // scratch: statistics | padded weights | partial sums
  const size_t o_st = 0, o_wp = 256, o_pa = kp_align(o_wp + sizeof(float) * (size_t)ldn);
  char* base = (char*)ctx->scratch(o_pa + sizeof(double) * (size_t)splits * ldm);
  KpArgs a;
  a.X = X; a.T = T; a.Xa = nullptr; a.Ta = nullptr; a.wpad = (float*)(base + o_wp); a.xmax = nullptr; a.tmax = nullptr;
  a.n = n; a.m = m; a.d = d; a.type = type; a.p = type == 2 ? p : 1; a.ldn = ldn; a.ldm = ldm; a.chunks = chunks; a.splits = splits;
  a.force_diff = 1;
  a.s2 = kp_s2(type, h);
  a.partial = (double*)(base + o_pa);
  a.dstats = (long long*)(base + o_st);
  hssk_rt::memset_async(a.dstats, 0, 16, ctx->stream);
  if (stats) hssk_watch_start(ctx, 4);
  HSSK_LAUNCH(kp_wpad_kernel, dim3((unsigned)((ldn + 255) / 256)), dim3(256), 0, ctx->stream, w, n, ldn, (float*)(base + o_wp));
  if (stats) { hssk_watch_stop(ctx, 4); hssk_watch_start(ctx, 6); }
  const dim3 grid((unsigned)nt, (unsigned)splits);
  if (type == 0) HSSK_LAUNCH((kp_wide_kernel<0, 32>), grid, dim3(256), 0, ctx->stream, a);
  else if (type == 1) HSSK_LAUNCH((kp_wide_kernel<1, 32>), grid, dim3(256), 0, ctx->stream, a);
  else if (type == 3) HSSK_LAUNCH((kp_wide_kernel<3, 32>), grid, dim3(256), 0, ctx->stream, a);
  else if (type == 4) HSSK_LAUNCH((kp_wide_kernel<4, 32>), grid, dim3(256), 0, ctx->stream, a);
  else HSSK_LAUNCH((kp_wide_kernel<2, 16>), grid, dim3(256), 0, ctx->stream, a);
  if (stats) { hssk_watch_stop(ctx, 6); hssk_watch_start(ctx, 4); }
  HSSK_LAUNCH(kp_reduce_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)a.partial, ldm, splits, m, pred);
  if (stats) hssk_watch_stop(ctx, 4);
  hssk_rt::check_launch();
  if (stats) {
    long long hs[2] = {0, 0};
    hssk_rt::d2h(hs, a.dstats, 16, ctx->stream);
    hssk_rt::sync(ctx->stream);
    const double ms_main = hssk_watch_read_ms(ctx, 6, nullptr), ms_rest = hssk_watch_read_ms(ctx, 4, nullptr);
    stats[0] = hs[0]; stats[1] = hs[1]; stats[2] = splits;
    stats[3] = (long long)std::llround((ms_main + ms_rest) * 1e3);
    stats[4] = (long long)std::llround(ms_main * 1e3);
    stats[5] = (long long)std::llround(ms_rest * 1e3);
  }
  HSSK_API_END
}
}  // namespace

extern "C" int hssk_kernel_predict_f32(hssk_ctx* ctx, const float* X, long long n, int d, int type, int p, double h, const float* w,
                                       const float* T, int m, float* pred, long long* stats) {
  return kp_predict("hssk_kernel_predict_f32", false, ctx, X, n, d, type, p, h, w, T, m, pred, stats);
}
extern "C" int hssk_kernel_predict_f32_wide(hssk_ctx* ctx, const float* X, long long n, int d, int type, int p, double h, const float* w,
                                            const float* T, int m, float* pred, long long* stats) {
  return kp_predict_wide("hssk_kernel_predict_f32_wide", false, ctx, X, n, d, type, p, h, w, T, m, pred, stats);
}
extern "C" int hssk_matern_predict_f32(hssk_ctx* ctx, const float* X, long long n, int d, int twice_nu, double h, const float* w,
                                       const float* T, int m, float* pred, long long* stats) {
  return kp_predict("hssk_matern_predict_f32", true, ctx, X, n, d, twice_nu == 3 ? 3 : (twice_nu == 5 ? 4 : -1), 1, h, w, T, m, pred, stats);
}
extern "C" int hssk_matern_predict_f32_wide(hssk_ctx* ctx, const float* X, long long n, int d, int twice_nu, double h, const float* w,
                                            const float* T, int m, float* pred, long long* stats) {
  return kp_predict_wide("hssk_matern_predict_f32_wide", true, ctx, X, n, d, twice_nu == 3 ? 3 : (twice_nu == 5 ? 4 : -1), 1, h, w, T, m, pred, stats);
}
