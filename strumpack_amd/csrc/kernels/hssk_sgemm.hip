// The sketch GEMM of a SINGLE-PRECISION operand that lies in HBM:  C(m x n) = alpha A(m x k) op(B) + beta C  with A the
// engine's FP64 R^T panel, B the caller's float matrix (never widened as a whole) and C the engine's FP64 sample panel.
// (reference: the float instantiation HSS/HSSMatrix.cpp:513-516 does this arithmetic in float throughout.)
//
// Arithmetic rules (include/hssk.h states them for the caller):
//   * A is rounded ONCE to float: a small kernel writes a zero-padded float copy of the panel (rows up to a multiple of
//     the row block, k up to a multiple of the stage depth) that all workgroups read through L2;
//   * products and sums of one K-chunk run on the FP32 matrix cores (v_mfma_f32_32x32x2_f32: bitwise a k-ordered fmaf
//     chain, one rounding per product, FP32 accumulate; gfx950 FP32 matrix peak 157.3 TFLOP/s = twice the FP64 one);
//   * the K-chunks' partial tiles are widened to FP64, written to scratch and summed in FP64 in chunk order by a second
//     kernel (the deterministic K-split of hssk_dgemm.hip), which also applies alpha / beta and stores C in FP64;
//   * nothing depends on timing: the result is bitwise the same from run to run.
//
// Tiling: the four-wave register-prefetch form of hssk_dgemm.hip (dgemm_kernel).  Workgroup = 256 threads (4 wave64 as
// 2 x 2), output tile BM x 64 with BM in {64, 128, 192} so that one workgroup covers all m sample rows when m <= 192 and B is
// streamed from HBM exactly once.  A wave owns BM / 2 x 32 of the tile: up to three 32 x 32 accumulators (48 registers).  K
// advances 16 per stage through double-buffered LDS (As[k][i], Bs[k][j], row stride = 32 floats more than a multiple of 64,
// so the two k rows a 32x32x2 fragment read touches fall into different bank halves); float operands halve the LDS and HBM
// bytes per k against the FP64 form.  The operands of stage s + 2 travel in registers while stage s computes.
// Interior tiles (whole 64 columns, k a multiple of 16, B 16-byte aligned with a leading dimension that is a multiple of
// 4) load 16 bytes per lane unmasked; everything else -- ragged edges, odd leading dimensions, narrow outputs -- takes the
// masked instantiation.  The padded float copy of A needs no mask in either.
#include "hssk_device.h"
#include "hssk_internal.h"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr int SBN = 64, SBK = 16;

// Af(i, kk) = (float) A(i, kk) inside m x k, 0 in the padding (ldaf rows, kpad columns); grid (row chunks, kk)
__global__ void narrow_panel_kernel(float* __restrict__ Af, long long ldaf, const double* __restrict__ A, long long lda,
                                    int m, long long k, long long kk0) {
  const long long kk = kk0 + blockIdx.y;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < ldaf; i += (long long)gridDim.x * blockDim.x)
    Af[i + kk * ldaf] = (i < m && kk < k) ? (float)A[i + kk * lda] : 0.f;
}

// FULL = true : interior tiles (see above): unmasked 16-byte loads of B.   FULL = false: masked 4-byte loads of B.
// TAG only separates the symbol of the short tail launch from the main one (per-kernel profiles stay readable)
template <int BM, bool TRANSB, bool FULL, int TAG = 0>
__global__ __launch_bounds__(256, 2) void sgemm_kernel(int m, long long n, long long k, const float* __restrict__ A, long long lda,
                                                       const float* __restrict__ B, long long ldb, double* __restrict__ P,
                                                       long long ldp, long long pstride, long long kchunk, int jtile0) {
  constexpr int LDA_S = BM + 32, LDB_S = SBN + 32;
  constexpr int WM = BM / 2;       // rows per wave
  constexpr int MT = WM / 32;      // 32 x 32 accumulators per wave
  constexpr int A4 = BM * SBK / 4 / 256;    // 16-byte pieces per thread and stage
  constexpr int B4 = SBN * SBK / 4 / 256;
  constexpr int B_PER_THREAD = SBN * SBK / 256;
  HSSK_SHARED float As[2 * SBK * LDA_S];
  HSSK_SHARED float Bs[2 * SBK * LDB_S];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  int bx = blockIdx.x;
  {  // XCD-aware tile order (hssk_dgemm.hip): XCD x (= id % 8) is handed a contiguous range of column tiles
    const int nx = gridDim.x, x = bx & 7, q = nx >> 3, r = nx & 7;
    bx = x * q + (x < r ? x : r) + (bx >> 3);
  }
  const long long j0 = (long long)(bx + jtile0) * SBN;
  const int i0 = blockIdx.y * BM;
  const long long kbeg = (long long)blockIdx.z * kchunk;
  const long long kend = kbeg + kchunk < k ? kbeg + kchunk : k;
  const int wm = (wave & 1) * WM, wn = (wave >> 1) * 32;

  hssk_f16v acc[MT];
#pragma unroll
  for (int a = 0; a < MT; a++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[a][r] = 0.f;

  const long long nst = (kend - kbeg + SBK - 1) / SBK;  // stages (the padded copy of A has whole stages)
  const float* Ak = A + i0 + kbeg * lda;
  const long long stepA = (long long)SBK * lda;
  int offA[A4], ldsA[A4];
#pragma unroll
  for (int r = 0; r < A4; r++) {
    const int e = tid + 256 * r;   // piece (i4, kk) with i = 4 i4
    const int i = 4 * (e % (BM / 4)), kk = e / (BM / 4);
    offA[r] = i + kk * (int)lda;
    ldsA[r] = kk * LDA_S + i;
  }

  // MFMAs of one k-stage; the LDS fragments of sub-step ks + 2 are requested before the MFMAs of sub-step ks issue
  auto compute = [&](int buf) {
    const float* as = As + buf * SBK * LDA_S + wm + l31;
    const float* bs = Bs + buf * SBK * LDB_S + wn + l31;
    float af[2][MT], bf[2];
#pragma unroll
    for (int a = 0; a < MT; a++) af[0][a] = as[h * LDA_S + a * 32];
    bf[0] = bs[h * LDB_S];
#pragma unroll
    for (int ks = 0; ks < SBK; ks += 2) {
      const int cur = (ks >> 1) & 1, nxt = cur ^ 1;
      if (ks + 2 < SBK) {
#pragma unroll
        for (int a = 0; a < MT; a++) af[nxt][a] = as[(ks + 2 + h) * LDA_S + a * 32];
        bf[nxt] = bs[(ks + 2 + h) * LDB_S];
      }
#pragma unroll
      for (int a = 0; a < MT; a++)   // swapped operands: lane holds C[i = l31][j = 8 (r / 4) + 4 h + r % 4]
        acc[a] = hssk_mfma_f32_32x32x2(bf[cur], af[cur][a], acc[a]);
    }
  };

  if (FULL) {
    const float* Bk = TRANSB ? B + j0 + kbeg * ldb : B + j0 * ldb + kbeg;
    const long long stepB = TRANSB ? (long long)SBK * ldb : (long long)SBK;
    int offB[B4], ldsB[B4];
#pragma unroll
    for (int r = 0; r < B4; r++) {
      const int e = tid + 256 * r;
      if (TRANSB) {  // op(B)(k,j) = B(j,k): four along j
        const int j = 4 * (e % (SBN / 4)), kk = e / (SBN / 4);
        offB[r] = j + kk * (int)ldb;
        ldsB[r] = kk * LDB_S + j;
      } else {       // op(B)(k,j) = B(k,j): four along k
        const int kk = 4 * (e % (SBK / 4)), j = e / (SBK / 4);
        offB[r] = kk + j * (int)ldb;
        ldsB[r] = kk * LDB_S + j;
      }
    }
    // two register sets: the global loads of stage s + 2 are issued while stage s computes
    hssk_f4 ra0[A4], rb0[B4], ra1[A4], rb1[B4];
    auto load = [&](hssk_f4 (&ra)[A4], hssk_f4 (&rb)[B4]) {
#pragma unroll
      for (int r = 0; r < A4; r++) ra[r] = *reinterpret_cast<const hssk_f4*>(Ak + offA[r]);
#pragma unroll
      for (int r = 0; r < B4; r++) rb[r] = *reinterpret_cast<const hssk_f4*>(Bk + offB[r]);
      Ak += stepA; Bk += stepB;
    };
    auto store = [&](int buf, const hssk_f4 (&ra)[A4], const hssk_f4 (&rb)[B4]) {
      float* as = As + buf * SBK * LDA_S;
      float* bs = Bs + buf * SBK * LDB_S;
#pragma unroll
      for (int r = 0; r < A4; r++) *reinterpret_cast<hssk_f4*>(as + ldsA[r]) = ra[r];
#pragma unroll
      for (int r = 0; r < B4; r++) {
        if (TRANSB) *reinterpret_cast<hssk_f4*>(bs + ldsB[r]) = rb[r];
        else {
#pragma unroll
          for (int q = 0; q < 4; q++) bs[ldsB[r] + q * LDB_S] = rb[r][q];
        }
      }
    };
    if (nst > 0) {
      load(ra0, rb0);                      // stage 0
      store(0, ra0, rb0);
      if (nst > 1) load(ra1, rb1);         // stage 1
      __syncthreads();
      long long st = 0;
      // LDS buffer of stage s is s & 1; register set of stage s is s & 1 as well
      for (; st + 2 < nst; st += 2) {
        load(ra0, rb0);                    // stage st+2
        compute(0);                        // stage st
        store(1, ra1, rb1);                // stage st+1 (loaded one full stage ago)
        __syncthreads();
        if (st + 3 < nst) load(ra1, rb1);  // stage st+3
        compute(1);                        // stage st+1
        store(0, ra0, rb0);                // stage st+2
        __syncthreads();
      }
      // here LDS[0] holds stage st; stage st+1 (if any) sits in (ra1, rb1)
      compute(0);
      if (st + 1 < nst) {
        store(1, ra1, rb1);
        __syncthreads();
        compute(1);
      }
    }
  } else {
    hssk_f4 ra[A4];
    float rb[B_PER_THREAD];
    auto load = [&](long long k0) {
#pragma unroll
      for (int r = 0; r < A4; r++) ra[r] = *reinterpret_cast<const hssk_f4*>(Ak + offA[r]);
      Ak += stepA;
#pragma unroll
      for (int r = 0; r < B_PER_THREAD; r++) {
        const int e = tid + 256 * r;
        if (TRANSB) {
          const int j = e % SBN, kk = e / SBN;
          rb[r] = (j0 + j < n && k0 + kk < kend) ? B[j0 + j + (k0 + kk) * ldb] : 0.f;
        } else {
          const int kk = e % SBK, j = e / SBK;
          rb[r] = (j0 + j < n && k0 + kk < kend) ? B[k0 + kk + (j0 + j) * ldb] : 0.f;
        }
      }
    };
    auto store = [&](int buf) {
      float* as = As + buf * SBK * LDA_S;
      float* bs = Bs + buf * SBK * LDB_S;
#pragma unroll
      for (int r = 0; r < A4; r++) *reinterpret_cast<hssk_f4*>(as + ldsA[r]) = ra[r];
#pragma unroll
      for (int r = 0; r < B_PER_THREAD; r++) {
        const int e = tid + 256 * r;
        if (TRANSB) bs[(e / SBN) * LDB_S + (e % SBN)] = rb[r];
        else bs[(e % SBK) * LDB_S + (e / SBK)] = rb[r];
      }
    };
    if (nst > 0) { load(kbeg); store(0); }
    __syncthreads();
    int buf = 0;
    long long k0 = kbeg;
    for (long long st = 0; st + 1 < nst; st++) {
      k0 += SBK;
      load(k0);
      compute(buf);
      store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
    if (nst > 0) compute(buf);
  }
  // partial tile, widened -> P (slice blockIdx.z), plain stores; the reduce kernel sums the slices in FP64
  double* Pz = P + (long long)blockIdx.z * pstride;
#pragma unroll
  for (int a = 0; a < MT; a++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int gi = i0 + wm + a * 32 + l31;
      const long long gj = j0 + wn + 8 * (r >> 2) + 4 * h + (r & 3);
      if (gi < m && gj < n) Pz[gi + gj * ldp] = (double)acc[a][r];
    }
}

// C = alpha * sum_z P_z + beta * C   in FP64, slices in order (fixed summation order -> deterministic)
__global__ void sgemm_reduce_kernel(int m, long long n, const double* __restrict__ P, long long ldp, long long pstride, int nz,
                                    double alpha, double beta, double* __restrict__ C, long long ldc) {
  const long long total = (long long)m * n;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(e % m);
    const long long j = e / m;
    double s = 0.;
    for (int z = 0; z < nz; z++) s += P[i + j * ldp + z * pstride];
    double* c = C + i + j * ldc;
    double v = alpha * s;
    if (beta != 0.) v += beta * (*c);
    *c = v;
  }
}
// few output elements, many slices (narrow outputs with a deep K-split): 16 elements x 16 z-lanes per workgroup, every lane
// sums its slices z = lane, lane + 16, ..., the 16 lane sums are added in lane order (fixed order as well)
__global__ void sgemm_reduce_wide_kernel(int m, long long n, const double* __restrict__ P, long long ldp, long long pstride, int nz,
                                         double alpha, double beta, double* __restrict__ C, long long ldc) {
  HSSK_SHARED double s_part[256];
  const int el = threadIdx.x & 15, zl = threadIdx.x >> 4;
  const long long total = (long long)m * n;
  for (long long e0 = (long long)blockIdx.x * 16; e0 < total; e0 += (long long)gridDim.x * 16) {
    const long long e = e0 + el;
    const int i = (int)(e % m);
    const long long j = e / m;
    double s = 0.;
    if (e < total) {
      const double* p = P + i + j * ldp;
      for (int z = zl; z < nz; z += 16) s += p[z * pstride];
    }
    s_part[threadIdx.x] = s;
    __syncthreads();
    if (zl == 0 && e < total) {
      double t = 0.;
      for (int q = 0; q < 16; q++) t += s_part[el + 16 * q];
      double* c = C + i + j * ldc;
      double v = alpha * t;
      if (beta != 0.) v += beta * (*c);
      *c = v;
    }
    __syncthreads();
  }
}

template <int BM, bool FULL, int TAG>
void launch_sgemm(hssk_ctx* ctx, int transB, dim3 grid, int m, long long n, long long k, const float* A, long long lda,
                  const float* B, long long ldb, double* P, long long ldp, long long pstride, long long kchunk, int jtile0) {
  if (grid.x == 0) return;
  if (transB)
    HSSK_LAUNCH((sgemm_kernel<BM, true, FULL, TAG>), grid, dim3(256), 0, ctx->stream, m, n, k, A, lda, B, ldb, P, ldp, pstride, kchunk, jtile0);
  else
    HSSK_LAUNCH((sgemm_kernel<BM, false, FULL, TAG>), grid, dim3(256), 0, ctx->stream, m, n, k, A, lda, B, ldb, P, ldp, pstride, kchunk, jtile0);
}
template <bool FULL, int TAG>
void launch_sbm(int BM, hssk_ctx* ctx, int transB, dim3 grid, int m, long long n, long long k, const float* A, long long lda,
                const float* B, long long ldb, double* P, long long ldp, long long pstride, long long kchunk, int jtile0) {
  if (BM == 192) launch_sgemm<192, FULL, TAG>(ctx, transB, grid, m, n, k, A, lda, B, ldb, P, ldp, pstride, kchunk, jtile0);
  else if (BM == 128) launch_sgemm<128, FULL, TAG>(ctx, transB, grid, m, n, k, A, lda, B, ldb, P, ldp, pstride, kchunk, jtile0);
  else launch_sgemm<64, FULL, TAG>(ctx, transB, grid, m, n, k, A, lda, B, ldb, P, ldp, pstride, kchunk, jtile0);
}

void sgemm_impl(hssk_ctx* ctx, int transB, int m, long long n, long long k, double alpha, const double* A, long long lda,
                const float* B, long long ldb, double beta, double* C, long long ldc) {
  if (m <= 0 || n <= 0) return;
  const int BM = m > 128 ? 192 : (m > 64 ? 128 : 64);
  const unsigned gm = (unsigned)((m + BM - 1) / BM);
  const long long ksteps = (k + SBK - 1) / SBK;
  const long long ldaf = (long long)gm * BM, kpad = std::max<long long>(ksteps, 1) * SBK;
  // interior tiles take the unmasked kernel; the ragged last columns (and any unaligned / odd-sized operand) the masked one
  const bool aligned = k > 0 && (k % SBK == 0) && (ldb % 4 == 0) && ((size_t)B % 16 == 0);
  static const int cus = hssk_rt::cu_count();
  const unsigned gn_full = aligned ? (unsigned)(n / SBN) : 0u;
  const long long edge_col0 = (long long)gn_full * SBN;
  const unsigned gn_edge = (unsigned)((n - edge_col0 + SBN - 1) / SBN);
  // Work decomposition of hssk_dgemm.hip: the CUs hold `slots` workgroups (two per CU); the full tiles are cut into a MAIN group
  // whose grid (tiles x K-split) fills whole rounds of the slots and a short TAIL group with a deeper K-split that fills one
  // last round; the ragged edge has its own masked launch.  Every group writes FP64 K-partials that one reduce pass folds into C.
  const long long slots = 2LL * cus;
  struct Group { long long col0 = 0, ntiles = 0; int split = 1; long long kchunk = SBK; int nz = 0; double* P = nullptr; long long cols = 0, vcols = 0; };
  auto chunk_of = [&](int split) {
    const long long c = ((ksteps + split - 1) / split) * SBK;
    return c > 0 ? c : (long long)SBK;
  };
  auto max_split = [&]() { return (int)std::max<long long>(1, std::min<long long>(256, ksteps / 24)); };
  auto one_round_split = [&](long long tiles) {
    if (tiles <= 0 || k <= 0) return 1;
    return (int)std::max<long long>(1, std::min<long long>(max_split(), slots / tiles));
  };
  Group gmain, gtail, gedge;
  if (gn_full) {
    const long long T = (long long)gm * gn_full;
    // cost model (units: one k-stage of one workgroup): rounds x (stages per chunk + epilogue) + reduce traffic per chunk and tile
    const double epi = 3.0, red = 0.0067;
    double best = 1e300;
    int best_s = 1;
    long long best_main = T;
    // K-chunks of at most ~1024 stages: the workgroups running together on an XCD stay within a window of the shared A panel
    const int sp_min = (int)std::min<long long>(std::min(max_split(), 64), (ksteps + 1023) / 1024);
    for (int sp = std::max(1, sp_min); sp <= std::min(max_split(), 64); sp++) {
      const long long r = (T * sp) / slots;                       // whole rounds
      long long tm = r > 0 ? std::min<long long>(T, (r * slots) / sp) : 0;
      if (gm > 1) tm = T;                                          // tall outputs: no tile regrouping
      const long long tt = T - tm;
      double cost = 0.;
      if (tm) cost += (double)((tm * sp + slots - 1) / slots) * ((double)(ksteps + sp - 1) / sp + epi) + red * sp * (double)tm;
      if (tt) {
        const int st = one_round_split(tt);
        cost += (double)((tt * st + slots - 1) / slots) * ((double)(ksteps + st - 1) / st + epi) + red * st * (double)tt + 2.0;
      }
      if (cost < best - 1e-9) { best = cost; best_s = sp; best_main = tm; }
    }
    if (const char* e = std::getenv("HSSK_SGEMM_SPLIT")) {   // tuning override: K-split of the main group
      const int sp = std::max(1, std::min(max_split(), std::atoi(e)));
      const long long r = (T * sp) / slots;
      best_s = sp;
      best_main = (gm > 1 || r == 0) ? T : std::min<long long>(T, (r * slots) / sp);
    }
    gmain.col0 = 0; gmain.ntiles = gm > 1 ? gn_full : best_main; gmain.split = best_s; gmain.cols = gmain.ntiles * SBN;
    gtail.col0 = gmain.cols; gtail.ntiles = gn_full - gmain.ntiles; gtail.split = one_round_split(gtail.ntiles); gtail.cols = gtail.ntiles * SBN;
  }
  gedge.col0 = edge_col0; gedge.ntiles = gn_edge; gedge.split = one_round_split((long long)gm * gn_edge); gedge.cols = n - edge_col0;
  const long long ldp = m;
  size_t ptot = 0;
  for (Group* g : {&gmain, &gtail, &gedge}) {
    if (!g->ntiles) continue;
    g->vcols = std::min(g->cols, n - g->col0);
    g->kchunk = chunk_of(g->split);
    g->nz = (int)std::max<long long>(1, (k + g->kchunk - 1) / g->kchunk);
    ptot += (size_t)ldp * g->cols * g->nz;
  }
  ptot = (ptot + 1) & ~size_t(1);   // (the float panel behind the partials starts 16-byte aligned)
  double* P = ctx->scratch(sizeof(double) * ptot + sizeof(float) * (size_t)ldaf * kpad);
  float* Af = (float*)(P + ptot);
  {
    double* q = P;
    for (Group* g : {&gmain, &gtail, &gedge}) {
      if (!g->ntiles) continue;
      g->P = q;
      q += (size_t)ldp * g->cols * g->nz;
    }
  }
  // A, rounded once to float, zero-padded
  for (long long c0 = 0; c0 < kpad; c0 += 65535) {   // (grid.y limit)
    const long long nc = std::min<long long>(65535, kpad - c0);
    HSSK_LAUNCH(narrow_panel_kernel, dim3((unsigned)((ldaf + 255) / 256), (unsigned)nc), dim3(256), 0, ctx->stream, Af, ldaf, A, lda, m, k, c0);
  }
  // partials of a group are addressed by absolute column: shift its base by the group's first column
  auto shifted = [&](const Group& g) { return g.P - g.col0 * ldp; };
  // the timed launch (hssk_last_dgemm_ms / _flops): the main group, or whatever carries the bulk
  const Group* timed = gmain.ntiles ? &gmain : (gtail.ntiles ? &gtail : &gedge);
  auto bracket = [&](const Group* g, auto&& launch) {
    if (!g->ntiles) return;
    if (g == timed) hssk_rt::event_record(ctx->ev0, ctx->stream);
    launch();
    if (g == timed) hssk_rt::event_record(ctx->ev1, ctx->stream);
  };
  auto grid_of = [&](const Group& g) { return dim3((unsigned)g.ntiles, gm, (unsigned)g.nz); };
  bracket(&gedge, [&] { launch_sbm<false, 0>(BM, ctx, transB, grid_of(gedge), m, n, k, Af, ldaf, B, ldb, shifted(gedge), ldp, ldp * gedge.cols, gedge.kchunk, (int)(gedge.col0 / SBN)); });
  bracket(&gtail, [&] { launch_sbm<true, 1>(BM, ctx, transB, grid_of(gtail), m, n, k, Af, ldaf, B, ldb, shifted(gtail), ldp, ldp * gtail.cols, gtail.kchunk, (int)(gtail.col0 / SBN)); });
  bracket(&gmain, [&] { launch_sbm<true, 0>(BM, ctx, transB, grid_of(gmain), m, n, k, Af, ldaf, B, ldb, shifted(gmain), ldp, ldp * gmain.cols, gmain.kchunk, (int)(gmain.col0 / SBN)); });
  ctx->d_clk = nullptr;   // (no shader-clock probe / workgroup trace in this kernel)
  ctx->dgemm_trace_wgs = 0;
  ctx->dgemm_timed = true;
  ctx->dgemm_timed_flops = 2.0 * (double)m * (double)timed->vcols * (double)k;
  for (const Group* g : {&gmain, &gtail, &gedge}) {
    if (!g->ntiles) continue;
    const long long total = (long long)m * g->vcols;
    const unsigned rb = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    if (g->nz >= 32 && total <= 65536)
      HSSK_LAUNCH(sgemm_reduce_wide_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, ctx->stream, m, g->vcols, (const double*)g->P, ldp, ldp * g->cols, g->nz, alpha, beta, C + g->col0 * ldc, ldc);
    else
      HSSK_LAUNCH(sgemm_reduce_kernel, dim3(rb), dim3(256), 0, ctx->stream, m, g->vcols, (const double*)g->P, ldp, ldp * g->cols, g->nz, alpha, beta, C + g->col0 * ldc, ldc);
  }
  hssk_rt::check_launch();
}

// dst = (float) src, column by column; grid (row chunks, columns)
__global__ void narrow_f32_kernel(float* __restrict__ dst, long long ldd, const double* __restrict__ src, long long lds, long long rows) {
  const long long j = blockIdx.y;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long long)gridDim.x * blockDim.x)
    dst[i + j * ldd] = (float)src[i + j * lds];
}

// element gather from a single-precision matrix, widened: B(i,j) = (double) A(I[i], J[j]); a workgroup per 8 columns of a request
struct SWork {
  int prob, chunk;
};
constexpr int S_COLS_PER_WG = 8;
__global__ void gather_elems_f32_kernel(const hssk_elem_desc* __restrict__ descs, const SWork* __restrict__ work) {
  const SWork w = work[blockIdx.x];
  const hssk_elem_desc p = descs[w.prob];
  const float* Af = (const float*)p.A;
  const int jlast = (w.chunk + 1) * S_COLS_PER_WG;
  const int jend = p.n < jlast ? p.n : jlast;
  for (int j = w.chunk * S_COLS_PER_WG; j < jend; j++) {
    const long long gj = p.J ? p.J[j] : (p.j0 + j);
    const bool cin = p.chi <= p.clo || (gj >= p.clo && gj < p.chi);
    const float* col = Af + gj * p.lda;
    for (int i = threadIdx.x; i < p.m; i += blockDim.x) {
      const long long gi = p.I ? p.I[i] : (p.i0 + i);
      const bool rin = p.rhi <= p.rlo || (gi >= p.rlo && gi < p.rhi);
      const double v = (cin && rin) ? (double)col[gi] : 0.;
      if (p.transpose) p.B[j + (size_t)i * p.ldb] = v;
      else p.B[i + (size_t)j * p.ldb] = v;
    }
  }
}

}  // namespace

extern "C" int hssk_sgemm_sketch(hssk_ctx* ctx, int transB, int m, long long n, long long k, double alpha, const double* A,
                                 long long lda, const float* B, long long ldb, double beta, double* C, long long ldc) {
  HSSK_API_BEGIN
  sgemm_impl(ctx, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);
  HSSK_API_END
}

extern "C" int hssk_narrow_f32(hssk_ctx* ctx, float* dst, long long ldd, const double* src, long long lds, long long rows,
                               long long cols) {
  HSSK_API_BEGIN
  if (rows <= 0 || cols <= 0) return 0;
  if (lds < rows || ldd < rows) HSSK_UNSUPPORTED("leading dimension smaller than the block");
  for (long long c0 = 0; c0 < cols; c0 += 65535) {   // (grid.y limit)
    const long long nc = std::min<long long>(65535, cols - c0);
    dim3 grid((unsigned)std::min<long long>(256, (rows + 255) / 256), (unsigned)nc);
    HSSK_LAUNCH(narrow_f32_kernel, grid, dim3(256), 0, ctx->stream, dst + c0 * ldd, ldd, src + c0 * lds, lds, rows);
  }
  hssk_rt::check_launch();
  HSSK_API_END
}

extern "C" int hssk_gather_elems_f32(hssk_ctx* ctx, const hssk_elem_desc* descs, int count) {
  HSSK_API_BEGIN
  std::vector<SWork> w;
  for (int p = 0; p < count; p++)
    if (descs[p].m > 0)
      for (int c = 0; c * S_COLS_PER_WG < descs[p].n; c++) w.push_back(SWork{p, c});
  if (w.empty()) return 0;
  auto* dd = (const hssk_elem_desc*)ctx->stage(descs, sizeof(*descs) * count);
  auto* dw = (const SWork*)ctx->stage(w.data(), sizeof(SWork) * w.size());
  HSSK_LAUNCH(gather_elems_f32_kernel, dim3((unsigned)w.size()), dim3(256), 0, ctx->stream, dd, dw);
  hssk_rt::check_launch();
  HSSK_API_END
}
