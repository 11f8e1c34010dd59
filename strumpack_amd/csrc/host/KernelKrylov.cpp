// Kernel<double>: solves with the exact kernel matrix from the kept model -- right-preconditioned restarted GMRES on the device, in
// FP64 and with the FP32 product inside the cycles.
#include "KernelModel.hpp"

namespace strumpack {
namespace kernel {

const Kernel<double>::Model& Kernel<double>::krylov_model(const char* what, double rtol, int maxit, int restart) const {
  const Model& M = model(what);
  require_exact_products(*this, what);
  if (!(rtol > 0.) || !std::isfinite(rtol)) throw std::invalid_argument(std::string(what) + ": rtol must be positive and finite");
  if (maxit < 1 || restart < 1) throw std::invalid_argument(std::string(what) + ": maxit and restart must be at least 1");
  if (inner_ == KrylovInner::FP32 && d() > 64)
    throw std::invalid_argument(std::string(what) + ": the FP32 inner product takes at most 64 coordinates (krylov_inner)");
  // Stopwatches 4 / 5 / 6 are not this code's alone (the compression and the prediction statistics use them too): whatever an
  // earlier caller that threw between its start and its read left recorded there is dropped, so that this call reads its own pairs.
  for (int w = 4; w <= 6; w++) hssk_watch_read_ms(M.ctx(), w, nullptr);
  if (inner_ == KrylovInner::FP32) hssk_watch_read_ms(M.ctx(), 7, nullptr);
  kry_ms_[0] = kry_ms_[1] = kry_ms_[2] = kry_ms_[3] = 0.;
  return M;
}

void Kernel<double>::krylov_finish(const Model& M, KrylovInfo& info) const {
  for (int w = 0; w < 3; w++) info.ms[w] = kry_ms_[w] = hssk_watch_read_ms(M.ctx(), w + 4, nullptr);
  info.ms[3] = kry_ms_[3] = inner_ == KrylovInner::FP32 ? hssk_watch_read_ms(M.ctx(), 7, nullptr) : 0.;
  const double st[6] = {(double)info.products, (double)info.products32, (double)info.fallbacks, (double)info.cycles, info.ms[0], info.ms[3]};
  std::copy(st, st + 6, kry_stats_);
}

void Kernel<double>::krylov_inner(KrylovInner p, double inner_rtol) {
  if (p != KrylovInner::FP64 && p != KrylovInner::FP32) throw std::invalid_argument("krylov_inner: unknown precision");
  if (!(inner_rtol > 0.) || !(inner_rtol < 1.)) throw std::invalid_argument("krylov_inner: inner_rtol must lie in (0, 1)");
  inner_ = p;
  inner_rtol_ = inner_rtol;
}

std::size_t Kernel<double>::krylov_prep_bytes() const {
  if (inner_ != KrylovInner::FP32) return 0;
  const long long b = hssk_kernel_matmul_f32_prep_bytes((long long)n(), int(d()));
  if (b < 0) throw std::invalid_argument("krylov_inner: the FP32 inner product takes at most 64 coordinates");
  return (std::size_t)b;
}

void Kernel<double>::krylov_prepare(const Model& M, KrylovWork& ws) const {
  if (!ws.prep) return;
  const hssk_kernel_spec spec = kept_spec(*this, M.dX, lambda_);
  ckk(hssk_kernel_matmul_f32_prep(M.ctx(), &spec, ws.prep, (long long)ws.prep_bytes));
}

// Stopwatches 4 / 5 / 6: products, solves, Krylov kernels (1 .. 3 belong to the variance loop this may run inside).
void Kernel<double>::krylov_block(const Model& M, KrylovWork& ws, int nc, double* dX, const double* dB, double rtol, int maxit, int restart,
                                  KrylovInfo& info) const {
  hssk_ctx* ctx = M.ctx();
  const long long nn = (long long)n();
  const int m = ws.m, ldh = m + 2;
  const size_t blk = (size_t)nn * nc;
  const hssk_kernel_spec spec = kept_spec(*this, M.dX, lambda_);
  // ||b|| per column
  std::vector<double> bn(nc, 0.), nrm(nc, 0.), res0(nc, 0.), res(nc, 0.);
  watched(ctx, 6, [&] { ckk(hssk_coldots(ctx, dB, nn, dB, nn, nn, nc, ws.norms)); });
  ckk(hssk_memcpy_d2h(ctx, bn.data(), ws.norms, (long long)sizeof(double) * nc));
  for (int c = 0; c < nc; c++) {
    bn[c] = std::sqrt(bn[c]);
    if (!(bn[c] > 0.)) ckk(hssk_memset_zero(ctx, dX + (size_t)c * nn, (long long)sizeof(double) * nn));   // b = 0: x = 0
  }
  // per column: R (m x m, upper triangle of the rotated Hessenberg matrix), the rotations, the rotated right-hand side
  std::vector<double> R((size_t)nc * m * m), cs((size_t)nc * m), sn((size_t)nc * m), g((size_t)nc * (m + 1)), Y((size_t)nc * m),
      H((size_t)nc * ldh);
  std::vector<int> its(nc, 0), kc(nc, 0);
  std::vector<char> conv(nc, 0);
  int steps = 0;
  bool first = true, all = false;
  // mixed mode: the product inside the cycles in FP32 until a true residual fails to decrease
  bool mixed = ws.prep != nullptr;
  std::vector<double> rprev(nc, 0.), thr(nc, 0.);
  for (;;) {
    // 1. the true residual of every column
    watched(ctx, 4, [&] { ckk(hssk_kernel_matmul(ctx, &spec, 0, dX, nn, nc, ws.W, nn, 0)); });
    info.products++;
    watched(ctx, 6, [&] { ckk(hssk_krylov_start(ctx, dB, nn, ws.W, nn, nn, nc, ws.V, nn, ws.norms)); });
    ckk(hssk_memcpy_d2h(ctx, nrm.data(), ws.norms, (long long)sizeof(double) * nc));
    // 2. who is done
    unsigned long long active = 0;
    for (int c = 0; c < nc; c++) {
      res[c] = bn[c] > 0. ? nrm[c] / bn[c] : 0.;
      conv[c] = !(bn[c] > 0.) || nrm[c] <= rtol * bn[c];
      if (!conv[c]) active |= 1ULL << c;
    }
    if (mixed && !first) {
      bool stuck = false;
      for (int c = 0; c < nc; c++) stuck = stuck || (!conv[c] && !(nrm[c] < rprev[c]));
      if (stuck) { mixed = false; info.fallbacks++; }
    }
    if (mixed) rprev = nrm;
    for (int c = 0; c < nc; c++) thr[c] = mixed ? std::max(rtol * bn[c], inner_rtol_ * nrm[c]) : rtol * bn[c];
    if (first) { res0 = res; first = false; }
    all = active == 0;
    if (all || steps >= maxit) break;
    info.cycles++;
    for (int c = 0; c < nc; c++) { kc[c] = 0; g[(size_t)c * (m + 1)] = nrm[c]; }
    // 3. the steps of the cycle
    for (int k = 0; k < m; k++) {
      ckk(hssk_memcpy_d2d(ctx, ws.Z, ws.V + (size_t)k * blk, (long long)sizeof(double) * blk));
      watched(ctx, 5, [&] { M.H.solve_device(nc, ws.Z, nn); });
      info.solves++;
      if (mixed) {
        watched(ctx, 7, [&] { ckk(hssk_kernel_matmul_f32(ctx, &spec, ws.prep, ws.Z, nn, nc, ws.W, nn, 0, nullptr)); });
        info.products32++;
      } else {
        watched(ctx, 4, [&] { ckk(hssk_kernel_matmul(ctx, &spec, 0, ws.Z, nn, nc, ws.W, nn, 0)); });
        info.products++;
      }
      watched(ctx, 6, [&] { ckk(hssk_krylov_orth(ctx, ws.V, nn, nn, nc, k, ws.W, nn, active, ws.Hout, ldh)); });
      ckk(hssk_memcpy_d2h(ctx, H.data(), ws.Hout, (long long)sizeof(double) * ldh * nc));   // (the only read-back of a step)
      steps++;
      for (int c = 0; c < nc; c++) {
        if (!((active >> c) & 1ULL)) continue;
        its[c]++;
        double* h = H.data() + (size_t)c * ldh;
        double *Rc = R.data() + (size_t)c * m * m, *cc = cs.data() + (size_t)c * m, *sc = sn.data() + (size_t)c * m, *gc = g.data() + (size_t)c * (m + 1);
        const double below = h[k + 1];
        for (int i = 0; i < k; i++) {
          const double t = cc[i] * h[i] + sc[i] * h[i + 1];
          h[i + 1] = -sc[i] * h[i] + cc[i] * h[i + 1];
          h[i] = t;
        }
        const double r = std::hypot(h[k], h[k + 1]);
        if (!(r > 0.) || !std::isfinite(r)) {   // a column of zeros (or not a number): the step adds nothing, the column rests
          active &= ~(1ULL << c);
          continue;
        }
        cc[k] = h[k] / r;
        sc[k] = h[k + 1] / r;
        h[k] = r;
        for (int i = 0; i <= k; i++) Rc[i + (size_t)k * m] = h[i];
        gc[k + 1] = -sc[k] * gc[k];
        gc[k] = cc[k] * gc[k];
        kc[c] = k + 1;
        if (std::abs(gc[k + 1]) <= thr[c] || below == 0.) active &= ~(1ULL << c);
      }
      if (!active || steps >= maxit) break;
    }
    // 4. x += M^-1 (V y), every column with its own number of steps
    int kmax = 0;
    std::fill(Y.begin(), Y.end(), 0.);
    for (int c = 0; c < nc; c++) {
      const double *Rc = R.data() + (size_t)c * m * m, *gc = g.data() + (size_t)c * (m + 1);
      double* y = Y.data() + (size_t)c * m;
      for (int i = kc[c] - 1; i >= 0; i--) {
        double s = gc[i];
        for (int j = i + 1; j < kc[c]; j++) s -= Rc[i + (size_t)j * m] * y[j];
        y[i] = s / Rc[i + (size_t)i * m];
      }
      kmax = std::max(kmax, kc[c]);
    }
    if (kmax == 0) break;   // (no column moved: nothing more to gain)
    ckk(hssk_memcpy_h2d(ctx, ws.Y, Y.data(), (long long)sizeof(double) * m * nc));
    watched(ctx, 6, [&] { ckk(hssk_krylov_combine(ctx, ws.V, nn, nn, nc, kmax, ws.Y, m, ws.U, nn, 0)); });
    watched(ctx, 5, [&] { M.H.solve_device(nc, ws.U, nn); });
    info.solves++;
    watched(ctx, 6, [&] { ckk(hssk_krylov_combine(ctx, ws.U, nn, nn, nc, 1, ws.ones, 1, dX, nn, 1)); });
  }
  for (int c = 0; c < nc; c++) {
    info.converged = info.converged && conv[c];
    info.iterations = std::max(info.iterations, its[c]);
    info.its.push_back(its[c]);
    info.residual.push_back(res[c]);
    info.residual0.push_back(res0[c]);
  }
}

KrylovInfo Kernel<double>::model_refine(double rtol, int maxit, int restart) {
  const Model& M = krylov_model("model_refine", rtol, maxit, restart);
  hssk_ctx* ctx = M.ctx();
  const long long nn = (long long)n();
  KrylovInfo info;
  KrylovWork ws(ctx, nn, 1, maxit, restart, true, krylov_prep_bytes());
  krylov_prepare(M, ws);
  ckk(hssk_memcpy_h2d(ctx, ws.B, M.labels.data(), (long long)sizeof(double) * nn));
  ckk(hssk_memcpy_h2d(ctx, ws.X, M.weights.data(), (long long)sizeof(double) * nn));
  krylov_block(M, ws, 1, ws.X, ws.B, rtol, maxit, restart, info);
  DenseMatrix<double> w(n(), 1);
  ckk(hssk_memcpy_d2h(ctx, w.data(), ws.X, (long long)sizeof(double) * nn));
  krylov_finish(M, info);
  model_->weights = w;
  return info;
}

DenseMatrix<double> Kernel<double>::model_solve(const DenseMatrix<double>& B, KrylovInfo* info, double rtol, int maxit, int restart) const {
  const Model& M = krylov_model("model_solve", rtol, maxit, restart);
  if (B.rows() != n()) throw std::invalid_argument("model_solve: one row per training point expected (cluster order)");
  hssk_ctx* ctx = M.ctx();
  const long long nn = (long long)n();
  const int m = int(B.cols()), CH = 64;
  KrylovInfo local;
  DenseMatrix<double> X(n(), m);
  if (m > 0) {
    KrylovWork ws(ctx, nn, std::min(m, CH), maxit, restart, true, krylov_prep_bytes());
    krylov_prepare(M, ws);
    for (int c0 = 0; c0 < m; c0 += CH) {
      const int nc = std::min(CH, m - c0);
      ckk(hssk_memcpy2d_h2d(ctx, ws.B, sizeof(double) * nn, B.ptr(0, c0), sizeof(double) * B.ld(), sizeof(double) * nn, nc));
      ckk(hssk_memcpy_d2d(ctx, ws.X, ws.B, (long long)sizeof(double) * nn * nc));
      watched(ctx, 5, [&] { M.H.solve_device(nc, ws.X, nn); });   // the first iterate H^-1 b
      local.solves++;
      krylov_block(M, ws, nc, ws.X, ws.B, rtol, maxit, restart, local);
      ckk(hssk_memcpy2d_d2h(ctx, X.ptr(0, c0), sizeof(double) * X.ld(), ws.X, sizeof(double) * nn, sizeof(double) * nn, nc));
    }
    krylov_finish(M, local);
  }
  if (info) *info = local;
  return X;
}

std::vector<double> Kernel<double>::predict_variance_exact(const DenseMatrix<double>& test, KrylovInfo* info, double rtol, int maxit, int restart) const {
  const Model& M = krylov_model("predict_variance_exact", rtol, maxit, restart);
  if (test.rows() != d()) throw std::invalid_argument("predict_variance_exact: test points have the wrong dimension");
  KrylovInfo local;
  if (test.cols() == 0) { if (info) *info = local; return {}; }
  KrylovWork ws(M.ctx(), (long long)n(), 64, maxit, restart, false, krylov_prep_bytes());
  krylov_prepare(M, ws);
  std::vector<double> var = variance_chunks(M, test, &ws, rtol, maxit, restart, &local);
  krylov_finish(M, local);
  if (info) *info = local;
  return var;
}

DenseMatrix<double> Kernel<double>::predict_covariance_exact(const DenseMatrix<double>& test, KrylovInfo* info, double rtol, int maxit, int restart) const {
  const Model& M = krylov_model("predict_covariance_exact", rtol, maxit, restart);
  if (test.rows() != d()) throw std::invalid_argument("predict_covariance_exact: test points have the wrong dimension");
  KrylovInfo local;
  if (test.cols() == 0) { if (info) *info = local; return DenseMatrix<double>(0, 0); }
  KrylovWork ws(M.ctx(), (long long)n(), 64, maxit, restart, false, krylov_prep_bytes());
  krylov_prepare(M, ws);
  DenseMatrix<double> C = covariance_chunks(M, test, &ws, rtol, maxit, restart, &local);
  krylov_finish(M, local);
  if (info) *info = local;
  return C;
}

std::vector<double> Kernel<double>::predict_variance_gradient_exact(const DenseMatrix<double>& test, DenseMatrix<double>& grad, KrylovInfo* info,
                                                                    double rtol, int maxit, int restart) const {
  const Model& M = krylov_model("predict_variance_gradient_exact", rtol, maxit, restart);
  require_point_gradient("predict_variance_gradient_exact");
  if (test.rows() != d()) throw std::invalid_argument("predict_variance_gradient_exact: test points have the wrong dimension");
  KrylovInfo local;
  if (test.cols() == 0) { grad = DenseMatrix<double>(d(), 0); if (info) *info = local; return {}; }
  KrylovWork ws(M.ctx(), (long long)n(), 64, maxit, restart, false, krylov_prep_bytes());
  krylov_prepare(M, ws);
  std::vector<double> var = variance_chunks(M, test, &ws, rtol, maxit, restart, &local, &grad);
  krylov_finish(M, local);
  if (info) *info = local;
  return var;
}

}  // namespace kernel
}  // namespace strumpack
