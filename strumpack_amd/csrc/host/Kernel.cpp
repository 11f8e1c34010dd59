// Kernel<double>::fit_HSS / predict (reference: kernel/KernelRegression.hpp:56-123) and the C interface of
// include/kernel/Kernel.h (reference: kernel/Kernel.cpp:43-180).
#include "Kernel.hpp"

#include <chrono>
#include <cstdlib>
#include <random>

#include "DevicePool.hpp"
#include "HSSMatrix.hpp"
#include "NeighborSearch.hpp"
#include "hssk.h"
#include "kernel/Kernel.h"

namespace strumpack {
namespace kernel {

namespace {
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct FitInfo {
  long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
thread_local FitInfo last_fit;
thread_local std::vector<int> last_nodes;
void ckk(int rc) { if (rc) throw std::runtime_error(hssk_last_error()); }
}  // namespace

// ---- the kept model of Kernel<double> ------------------------------------------------------------------------------------------
struct Kernel<double>::Model {
  HSS::HSSMatrix<double> H;            // compressed K + lambda I with its ULV factors
  std::vector<double> labels;          // in cluster order
  DenseMatrix<double> weights;
  double* dX = nullptr;                // cluster-ordered points, d x n (device pool)
  size_t bX = 0;
  explicit Model(HSS::HSSMatrix<double>&& h) : H(std::move(h)) {}
  hssk_ctx* ctx() const { return H.engine()->ctx(); }
  ~Model() {
    if (dX) {
      hssk_sync(ctx());   // (nothing in flight may still read the chunk)
      DevicePool::get().release(dX, bX);
    }
  }
};

Kernel<double>::Kernel(DenseM_t& data, scalar_t lambda) : data_(data), lambda_(lambda) {}
Kernel<double>::~Kernel() = default;
void Kernel<double>::keep_model(bool keep) {
  keep_model_ = keep;
  if (!keep) model_.reset();
}
bool Kernel<double>::has_model() const { return bool(model_); }
const Kernel<double>::Model& Kernel<double>::model(const char* what) const {
  if (!model_) throw std::logic_error(std::string(what) + ": no kept model (keep_model(true) before fit_HSS; built-in kernels only)");
  return *model_;
}
double Kernel<double>::logabsdet() const { return model("logabsdet").H.logabsdet(); }
const std::vector<double>& Kernel<double>::model_labels() const { return model("model_labels").labels; }
const DenseMatrix<double>& Kernel<double>::model_weights() const { return model("model_weights").weights; }
void Kernel<double>::model_write(const std::string& path) const { model("model_write").H.write(path); }

double Kernel<double>::log_marginal_likelihood() const {
  const Model& M = model("log_marginal_likelihood");
  const double ld = M.H.logabsdet();
  long double ya = 0.L;
  for (std::size_t i = 0; i < M.labels.size(); i++) ya += (long double)M.labels[i] * (long double)M.weights(i, 0);
  const long double two_pi = 6.283185307179586476925286766559L;
  return (double)(-0.5L * ya - 0.5L * (long double)ld - 0.5L * (long double)M.labels.size() * std::log(two_pi));
}

DenseMatrix<double> Kernel<double>::model_set_lambda(double lambda) {
  model("model_set_lambda");
  Model& M = *model_;
  M.H.shift(lambda - lambda_);
  lambda_ = lambda;
  M.H.factor();
  DenseMatrix<double> w(n(), 1, M.labels.data(), n());
  M.H.solve(w);
  M.weights = w;
  return w;
}

// the device blocks of a Krylov call, for blocks of at most ncmax columns: restart + 1 basis blocks, Z (what the ULV solve works
// on: always this buffer, so that its recorded sweep is replayed), W (the product; the residual's A x at the start of a cycle),
// U (the update), B and X for callers that have none, and the small coefficient arrays
struct Kernel<double>::KrylovWork {
  long long n;
  int ncmax, m;   // m: steps of a cycle = min(restart, maxit)
  PoolBuf bV, bZ, bW, bU, bB, bX, bS, bP;
  double *V, *Z, *W, *U, *B, *X, *Y, *Hout, *norms, *ones;
  void* prep = nullptr;   // mixed mode: the prepared float points of hssk_kernel_matmul_f32 (prep_bytes > 0)
  std::size_t prep_bytes;
  KrylovWork(hssk_ctx* ctx, long long n_, int ncmax_, int maxit, int restart, bool own_bx, std::size_t prep_bytes_ = 0)
      : n(n_), ncmax(ncmax_), m(std::min(restart, maxit)), bV(ctx, sizeof(double) * n_ * ncmax_ * (size_t)(m + 1)), bZ(ctx, sizeof(double) * n_ * ncmax_),
        bW(ctx, sizeof(double) * n_ * ncmax_), bU(ctx, sizeof(double) * n_ * ncmax_), bB(ctx, sizeof(double) * n_ * ncmax_),
        bX(ctx, own_bx ? sizeof(double) * n_ * ncmax_ : 0), bS(ctx, sizeof(double) * (size_t)ncmax_ * (2 * m + 4)), bP(ctx, prep_bytes_),
        prep_bytes(prep_bytes_) {
    if (prep_bytes) prep = bP.p;
    V = (double*)bV.p; Z = (double*)bZ.p; W = (double*)bW.p; U = (double*)bU.p; B = (double*)bB.p; X = (double*)bX.p;
    Y = (double*)bS.p; Hout = Y + (size_t)ncmax * m; norms = Hout + (size_t)ncmax * (m + 2); ones = norms + ncmax;
    const std::vector<double> one(ncmax, 1.);
    ckk(hssk_memcpy_h2d(ctx, ones, one.data(), (long long)sizeof(double) * ncmax));
  }
};

std::vector<double> Kernel<double>::predict_variance(const DenseMatrix<double>& test) const {
  const Model& M = model("predict_variance");
  if (test.rows() != d()) throw std::invalid_argument("predict_variance: test points have the wrong dimension");
  return variance_chunks(M, test, nullptr, 0., 0, 0, nullptr);
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

std::vector<double> Kernel<double>::variance_chunks(const Model& M, const DenseMatrix<double>& test, KrylovWork* ws, double rtol, int maxit, int restart,
                                                    KrylovInfo* info) const {
  const int m = int(test.cols()), dim = int(d()), CH = 64;
  const long long nn = (long long)n();
  std::vector<double> var(m, 0.);
  var_ms_[0] = var_ms_[1] = var_ms_[2] = 0.;
  if (m == 0) return var;
  hssk_ctx* ctx = M.ctx();
  PoolBuf bT(ctx, sizeof(double) * dim * m), bK(ctx, sizeof(double) * nn * CH), bD(ctx, sizeof(double) * CH * CH), bP(ctx, sizeof(double) * m);
  double *dT = (double*)bT.p, *dK = (double*)bK.p, *dD = (double*)bD.p, *dP = (double*)bP.p;
  ckk(hssk_memcpy2d_h2d(ctx, dT, sizeof(double) * dim, test.data(), sizeof(double) * test.ld(), sizeof(double) * dim, m));
  std::vector<double> ktt(m, 0.), quad(m, 0.);
  const hssk_kernel_spec spec{M.dX, nn, dim, device_type(), degree(), width(), 0.};
  for (int c0 = 0; c0 < m; c0 += CH) {
    const int mc = std::min(CH, m - c0);
    const double* dTc = dT + (size_t)c0 * dim;
    hssk_watch_start(ctx, 1);
    ckk(hssk_kernel_cross(ctx, &spec, dTc, mc, dK, nn));
    hssk_watch_stop(ctx, 1);
    // k(t_c, t_c) by the same pair function: the diagonal of the chunk's own kernel block
    const hssk_kernel_spec self{dTc, (long long)mc, dim, device_type(), degree(), width(), 0.};
    ckk(hssk_kernel_cross(ctx, &self, dTc, mc, dD, mc));
    ckk(hssk_memcpy2d_d2h(ctx, ktt.data() + c0, sizeof(double), dD, sizeof(double) * (mc + 1), sizeof(double), mc));
    if (ws) ckk(hssk_memcpy_d2d(ctx, ws->B, dK, (long long)sizeof(double) * nn * mc));   // (the right-hand sides of the exact solve)
    hssk_watch_start(ctx, 2);
    M.H.solve_device(mc, dK, nn);
    hssk_watch_stop(ctx, 2);
    if (ws) {   // from H^-1 k on: the exact solve of the chunk's columns
      info->solves++;
      krylov_block(M, *ws, mc, dK, ws->B, rtol, maxit, restart, *info);
    }
    hssk_watch_start(ctx, 3);
    ckk(hssk_kernel_predict_cols(ctx, &spec, dK, nn, dTc, mc, dP + c0));
    hssk_watch_stop(ctx, 3);
  }
  ckk(hssk_memcpy_d2h(ctx, quad.data(), dP, (long long)sizeof(double) * m));
  for (int w = 0; w < 3; w++) var_ms_[w] = hssk_watch_read_ms(ctx, w + 1, nullptr);
  for (int c = 0; c < m; c++) var[c] = ktt[c] - quad[c];
  return var;
}

// ---- gradient of the log marginal likelihood, residual of the fit against the exact kernel matrix -------------
DenseMatrix<double> Kernel<double>::model_probes(int m, unsigned long long seed) const {
  model("model_probes");
  if (m < 1) throw std::invalid_argument("model_probes: at least one probe vector");
  DenseMatrix<double> Z(n(), m);
  std::mt19937_64 gen(seed);
  for (int c = 0; c < m; c++) {
    unsigned long long word = 0;
    for (std::size_t i = 0; i < n(); i++) {
      if (i % 64 == 0) word = gen();
      Z(i, c) = ((word >> (i % 64)) & 1ULL) ? 1. : -1.;
    }
  }
  return Z;
}

namespace {
// Block c0 of alpha | Z for both gradients: nc columns, the first of them alpha iff lead, the others the probes from z0 on.  They
// go to dB, their copy to dS, and S = H^-1 B is solved there (stopwatch 2) -- once per block, the same buffer for every block:
// the recorded sweep is replayed.
struct GradBlock { int nc, lead, z0; };
template <class MODEL>
GradBlock grad_block(const MODEL& M, const DenseMatrix<double>& Z, int c0, int CH, double* dB, double* dS) {
  const long long nn = (long long)Z.rows();
  hssk_ctx* ctx = M.ctx();
  const int nc = std::min(CH, int(Z.cols()) + 1 - c0), lead = c0 == 0 ? 1 : 0, z0 = c0 == 0 ? 0 : c0 - 1, nz = nc - lead;
  if (lead) ckk(hssk_memcpy_h2d(ctx, dB, M.weights.data(), (long long)sizeof(double) * nn));
  if (nz > 0) ckk(hssk_memcpy2d_h2d(ctx, dB + (size_t)lead * nn, sizeof(double) * nn, Z.ptr(0, z0), sizeof(double) * Z.ld(), sizeof(double) * nn, nz));
  ckk(hssk_memcpy_d2d(ctx, dS, dB, (long long)sizeof(double) * nn * nc));
  hssk_watch_start(ctx, 2);
  M.H.solve_device(nc, dS, nn);
  hssk_watch_stop(ctx, 2);
  return {nc, lead, z0};
}
}  // namespace

LmlGradient Kernel<double>::log_marginal_likelihood_gradient(int m, unsigned long long seed) const {
  model("log_marginal_likelihood_gradient");
  if (m < 1) throw std::invalid_argument("log_marginal_likelihood_gradient: at least one probe vector");
  return log_marginal_likelihood_gradient(model_probes(m, seed));
}

LmlGradient Kernel<double>::log_marginal_likelihood_gradient(const DenseMatrix<double>& Z) const {
  const Model& M = model("log_marginal_likelihood_gradient");
  if (device_type() != 0 && device_type() != 1) throw std::invalid_argument("log_marginal_likelihood_gradient: Gauss and Laplace kernels only");
  if (Z.cols() < 1) throw std::invalid_argument("log_marginal_likelihood_gradient: at least one probe vector");
  if (Z.rows() != n()) throw std::invalid_argument("log_marginal_likelihood_gradient: one probe row per training point expected (cluster order)");
  const int m = int(Z.cols()), dim = int(d()), CH = 64;
  const long long nn = (long long)n();
  hssk_ctx* ctx = M.ctx();
  grad_ms_[0] = grad_ms_[1] = grad_ms_[2] = 0.;
  // B: alpha | the probes, S = H^-1 B, G = K' B; the dots of a block: [0, 64) S.G, [64, 128) S.B, [128] alpha.G(:, 0)
  PoolBuf bB(ctx, sizeof(double) * nn * CH), bS(ctx, sizeof(double) * nn * CH), bG(ctx, sizeof(double) * nn * CH), bD(ctx, sizeof(double) * (2 * CH + 1));
  double *dB = (double*)bB.p, *dS = (double*)bS.p, *dG = (double*)bG.p, *dD = (double*)bD.p;
  const hssk_kernel_spec spec{M.dX, nn, dim, device_type(), degree(), width(), 0.};
  LmlGradient g;
  g.th.assign(m, 0.);
  g.tl.assign(m, 0.);
  std::vector<double> dots(2 * CH + 1, 0.);
  double aga = 0.;
  for (int c0 = 0; c0 < m + 1; c0 += CH) {   // column c of alpha | Z
    const GradBlock b = grad_block(M, Z, c0, CH, dB, dS);
    const int nc = b.nc, lead = b.lead, z0 = b.z0;
    hssk_watch_start(ctx, 1);
    ckk(hssk_kernel_matmul(ctx, &spec, 1, dB, nn, nc, dG, nn, 0));
    hssk_watch_stop(ctx, 1);
    hssk_watch_start(ctx, 3);
    ckk(hssk_coldots(ctx, dS, nn, dG, nn, nn, nc, dD));
    ckk(hssk_coldots(ctx, dS, nn, dB, nn, nn, nc, dD + CH));
    if (lead) ckk(hssk_coldots(ctx, dB, nn, dG, nn, nn, 1, dD + 2 * CH));
    hssk_watch_stop(ctx, 3);
    ckk(hssk_memcpy_d2h(ctx, dots.data(), dD, (long long)sizeof(double) * (2 * CH + 1)));
    for (int c = lead; c < nc; c++) { g.th[z0 + c - lead] = dots[c]; g.tl[z0 + c - lead] = dots[CH + c]; }
    if (lead) aga = dots[2 * CH];
  }
  for (int w = 0; w < 3; w++) grad_ms_[w] = hssk_watch_read_ms(ctx, w + 1, nullptr);
  long double aa = 0.L, sh = 0.L, sl = 0.L;
  for (long long i = 0; i < nn; i++) aa += (long double)M.weights(i, 0) * (long double)M.weights(i, 0);
  for (int k = 0; k < m; k++) { sh += (long double)g.th[k]; sl += (long double)g.tl[k]; }
  g.quad_h = 0.5 * aga;
  g.quad_lambda = (double)(0.5L * aa);
  g.trace_h = (double)(sh / m);
  g.trace_lambda = (double)(sl / m);
  g.dh = g.quad_h - 0.5 * g.trace_h;
  g.dlambda = g.quad_lambda - 0.5 * g.trace_lambda;
  return g;
}

// ---- the same gradient per coordinate: one length scale each ---------------------------------------------------
LmlGradientCoords Kernel<double>::log_marginal_likelihood_gradient_coords(int m, unsigned long long seed) const {
  model("log_marginal_likelihood_gradient_coords");
  if (m < 1) throw std::invalid_argument("log_marginal_likelihood_gradient_coords: at least one probe vector");
  return log_marginal_likelihood_gradient_coords(model_probes(m, seed));
}

LmlGradientCoords Kernel<double>::log_marginal_likelihood_gradient_coords(const DenseMatrix<double>& Z) const {
  const char* what = "log_marginal_likelihood_gradient_coords";
  const Model& M = model(what);
  if (device_type() != 0 && device_type() != 1) throw std::invalid_argument(std::string(what) + ": Gauss and Laplace kernels only");
  if (d() > 64) throw std::invalid_argument(std::string(what) + ": at most 64 coordinates");
  if (Z.cols() < 1) throw std::invalid_argument(std::string(what) + ": at least one probe vector");
  if (Z.rows() != n()) throw std::invalid_argument(std::string(what) + ": one probe row per training point expected (cluster order)");
  const int m = int(Z.cols()), dim = int(d()), CH = 64, group = std::min(dim, hssk_kernel_matmul_coord_group());
  const long long nn = (long long)n();
  const size_t blk = (size_t)nn * CH;
  hssk_ctx* ctx = M.ctx();
  grad_ms_[0] = grad_ms_[1] = grad_ms_[2] = 0.;
  // B: alpha | the probes, S = H^-1 B, G_j = (K o D_j) B for one group of coordinates at a time; the dots of a block:
  // [j CH, j CH + nc) S.G_j, [dim CH + j] alpha.G_j(:, 0).  Every buffer before any computation.
  PoolBuf bB(ctx, sizeof(double) * blk), bS(ctx, sizeof(double) * blk), bG(ctx, sizeof(double) * blk * group),
      bD(ctx, sizeof(double) * (size_t)dim * (CH + 1));
  double *dB = (double*)bB.p, *dS = (double*)bS.p, *dG = (double*)bG.p, *dD = (double*)bD.p;
  const hssk_kernel_spec spec{M.dX, nn, dim, device_type(), degree(), width(), 0.};
  LmlGradientCoords g;
  g.m = m;
  g.dtheta.assign(dim, 0.);
  g.quad.assign(dim, 0.);
  g.trace.assign(dim, 0.);
  g.tc.assign((size_t)dim * m, 0.);
  std::vector<double> dots((size_t)dim * (CH + 1), 0.);
  for (int c0 = 0; c0 < m + 1; c0 += CH) {   // column c of alpha | Z
    const GradBlock b = grad_block(M, Z, c0, CH, dB, dS);
    const int nc = b.nc, lead = b.lead, z0 = b.z0;
    for (int j0 = 0; j0 < dim; j0 += group) {
      const int nj = std::min(group, dim - j0);
      hssk_watch_start(ctx, 1);
      ckk(hssk_kernel_matmul_coord(ctx, &spec, j0, nj, dB, nn, nc, dG, nn, (long long)blk, 0));
      hssk_watch_stop(ctx, 1);
      hssk_watch_start(ctx, 3);
      for (int jj = 0; jj < nj; jj++) {
        ckk(hssk_coldots(ctx, dS, nn, dG + jj * blk, nn, nn, nc, dD + (size_t)(j0 + jj) * CH));
        if (lead) ckk(hssk_coldots(ctx, dB, nn, dG + jj * blk, nn, nn, 1, dD + (size_t)dim * CH + j0 + jj));
      }
      hssk_watch_stop(ctx, 3);
    }
    ckk(hssk_memcpy_d2h(ctx, dots.data(), dD, (long long)sizeof(double) * dim * (CH + 1)));
    for (int j = 0; j < dim; j++) {
      for (int c = lead; c < nc; c++) g.tc[(size_t)j * m + z0 + c - lead] = dots[(size_t)j * CH + c];
      if (lead) g.quad[j] = 0.5 * dots[(size_t)dim * CH + j];
    }
  }
  for (int w = 0; w < 3; w++) grad_ms_[w] = hssk_watch_read_ms(ctx, w + 1, nullptr);
  for (int j = 0; j < dim; j++) {
    long double s = 0.L;
    for (int k = 0; k < m; k++) s += (long double)g.tc[(size_t)j * m + k];
    g.trace[j] = (double)(s / m);
    g.dtheta[j] = g.quad[j] - 0.5 * g.trace[j];
  }
  return g;
}

double Kernel<double>::model_residual() const {
  const Model& M = model("model_residual");
  if (device_type() != 0 && device_type() != 1) throw std::invalid_argument("model_residual: Gauss and Laplace kernels only");
  const long long nn = (long long)n();
  hssk_ctx* ctx = M.ctx();
  PoolBuf bB(ctx, sizeof(double) * nn), bG(ctx, sizeof(double) * nn);
  const hssk_kernel_spec spec{M.dX, nn, int(d()), device_type(), degree(), width(), lambda_};
  ckk(hssk_memcpy_h2d(ctx, bB.p, M.weights.data(), (long long)sizeof(double) * nn));
  ckk(hssk_kernel_matmul(ctx, &spec, 0, (const double*)bB.p, nn, 1, (double*)bG.p, nn, 0));
  std::vector<double> r(nn, 0.);
  ckk(hssk_memcpy_d2h(ctx, r.data(), bG.p, (long long)sizeof(double) * nn));
  long double num = 0.L, den = 0.L;
  for (long long i = 0; i < nn; i++) {
    const long double e = (long double)M.labels[i] - (long double)r[i];
    num += e * e;
    den += (long double)M.labels[i] * (long double)M.labels[i];
  }
  return (double)std::sqrt(num / den);
}

// ---- solves with the exact kernel matrix: right-preconditioned restarted GMRES on the device ---------------------
const Kernel<double>::Model& Kernel<double>::krylov_model(const char* what, double rtol, int maxit, int restart) const {
  const Model& M = model(what);
  if (device_type() != 0 && device_type() != 1) throw std::invalid_argument(std::string(what) + ": Gauss and Laplace kernels only (no ANOVA product)");
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
  const hssk_kernel_spec spec{M.dX, (long long)n(), int(d()), device_type(), degree(), width(), lambda_};
  ckk(hssk_kernel_matmul_f32_prep(M.ctx(), &spec, ws.prep, (long long)ws.prep_bytes));
}

// Stopwatches 4 / 5 / 6: products, solves, Krylov kernels (1 .. 3 belong to the variance loop this may run inside).
void Kernel<double>::krylov_block(const Model& M, KrylovWork& ws, int nc, double* dX, const double* dB, double rtol, int maxit, int restart,
                                  KrylovInfo& info) const {
  hssk_ctx* ctx = M.ctx();
  const long long nn = (long long)n();
  const int m = ws.m, ldh = m + 2;
  const size_t blk = (size_t)nn * nc;
  const hssk_kernel_spec spec{M.dX, nn, int(d()), device_type(), degree(), width(), lambda_};
  // ||b|| per column
  std::vector<double> bn(nc, 0.), nrm(nc, 0.), res0(nc, 0.), res(nc, 0.);
  hssk_watch_start(ctx, 6);
  ckk(hssk_coldots(ctx, dB, nn, dB, nn, nn, nc, ws.norms));
  hssk_watch_stop(ctx, 6);
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
    hssk_watch_start(ctx, 4);
    ckk(hssk_kernel_matmul(ctx, &spec, 0, dX, nn, nc, ws.W, nn, 0));
    hssk_watch_stop(ctx, 4);
    info.products++;
    hssk_watch_start(ctx, 6);
    ckk(hssk_krylov_start(ctx, dB, nn, ws.W, nn, nn, nc, ws.V, nn, ws.norms));
    hssk_watch_stop(ctx, 6);
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
      hssk_watch_start(ctx, 5);
      M.H.solve_device(nc, ws.Z, nn);
      hssk_watch_stop(ctx, 5);
      info.solves++;
      if (mixed) {
        hssk_watch_start(ctx, 7);
        ckk(hssk_kernel_matmul_f32(ctx, &spec, ws.prep, ws.Z, nn, nc, ws.W, nn, 0, nullptr));
        hssk_watch_stop(ctx, 7);
        info.products32++;
      } else {
        hssk_watch_start(ctx, 4);
        ckk(hssk_kernel_matmul(ctx, &spec, 0, ws.Z, nn, nc, ws.W, nn, 0));
        hssk_watch_stop(ctx, 4);
        info.products++;
      }
      hssk_watch_start(ctx, 6);
      ckk(hssk_krylov_orth(ctx, ws.V, nn, nn, nc, k, ws.W, nn, active, ws.Hout, ldh));
      hssk_watch_stop(ctx, 6);
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
    hssk_watch_start(ctx, 6);
    ckk(hssk_krylov_combine(ctx, ws.V, nn, nn, nc, kmax, ws.Y, m, ws.U, nn, 0));
    hssk_watch_stop(ctx, 6);
    hssk_watch_start(ctx, 5);
    M.H.solve_device(nc, ws.U, nn);
    hssk_watch_stop(ctx, 5);
    info.solves++;
    hssk_watch_start(ctx, 6);
    ckk(hssk_krylov_combine(ctx, ws.U, nn, nn, nc, 1, ws.ones, 1, dX, nn, 1));
    hssk_watch_stop(ctx, 6);
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
      hssk_watch_start(ctx, 5);
      M.H.solve_device(nc, ws.X, nn);   // the first iterate H^-1 b
      hssk_watch_stop(ctx, 5);
      local.solves++;
      krylov_block(M, ws, nc, ws.X, ws.B, rtol, maxit, restart, local);
      ckk(hssk_memcpy2d_d2h(ctx, X.ptr(0, c0), sizeof(double) * X.ld(), ws.X, sizeof(double) * nn, sizeof(double) * nn, nc));
    }
    krylov_finish(M, local);
  }
  if (info) *info = local;
  return X;
}

DenseMatrix<double> Kernel<double>::fit_HSS(std::vector<double>& labels, const HSS::HSSOptions<double>& opts) {
  if (labels.size() != n()) throw std::invalid_argument("fit_HSS: one label per training point expected");
  model_.reset();   // (the model of an earlier fit goes before the new compression asks for memory)
  double t0 = now();
  if (opts.verbose()) std::cout << "# starting HSS compression..." << std::endl;
  HSS::HSSMatrix<double> H(*this, opts);
  // labels to the cluster order: new label i = old label perm[i] (lapmt, forward)
  {
    std::vector<double> old(labels);
    for (std::size_t i = 0; i < labels.size(); i++) labels[i] = old[perm_[i] - 1];
  }
  double t1 = now();
  if (opts.verbose()) {
    std::cout << "# HSS compression time = " << t1 - t0 << std::endl;
    if (H.is_compressed())
      std::cout << "# created HSS matrix of dimension " << H.rows() << " x " << H.cols() << " with " << H.levels() << " levels" << std::endl
                << "# compression succeeded!" << std::endl;
    else std::cout << "# compression failed!!!" << std::endl;
    std::cout << "# rank(H) = " << H.rank() << std::endl << "# HSS memory(H) = " << H.memory() / 1e6 << " MB " << std::endl << std::endl
              << "# factorization start" << std::endl;
  }
  H.factor();
  double t2 = now();
  if (opts.verbose()) std::cout << "# factorization time = " << t2 - t1 << std::endl << "# solution start..." << std::endl;
  DenseMatrix<double> weights(n(), 1, labels.data(), n());
  H.solve(weights);
  double t3 = now();
  if (opts.verbose()) std::cout << "# solve time = " << t3 - t2 << std::endl;
  last_fit.v[0] = H.is_compressed(); last_fit.v[1] = (long long)H.levels(); last_fit.v[2] = (long long)H.rank();
  last_fit.v[3] = (long long)H.memory(); last_fit.v[4] = H.engine()->stats().d_final;
  last_nodes.assign(6 * (size_t)H.engine()->num_nodes(), 0);
  H.engine()->node_info(last_nodes.data());
  last_fit.v[5] = (long long)((t1 - t0) * 1e6); last_fit.v[6] = (long long)((t2 - t1) * 1e6); last_fit.v[7] = (long long)((t3 - t2) * 1e6);
  if (keep_model_ && device_type() >= 0 && n() > 0) {
    std::unique_ptr<Model> M(new Model(std::move(H)));
    M->labels = labels;
    M->weights = weights;
    M->bX = sizeof(double) * d() * n();
    M->dX = (double*)DevicePool::get().acquire(M->bX);
    if (!M->dX) throw std::runtime_error(hssk_last_error());
    ckk(hssk_memcpy2d_h2d(M->ctx(), M->dX, sizeof(double) * d(), data_.data(), sizeof(double) * data_.ld(), sizeof(double) * d(), (long long)n()));
    model_ = std::move(M);
  }
  return weights;
}

std::vector<double> Kernel<double>::predict(const DenseMatrix<double>& test, const DenseMatrix<double>& weights) const {
  if (test.rows() != d()) throw std::invalid_argument("predict: test points have the wrong dimension");
  if (weights.rows() != n()) throw std::invalid_argument("predict: one weight per training point expected");
  const int m = int(test.cols()), dim = int(d());
  std::vector<double> prediction(m, 0.);
  if (m == 0) return prediction;
  if (device_type() < 0) {
    // a user-defined kernel function (only its virtual evaluation is known): the sums on the host
    for (int c = 0; c < m; c++) {
      double s = 0.;
      for (std::size_t r = 0; r < n(); r++) s += weights(r, 0) * eval_kernel_function(data_.ptr(0, r), test.ptr(0, c));
      prediction[c] = s;
    }
    return prediction;
  }
  int dev = 0;
  if (const char* e = std::getenv("STRUMPACK_AMD_DEVICE")) dev = std::atoi(e);
  hssk_ctx* ctx = nullptr;
  ckk(hssk_ctx_create(&ctx, dev));
  void *dX = nullptr, *dT = nullptr, *dw = nullptr, *dp = nullptr;
  try {
    auto dalloc = [](long long bytes) { void* q = hssk_malloc(bytes); if (!q) throw std::runtime_error(hssk_last_error()); return q; };
    dX = dalloc((long long)sizeof(double) * dim * n());
    dT = dalloc((long long)sizeof(double) * dim * m);
    dw = dalloc((long long)sizeof(double) * n());
    dp = dalloc((long long)sizeof(double) * m);
    ckk(hssk_memcpy2d_h2d(ctx, dX, sizeof(double) * dim, data_.data(), sizeof(double) * data_.ld(), sizeof(double) * dim, (long long)n()));
    ckk(hssk_memcpy2d_h2d(ctx, dT, sizeof(double) * dim, test.data(), sizeof(double) * test.ld(), sizeof(double) * dim, m));
    ckk(hssk_memcpy_h2d(ctx, dw, weights.data(), (long long)sizeof(double) * n()));
    hssk_kernel_spec spec{(const double*)dX, (long long)n(), dim, device_type(), degree(), width(), 0.};
    ckk(hssk_kernel_predict(ctx, &spec, (const double*)dw, (const double*)dT, m, (double*)dp));
    ckk(hssk_memcpy_d2h(ctx, prediction.data(), dp, (long long)sizeof(double) * m));
    ckk(hssk_sync(ctx));
  } catch (...) {
    hssk_free(dX); hssk_free(dT); hssk_free(dw); hssk_free(dp);
    hssk_ctx_destroy(ctx);
    throw;
  }
  hssk_free(dX); hssk_free(dT); hssk_free(dw); hssk_free(dp);
  hssk_ctx_destroy(ctx);
  return prediction;
}

// ---- Kernel<float>: promoted fit, native FP32 prediction from a model that stays in HBM --------------------------------
struct Kernel<float>::Resident {
  hssk_ctx* ctx = nullptr;
  float *dX = nullptr, *dw = nullptr;   // cluster-ordered points (d x n) and the weights of the last fit (device pool)
  size_t bX = 0, bw = 0;
  const float* src = nullptr;           // the host array dX is a copy of
  size_t n = 0, d = 0;
  bool have_w = false;
  void drop() {
    if (ctx && (dX || dw)) hssk_sync(ctx);
    if (dX) DevicePool::get().release(dX, bX);
    if (dw) DevicePool::get().release(dw, bw);
    dX = dw = nullptr; bX = bw = 0; src = nullptr; have_w = false;
  }
  ~Resident() {
    drop();
    if (ctx) hssk_ctx_destroy(ctx);
  }
};

namespace {
// a user-defined float kernel function in front of the FP64 front end (its points are exactly the widened floats)
class PromotedUserKernel : public Kernel<double> {
 public:
  PromotedUserKernel(DenseMatrix<double>& data, const Kernel<float>& f) : Kernel<double>(data, f.lambda()), f_(f) {}

 protected:
  const Kernel<float>& f_;
  double eval_kernel_function(const double* x, const double* y) const override {
    std::vector<float> a(d()), b(d());
    for (std::size_t i = 0; i < d(); i++) { a[i] = (float)x[i]; b[i] = (float)y[i]; }
    return (double)f_.kernel_function(a.data(), b.data());
  }
};
HSS::HSSOptions<double> widen(const HSS::HSSOptions<float>& o) {
  HSS::HSSOptions<double> w;
  w.set_rel_tol(o.rel_tol()); w.set_abs_tol(o.abs_tol()); w.set_leaf_size(o.leaf_size()); w.set_pivot_threshold(o.pivot_threshold());
  w.set_max_rank(o.max_rank()); w.set_verbose(o.verbose());
  w.set_d0(o.d0()); w.set_dd(o.dd()); w.set_p(o.p()); w.set_random_engine(o.random_engine());
  w.set_random_distribution(o.random_distribution()); w.set_compression_algorithm(o.compression_algorithm());
  w.set_compression_sketch(o.compression_sketch()); w.set_nnz0(o.nnz0()); w.set_nnz(o.nnz()); w.set_SJLT_algo(o.SJLT_algo());
  w.set_user_defined_random(o.user_defined_random()); w.set_symmetric_operand(o.symmetric_operand());
  w.set_factor_ahead(o.factor_ahead()); w.set_synchronized_compression(o.synchronized_compression()); w.set_log_ranks(o.log_ranks());
  w.set_clustering_algorithm(o.clustering_algorithm()); w.set_approximate_neighbors(o.approximate_neighbors());
  w.set_ann_iterations(o.ann_iterations()); w.set_neighbor_search(o.neighbor_search());
  return w;
}
}  // namespace

Kernel<float>::Kernel(DenseMatrix<float>& data, float lambda) : data_(data), lambda_(lambda) {}
Kernel<float>::~Kernel() = default;
bool Kernel<float>::fitted() const { return res_ && res_->have_w; }

DenseMatrix<float> Kernel<float>::fit_HSS(std::vector<float>& labels, const HSS::HSSOptions<float>& opts) { return fit_HSS(labels, widen(opts)); }

DenseMatrix<float> Kernel<float>::fit_HSS(std::vector<float>& labels, const HSS::HSSOptions<double>& opts) {
  if (labels.size() != n()) throw std::invalid_argument("fit_HSS: one label per training point expected");
  if (res_) res_->drop();
  const std::size_t nn = n(), dd = d();
  DenseMatrix<double> Xd(dd, nn);
  for (std::size_t i = 0; i < nn; i++)
    for (std::size_t j = 0; j < dd; j++) Xd(j, i) = (double)data_(j, i);
  std::unique_ptr<Kernel<double>> Kd;
  switch (device_type()) {
    case 0: Kd.reset(new GaussKernel<double>(Xd, (double)width(), (double)lambda_)); break;
    case 1: Kd.reset(new LaplaceKernel<double>(Xd, (double)width(), (double)lambda_)); break;
    case 2: Kd.reset(new ANOVAKernel<double>(Xd, (double)width(), (double)lambda_, degree())); break;
    default: Kd.reset(new PromotedUserKernel(Xd, *this));
  }
  if (neighbors()) Kd->set_neighbors(neighbors(), neighbor_count());
  std::vector<double> ld(labels.begin(), labels.end());
  DenseMatrix<double> wd = Kd->fit_HSS(ld, opts);
  // the cluster order back into the caller's arrays (narrowing widened floats is exact), the solution rounded once
  perm_ = Kd->permutation();
  for (std::size_t i = 0; i < nn; i++) {
    for (std::size_t j = 0; j < dd; j++) data_(j, i) = (float)Xd(j, i);
    labels[i] = (float)ld[i];
  }
  DenseMatrix<float> w(nn, 1);
  for (std::size_t i = 0; i < nn; i++) w(i, 0) = (float)wd(i, 0);
  if (device_type() >= 0 && nn > 0) {
    // the model stays in HBM: a prediction uploads test points only
    if (!res_) res_.reset(new Resident());
    Resident& R = *res_;
    if (!R.ctx) {
      int dev = 0;
      if (const char* e = std::getenv("STRUMPACK_AMD_DEVICE")) dev = std::atoi(e);
      ckk(hssk_ctx_create(&R.ctx, dev));
    }
    R.bX = sizeof(float) * dd * nn; R.bw = sizeof(float) * nn;
    R.dX = (float*)DevicePool::get().acquire(R.bX);
    R.dw = (float*)DevicePool::get().acquire(R.bw);
    if (!R.dX || !R.dw) { R.drop(); throw std::runtime_error(hssk_last_error()); }
    ckk(hssk_memcpy2d_h2d(R.ctx, R.dX, sizeof(float) * dd, data_.data(), sizeof(float) * data_.ld(), sizeof(float) * dd, (long long)nn));
    ckk(hssk_memcpy_h2d(R.ctx, R.dw, w.data(), (long long)R.bw));
    R.src = data_.data(); R.n = nn; R.d = dd; R.have_w = true;
  }
  return w;
}

// test points: on the host (test_host, leading dimension ldt) or in HBM (test_dev); weights: on the host, or null = the resident
// ones; result to the host (out_host) or to HBM (out_dev)
void Kernel<float>::run_predict(int m, const float* test_host, int ldt, const float* test_dev, const float* weights_host,
                                float* out_host, float* out_dev) const {
  for (auto& v : pstats_) v = 0;
  if (m == 0) return;
  const std::size_t nn = n(), dd = d();
  if (!res_) res_.reset(new Resident());
  Resident& R = *res_;
  if (!R.ctx) {
    int dev = 0;
    if (const char* e = std::getenv("STRUMPACK_AMD_DEVICE")) dev = std::atoi(e);
    ckk(hssk_ctx_create(&R.ctx, dev));
  }
  long long uploaded = 0;
  const bool resident = R.dX && R.src == data_.data() && R.n == nn && R.d == dd;
  if (!resident) {
    R.drop();
    R.bX = sizeof(float) * dd * nn;
    R.dX = (float*)DevicePool::get().acquire(R.bX);
    if (!R.dX) { R.drop(); throw std::runtime_error(hssk_last_error()); }
    ckk(hssk_memcpy2d_h2d(R.ctx, R.dX, sizeof(float) * dd, data_.data(), sizeof(float) * data_.ld(), sizeof(float) * dd, (long long)nn));
    R.src = data_.data(); R.n = nn; R.d = dd;
    uploaded += (long long)R.bX;
  }
  if (!weights_host && !R.have_w) throw std::invalid_argument("predict: no fit");
  std::unique_ptr<PoolBuf> wbuf, tbuf, pbuf;
  const float* dw = R.dw;
  if (weights_host) {
    wbuf.reset(new PoolBuf(R.ctx, sizeof(float) * nn));
    ckk(hssk_memcpy_h2d(R.ctx, wbuf->p, weights_host, (long long)(sizeof(float) * nn)));
    uploaded += (long long)(sizeof(float) * nn);
    dw = (const float*)wbuf->p;
  }
  const float* dT = test_dev;
  if (!dT) {
    tbuf.reset(new PoolBuf(R.ctx, sizeof(float) * dd * m));
    ckk(hssk_memcpy2d_h2d(R.ctx, tbuf->p, sizeof(float) * dd, test_host, sizeof(float) * ldt, sizeof(float) * dd, m));
    uploaded += (long long)(sizeof(float) * dd * m);
    dT = (const float*)tbuf->p;
  }
  float* dp = out_dev;
  if (!dp) { pbuf.reset(new PoolBuf(R.ctx, sizeof(float) * m)); dp = (float*)pbuf->p; }
  long long st[6];
  // (beyond 64 coordinates: the entry whose points pass through the LDS in chunks)
  ckk((dd <= 64 ? hssk_kernel_predict_f32 : hssk_kernel_predict_f32_wide)(R.ctx, R.dX, (long long)nn, (int)dd, device_type(), degree(),
                                                                          (double)width(), dw, dT, m, dp, st));
  if (out_host) ckk(hssk_memcpy_d2h(R.ctx, out_host, dp, (long long)(sizeof(float) * m)));
  ckk(hssk_sync(R.ctx));
  pstats_[0] = st[0]; pstats_[1] = st[1]; pstats_[2] = st[2]; pstats_[3] = st[3]; pstats_[4] = uploaded; pstats_[5] = resident ? 1 : 0;
}

std::vector<float> Kernel<float>::predict(const DenseMatrix<float>& test, const DenseMatrix<float>& weights) const {
  if (test.rows() != d()) throw std::invalid_argument("predict: test points have the wrong dimension");
  if (weights.rows() != n()) throw std::invalid_argument("predict: one weight per training point expected");
  const int m = int(test.cols());
  std::vector<float> prediction(m, 0.f);
  if (m == 0) return prediction;
  if (device_type() < 0) {
    // a user-defined kernel function: the sums on the host, in float
    for (int c = 0; c < m; c++) {
      float s = 0.f;
      for (std::size_t r = 0; r < n(); r++) s += weights(r, 0) * eval_kernel_function(data_.ptr(0, r), test.ptr(0, c));
      prediction[c] = s;
    }
    return prediction;
  }
  run_predict(m, test.data(), test.ld(), nullptr, weights.data(), prediction.data(), nullptr);
  return prediction;
}

std::vector<float> Kernel<float>::predict(const DenseMatrix<float>& test) const {
  if (test.rows() != d()) throw std::invalid_argument("predict: test points have the wrong dimension");
  if (!fitted()) throw std::invalid_argument("predict: no fit");
  std::vector<float> prediction(test.cols(), 0.f);
  run_predict(int(test.cols()), test.data(), test.ld(), nullptr, nullptr, prediction.data(), nullptr);
  return prediction;
}

int Kernel<float>::predict_device(int m, const float* dtest, float* dpred) const {
  if (!fitted() || m < 0) return 1;
  if (m == 0) return 0;
  if (!hssk_is_device_pointer(dtest) || !hssk_is_device_pointer(dpred)) return 2;
  run_predict(m, nullptr, 0, dtest, nullptr, nullptr, dpred);
  return 0;
}

const long long* last_fit_info() { return last_fit.v; }
const std::vector<int>& last_fit_nodes() { return last_nodes; }

}  // namespace kernel
}  // namespace strumpack

// ---- C interface ---------------------------------------------------------------------------------------
using namespace strumpack;
namespace {
struct KernelRegression {
  int precision = 0;   // the tag of the handle: 0 = double (K, training, weights), 1 = float (Kf, trainingf, weightsf)
  std::unique_ptr<kernel::Kernel<double>> K;
  DenseMatrix<double> training, weights;
  std::unique_ptr<kernel::Kernel<float>> Kf;
  DenseMatrix<float> trainingf, weightsf;
  float* caller_train = nullptr;   // the float caller's array: reordered in place by the fit
  bool any() const { return precision ? bool(Kf) : bool(K); }
  long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int> nodes;   // node table of the last fit (6 ints per node)
};
void report(const std::exception& e) { std::cerr << "Operation failed: " << e.what() << std::endl; }
}  // namespace

extern "C" {

STRUMPACKKernel STRUMPACK_create_kernel_double(int n, int d, double* train, double h, double lambda, int p, int type) {
  try {
    auto kr = new KernelRegression();
    kr->training = DenseMatrix<double>(d, n, train, d);
    switch (type) {
      case 0: kr->K.reset(new kernel::GaussKernel<double>(kr->training, h, lambda)); break;
      case 1: kr->K.reset(new kernel::LaplaceKernel<double>(kr->training, h, lambda)); break;
      case 2: kr->K.reset(new kernel::ANOVAKernel<double>(kr->training, h, lambda, p)); break;
      default: std::cout << "ERROR: Kernel type not recognized!" << std::endl;
    }
    return kr;
  } catch (const std::exception& e) { report(e); return nullptr; }
}
void STRUMPACK_destroy_kernel_double(STRUMPACKKernel K) { delete static_cast<KernelRegression*>(K); }

void STRUMPACK_kernel_fit_HSS_double(STRUMPACKKernel K, double* labels, int argc, char* argv[]) {
  try {
    auto kr = static_cast<KernelRegression*>(K);
    if (!kr || kr->precision != 0 || !kr->K) throw std::invalid_argument("no kernel");
    std::vector<double> vl(labels, labels + kr->K->n());
    HSS::HSSOptions<double> opts;
    opts.set_verbose(false);
    opts.set_clustering_algorithm(ClusteringAlgorithm::COBBLE);   // kernel/Kernel.cpp:82
    opts.set_from_command_line(argc, argv);
    kr->weights = kr->K->fit_HSS(vl, opts);
    std::copy(kernel::last_fit_info(), kernel::last_fit_info() + 8, kr->info);
    kr->nodes = kernel::last_fit_nodes();
  } catch (const std::exception& e) { report(e); }
}
void STRUMPACK_kernel_predict_double(STRUMPACKKernel K, int m, double* test, double* prediction) {
  try {
    auto kr = static_cast<KernelRegression*>(K);
    if (!kr || kr->precision != 0 || !kr->K) throw std::invalid_argument("no kernel");
    DenseMatrix<double> t(kr->K->d(), m, test, kr->K->d());
    auto pred = kr->K->predict(t, kr->weights);
    std::copy(pred.begin(), pred.end(), prediction);
  } catch (const std::exception& e) { report(e); }
}

STRUMPACKKernel STRUMPACK_create_kernel_float(int n, int d, float* train, float h, float lambda, int p, int type) {
  try {
    auto kr = new KernelRegression();
    kr->precision = 1;
    kr->caller_train = train;
    kr->trainingf = DenseMatrix<float>(d, n, train, d);
    switch (type) {
      case 0: kr->Kf.reset(new kernel::GaussKernel<float>(kr->trainingf, h, lambda)); break;
      case 1: kr->Kf.reset(new kernel::LaplaceKernel<float>(kr->trainingf, h, lambda)); break;
      case 2: kr->Kf.reset(new kernel::ANOVAKernel<float>(kr->trainingf, h, lambda, p)); break;
      default: std::cout << "ERROR: Kernel type not recognized!" << std::endl;
    }
    return kr;
  } catch (const std::exception& e) { report(e); return nullptr; }
}
void STRUMPACK_destroy_kernel_float(STRUMPACKKernel K) { delete static_cast<KernelRegression*>(K); }

void STRUMPACK_kernel_fit_HSS_float(STRUMPACKKernel K, float* labels, int argc, char* argv[]) {
  try {
    auto kr = static_cast<KernelRegression*>(K);
    if (!kr || kr->precision != 1 || !kr->Kf) throw std::invalid_argument("no float kernel");
    const std::size_t n = kr->Kf->n(), d = kr->Kf->d();
    std::vector<float> vl(labels, labels + n);
    HSS::HSSOptions<double> opts;   // (the promoted fit's options: tolerances do not pass through a float)
    opts.set_verbose(false);
    opts.set_clustering_algorithm(ClusteringAlgorithm::COBBLE);
    opts.set_from_command_line(argc, argv);
    kr->weightsf = kr->Kf->fit_HSS(vl, opts);
    // the cluster order reaches the caller's arrays, as in the reference (which works on them in place)
    std::copy(vl.begin(), vl.end(), labels);
    if (kr->caller_train) std::copy(kr->trainingf.data(), kr->trainingf.data() + n * d, kr->caller_train);
    std::copy(kernel::last_fit_info(), kernel::last_fit_info() + 8, kr->info);
    kr->nodes = kernel::last_fit_nodes();
  } catch (const std::exception& e) { report(e); }
}
void STRUMPACK_kernel_predict_float(STRUMPACKKernel K, int m, float* test, float* prediction) {
  try {
    auto kr = static_cast<KernelRegression*>(K);
    if (!kr || kr->precision != 1 || !kr->Kf) throw std::invalid_argument("no float kernel");
    DenseMatrix<float> t(kr->Kf->d(), m, test, kr->Kf->d());
    auto pred = kr->Kf->predict(t);
    std::copy(pred.begin(), pred.end(), prediction);
  } catch (const std::exception& e) { report(e); }
}
int SPX_kernel_predict_device_float(STRUMPACKKernel K, int m, const float* dtest, float* dpred) {
  try {
    auto kr = static_cast<KernelRegression*>(K);
    if (!kr || kr->precision != 1 || !kr->Kf) return 1;
    return kr->Kf->predict_device(m, dtest, dpred);
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_predict_stats(STRUMPACKKernel K, long long* out) {
  auto kr = static_cast<KernelRegression*>(K);
  if (!kr || kr->precision != 1 || !kr->Kf) return 1;
  std::copy(kr->Kf->predict_stats(), kr->Kf->predict_stats() + 6, out);
  return 0;
}
int SPX_approximate_neighbors(int n, int d, const double* data, int iterations, int k, int* ann, double* scores) {
  try {
    DenseMatrix<double> p(d, n, data, d);
    DenseMatrix<std::uint32_t> nb;
    DenseMatrix<double> sc;
    find_approximate_neighbors(p, iterations, k, nb, sc);
    for (size_t i = 0; i < (size_t)k * n; i++) { ann[i] = (int)nb.data()[i]; if (scores) scores[i] = sc.data()[i]; }
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_set_neighbors(STRUMPACKKernel K, int k, const int* ann) {
  auto kr = static_cast<KernelRegression*>(K);
  if (!kr || !kr->any()) return 1;
  if (kr->precision) kr->Kf->set_neighbors(ann, k);
  else kr->K->set_neighbors(ann, k);
  return 0;
}
int SPX_kernel_node_info(STRUMPACKKernel K, int* out, int cap) {
  auto kr = static_cast<KernelRegression*>(K);
  if (!kr) return -1;
  int c = (int)kr->nodes.size() / 6;
  std::copy(kr->nodes.begin(), kr->nodes.begin() + 6 * std::min(c, cap), out);
  return c;
}
int SPX_kernel_fit_info(STRUMPACKKernel K, long long* out) {
  auto kr = static_cast<KernelRegression*>(K);
  if (!kr) return 1;
  std::copy(kr->info, kr->info + 8, out);
  return 0;
}
int SPX_kernel_permutation(STRUMPACKKernel K, int* perm) {
  auto kr = static_cast<KernelRegression*>(K);
  if (!kr || !kr->any()) return 1;
  const std::vector<int>& pm = kr->precision ? kr->Kf->permutation() : kr->K->permutation();
  std::copy(pm.begin(), pm.end(), perm);
  return 0;
}
int SPX_kernel_weights(STRUMPACKKernel K, double* w) {
  auto kr = static_cast<KernelRegression*>(K);
  if (kr && kr->precision) {   // the float weights, widened
    if (kr->weightsf.rows() == 0) return 1;
    for (std::size_t i = 0; i < kr->weightsf.rows(); i++) w[i] = (double)kr->weightsf(i, 0);
    return 0;
  }
  if (!kr || kr->weights.rows() == 0) return 1;
  std::copy(kr->weights.data(), kr->weights.data() + kr->weights.rows(), w);
  return 0;
}
// ---- the kept model (double handles, built-in kernels): every call returns non-zero, outputs untouched, without one
namespace {
kernel::Kernel<double>* model_of(STRUMPACKKernel K) {
  auto kr = static_cast<KernelRegression*>(K);
  if (!kr || kr->precision != 0 || !kr->K || kr->K->device_type() < 0 || !kr->K->has_model()) return nullptr;
  return kr->K.get();
}
}  // namespace
int SPX_kernel_keep_model(STRUMPACKKernel K, int keep) {
  try {
    auto kr = static_cast<KernelRegression*>(K);
    if (!kr || kr->precision != 0 || !kr->K || kr->K->device_type() < 0) return 1;
    kr->K->keep_model(keep != 0);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_logabsdet(STRUMPACKKernel K, double* out) {
  try {
    auto k = model_of(K);
    if (!k || !out) return 1;
    const double v = k->logabsdet();
    *out = v;
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_log_marginal_likelihood(STRUMPACKKernel K, double* out) {
  try {
    auto k = model_of(K);
    if (!k || !out) return 1;
    const double v = k->log_marginal_likelihood();
    *out = v;
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_predict_variance_double(STRUMPACKKernel K, int m, const double* test, double* var) {
  try {
    auto k = model_of(K);
    if (!k || m < 0 || (m > 0 && (!test || !var))) return 1;
    DenseMatrix<double> t(k->d(), m, test, k->d());
    const std::vector<double> v = k->predict_variance(t);
    std::copy(v.begin(), v.end(), var);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_variance_ms(STRUMPACKKernel K, double* out) {
  auto k = model_of(K);
  if (!k || !out) return 1;
  std::copy(k->variance_ms(), k->variance_ms() + 3, out);
  return 0;
}
int SPX_kernel_model_set_lambda(STRUMPACKKernel K, double lambda) {
  try {
    auto k = model_of(K);
    if (!k) return 1;
    static_cast<KernelRegression*>(K)->weights = k->model_set_lambda(lambda);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_model_write(STRUMPACKKernel K, const char* path) {
  try {
    auto k = model_of(K);
    if (!k || !path) return 1;
    k->model_write(path);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_model_labels(STRUMPACKKernel K, double* y) {
  try {
    auto k = model_of(K);
    if (!k || !y) return 1;
    std::copy(k->model_labels().begin(), k->model_labels().end(), y);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_model_points(STRUMPACKKernel K, double* x) {
  try {
    auto k = model_of(K);
    if (!k || !x) return 1;
    for (std::size_t i = 0; i < k->n(); i++) std::copy(k->data().ptr(0, i), k->data().ptr(0, i) + k->d(), x + i * k->d());
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}

int SPX_kernel_lml_gradient(STRUMPACKKernel K, int m, const double* Z, unsigned long long seed, double grad[2], double* terms) {
  try {
    auto k = model_of(K);
    if (!k || m < 1 || !grad) return 1;
    const kernel::LmlGradient g = Z ? k->log_marginal_likelihood_gradient(DenseMatrix<double>(k->n(), m, Z, k->n()))
                                    : k->log_marginal_likelihood_gradient(m, seed);
    grad[0] = g.dh;
    grad[1] = g.dlambda;
    if (terms) {
      terms[0] = g.quad_h; terms[1] = g.quad_lambda; terms[2] = g.trace_h; terms[3] = g.trace_lambda;
      std::copy(g.th.begin(), g.th.end(), terms + 4);
      std::copy(g.tl.begin(), g.tl.end(), terms + 4 + m);
    }
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_lml_gradient_coords(STRUMPACKKernel K, int m, const double* Z, unsigned long long seed, double* grad, double* terms) {
  try {
    auto k = model_of(K);
    if (!k || m < 1 || !grad) return 1;
    const kernel::LmlGradientCoords g = Z ? k->log_marginal_likelihood_gradient_coords(DenseMatrix<double>(k->n(), m, Z, k->n()))
                                          : k->log_marginal_likelihood_gradient_coords(m, seed);
    const std::size_t dim = k->d();
    std::copy(g.dtheta.begin(), g.dtheta.end(), grad);
    if (terms) {
      std::copy(g.quad.begin(), g.quad.end(), terms);
      std::copy(g.trace.begin(), g.trace.end(), terms + dim);
      std::copy(g.tc.begin(), g.tc.end(), terms + 2 * dim);
    }
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_model_probes(STRUMPACKKernel K, int m, unsigned long long seed, double* Z) {
  try {
    auto k = model_of(K);
    if (!k || m < 1 || !Z) return 1;
    const DenseMatrix<double> P = k->model_probes(m, seed);
    for (int c = 0; c < m; c++) std::copy(P.ptr(0, c), P.ptr(0, c) + k->n(), Z + (size_t)c * k->n());
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_model_residual(STRUMPACKKernel K, double* out) {
  try {
    auto k = model_of(K);
    if (!k || !out) return 1;
    const double v = k->model_residual();
    *out = v;
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_gradient_ms(STRUMPACKKernel K, double* out) {
  auto k = model_of(K);
  if (!k || !out) return 1;
  std::copy(k->gradient_ms(), k->gradient_ms() + 3, out);
  return 0;
}

// ---- solves with the exact kernel matrix ----
namespace {
// info: 8 + 2 m doubles (include/kernel/Kernel.h)
void krylov_info_out(const kernel::KrylovInfo& I, double* info) {
  if (!info) return;
  const std::size_t m = I.its.size();
  info[0] = I.converged ? 1. : 0.; info[1] = I.iterations; info[2] = (double)I.products; info[3] = (double)I.solves; info[4] = (double)I.cycles;
  info[5] = m ? *std::max_element(I.residual0.begin(), I.residual0.end()) : 0.;
  info[6] = m ? *std::max_element(I.residual.begin(), I.residual.end()) : 0.;
  info[7] = (double)m;
  std::copy(I.residual.begin(), I.residual.end(), info + 8);
  for (std::size_t c = 0; c < m; c++) info[8 + m + c] = I.its[c];
}
}  // namespace
int SPX_kernel_model_refine(STRUMPACKKernel K, double rtol, int maxit, int restart, double* info) {
  try {
    auto k = model_of(K);
    if (!k) return 1;
    const kernel::KrylovInfo I = k->model_refine(rtol, maxit, restart);
    static_cast<KernelRegression*>(K)->weights = k->model_weights();
    krylov_info_out(I, info);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_model_solve(STRUMPACKKernel K, int m, const double* B, int ldb, double* X, int ldx, double rtol, int maxit, int restart,
                           double* info) {
  try {
    auto k = model_of(K);
    if (!k || m < 0 || (m > 0 && (!B || !X || ldb < (int)k->n() || ldx < (int)k->n()))) return 1;
    kernel::KrylovInfo I;
    const DenseMatrix<double> S = k->model_solve(DenseMatrix<double>(k->n(), m, B, ldb), &I, rtol, maxit, restart);
    for (int c = 0; c < m; c++) std::copy(S.ptr(0, c), S.ptr(0, c) + k->n(), X + (size_t)c * ldx);
    krylov_info_out(I, info);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_predict_variance_exact_double(STRUMPACKKernel K, int m, const double* test, double* var, double rtol, int maxit, int restart,
                                             double* info) {
  try {
    auto k = model_of(K);
    if (!k || m < 0 || (m > 0 && (!test || !var))) return 1;
    kernel::KrylovInfo I;
    DenseMatrix<double> t(k->d(), m, test, k->d());
    const std::vector<double> v = k->predict_variance_exact(t, &I, rtol, maxit, restart);
    std::copy(v.begin(), v.end(), var);
    krylov_info_out(I, info);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_set_krylov_inner(STRUMPACKKernel K, int precision, double inner_rtol) {
  try {
    auto kr = static_cast<KernelRegression*>(K);
    if (!kr || kr->precision != 0 || !kr->K || kr->K->device_type() < 0) return 1;
    if (precision != 0 && precision != 1) return 1;
    if (std::isnan(inner_rtol)) return 1;
    kr->K->krylov_inner(precision ? kernel::KrylovInner::FP32 : kernel::KrylovInner::FP64,
                        inner_rtol <= 0. ? kernel::KRYLOV_INNER_RTOL_DEFAULT : inner_rtol);
    return 0;
  } catch (const std::exception& e) { report(e); return 1; }
}
int SPX_kernel_krylov_inner(STRUMPACKKernel K, int* precision, double* inner_rtol) {
  auto kr = static_cast<KernelRegression*>(K);
  if (!kr || kr->precision != 0 || !kr->K || kr->K->device_type() < 0) return 1;
  if (precision) *precision = kr->K->krylov_inner() == kernel::KrylovInner::FP32 ? 1 : 0;
  if (inner_rtol) *inner_rtol = kr->K->krylov_inner_rtol();
  return 0;
}
int SPX_kernel_krylov_stats(STRUMPACKKernel K, double out[6]) {
  auto k = model_of(K);
  if (!k || !out || (k->device_type() != 0 && k->device_type() != 1)) return 1;
  std::copy(k->krylov_stats(), k->krylov_stats() + 6, out);
  return 0;
}
int SPX_kernel_krylov_ms(STRUMPACKKernel K, double out[3]) {
  auto k = model_of(K);
  if (!k || !out || (k->device_type() != 0 && k->device_type() != 1)) return 1;   // (ANOVA: none of the three calls exists)
  std::copy(k->krylov_ms(), k->krylov_ms() + 3, out);
  return 0;
}

int SPX_clustering(int n, int d, double* data, int algo, int leaf_size, int* perm, int* leaf_sizes, int cap) {
  try {
    DenseMatrix<double> p(d, n, data, d);
    std::vector<int> pm;
    static const ClusteringAlgorithm algos[] = {ClusteringAlgorithm::NATURAL, ClusteringAlgorithm::TWO_MEANS, ClusteringAlgorithm::KD_TREE,
                                                ClusteringAlgorithm::PCA, ClusteringAlgorithm::COBBLE};
    if (algo < 0 || algo > 4) throw std::invalid_argument("clustering algorithm out of range");
    auto t = binary_tree_clustering(algos[algo], p, pm, leaf_size);
    std::copy(p.data(), p.data() + (size_t)d * n, data);
    std::copy(pm.begin(), pm.end(), perm);
    int c = 0;
    std::function<void(const structured::ClusterTree&)> walk = [&](const structured::ClusterTree& nd) {
      if (nd.c.empty()) { if (c < cap) leaf_sizes[c] = nd.size; c++; }
      else for (auto& ch : nd.c) walk(ch);
    };
    walk(t);
    return c;
  } catch (const std::exception& e) { report(e); return -1; }
}

int SPX_clustering_device(int n, int d, double* data, int algo, int leaf_size, int* perm, int* leaf_sizes, int cap, int* status) {
  try {
    DenseMatrix<double> p(d, n, data, d);
    std::vector<int> pm;
    static const ClusteringAlgorithm algos[] = {ClusteringAlgorithm::NATURAL, ClusteringAlgorithm::TWO_MEANS, ClusteringAlgorithm::KD_TREE,
                                                ClusteringAlgorithm::PCA, ClusteringAlgorithm::COBBLE};
    if (algo < 0 || algo > 4) throw std::invalid_argument("clustering algorithm out of range");
    int dev = 0;
    if (const char* e = std::getenv("STRUMPACK_AMD_DEVICE")) dev = std::atoi(e);
    structured::ClusterTree t(0);
    const int st = binary_tree_clustering_device(algos[algo], p, pm, (std::size_t)leaf_size, dev, t);
    if (status) *status = st;
    if (st) return 0;
    std::copy(p.data(), p.data() + (size_t)d * n, data);
    std::copy(pm.begin(), pm.end(), perm);
    int c = 0;
    std::function<void(const structured::ClusterTree&)> walk = [&](const structured::ClusterTree& nd) {
      if (nd.c.empty()) { if (c < cap) leaf_sizes[c] = nd.size; c++; }
      else for (auto& ch : nd.c) walk(ch);
    };
    walk(t);
    return c;
  } catch (const std::exception& e) { report(e); return -1; }
}

}  // extern "C"
