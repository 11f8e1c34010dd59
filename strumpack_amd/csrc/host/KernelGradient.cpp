// Kernel<double>: the gradients of the log marginal likelihood and the residual of the fit against the exact kernel matrix, from the
// kept model.
#include <random>

#include "KernelModel.hpp"

namespace strumpack {
namespace kernel {

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

// what both gradients ask of their probes Z (and of d() where dmax is given), and of m before they draw model_probes(m, seed)
const Kernel<double>::Model& Kernel<double>::check_probes(const char* what, const DenseMatrix<double>& Z, std::size_t dmax) const {
  const Model& M = model(what);
  require_exact_products(*this, what);
  if (dmax && d() > dmax) throw std::invalid_argument(std::string(what) + ": at most " + std::to_string(dmax) + " coordinates");
  if (Z.cols() < 1) throw std::invalid_argument(std::string(what) + ": at least one probe vector");
  if (Z.rows() != n()) throw std::invalid_argument(std::string(what) + ": one probe row per training point expected (cluster order)");
  return M;
}
DenseMatrix<double> Kernel<double>::seeded_probes(const char* what, int m, unsigned long long seed) const {
  model(what);
  if (m < 1) throw std::invalid_argument(std::string(what) + ": at least one probe vector");
  return model_probes(m, seed);
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
  watched(ctx, 2, [&] { M.H.solve_device(nc, dS, nn); });
  return {nc, lead, z0};
}
}  // namespace

LmlGradient Kernel<double>::log_marginal_likelihood_gradient(int m, unsigned long long seed) const {
  return log_marginal_likelihood_gradient(seeded_probes("log_marginal_likelihood_gradient", m, seed));
}

LmlGradient Kernel<double>::log_marginal_likelihood_gradient(const DenseMatrix<double>& Z) const {
  const Model& M = check_probes("log_marginal_likelihood_gradient", Z);
  const int m = int(Z.cols()), CH = 64;
  const long long nn = (long long)n();
  hssk_ctx* ctx = M.ctx();
  grad_ms_[0] = grad_ms_[1] = grad_ms_[2] = 0.;
  // B: alpha | the probes, S = H^-1 B, G = K' B; the dots of a block: [0, 64) S.G, [64, 128) S.B, [128] alpha.G(:, 0)
  PoolBuf bB(ctx, sizeof(double) * nn * CH), bS(ctx, sizeof(double) * nn * CH), bG(ctx, sizeof(double) * nn * CH), bD(ctx, sizeof(double) * (2 * CH + 1));
  double *dB = (double*)bB.p, *dS = (double*)bS.p, *dG = (double*)bG.p, *dD = (double*)bD.p;
  const hssk_kernel_spec spec = kept_spec(*this, M.dX, 0.);
  LmlGradient g;
  g.th.assign(m, 0.);
  g.tl.assign(m, 0.);
  std::vector<double> dots(2 * CH + 1, 0.);
  double aga = 0.;
  for (int c0 = 0; c0 < m + 1; c0 += CH) {   // column c of alpha | Z
    const GradBlock b = grad_block(M, Z, c0, CH, dB, dS);
    const int nc = b.nc, lead = b.lead, z0 = b.z0;
    watched(ctx, 1, [&] { ckk(hssk_kernel_matmul(ctx, &spec, 1, dB, nn, nc, dG, nn, 0)); });
    watched(ctx, 3, [&] {
      ckk(hssk_coldots(ctx, dS, nn, dG, nn, nn, nc, dD));
      ckk(hssk_coldots(ctx, dS, nn, dB, nn, nn, nc, dD + CH));
      if (lead) ckk(hssk_coldots(ctx, dB, nn, dG, nn, nn, 1, dD + 2 * CH));
    });
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
  return log_marginal_likelihood_gradient_coords(seeded_probes("log_marginal_likelihood_gradient_coords", m, seed));
}

LmlGradientCoords Kernel<double>::log_marginal_likelihood_gradient_coords(const DenseMatrix<double>& Z) const {
  const char* what = "log_marginal_likelihood_gradient_coords";
  const Model& M = check_probes(what, Z, 64);
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
  const hssk_kernel_spec spec = kept_spec(*this, M.dX, 0.);
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
      watched(ctx, 1, [&] { ckk(hssk_kernel_matmul_coord(ctx, &spec, j0, nj, dB, nn, nc, dG, nn, (long long)blk, 0)); });
      watched(ctx, 3, [&] {
        for (int jj = 0; jj < nj; jj++) {
          ckk(hssk_coldots(ctx, dS, nn, dG + jj * blk, nn, nn, nc, dD + (size_t)(j0 + jj) * CH));
          if (lead) ckk(hssk_coldots(ctx, dB, nn, dG + jj * blk, nn, nn, 1, dD + (size_t)dim * CH + j0 + jj));
        }
      });
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
  require_exact_products(*this, "model_residual");
  const long long nn = (long long)n();
  hssk_ctx* ctx = M.ctx();
  PoolBuf bB(ctx, sizeof(double) * nn), bG(ctx, sizeof(double) * nn);
  const hssk_kernel_spec spec = kept_spec(*this, M.dX, lambda_);
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

}  // namespace kernel
}  // namespace strumpack
