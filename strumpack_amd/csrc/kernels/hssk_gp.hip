// What a Gaussian-process reading of kernel ridge regression needs beyond the fit: the log-determinant of the factored matrix
// and, per test point, the cross-kernel column and its product with the solved column (the predictive variance).
//
// hssk_kernel_cross / hssk_kernel_predict_cols are the prediction kernels of hssk_kpair.h in their other two modes: the pair
// arithmetic and the order of every sum are those of hssk_kernel_predict.
//
// log|det| of a batch of triangular factors (hssk_logabsdet_vbatched): partial[k] = sum_{i < n} log|A_k(i, i)| and the sum of
// the partials.  The ULV factorization of an HSS matrix keeps its determinant on the diagonals of the triangles it eliminates
// with (the transposed L of every node's LQ, the root's LU); DeviceHSS::logabsdet (host/hss_factor.cpp) lists them here.
//
// One wave per descriptor: lane l adds the logarithms of the diagonal entries l, l + 64, ... in that order (a strided gather:
// one 8-byte load per entry, n / 64 dependent logarithms per lane), the 64 lane sums are added on the DPP network.  A second
// launch of one wave adds the partials strictly in index order: 64 at a time are loaded by the lanes and read back lane by lane
// through scalar registers.  No atomics, every order fixed: the result is bitwise repeatable.  What IEEE gives is what comes
// out: a zero on a diagonal makes its partial and the total -inf, a NaN stays a NaN.
#include "hssk_device.h"
#include "hssk_internal.h"
#include "hssk_kpair.h"

namespace {

__global__ __launch_bounds__(64) void logabsdet_kernel(const hssk_logdet_desc* __restrict__ descs, double* __restrict__ partial) {
  const hssk_logdet_desc p = descs[blockIdx.x];
  const int lane = threadIdx.x;
  double s = 0.;
  for (int i = lane; i < p.n; i += 64) s += log(fabs(hssk_gload(p.A, (size_t)i * p.lda + i)));
  s = hssk_wave_sum(s);   // (every lane takes part, also those without an entry)
  if (lane == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void logabsdet_total_kernel(const double* __restrict__ partial, int count, double* __restrict__ out) {
  const int lane = threadIdx.x;
  double s = 0.;
  for (int k0 = 0; k0 < count; k0 += 64) {
    const double v = k0 + lane < count ? partial[k0 + lane] : 0.;
    const int top = min(64, count - k0);
    for (int j = 0; j < top; j++) s += hssk_bcast_lane(v, j);   // (the same sum in every lane)
  }
  if (lane == 0) out[0] = s;
}

// the kernel of hssk_kpair.h for this spec in mode MODE; w / ldw: the weight columns (PR_COLS), out / ldo: the block (PR_CROSS) or
// the m sums (PR_COLS)
template <int MODE>
int gp_launch(hssk_ctx* ctx, const char* who, const hssk_kernel_spec* spec, const double* w, size_t ldw, const double* T, int m, double* out,
              size_t ldo) {
  if (!ctx || !spec) throw std::invalid_argument(std::string(who) + ": no context or kernel");
  if (m < 0) throw std::invalid_argument(std::string(who) + ": negative test point count");
  if (m == 0) return 0;
  check_spec(*spec);
  if (!T || !out) throw std::invalid_argument(std::string(who) + ": null pointer");
  if (spec->n > 0 && MODE == PR_COLS && !w) throw std::invalid_argument(std::string(who) + ": null pointer");
  if (spec->n > 0 && (MODE == PR_COLS ? ldw : ldo) < (size_t)spec->n) throw std::invalid_argument(std::string(who) + ": leading dimension below the training point count");
  const bool wide = spec->d > PR_DMAX;
  if ((wide ? PR_LDS_WIDE : PR_LDS_POINT) > hssk_rt::max_lds_per_workgroup()) {
    hssk_set_error(std::string(who) + ": the point tiles do not fit the LDS of this device");
    return 2;
  }
  const dim3 grid((unsigned)((m + PR_T - 1) / PR_T));
  const bool matern = spec->type >= 3;
  if (!wide && matern) HSSK_LAUNCH((kernel_predict_kernel<MODE, true>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (!wide) HSSK_LAUNCH((kernel_predict_kernel<MODE>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 3) HSSK_LAUNCH((kernel_predict_wide_kernel<3, 32, MODE>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 4) HSSK_LAUNCH((kernel_predict_wide_kernel<4, 32, MODE>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 0) HSSK_LAUNCH((kernel_predict_wide_kernel<0, 32, MODE>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else if (spec->type == 1) HSSK_LAUNCH((kernel_predict_wide_kernel<1, 32, MODE>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  else HSSK_LAUNCH((kernel_predict_wide_kernel<2, 8, MODE>), grid, dim3(PR_T), 0, ctx->stream, *spec, w, ldw, T, m, out, ldo);
  hssk_rt::check_launch();
  return 0;
}

}  // namespace

extern "C" int hssk_kernel_cross(hssk_ctx* ctx, const hssk_kernel_spec* spec, const double* T, int m, double* out, long long ldo) {
  HSSK_API_BEGIN
  if (ldo < 0) throw std::invalid_argument("hssk_kernel_cross: negative leading dimension");
  if (const int rc = gp_launch<PR_CROSS>(ctx, "hssk_kernel_cross", spec, nullptr, 0, T, m, out, (size_t)ldo)) return rc;
  HSSK_API_END
}

extern "C" int hssk_kernel_predict_cols(hssk_ctx* ctx, const hssk_kernel_spec* spec, const double* W, long long ldw, const double* T, int m,
                                        double* pred) {
  HSSK_API_BEGIN
  if (ldw < 0) throw std::invalid_argument("hssk_kernel_predict_cols: negative leading dimension");
  if (const int rc = gp_launch<PR_COLS>(ctx, "hssk_kernel_predict_cols", spec, W, (size_t)ldw, T, m, pred, 0)) return rc;
  HSSK_API_END
}

extern "C" int hssk_logabsdet_vbatched(hssk_ctx* ctx, const hssk_logdet_desc* descs, int count, double* partial, double* out) {
  HSSK_API_BEGIN
  if (!ctx) throw std::invalid_argument("hssk_logabsdet_vbatched: no context");
  if (count < 0) throw std::invalid_argument("hssk_logabsdet_vbatched: negative count");
  if (!out || (count > 0 && (!descs || !partial))) throw std::invalid_argument("hssk_logabsdet_vbatched: null pointer");
  for (int k = 0; k < count; k++)
    if (descs[k].n < 0 || descs[k].lda < std::max(descs[k].n, 1) || (descs[k].n > 0 && !descs[k].A))
      throw std::invalid_argument("hssk_logabsdet_vbatched: descriptor " + std::to_string(k) + " needs n >= 0, lda >= max(n, 1) and a matrix");
  if (count > 0) {
    auto* dd = (const hssk_logdet_desc*)ctx->stage(descs, sizeof(*descs) * count);
    HSSK_LAUNCH(logabsdet_kernel, dim3((unsigned)count), dim3(64), 0, ctx->stream, dd, partial);
  }
  HSSK_LAUNCH(logabsdet_total_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double*)partial, count, out);
  hssk_rt::check_launch();
  HSSK_API_END
}
