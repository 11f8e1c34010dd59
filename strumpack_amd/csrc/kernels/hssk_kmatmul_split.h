// The split of the training points and the reduction of the split partials, shared by the three exact kernel-matrix products
// (hssk_kernel_matmul, hssk_kernel_matmul_coord, hssk_kernel_matmul_f32).  Host code only.
#pragma once
#include <algorithm>

#include "hssk_internal.h"

namespace {

// s splits of per training points each: whole stages, none empty.  stage: training points per stage of the kernel; requested:
// the caller's count (0: the automatic one)
struct KmSplit { long long s, per; };
inline KmSplit km_split_plan(long long n, int stage, int requested, int automatic) {
  const long long stages = (n + stage - 1) / stage;
  const long long s = std::min<long long>(requested > 0 ? requested : automatic, std::min<long long>(stages, 65535));
  const long long per = ((stages + s - 1) / s) * stage;
  return {(n + per - 1) / per, per};
}

// out (leading dimension ldo) = the sum of the s slabs of n x nc partials (leading dimension n) from part on: the partials in split
// order; a padded output one column at a time
inline int km_reduce_splits(hssk_ctx* ctx, const double* part, long long n, int nc, int s, double* out, long long ldo) {
  const long long slab = n * nc;
  if (ldo == n) return hssk_sum_slabs(ctx, part, slab, slab, s, out);
  for (int c = 0; c < nc; c++)
    if (const int rc = hssk_sum_slabs(ctx, part + (size_t)c * n, n, slab, s, out + (size_t)c * ldo)) return rc;
  return 0;
}

}  // namespace
