/*!
 * \file src/gpu/optim_kernels.hip
 * \brief L1: a fused optimizer step on the touched rows of a parameter table
 *  (lazy AdaGrad / FTRL-Proximal for row-sparse minibatch steps).
 *
 *  param and every state tensor are row-major [features x width] f32; grad is
 *  [nrows x width], row u belonging to table row ids[u] (ids == nullptr: row
 *  u, the dense identity).  ids are strictly ascending, so every element of
 *  the table has one owner: no atomics, and the same inputs give the same
 *  bytes.  A row whose id is >= features, or is not strictly between its
 *  neighbours' ids, is skipped (no address is formed from it) and sets
 *  kLazyErrIds.  Rows not named in ids are neither read nor written.
 *
 *  One thread per (row, 4 columns) with 16-byte accesses when width % 4 == 0
 *  and all tensors are 16-byte aligned, else one thread per element.  The
 *  arithmetic is written out step by step and compiled with -ffp-contract=off:
 *
 *  adagrad (lr, eps, l2), state n:
 *      g' = g + l2 * w;  n += g' * g';  w -= lr * g' / (sqrt(n) + eps)
 *  ftrl (alpha, beta, l1, l2), state z, n:
 *      s = (sqrt(n + g * g) - sqrt(n)) / alpha;  z += g - s * w;  n += g * g
 *      w = |z| <= l1 ? 0 : -(z - sign(z) * l1) / ((beta + sqrt(n)) / alpha + l2)
 */
#include <dmlc/gpu/hip_utils.h>
#include <dmlc/logging.h>
#include <hip/hip_runtime.h>

#include "./kernels.h"
#include "./launch_common.h"

namespace dmlc {
namespace gpu {

namespace {
constexpr int kThreads = 256;

template <int kRule>
__device__ __forceinline__ void update_one(float g, const LazyHyper& h, float* w, float* s0,
                                           float* s1) {
  if constexpr (kRule == kLazyAdagrad) {
    const float lr = h.a, eps = h.b, l2 = h.c;
    const float gp = g + l2 * *w;
    const float n = *s0 + gp * gp;
    *s0 = n;
    *w = *w - lr * gp / (sqrtf(n) + eps);
  } else {
    const float alpha = h.a, beta = h.b, l1 = h.c, l2 = h.d;
    const float n0 = *s1;
    const float gg = g * g;
    const float s = (sqrtf(n0 + gg) - sqrtf(n0)) / alpha;
    const float z = *s0 + (g - s * *w);
    const float n = n0 + gg;
    *s0 = z;
    *s1 = n;
    if (fabsf(z) <= l1) {
      *w = 0.0f;
    } else {
      const float sl1 = z < 0.0f ? -l1 : l1;
      *w = -(z - sl1) / ((beta + sqrtf(n)) / alpha + l2);
    }
  }
}

/*! \brief the table row of grad row u, or false (flagged) if it may not be touched */
__device__ __forceinline__ bool owner_row(const int64_t* __restrict__ ids, uint64_t u,
                                          uint64_t nrows, uint64_t features, uint64_t* row) {
  if (ids == nullptr) {
    *row = u;
    return u < features;
  }
  const uint64_t id = static_cast<uint64_t>(ids[u]);  // a negative id is huge
  *row = id;
  if (id >= features) return false;
  if (u > 0 && static_cast<uint64_t>(ids[u - 1]) >= id) return false;
  if (u + 1 < nrows && static_cast<uint64_t>(ids[u + 1]) <= id) return false;
  return true;
}

template <int kRule, int kVec>
__global__ __launch_bounds__(kThreads) void k_lazy_update(
    float* __restrict__ param, const int64_t* __restrict__ ids, const float* __restrict__ grad,
    float* __restrict__ state0, float* __restrict__ state1, uint64_t features, uint64_t nrows,
    uint64_t width, LazyHyper h, uint32_t* error) {
  const uint64_t per_row = width / kVec;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (t >= nrows * per_row) return;
  const uint64_t u = t / per_row, c = (t - u * per_row) * kVec;
  uint64_t row;
  if (!owner_row(ids, u, nrows, features, &row)) {
    if (c == 0) atomicOr(error, kLazyErrIds);  // the status word, not an output
    return;
  }
  const uint64_t at = row * width + c;
  if constexpr (kVec == 4) {
    const float4 g4 = *reinterpret_cast<const float4*>(grad + u * width + c);
    float4 w4 = *reinterpret_cast<const float4*>(param + at);
    float4 a4 = *reinterpret_cast<const float4*>(state0 + at);
    float4 b4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (kRule == kLazyFtrl) b4 = *reinterpret_cast<const float4*>(state1 + at);
    update_one<kRule>(g4.x, h, &w4.x, &a4.x, &b4.x);
    update_one<kRule>(g4.y, h, &w4.y, &a4.y, &b4.y);
    update_one<kRule>(g4.z, h, &w4.z, &a4.z, &b4.z);
    update_one<kRule>(g4.w, h, &w4.w, &a4.w, &b4.w);
    *reinterpret_cast<float4*>(param + at) = w4;
    *reinterpret_cast<float4*>(state0 + at) = a4;
    if constexpr (kRule == kLazyFtrl) *reinterpret_cast<float4*>(state1 + at) = b4;
  } else {
    float w = param[at], a = state0[at], b = 0.0f;
    if constexpr (kRule == kLazyFtrl) b = state1[at];
    update_one<kRule>(grad[u * width + c], h, &w, &a, &b);
    param[at] = w;
    state0[at] = a;
    if constexpr (kRule == kLazyFtrl) state1[at] = b;
  }
}
}  // namespace

void LaunchLazyUpdate(int rule, float* param, const int64_t* ids, const float* grad,
                      float* state0, float* state1, uint64_t features, uint64_t nrows,
                      uint64_t width, const LazyHyper& hyper, uint32_t* error,
                      hipStream_t stream) {
  CHECK(rule == kLazyAdagrad || rule == kLazyFtrl) << "lazy update: unknown rule " << rule;
  if (nrows == 0 || width == 0) return;
  CHECK(param != nullptr && grad != nullptr && state0 != nullptr && error != nullptr &&
        (rule != kLazyFtrl || state1 != nullptr))
      << "lazy update: a tensor is missing";
  CHECK(ids != nullptr || nrows <= features) << "lazy update: more rows than the table has";
  const bool vec = width % 4 == 0 && Aligned16(param) && Aligned16(grad) && Aligned16(state0) &&
                   (rule != kLazyFtrl || Aligned16(state1));
  const uint64_t per_row = vec ? width / 4 : width;
  CHECK_LE(nrows, ((1ull << 31) - 1) * kThreads / per_row)
      << "lazy update: too many elements for one launch";
  const uint64_t blocks = (nrows * per_row + kThreads - 1) / kThreads;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0, stream,
                       param, ids, grad, state0, state1, features, nrows, width, hyper, error);
  };
  if (rule == kLazyAdagrad) {
    vec ? launch(k_lazy_update<kLazyAdagrad, 4>) : launch(k_lazy_update<kLazyAdagrad, 1>);
  } else {
    vec ? launch(k_lazy_update<kLazyFtrl, 4>) : launch(k_lazy_update<kLazyFtrl, 1>);
  }
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
