/*!
 * \file src/gpu/spmm_kernels.hip
 * \brief M1 / M1p CSR x dense SpMM and M2 its transposed, atomic form (f32).
 *
 * M1  Y[r, :] = sum_j value[j] * W[index[j], :] (+ bias)      k_spmm<Unit, CsrEntries>
 * M1p the same over interleaved (u32 index, f32 value) pairs   k_spmm<Unit, PairEntries>
 * M2  G[index[j], :] += value[j] * D[r, :]  (no-return atomics) k_spmm_t
 *
 * Slots layout.  A row belongs to a group of `group` lanes (16, 32 or 64, so
 * 16, 8 or 4 rows per 256-thread workgroup); the group is split into entry
 * slots times column lanes: `cpr` consecutive lanes share one W row, each
 * holding one Unit of it (float4 through one 16-byte load when k % 4 == 0,
 * else one float), and group / cpr entries are in flight at once.  cpr =
 * min(64, next_pow2(k / 4 or k)); group = clamp(4 cpr, 16, 64): the survey's
 * rows carry 20-60 entries, so small k shares a wave between four rows as K11
 * does.  More than 64 units (scalar k > 64) take further column passes over
 * the row.  Every lane sums its slot's entries j = b + slot, b + slot + slots,
 * ... in that order, the slots are then folded by __shfl_xor from the widest
 * distance down: the summation order depends on k alone, there are no
 * atomics in M1 / M1p, and the output bytes are a pure function of the
 * inputs.  value == nullptr is a template parameter, not a branch in the loop.
 *
 * M2 always uses the one-float-per-lane layout: the cpr lanes of one entry
 * then cover one contiguous 4 * min(k, 64)-byte segment of a G row in every
 * atomic wave-instruction (MI355X_MICROARCH.md, Global float atomics).
 */
#include <dmlc/gpu/hip_utils.h>
#include <dmlc/logging.h>
#include <hip/hip_runtime.h>

#include "./device_common.h"
#include "./kernels.h"
#include "./launch_common.h"

namespace dmlc {
namespace gpu {

namespace {
constexpr int kThreads = 256;

/*! \brief entries of a CSR with separate index / value arrays */
template <typename IndexType, bool kHasValue>
struct CsrEntries {
  const IndexType* __restrict__ index;
  const float* __restrict__ value;
  __device__ __forceinline__ void Load(uint64_t j, size_t* idx, float* v) const {
    *idx = static_cast<size_t>(index[j]);
    *v = kHasValue ? value[j] : 1.0f;
  }
};

/*! \brief entries of a transpose: one 8-byte (u32 index, f32 value) load each */
struct PairEntries {
  const uint2* __restrict__ iv;
  __device__ __forceinline__ void Load(uint64_t j, size_t* idx, float* v) const {
    const uint2 p = iv[j];
    *idx = p.x;
    *v = __uint_as_float(p.y);
  }
};

// the two units a lane can hold: one column (4-byte loads) or a column quad (16-byte loads)
__device__ __forceinline__ float Zero(const float*) { return 0.0f; }
__device__ __forceinline__ float4 Zero(const float4*) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void Fma(float v, float w, float* acc) { *acc = fmaf(v, w, *acc); }
__device__ __forceinline__ void Fma(float v, const float4& w, float4* acc) {
  acc->x = fmaf(v, w.x, acc->x);
  acc->y = fmaf(v, w.y, acc->y);
  acc->z = fmaf(v, w.z, acc->z);
  acc->w = fmaf(v, w.w, acc->w);
}
__device__ __forceinline__ void Add(const float& o, float* acc) { *acc += o; }
__device__ __forceinline__ void Add(const float4& o, float4* acc) {
  acc->x += o.x;
  acc->y += o.y;
  acc->z += o.z;
  acc->w += o.w;
}
__device__ __forceinline__ float ShflXor(float v, int d) { return __shfl_xor(v, d, dev::kWave); }
__device__ __forceinline__ float4 ShflXor(const float4& v, int d) {
  return make_float4(__shfl_xor(v.x, d, dev::kWave), __shfl_xor(v.y, d, dev::kWave),
                     __shfl_xor(v.z, d, dev::kWave), __shfl_xor(v.w, d, dev::kWave));
}

/*!
 * \brief M1 / M1p.  units = k / 4 (Unit = float4) or k (Unit = float); cpr and
 *  group are powers of two, cpr <= group <= 64, kThreads % group == 0.  All
 *  lanes of a group run the same row and the same column pass, so every
 *  shuffle partner (xor distance < group) is active.
 */
template <typename Unit, typename Entries>
__global__ __launch_bounds__(kThreads) void k_spmm(const uint64_t* __restrict__ offset,
                                                   const Entries src, size_t nrows,
                                                   const float* __restrict__ w,
                                                   const float* __restrict__ bias, int units,
                                                   int cpr, int group, float* __restrict__ y) {
  const int in_group = threadIdx.x & (group - 1);
  const int col = in_group & (cpr - 1);
  const int slot = in_group / cpr;
  const int slots = group / cpr;
  const size_t per_block = kThreads / group;
  const size_t stride = static_cast<size_t>(gridDim.x) * per_block;
  const Unit* __restrict__ wu = reinterpret_cast<const Unit*>(w);
  const Unit* __restrict__ bu = reinterpret_cast<const Unit*>(bias);
  Unit* __restrict__ yu = reinterpret_cast<Unit*>(y);
  for (size_t r = blockIdx.x * per_block + threadIdx.x / group; r < nrows; r += stride) {
    const uint64_t b = offset[r], e = offset[r + 1];
    for (int c0 = 0; c0 < units; c0 += cpr) {
      const int c = c0 + col;
      const bool live = c < units;
      Unit acc = Zero(static_cast<const Unit*>(nullptr));
      if (live) {
#pragma unroll 2
        for (uint64_t j = b + slot; j < e; j += slots) {
          size_t idx;
          float v;
          src.Load(j, &idx, &v);
          Fma(v, wu[idx * units + c], &acc);
        }
      }
      for (int d = group >> 1; d >= cpr; d >>= 1) Add(ShflXor(acc, d), &acc);
      if (live && slot == 0) {
        if (bu != nullptr) Add(bu[c], &acc);
        yu[r * units + c] = acc;
      }
    }
  }
}

/*! \brief M2: one float per lane; the cpr lanes of an entry add one contiguous
 *  segment of a G row per wave-instruction */
template <typename IndexType, bool kHasValue>
__global__ __launch_bounds__(kThreads) void k_spmm_t(const uint64_t* __restrict__ offset,
                                                     const CsrEntries<IndexType, kHasValue> src,
                                                     size_t nrows, const float* __restrict__ d,
                                                     int k, int cpr, int group,
                                                     float* __restrict__ g) {
  const int in_group = threadIdx.x & (group - 1);
  const int col = in_group & (cpr - 1);
  const int slot = in_group / cpr;
  const int slots = group / cpr;
  const size_t per_block = kThreads / group;
  const size_t stride = static_cast<size_t>(gridDim.x) * per_block;
  for (size_t r = blockIdx.x * per_block + threadIdx.x / group; r < nrows; r += stride) {
    const uint64_t b = offset[r], e = offset[r + 1];
    for (int c = col; c < k; c += cpr) {
      const float dr = d[r * k + c];
      for (uint64_t j = b + slot; j < e; j += slots) {
        size_t idx;
        float v;
        src.Load(j, &idx, &v);
        atomicAdd(&g[idx * k + c], v * dr);
      }
    }
  }
}

/*! \brief lanes per entry and lanes per row for `units` units per row */
void Layout(int units, int* cpr, int* group) {
  *cpr = NextPow2(units) < dev::kWave ? NextPow2(units) : dev::kWave;
  *group = 4 * *cpr < 16 ? 16 : (4 * *cpr > dev::kWave ? dev::kWave : 4 * *cpr);
}

template <typename Entries>
void LaunchSpMM(const uint64_t* offset, const Entries& src, size_t nrows, const float* w,
                const float* bias, int k, float* y, hipStream_t stream) {
  CHECK(k >= 1 && k <= kSpMMMaxCols) << "spmm: k must be in [1, " << kSpMMMaxCols << "], got " << k;
  if (nrows == 0) return;
  int cpr, group;
  // 16-byte loads need k % 4 == 0 and 16-byte aligned bases (row starts are then aligned too)
  if (k % 4 == 0 && Aligned16(w) && Aligned16(y) && Aligned16(bias)) {
    Layout(k / 4, &cpr, &group);
    hipLaunchKernelGGL((k_spmm<float4, Entries>), dim3(GridFor(nrows, kThreads / group)),
                       dim3(kThreads), 0, stream, offset, src, nrows, w, bias, k / 4, cpr, group, y);
  } else {
    Layout(k, &cpr, &group);
    hipLaunchKernelGGL((k_spmm<float, Entries>), dim3(GridFor(nrows, kThreads / group)),
                       dim3(kThreads), 0, stream, offset, src, nrows, w, bias, k, cpr, group, y);
  }
  DMLC_HIP_CHECK_LAUNCH();
}
}  // namespace

void LaunchCSRSpMM(const CsrView& csr, const float* w, const float* bias, int k, float* y,
                   hipStream_t stream) {
  CheckView("spmm", csr, true);
  if (csr.paired) {
    LaunchSpMM(csr.offset, PairEntries{static_cast<const uint2*>(csr.index)}, csr.nrows, w, bias,
               k, y, stream);
    return;
  }
  DispatchIndexValue(csr, [&](auto tag, auto has_value) {
    using IndexType = decltype(tag);
    using Entries = CsrEntries<IndexType, decltype(has_value)::value>;
    LaunchSpMM(csr.offset, Entries{IndexOf<IndexType>(csr), csr.value}, csr.nrows, w, bias, k, y,
               stream);
  });
}

void LaunchCSRSpMMT(const CsrView& csr, const float* d, int k, float* g, hipStream_t stream) {
  CheckView("spmm_t", csr, false);
  CHECK(k >= 1 && k <= kSpMMMaxCols) << "spmm_t: k must be in [1, " << kSpMMMaxCols << "], got " << k;
  const size_t nrows = csr.nrows;
  if (nrows == 0) return;
  int cpr, group;
  Layout(k, &cpr, &group);
  const dim3 grid(GridFor(nrows, kThreads / group));
  DispatchIndexValue(csr, [&](auto tag, auto has_value) {
    using IndexType = decltype(tag);
    constexpr bool kHasValue = decltype(has_value)::value;
    using Entries = CsrEntries<IndexType, kHasValue>;
    hipLaunchKernelGGL((k_spmm_t<IndexType, kHasValue>), grid, dim3(kThreads), 0, stream,
                       csr.offset, Entries{IndexOf<IndexType>(csr), csr.value}, nrows, d, k, cpr,
                       group, g);
  });
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
