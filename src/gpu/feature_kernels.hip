/*!
 * \file src/gpu/feature_kernels.hip
 * \brief K9 hashed dense batches (f32 / OCP fp8 e4m3), K10 offset rebase,
 *  K11 CSR SpMV and transposed SpMV, fills.
 *
 * K11 maps one row to a 16-lane group (4 rows per wave64): the survey's rows
 * carry 20-60 non-zeros, so a whole wave per row would idle half of it; the
 * group reduces with __shfl_xor at width 16.  The transposed product
 * scatters with hardware f32 atomics (global_atomic_add_f32, built with
 * -munsafe-fp-atomics), the right tool at this FLOP/byte ratio
 * (cdna_hip_programming.md Guideline 12).
 * K9 accumulates one row per wave in LDS (ds_add_f32) and converts pairs of
 * f32 to fp8 with the gfx950 v_cvt_pk_fp8_f32 instruction.
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
constexpr int kGroup = 16;

__global__ void k_fill(float* __restrict__ p, size_t n, float v) {
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    p[i] = v;
  }
}

__global__ void k_rebase(const uint64_t* __restrict__ src, size_t n, uint64_t src_base,
                         uint64_t dst_base, uint64_t* __restrict__ dst) {
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    dst[i] = src[i] - src_base + dst_base;
  }
}

template <typename IndexType>
__global__ __launch_bounds__(kThreads) void k_spmv(const uint64_t* __restrict__ offset,
                                                   const IndexType* __restrict__ index,
                                                   const float* __restrict__ value, size_t nrows,
                                                   const float* __restrict__ w, float bias,
                                                   float* __restrict__ y) {
  const size_t ngroups = static_cast<size_t>(gridDim.x) * (kThreads / kGroup);
  const int g = threadIdx.x % kGroup;
  for (size_t r = blockIdx.x * static_cast<size_t>(kThreads / kGroup) + threadIdx.x / kGroup;
       r < nrows; r += ngroups) {
    const uint64_t b = offset[r], e = offset[r + 1];
    float acc = 0.0f;
    for (uint64_t j = b + g; j < e; j += kGroup) {
      const float v = value != nullptr ? value[j] : 1.0f;
      acc += v * w[index[j]];
    }
#pragma unroll
    for (int d = kGroup / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, kGroup);
    if (g == 0) y[r] = acc + bias;
  }
}

/*! \brief k_spmv over interleaved (u32 index, f32 value) pairs (the paired
 *  transpose output): one 8-byte load per entry */
__global__ __launch_bounds__(kThreads) void k_spmv_pairs(const uint64_t* __restrict__ offset,
                                                         const uint2* __restrict__ iv,
                                                         size_t nrows, const float* __restrict__ w,
                                                         float bias, float* __restrict__ y) {
  const size_t ngroups = static_cast<size_t>(gridDim.x) * (kThreads / kGroup);
  const int g = threadIdx.x % kGroup;
  for (size_t r = blockIdx.x * static_cast<size_t>(kThreads / kGroup) + threadIdx.x / kGroup;
       r < nrows; r += ngroups) {
    const uint64_t b = offset[r], e = offset[r + 1];
    float acc = 0.0f;
    for (uint64_t j = b + g; j < e; j += kGroup) {
      const uint2 p = iv[j];
      acc += __uint_as_float(p.y) * w[p.x];
    }
#pragma unroll
    for (int d = kGroup / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, kGroup);
    if (g == 0) y[r] = acc + bias;
  }
}

template <typename IndexType>
__global__ __launch_bounds__(kThreads) void k_spmvt(const uint64_t* __restrict__ offset,
                                                    const IndexType* __restrict__ index,
                                                    const float* __restrict__ value, size_t nrows,
                                                    const float* __restrict__ d,
                                                    float* __restrict__ grad) {
  const size_t ngroups = static_cast<size_t>(gridDim.x) * (kThreads / kGroup);
  const int g = threadIdx.x % kGroup;
  for (size_t r = blockIdx.x * static_cast<size_t>(kThreads / kGroup) + threadIdx.x / kGroup;
       r < nrows; r += ngroups) {
    const uint64_t b = offset[r], e = offset[r + 1];
    const float dr = d[r];
    if (dr == 0.0f) continue;
    for (uint64_t j = b + g; j < e; j += kGroup) {
      const float v = value != nullptr ? value[j] : 1.0f;
      atomicAdd(&grad[index[j]], v * dr);
    }
  }
}


/*! \brief one row per wave; LDS row buffer of `dim` floats per wave */
template <typename IndexType, bool kFP8>
__global__ __launch_bounds__(kThreads) void k_hashed_dense(
    const uint64_t* __restrict__ offset, const IndexType* __restrict__ index,
    const float* __restrict__ value, const IndexType* __restrict__ field, size_t nrows, int dim,
    float scale, uint32_t seed, void* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wid = threadIdx.x / dev::kWave;
  const int lane = dev::lane_id();
  float* row = smem + static_cast<size_t>(wid) * dim;
  const size_t nwaves = static_cast<size_t>(gridDim.x) * (kThreads / dev::kWave);
  // rows are zeroed once here, then by the readout that consumes them
  for (int c = lane; c < dim; c += dev::kWave) row[c] = 0.0f;
  dev::wave_sync();
  const bool wide = (dim & 15) == 0;  // 16 columns per lane: b128 LDS ops, 16 B stores
  for (size_t r = blockIdx.x * static_cast<size_t>(kThreads / dev::kWave) + wid; r < nrows;
       r += nwaves) {
    const uint64_t b = offset[r], e = offset[r + 1];
    for (uint64_t j = b + lane; j < e; j += dev::kWave) {
      const uint64_t key = dev::hash_key(static_cast<uint64_t>(index[j]),
                                         field != nullptr ? static_cast<uint64_t>(field[j]) : 0,
                                         field != nullptr);
      const uint32_t h = dev::hash_u64(key, seed);
      const int bucket = static_cast<int>(h % static_cast<uint32_t>(dim));
      const float sign = (h & 0x80000000u) ? -1.0f : 1.0f;
      const float v = value != nullptr ? value[j] : 1.0f;
      atomicAdd(&row[bucket], sign * v);
    }
    dev::wave_sync();
    if (wide) {
      float4* r4 = reinterpret_cast<float4*>(row);
      const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int c = lane * 16; c < dim; c += dev::kWave * 16) {
        float4 x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          x[q] = r4[c / 4 + q];
          r4[c / 4 + q] = z;
        }
        if constexpr (kFP8) {
          uint32_t w[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            int pk = __builtin_amdgcn_cvt_pk_fp8_f32(x[q].x * scale, x[q].y * scale, 0, false);
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(x[q].z * scale, x[q].w * scale, pk, true);
            w[q] = static_cast<uint32_t>(pk);
          }
          *reinterpret_cast<uint4*>(static_cast<uint8_t*>(out) + r * dim + c) =
              make_uint4(w[0], w[1], w[2], w[3]);
        } else {
          // rebuilt per element: a plain float4 array copy here went through scratch
          float4* o = reinterpret_cast<float4*>(static_cast<float*>(out) + r * dim + c);
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = make_float4(x[q].x, x[q].y, x[q].z, x[q].w);
        }
      }
    } else if constexpr (kFP8) {
      // 4 columns per lane-iteration -> one 32-bit store of 4 fp8 (e4m3, OCP on gfx950)
      uint32_t* o = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(out) + r * dim);
      for (int c = lane * 4; c < dim; c += dev::kWave * 4) {
        int packed = __builtin_amdgcn_cvt_pk_fp8_f32(row[c] * scale, row[c + 1] * scale, 0, false);
        packed = __builtin_amdgcn_cvt_pk_fp8_f32(row[c + 2] * scale, row[c + 3] * scale, packed, true);
        o[c / 4] = static_cast<uint32_t>(packed);
        row[c] = row[c + 1] = row[c + 2] = row[c + 3] = 0.0f;
      }
    } else {
      float* o = static_cast<float*>(out) + r * dim;
      for (int c = lane; c < dim; c += dev::kWave) {
        o[c] = row[c];
        row[c] = 0.0f;
      }
    }
    dev::wave_sync();
  }
}
}  // namespace

void LaunchFill(float* p, size_t n, float v, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_fill, dim3(GridFor(n, kThreads)), dim3(kThreads), 0, stream, p, n, v);
}

namespace {
/*! \brief one row pointer per lane; its page by binary search of the (small,
 *  L2-resident) page table */
__global__ __launch_bounds__(kThreads) void k_page_rebase(uint64_t* __restrict__ offset,
                                                          size_t nrows,
                                                          const uint64_t* __restrict__ row_end,
                                                          const uint64_t* __restrict__ nnz_base,
                                                          int npages) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t r = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; r < nrows;
       r += stride) {
    int lo = 0, hi = npages - 1;  // first page whose cumulative row end exceeds r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (row_end[mid] > r) {
        hi = mid;
      } else {
        lo = mid + 1;
      }
    }
    offset[r + 1] += nnz_base[lo];
  }
}
}  // namespace

void LaunchPageRebase(uint64_t* offset, size_t nrows, const uint64_t* page_row_end,
                      const uint64_t* page_nnz_base, int npages, hipStream_t stream) {
  if (nrows == 0 || npages == 0) return;
  hipLaunchKernelGGL(k_page_rebase, dim3(GridFor(nrows, kThreads)), dim3(kThreads), 0, stream,
                     offset, nrows, page_row_end, page_nnz_base, npages);
}

void LaunchOffsetRebase(const uint64_t* src_offset, size_t nrows, uint64_t src_base,
                        uint64_t dst_base, uint64_t* dst_offset, hipStream_t stream) {
  hipLaunchKernelGGL(k_rebase, dim3(GridFor(nrows + 1, kThreads)), dim3(kThreads), 0, stream,
                     src_offset, nrows + 1, src_base, dst_base, dst_offset);
}

void LaunchCSRSpMV(const CsrView& csr, const float* w, float bias, float* y, hipStream_t stream) {
  CheckView("spmv", csr, true);
  const size_t nrows = csr.nrows;
  if (nrows == 0) return;
  if (csr.paired) {
    hipLaunchKernelGGL(k_spmv_pairs, dim3(GridFor(nrows, kThreads / kGroup)), dim3(kThreads), 0,
                       stream, csr.offset, static_cast<const uint2*>(csr.index), nrows, w, bias, y);
  } else {
    DispatchIndex(csr, [&](auto tag) {
      using IndexType = decltype(tag);
      hipLaunchKernelGGL(k_spmv<IndexType>, dim3(GridFor(nrows, kThreads / kGroup)),
                         dim3(kThreads), 0, stream, csr.offset, IndexOf<IndexType>(csr), csr.value,
                         nrows, w, bias, y);
    });
  }
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchCSRSpMVT(const CsrView& csr, const float* d, float* g, hipStream_t stream) {
  CheckView("spmv_t", csr, false);
  const size_t nrows = csr.nrows;
  if (nrows == 0) return;
  DispatchIndex(csr, [&](auto tag) {
    using IndexType = decltype(tag);
    hipLaunchKernelGGL(k_spmvt<IndexType>, dim3(GridFor(nrows, kThreads / kGroup)), dim3(kThreads),
                       0, stream, csr.offset, IndexOf<IndexType>(csr), csr.value, nrows, d, g);
  });
  DMLC_HIP_CHECK_LAUNCH();
}

namespace {
/*! \brief K9 into fp8 (x scale) or f32 rows */
template <bool kFP8>
void LaunchHashedDense(const CsrView& csr, int dim, float scale, uint32_t seed, void* out,
                       hipStream_t stream) {
  CheckView("hashed_dense", csr, false);
  const size_t nrows = csr.nrows;
  if (nrows == 0) return;
  const size_t lds = static_cast<size_t>(dim) * sizeof(float) * (kThreads / dev::kWave);
  DispatchIndex(csr, [&](auto tag) {
    using IndexType = decltype(tag);
    PrepareLdsLaunch(k_hashed_dense<IndexType, kFP8>, lds);
    hipLaunchKernelGGL((k_hashed_dense<IndexType, kFP8>),
                       dim3(GridFor(nrows, kThreads / dev::kWave)), dim3(kThreads), lds, stream,
                       csr.offset, IndexOf<IndexType>(csr), csr.value, FieldOf<IndexType>(csr),
                       nrows, dim, scale, seed, out);
  });
  DMLC_HIP_CHECK_LAUNCH();
}
}  // namespace

void LaunchHashedDenseFP8(const CsrView& csr, int dim, float scale, uint32_t seed, uint8_t* out,
                          hipStream_t stream) {
  LaunchHashedDense<true>(csr, dim, scale, seed, out, stream);
}

void LaunchHashedDenseF32(const CsrView& csr, int dim, uint32_t seed, float* out,
                          hipStream_t stream) {
  LaunchHashedDense<false>(csr, dim, 1.0f, seed, out, stream);
}

}  // namespace gpu
}  // namespace dmlc
