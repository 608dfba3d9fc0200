/*!
 * \file src/gpu/compact_kernels.hip
 * \brief U1 - U4: the distinct feature ids of a CSR batch and every entry's
 *  position among them (row-sparse minibatch steps), without a sort.
 *
 *  The set of touched ids is a bitmap of num_features bits; the K3 scan of the
 *  per-word popcounts numbers its members.
 *
 *  U1 k_compact_mark   one lane per entry of [base, base + nnz): set bit `id`.
 *                      The bit is tested by a plain load first, so a feature
 *                      that occurs in every row costs an atomic only until the
 *                      set bit is seen, not one per row.  An id >= num_features
 *                      forms no address and sets kCompactErrIndex.
 *  U2 k_compact_count  one lane per 64-bit word: its popcount, as u64 for
 *                      LaunchScanU64 (in place: counts become prefixes).
 *  U3 k_compact_emit   one lane per word: its set bits, ascending, as ids from
 *                      ids[prefix[w]] on -- ids come out strictly ascending.
 *  U4 k_compact_remap  one lane per entry: slot = prefix[id >> 6] + popcount of
 *                      the word's bits below bit id & 63.
 *
 *  The atomics only build a set: which lane sets a bit first changes nothing,
 *  so the output bytes are a pure function of the inputs.
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

/*! \brief one thread ORs the wave's error into the status word (not an output) */
__device__ __forceinline__ void report(bool bad, uint32_t bit, uint32_t* error) {
  const uint64_t m = __ballot(bad);
  if (m != 0 && dev::lane_id() == __builtin_ctzll(m)) atomicOr(error, bit);
}

template <typename IndexType>
__global__ __launch_bounds__(kThreads) void k_compact_mark(const IndexType* __restrict__ index,
                                                           uint64_t base, uint64_t nnz,
                                                           uint64_t num_features, uint32_t* bits,
                                                           uint32_t* error) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  bool bad = false;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j < nnz;
       j += stride) {
    const uint64_t id = static_cast<uint64_t>(index[base + j]);
    if (id >= num_features) {  // num_features <= 2^32: a 64-bit id above it ends here too
      bad = true;
      continue;
    }
    // the bitmap as 32-bit words (little endian: bit id of the u64 words U2 reads)
    uint32_t* const word = bits + (id >> 5);
    const uint32_t bit = 1u << (id & 31u);
    if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0u) {
      atomicOr(word, bit);
    }
  }
  report(bad, kCompactErrIndex, error);
}

__global__ __launch_bounds__(kThreads) void k_compact_count(const uint64_t* __restrict__ bitmap,
                                                            size_t words,
                                                            uint64_t* __restrict__ counts) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (w < words) counts[w] = static_cast<uint64_t>(__popcll(bitmap[w]));
}

__global__ __launch_bounds__(kThreads) void k_compact_emit(const uint64_t* __restrict__ bitmap,
                                                           const uint64_t* __restrict__ prefix,
                                                           size_t words, uint64_t capacity,
                                                           int64_t* __restrict__ ids) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (w >= words) return;
  uint64_t m = bitmap[w];
  uint64_t p = prefix[w];
  while (m != 0) {
    const int b = __builtin_ctzll(m);
    m &= m - 1;
    if (p < capacity) ids[p] = static_cast<int64_t>((static_cast<uint64_t>(w) << 6) | b);
    ++p;
  }
}

template <typename IndexType>
__global__ __launch_bounds__(kThreads) void k_compact_remap(const IndexType* __restrict__ index,
                                                            uint64_t base, uint64_t nnz,
                                                            uint64_t num_features,
                                                            const uint64_t* __restrict__ bitmap,
                                                            const uint64_t* __restrict__ prefix,
                                                            int32_t* __restrict__ slot) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j < nnz;
       j += stride) {
    const uint64_t id = static_cast<uint64_t>(index[base + j]);
    uint64_t s = 0;  // a flagged entry (U1 reported it) gets slot 0
    if (id < num_features) {
      const uint64_t below = bitmap[id >> 6] & ((1ull << (id & 63u)) - 1ull);
      s = prefix[id >> 6] + static_cast<uint64_t>(__popcll(below));
    }
    slot[j] = static_cast<int32_t>(s);
  }
}

size_t Words(uint64_t num_features) { return static_cast<size_t>((num_features + 63) / 64); }
/*! \brief words of the bitmap and of the counts: even, so that the counts
 *  behind a 16-byte aligned bitmap are 16-byte aligned (the scan's loads) */
size_t PaddedWords(uint64_t num_features) { return (Words(num_features) + 1) & ~size_t{1}; }

void CheckArgs(const char* op, const CsrView& csr, uint64_t nnz, uint64_t num_features,
               const void* scratch) {
  CheckView(op, csr, false);
  CHECK(num_features >= 1 && num_features <= kCompactMaxFeatures)
      << op << ": num_features must be in [1, 2^32], got " << num_features;
  CHECK_LT(nnz, 1ull << 31) << op << ": a batch must have fewer than 2^31 entries";
  CHECK(Aligned16(scratch)) << op << ": scratch must be 16-byte aligned";
}
}  // namespace

size_t CompactScratchBytes(uint64_t num_features) {
  const size_t words = Words(num_features);
  return 8 * (2 * PaddedWords(num_features) + ScanPartials(words) + 1);
}

void LaunchCompactMark(const CsrView& csr, uint64_t base, uint64_t nnz, uint64_t num_features,
                       void* scratch, uint32_t* error, hipStream_t stream) {
  CheckArgs("compact mark", csr, nnz, num_features, scratch);
  // every call starts from an empty set, in stream order
  DMLC_HIP_CHECK(hipMemsetAsync(scratch, 0, 8 * PaddedWords(num_features), stream));
  if (nnz == 0) return;
  DispatchIndex(csr, [&](auto tag) {
    using IndexType = decltype(tag);
    hipLaunchKernelGGL(k_compact_mark<IndexType>, dim3(GridFor(nnz, kThreads)), dim3(kThreads), 0,
                       stream, IndexOf<IndexType>(csr), base, nnz, num_features,
                       static_cast<uint32_t*>(scratch), error);
  });
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchCompactCount(uint64_t num_features, void* scratch, uint64_t* total,
                        hipStream_t stream) {
  CHECK(num_features >= 1 && num_features <= kCompactMaxFeatures && Aligned16(scratch))
      << "compact count: bad num_features or scratch";
  const size_t words = Words(num_features), padded = PaddedWords(num_features);
  uint64_t* const bitmap = static_cast<uint64_t*>(scratch);
  uint64_t* const counts = bitmap + padded;
  hipLaunchKernelGGL(k_compact_count, dim3((words + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, bitmap, words, counts);
  DMLC_HIP_CHECK_LAUNCH();
  LaunchScanU64(counts, words, counts + padded, total, stream);
}

void LaunchCompactEmit(uint64_t num_features, const void* scratch, uint64_t capacity, int64_t* ids,
                       hipStream_t stream) {
  CHECK(num_features >= 1 && num_features <= kCompactMaxFeatures && Aligned16(scratch))
      << "compact emit: bad num_features or scratch";
  if (capacity == 0) return;
  const size_t words = Words(num_features), padded = PaddedWords(num_features);
  const uint64_t* const bitmap = static_cast<const uint64_t*>(scratch);
  hipLaunchKernelGGL(k_compact_emit, dim3((words + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, bitmap, bitmap + padded, words, capacity, ids);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchCompactRemap(const CsrView& csr, uint64_t base, uint64_t nnz, uint64_t num_features,
                        const void* scratch, int32_t* slot, hipStream_t stream) {
  CheckArgs("compact remap", csr, nnz, num_features, scratch);
  if (nnz == 0) return;
  const uint64_t* const bitmap = static_cast<const uint64_t*>(scratch);
  const uint64_t* const prefix = bitmap + PaddedWords(num_features);
  DispatchIndex(csr, [&](auto tag) {
    using IndexType = decltype(tag);
    hipLaunchKernelGGL(k_compact_remap<IndexType>, dim3(GridFor(nnz, kThreads)), dim3(kThreads),
                       0, stream, IndexOf<IndexType>(csr), base, nnz, num_features, bitmap, prefix,
                       slot);
  });
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
