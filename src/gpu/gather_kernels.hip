/*!
 * \file src/gpu/gather_kernels.hip
 * \brief G1 / G2: gather rows r0, r1, ... of a device CSR into a CSR batch
 *  (row-shuffled minibatches from a resident shard).
 *
 *  G1 k_gather_count  one lane per selected row: its length (a bad id or a
 *                     row pointer the source arrays cannot hold counts 0 and
 *                     sets an error bit) and its label / weight / qid.
 *  K3 LaunchScanU64   the lengths become the batch's row pointer.
 *  G2 k_gather_fill   organised by OUTPUT position: a wave owns kGatherRun
 *                     consecutive output entries, whatever rows they belong
 *                     to, so every store is coalesced and every wave has the
 *                     same work -- one 100 000-entry row among one-entry rows,
 *                     or half the selection empty, changes nothing.  The wave
 *                     finds the selected row of its first entry by one
 *                     wave-uniform binary search in the scanned row pointer
 *                     and walks forward from there with the row-end window of
 *                     transpose_kernels.hip (T3b): lane j holds the end of
 *                     selected row wbase + j and what to add to an output
 *                     position of that row to get its source position; an
 *                     entry's row is wbase + the number of ends at or before
 *                     it.  One row lookup serves index, value and field.
 *
 *  All positions are 64-bit.  No atomics touch the outputs: their bytes are a
 *  pure function of the inputs.
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
constexpr int kWaves = kThreads / dev::kWave;
/*! \brief 64-entry groups of a wave's run */
constexpr int kGroups = 8;
constexpr uint64_t kGatherRun = static_cast<uint64_t>(kGroups) * dev::kWave;
/*! \brief a launch's threads per grid dimension stay below 2^32 */
constexpr uint64_t kMaxBlocks = (1ull << 32) / kThreads;

/*! \brief a selection entry as an unsigned row id (negative ids become huge) */
__device__ __forceinline__ uint64_t row_id(const int32_t* rows, size_t i) {
  return static_cast<uint64_t>(static_cast<int64_t>(rows[i]));
}
__device__ __forceinline__ uint64_t row_id(const int64_t* rows, size_t i) {
  return static_cast<uint64_t>(rows[i]);
}

template <typename RowT>
__global__ __launch_bounds__(kThreads) void k_gather_count(
    const uint64_t* __restrict__ offset, uint64_t nrows_src, uint64_t src_entries,
    const RowT* __restrict__ rows, size_t n_sel, const float* __restrict__ label,
    const float* __restrict__ weight, const uint64_t* __restrict__ qid,
    uint64_t* __restrict__ out_offset, float* __restrict__ out_label,
    float* __restrict__ out_weight, uint64_t* __restrict__ out_qid, uint32_t* error) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n_sel) return;
  const uint64_t r = row_id(rows, i);
  uint64_t len = 0;
  uint32_t err = 0;
  const bool ok = r < nrows_src;
  if (ok) {
    const uint64_t b = offset[r], e = offset[r + 1];
    if (b <= e && e <= src_entries) {
      len = e - b;
    } else {
      err = kGatherErrSource;
    }
  } else {
    err = kGatherErrRow;
  }
  out_offset[i] = len;
  if (label != nullptr) out_label[i] = ok ? label[r] : 0.0f;
  if (weight != nullptr) out_weight[i] = ok ? weight[r] : 0.0f;
  if (qid != nullptr) out_qid[i] = ok ? qid[r] : 0ull;
  if (err != 0) atomicOr(error, err);  // the status word, not an output
}

/*! \brief x of lane `src`, 64-bit (two bpermutes) */
__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(x), src, dev::kWave);
  const uint32_t hi = __shfl(static_cast<uint32_t>(x >> 32), src, dev::kWave);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

template <typename IndexType, typename RowT>
__global__ __launch_bounds__(kThreads) void k_gather_fill(
    const uint64_t* __restrict__ offset, uint64_t nrows_src, uint64_t src_entries,
    const RowT* __restrict__ rows, size_t n_sel, const uint64_t* __restrict__ out_offset,
    uint64_t* __restrict__ out_close, const uint64_t* __restrict__ total_ptr,
    const IndexType* __restrict__ index, const float* __restrict__ value,
    const IndexType* __restrict__ field, IndexType* __restrict__ out_index,
    float* __restrict__ out_value, IndexType* __restrict__ out_field, uint64_t out_capacity,
    uint32_t* error) {
  __shared__ uint32_t s_ends[kWaves][dev::kWave];
  const int lane = dev::lane_id();
  const int w = threadIdx.x / dev::kWave;
  const uint64_t total = *total_ptr;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the one-lane tail: the closing row pointer out_offset[n_sel] (nobody
    // reads it here -- the waves below take the last row's end from `total`)
    // and the capacity bit (single writer, after G1 in stream order)
    *out_close = total;
    if (total > out_capacity) *error |= kGatherErrCapacity;
  }
  const uint64_t lim = total < out_capacity ? total : out_capacity;
  const uint64_t p0 =
      (static_cast<uint64_t>(blockIdx.x) * kWaves + dev::uniform(static_cast<uint32_t>(w))) *
      kGatherRun;
  if (p0 >= lim) return;
  const uint64_t p1 = p0 + kGatherRun < lim ? p0 + kGatherRun : lim;

  // the last selected row that starts at or before p (p < total, so that row
  // holds p: the rows after it start later, empty rows before it are skipped)
  auto find_row = [&](uint64_t p) {
    size_t lo = 0, hi = n_sel;  // out_offset[lo] <= p; every row from hi on starts after p
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      if (out_offset[mid] <= p) {
        lo = mid;
      } else {
        hi = mid;
      }
    }
    return lo;
  };
  // lane j: the end of selected row wb + j (past the selection: never)
  auto window_end = [&](size_t wb) {
    const size_t i = wb + lane + 1;
    return i < n_sel ? out_offset[i] : (i == n_sel ? total : ~0ull);
  };
  // lane j: source position - output position of the entries of row wb + j
  auto window_delta = [&](size_t wb) {
    const size_t i = wb + lane;
    uint64_t d = 0;
    if (i < n_sel) {
      const uint64_t r = row_id(rows, i);
      if (r < nrows_src) d = offset[r] - out_offset[i];
    }
    return d;
  };

  size_t wbase = find_row(p0);
  uint64_t wend = window_end(wbase);
  uint64_t wdelta = window_delta(wbase);
  uint64_t src[kGroups];
#pragma unroll
  for (int gi = 0; gi < kGroups; ++gi) {
    const uint64_t g = p0 + static_cast<uint64_t>(gi) * dev::kWave;
    const uint64_t p = g + lane;
    const bool valid = p < p1;
    src[gi] = 0;
    bool found = !valid;
    if (g >= p1) continue;  // wave-uniform: the tail of the last run
    for (;;) {
      // ends before the group start (rows of earlier groups still in the
      // window) count as at or before every entry
      const uint32_t rel = wend <= g ? 0u
                           : wend - g >= 0xFFFFFFFFull ? 0xFFFFFFFFu
                                                       : static_cast<uint32_t>(wend - g);
      uint32_t* const ends = s_ends[w];
      ends[lane] = 0u;
      dev::wave_sync();
      if (rel < static_cast<uint32_t>(dev::kWave)) atomicAdd(&ends[rel], 1u);
      dev::wave_sync();
      // row ends at or before this lane's entry (64: the whole window)
      const uint32_t n = dev::wave_incl_scan_u32(ends[lane]);
      dev::wave_sync();  // every lane has read its count before the next reset
      const uint64_t d = shfl64(wdelta, static_cast<int>(n & 63u));
      if (!found && n < static_cast<uint32_t>(dev::kWave)) {
        src[gi] = p + d;
        found = true;
      }
      const uint64_t todo = __ballot(!found);
      if (todo == 0) break;
      // more than 64 row ends before some entry: move the window on (forward
      // only); a block of empty rows wider than the next window too is
      // skipped by a search for the first entry still without a row
      const uint64_t pnext = g + static_cast<uint64_t>(__builtin_ctzll(todo));
      wbase += dev::kWave;
      wend = window_end(wbase);
      if (dev::uniform(shfl64(wend, dev::kWave - 1)) <= pnext) {
        wbase = find_row(pnext);
        wend = window_end(wbase);
      }
      wdelta = window_delta(wbase);
    }
  }
  // every row is known: the loads of the whole run go out together
  IndexType vi[kGroups];
  IndexType vf[kGroups];
  float vv[kGroups];
  bool stray = false;
#pragma unroll
  for (int gi = 0; gi < kGroups; ++gi) {
    const bool valid = p0 + static_cast<uint64_t>(gi) * dev::kWave + lane < p1;
    // G1 admitted only rows inside the source arrays; a position outside them
    // (the row pointer changed since) is not read
    const bool ok = valid && src[gi] < src_entries;
    stray |= valid && !ok;
    vi[gi] = ok ? index[src[gi]] : IndexType(0);
    vv[gi] = (ok && value != nullptr) ? value[src[gi]] : 0.0f;
    vf[gi] = (ok && field != nullptr) ? field[src[gi]] : IndexType(0);
  }
  if (stray) atomicOr(error, kGatherErrSource);  // the status word, not an output
#pragma unroll
  for (int gi = 0; gi < kGroups; ++gi) {
    const uint64_t p = p0 + static_cast<uint64_t>(gi) * dev::kWave + lane;
    if (p < p1) {
      out_index[p] = vi[gi];
      if (value != nullptr) out_value[p] = vv[gi];
      if (field != nullptr) out_field[p] = vf[gi];
    }
  }
}
}  // namespace

uint64_t CSRGatherRunEntries() { return kGatherRun; }

size_t CSRGatherScratchWords(size_t n_sel) { return ScanPartials(n_sel) + 2; }

void LaunchCSRGatherCount(const uint64_t* offset, uint64_t nrows_src, uint64_t src_entries,
                          const void* rows, bool rows64, size_t n_sel, const float* label,
                          const float* weight, const uint64_t* qid, uint64_t* out_offset,
                          float* out_label, float* out_weight, uint64_t* out_qid, uint32_t* error,
                          hipStream_t stream) {
  if (n_sel == 0) return;
  const size_t blocks = (n_sel + kThreads - 1) / kThreads;
  CHECK_LT(blocks, kMaxBlocks) << "gather: too many selected rows";
  if (rows64) {
    hipLaunchKernelGGL(k_gather_count<int64_t>, dim3(blocks), dim3(kThreads), 0, stream, offset,
                       nrows_src, src_entries, static_cast<const int64_t*>(rows), n_sel, label,
                       weight, qid, out_offset, out_label, out_weight, out_qid, error);
  } else {
    hipLaunchKernelGGL(k_gather_count<int32_t>, dim3(blocks), dim3(kThreads), 0, stream, offset,
                       nrows_src, src_entries, static_cast<const int32_t*>(rows), n_sel, label,
                       weight, qid, out_offset, out_label, out_weight, out_qid, error);
  }
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchCSRGatherFill(const CsrView& src, uint64_t src_entries, const void* rows, bool rows64,
                         size_t n_sel, uint64_t* out_offset, const uint64_t* total,
                         void* out_index, float* out_value, void* out_field,
                         uint64_t out_capacity, uint32_t* error, hipStream_t stream) {
  CheckView("gather", src, false);
  // the entry count is on the device only: one wave per run of the capacity
  // (waves past the total leave at once), at least the tail's workgroup
  constexpr uint64_t kPerBlock = kGatherRun * kWaves;
  uint64_t blocks = (out_capacity + kPerBlock - 1) / kPerBlock;
  if (blocks == 0) blocks = 1;
  CHECK_LT(blocks, kMaxBlocks) << "gather: out_capacity too large for one launch";
  const uint64_t nrows_src = src.nrows;
  DispatchIndex(src, [&](auto tag) {
    using IndexType = decltype(tag);
    const IndexType* index = IndexOf<IndexType>(src);
    const IndexType* field = FieldOf<IndexType>(src);
    IndexType* oindex = static_cast<IndexType*>(out_index);
    IndexType* ofield = static_cast<IndexType*>(out_field);
    if (rows64) {
      hipLaunchKernelGGL((k_gather_fill<IndexType, int64_t>), dim3(blocks), dim3(kThreads), 0,
                         stream, src.offset, nrows_src, src_entries,
                         static_cast<const int64_t*>(rows), n_sel, out_offset, out_offset + n_sel,
                         total, index, src.value, field, oindex, out_value, ofield, out_capacity,
                         error);
    } else {
      hipLaunchKernelGGL((k_gather_fill<IndexType, int32_t>), dim3(blocks), dim3(kThreads), 0,
                         stream, src.offset, nrows_src, src_entries,
                         static_cast<const int32_t*>(rows), n_sel, out_offset, out_offset + n_sel,
                         total, index, src.value, field, oindex, out_value, ofield, out_capacity,
                         error);
    }
  });
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
