/*!
 * \file src/gpu/gbdt_kernels.hip
 * \brief GB1 - GB5: histogram gradient-boosted trees on the column-major
 *  binned matrix (the transpose of a device CSR with one 8-bit bin per entry).
 *
 *  GB1 k_gbdt_cuts     one wave per column of the sorted (feature << 32 |
 *                      ordered value) keys: the quantile candidates
 *                      s[(i n + B - 1) / B - 1], i = 1 .. B (every entry when
 *                      n <= B), kept where they differ from the one before.
 *                      Run twice: counts per column, then -- behind a scan of
 *                      the counts -- the cut values at cut_ptr[f].
 *  GB2 k_gbdt_bin      one workgroup per segment: bin = #cuts of the column
 *                      below x, capped at the last one, by a binary search in
 *                      the segment's cuts staged in LDS.
 *  GB3 k_gbdt_hist     one workgroup per segment: (node, bin) sums of the
 *                      quantised gradients in LDS, flushed once per cell.
 *  GB4 k_gbdt_split_*  one lane per (node, feature) scans the feature's bins;
 *                      a workgroup, then one workgroup per node, reduce to the
 *                      best candidate under a total order.
 *  GB5 k_gbdt_advance_* one pass over pos (default side, leaves), then the
 *                      split columns' entries filtered by pos == node.
 *
 *  Segments.  The entries of the column-major matrix, in storage order, are
 *  cut every kGbdtSegmentEntries: workgroup s owns entries [s S, (s + 1) S).
 *  A segment is a piece of one long column or a run of short ones, so a hot
 *  feature is spread over as many workgroups as it has segments and short
 *  columns share one.  The workgroup finds its first and last column by a
 *  binary search in the column pointer and each lane its entry's column by one
 *  between them, over the segment's column pointers staged in LDS (up to
 *  kColsLds; a segment of more columns searches global memory).  The columns
 *  of a segment are taken in groups of consecutive columns whose cuts (GB2) or
 *  node x bin cells (GB3) fit the LDS table.
 *
 *  GB3's table holds kGbdtCells (int64 g, int64 h) cells.  A group of W bins
 *  takes min(N, kGbdtCells / W) nodes per pass and streams its entries once
 *  per pass: 64 nodes on a 256-cut column are 5 passes of 15 nodes, not a
 *  spill to global atomics.  A column that lies inside one segment is written
 *  by plain stores; a column cut by a segment boundary adds its non-zero cells
 *  with one 64-bit atomic each.  The sums are integers: no order changes them.
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
constexpr int64_t kSeg = kGbdtSegmentEntries;
/*! \brief floats of cuts GB2 stages per group of columns */
constexpr int kCutsLds = 8192;
/*! \brief (g, h) cells of GB3's LDS table: 60 KiB, two workgroups per CU */
constexpr int kGbdtCells = 3840;
static_assert(kCutsLds >= static_cast<int>(kGbdtMaxBins) &&
              kGbdtCells >= static_cast<int>(kGbdtMaxBins), "a column's cuts fit one group");

/*! \brief one thread ORs the wave's error into the status word (not an output) */
__device__ __forceinline__ void report(bool bad, uint32_t bit, uint32_t* error) {
  const uint64_t m = __ballot(bad);
  if (m != 0 && dev::lane_id() == __builtin_ctzll(m)) atomicOr(error, bit);
}

/*! \brief the largest k in [lo, hi) with ptr[k] <= x; ptr ascends and ptr[lo] <= x */
__device__ __forceinline__ int64_t last_le(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi,
                                           int64_t x) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ptr[mid] <= x) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

/*! \brief column pointers of a segment staged in LDS (relative to the segment's first entry):
 *  with GB3's table 65 512 of the 65 536 bytes a workgroup may declare */
constexpr int kColsLds = 1016;

/*! \brief last_le over the staged pointers */
__device__ __forceinline__ int last_le_lds(const uint32_t* s, int lo, int hi, uint32_t x) {
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (s[mid] <= x) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

/*!
 * \brief stage col_ptr[f_lo .. f_hi + 1] - base, clamped to [0, kSeg], in s_col when they fit
 *  (a segment of up to kColsLds - 1 columns): every lane then finds its entry's column in LDS
 *  instead of global memory, on every node pass.  Clamping keeps the order and every answer for
 *  an entry of the segment.  Returns whether they were staged; contains a barrier.
 */
__device__ __forceinline__ bool stage_columns(const int64_t* __restrict__ col_ptr, int64_t f_lo,
                                              int64_t f_hi, int64_t base, uint32_t* s_col) {
  const int64_t n = f_hi - f_lo + 2;
  if (n > kColsLds) return false;
  for (int64_t k = threadIdx.x; k < n; k += kThreads) {
    const int64_t d = col_ptr[f_lo + k] - base;
    s_col[k] = static_cast<uint32_t>(d < 0 ? 0 : (d > kSeg ? kSeg : d));
  }
  __syncthreads();
  return true;
}

/*! \brief the column in [fa, fb) of entry j of the segment that starts at base */
__device__ __forceinline__ int64_t column_of(bool staged, const uint32_t* s_col,
                                             const int64_t* __restrict__ col_ptr, int64_t f_lo,
                                             int64_t fa, int64_t fb, int64_t base, int64_t j) {
  if (staged) {
    return f_lo + last_le_lds(s_col, static_cast<int>(fa - f_lo), static_cast<int>(fb - f_lo),
                              static_cast<uint32_t>(j - base));
  }
  return last_le(col_ptr, fa, fb, j);
}

/*! \brief a value every thread of the workgroup gets from thread 0 (two barriers) */
__device__ __forceinline__ int64_t block_bcast(int64_t v, int64_t* slot) {
  if (threadIdx.x == 0) *slot = v;
  __syncthreads();
  const int64_t r = *slot;
  __syncthreads();
  return r;
}

/*! \brief the columns [f_lo, f_hi] that hold entries base and end - 1 */
__device__ __forceinline__ void segment_columns(const int64_t* __restrict__ col_ptr, int64_t nfeat,
                                                int64_t base, int64_t end, int64_t* slot,
                                                int64_t* f_lo, int64_t* f_hi) {
  int64_t a = 0, b = 0;
  if (threadIdx.x == 0) {
    a = last_le(col_ptr, 0, nfeat, base);
    b = last_le(col_ptr, a, nfeat, end - 1);
  }
  *f_lo = block_bcast(a, slot);
  *f_hi = block_bcast(b, slot);
}

/*! \brief the end fb of the group of columns [fa, fb), fb <= f_end, whose cuts
 *  [cut_ptr[fa], cut_ptr[fb]) number at most `room`; at least one column */
__device__ __forceinline__ int64_t group_end(const int64_t* __restrict__ cut_ptr, int64_t fa,
                                             int64_t f_end, int64_t room, int64_t* slot) {
  int64_t fb = 0;
  if (threadIdx.x == 0) {
    fb = last_le(cut_ptr, fa, f_end + 1, cut_ptr[fa] + room);
    if (fb <= fa) fb = fa + 1;
  }
  return block_bcast(fb, slot);
}

/*! \brief the float whose order-preserving u32 is u */
__device__ __forceinline__ float ordered_to_float(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) != 0u ? (u ^ 0x80000000u) : ~u);
}

// ---------------------------------------------------------------- GB1
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void k_gbdt_cuts(const int64_t* __restrict__ keys,
                                                        const int64_t* __restrict__ col_ptr,
                                                        int64_t nfeat, int64_t nnz, uint32_t max_bins,
                                                        int64_t* __restrict__ counts,
                                                        const int64_t* __restrict__ cut_ptr,
                                                        float* __restrict__ cut, int64_t capacity,
                                                        uint32_t* error) {
  const int lane = dev::lane_id();
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWaves;
  bool bad = false;
  for (int64_t f = static_cast<int64_t>(blockIdx.x) * kWaves + threadIdx.x / dev::kWave; f < nfeat;
       f += nwaves) {
    const int64_t lo = col_ptr[f];
    int64_t n = col_ptr[f + 1] - lo;
    if (lo < 0 || n < 0 || lo + n > nnz) n = 0;  // not a column pointer of these keys
    const uint64_t un = static_cast<uint64_t>(n);
    const uint32_t m = un < max_bins ? static_cast<uint32_t>(un) : max_bins;
    // candidate k (0-based) of the m: entry k when all are taken, else the quantile
    auto pick = [&](uint32_t k) -> int64_t {
      if (un <= max_bins) return k;
      return static_cast<int64_t>(((static_cast<uint64_t>(k) + 1) * un + max_bins - 1) / max_bins - 1);
    };
    if (!kEmit && n > 0 && lane == 0) {
      // NaNs sort to the ends: below -inf with the sign bit, above +inf without
      const uint32_t first = static_cast<uint32_t>(keys[lo]);
      const uint32_t last = static_cast<uint32_t>(keys[lo + n - 1]);
      bad |= first < 0x007FFFFFu || last > 0xFF800000u;
    }
    int64_t out = kEmit ? cut_ptr[f] : 0;
    uint32_t total = 0;
    for (uint32_t k0 = 0; k0 < m; k0 += dev::kWave) {
      const uint32_t k = k0 + lane;
      bool keep = false;
      uint32_t u = 0;
      if (k < m) {
        u = static_cast<uint32_t>(keys[lo + pick(k)]);
        keep = k == 0 || u != static_cast<uint32_t>(keys[lo + pick(k - 1)]);
      }
      const uint64_t mask = __ballot(keep);
      if (kEmit && keep) {
        const int64_t p = out + __popcll(mask & ((1ull << lane) - 1ull));
        if (p < capacity) cut[p] = ordered_to_float(u);
      }
      const uint32_t kept = static_cast<uint32_t>(__popcll(mask));
      out += kept;
      total += kept;
    }
    if (!kEmit && lane == 0) counts[f] = total;
  }
  if (!kEmit) report(bad, kGbdtErrNaN, error);
}

// ---------------------------------------------------------------- GB2
__global__ __launch_bounds__(kThreads) void k_gbdt_bin(const int64_t* __restrict__ col_ptr,
                                                       const uint32_t* __restrict__ rows_in,
                                                       const float* __restrict__ vals_in,
                                                       int64_t stride, int64_t nnz, int64_t nfeat,
                                                       const int64_t* __restrict__ cut_ptr,
                                                       const float* __restrict__ cut,
                                                       int32_t* __restrict__ row_out,
                                                       uint8_t* __restrict__ bin_out,
                                                       uint32_t* error) {
  __shared__ float s_cut[kCutsLds];
  __shared__ uint32_t s_col[kColsLds];
  __shared__ int64_t s_slot;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSeg;
  const int64_t end = base + kSeg < nnz ? base + kSeg : nnz;
  int64_t f_lo, f_hi;
  segment_columns(col_ptr, nfeat, base, end, &s_slot, &f_lo, &f_hi);
  const bool staged = stage_columns(col_ptr, f_lo, f_hi, base, s_col);
  bool bad = false;
  for (int64_t fa = f_lo; fa <= f_hi;) {
    const int64_t fb = group_end(cut_ptr, fa, f_hi + 1, kCutsLds, &s_slot);
    const int64_t c0 = cut_ptr[fa];
    int64_t width = cut_ptr[fb] - c0;
    if (width > kCutsLds) width = kCutsLds;  // a column of more than kGbdtMaxBins cuts: refused above
    for (int64_t i = threadIdx.x; i < width; i += kThreads) s_cut[i] = cut[c0 + i];
    __syncthreads();
    const int64_t e0 = col_ptr[fa] > base ? col_ptr[fa] : base;
    const int64_t e1 = col_ptr[fb] < end ? col_ptr[fb] : end;
    for (int64_t j = e0 + threadIdx.x; j < e1; j += kThreads) {
      const int64_t f = column_of(staged, s_col, col_ptr, f_lo, fa, fb, base, j);
      const int64_t cl = cut_ptr[f] - c0;
      int64_t nc = cut_ptr[f + 1] - cut_ptr[f];
      if (cl + nc > width) nc = width - cl;
      const float x = vals_in != nullptr ? vals_in[j * stride] : 1.0f;
      bad |= x != x;
      // the cuts ascend strictly: the first one that is >= x
      int64_t lo = 0, hi = nc;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (s_cut[cl + mid] < x) {
          lo = mid + 1;
        } else {
          hi = mid;
        }
      }
      if (lo >= nc) lo = nc > 0 ? nc - 1 : 0;
      row_out[j] = static_cast<int32_t>(rows_in[j * stride]);
      bin_out[j] = static_cast<uint8_t>(lo);
    }
    __syncthreads();
    fa = fb;
  }
  report(bad, kGbdtErrNaN, error);
}

// ---------------------------------------------------------------- GB3
__global__ __launch_bounds__(kThreads) void k_gbdt_hist(
    const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row,
    const uint8_t* __restrict__ bin, int64_t nnz, int64_t nfeat, const int64_t* __restrict__ cut_ptr,
    int64_t total_bins, const float* __restrict__ grad, const float* __restrict__ hess,
    const int32_t* __restrict__ pos, int64_t rows, int32_t first_node, int32_t num_nodes, double scale,
    unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long s_acc[2 * kGbdtCells];
  __shared__ uint32_t s_col[kColsLds];
  __shared__ int64_t s_slot;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSeg;
  const int64_t end = base + kSeg < nnz ? base + kSeg : nnz;
  int64_t f_lo, f_hi;
  segment_columns(col_ptr, nfeat, base, end, &s_slot, &f_lo, &f_hi);
  const bool staged = stage_columns(col_ptr, f_lo, f_hi, base, s_col);
  // bins of a column that other segments hold entries of: [.., head_end) and [tail_begin, ..)
  const int64_t head_end = col_ptr[f_lo] < base ? cut_ptr[f_lo + 1] : -1;
  const int64_t tail_begin = col_ptr[f_hi + 1] > end ? cut_ptr[f_hi] : total_bins;
  int64_t room = kGbdtCells / num_nodes;
  if (room < static_cast<int64_t>(kGbdtMaxBins)) room = kGbdtMaxBins;
  for (int64_t fa = f_lo; fa <= f_hi;) {
    const int64_t fb = group_end(cut_ptr, fa, f_hi + 1, room, &s_slot);
    const int64_t c0 = cut_ptr[fa];
    int64_t width = cut_ptr[fb] - c0;
    if (width > kGbdtCells) width = kGbdtCells;
    const int64_t e0 = col_ptr[fa] > base ? col_ptr[fa] : base;
    const int64_t e1 = col_ptr[fb] < end ? col_ptr[fb] : end;
    if (width > 0 && c0 + width <= total_bins) {
      int64_t per_pass = kGbdtCells / width;
      if (per_pass > num_nodes) per_pass = num_nodes;
      for (int64_t n0 = 0; n0 < num_nodes; n0 += per_pass) {
        const int64_t nn = n0 + per_pass <= num_nodes ? per_pass : num_nodes - n0;
        const int64_t cells = nn * width;
        for (int64_t i = threadIdx.x; i < 2 * cells; i += kThreads) s_acc[i] = 0ull;
        __syncthreads();
        for (int64_t j = e0 + threadIdx.x; j < e1; j += kThreads) {
          const int64_t f = column_of(staged, s_col, col_ptr, f_lo, fa, fb, base, j);
          const int64_t cl = cut_ptr[f] - c0;
          const int64_t nc = cut_ptr[f + 1] - cut_ptr[f];
          const int64_t b = bin[j];
          const uint64_t r = static_cast<uint32_t>(row[j]);
          if (cl < 0 || b >= nc || cl + b >= width || r >= static_cast<uint64_t>(rows)) continue;
          const int64_t node = static_cast<int64_t>(pos[r]) - first_node - n0;
          if (node < 0 || node >= nn) continue;
          const long long qg = __double2ll_rn(static_cast<double>(grad[r]) * scale);
          const long long qh = __double2ll_rn(static_cast<double>(hess[r]) * scale);
          unsigned long long* const cell = s_acc + 2 * (node * width + cl + b);
          atomicAdd(cell, static_cast<unsigned long long>(qg));
          atomicAdd(cell + 1, static_cast<unsigned long long>(qh));
        }
        __syncthreads();
        const uint32_t width32 = static_cast<uint32_t>(width);  // cells <= kGbdtCells
        for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(cells); i += kThreads) {
          const int64_t node = i / width32, gb = c0 + i % width32;
          const unsigned long long g = s_acc[2 * i], h = s_acc[2 * i + 1];
          unsigned long long* const dst = hist + 2 * ((n0 + node) * total_bins + gb);
          if (gb >= head_end && gb < tail_begin) {
            dst[0] = g;
            dst[1] = h;
          } else {
            if (g != 0ull) atomicAdd(dst, g);
            if (h != 0ull) atomicAdd(dst + 1, h);
          }
        }
        __syncthreads();
      }
    }
    fa = fb;
  }
}

// ---------------------------------------------------------------- GB4
/*! \brief a split candidate; key = feature << 9 | bin << 1 | missing-left */
struct Cand {
  double gain;
  unsigned long long key;
};
constexpr unsigned long long kNoKey = ~0ull;

/*! \brief a total order: the greater gain, then the lower (feature, bin), then missing-right */
__device__ __forceinline__ Cand better(const Cand& a, const Cand& b) {
  return (a.gain > b.gain || (a.gain == b.gain && a.key < b.key)) ? a : b;
}

/*! \brief the workgroup's best candidate, in thread 0 */
__device__ __forceinline__ Cand block_best(Cand c) {
  __shared__ double s_gain[kWaves];
  __shared__ unsigned long long s_key[kWaves];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    Cand o;
    o.gain = __shfl_xor(c.gain, d, dev::kWave);
    o.key = __shfl_xor(c.key, d, dev::kWave);
    c = better(c, o);
  }
  if (dev::lane_id() == 0) {
    s_gain[threadIdx.x / dev::kWave] = c.gain;
    s_key[threadIdx.x / dev::kWave] = c.key;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) c = better(c, Cand{s_gain[w], s_key[w]});
  }
  return c;
}

__global__ __launch_bounds__(kThreads) void k_gbdt_split_scan(
    const long long* __restrict__ hist, const long long* __restrict__ node_sum,
    const int64_t* __restrict__ cut_ptr, int64_t nfeat, int64_t total_bins, double scale,
    double reg_lambda, double gamma, double min_child_weight, Cand* __restrict__ partial) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t node = blockIdx.y;
  Cand best{0.0, kNoKey};
  if (f < nfeat) {
    const int64_t c0 = cut_ptr[f];
    int64_t nc = cut_ptr[f + 1] - c0;
    if (c0 < 0 || c0 + nc > total_bins || nc > static_cast<int64_t>(kGbdtMaxBins)) nc = 0;
    if (nc > 0) {
      const long long* const h = hist + 2 * (node * total_bins + c0);
      const long long ng = node_sum[2 * node], nh = node_sum[2 * node + 1];
      long long tg = 0, th = 0;
      for (int64_t t = 0; t < nc; ++t) {
        tg += h[2 * t];
        th += h[2 * t + 1];
      }
      const long long miss_g = ng - tg, miss_h = nh - th;  // rows without an entry in f
      const double g_all = static_cast<double>(ng) / scale, h_all = static_cast<double>(nh) / scale;
      const double parent = g_all * g_all / (h_all + reg_lambda);
      long long lg = 0, lh = 0;
      for (int64_t t = 0; t < nc; ++t) {
        lg += h[2 * t];
        lh += h[2 * t + 1];
        for (int dir = 0; dir < 2; ++dir) {  // 0: missing goes right, 1: left
          const long long qgl = lg + (dir != 0 ? miss_g : 0ll), qhl = lh + (dir != 0 ? miss_h : 0ll);
          const double gl = static_cast<double>(qgl) / scale, hl = static_cast<double>(qhl) / scale;
          const double gr = static_cast<double>(ng - qgl) / scale;
          const double hr = static_cast<double>(nh - qhl) / scale;
          if (!(hl >= min_child_weight && hr >= min_child_weight)) continue;
          const double gain =
              0.5 * (gl * gl / (hl + reg_lambda) + gr * gr / (hr + reg_lambda) - parent) - gamma;
          if (gain > 0.0) {
            const unsigned long long key = (static_cast<unsigned long long>(f) << 9) |
                                           (static_cast<unsigned long long>(t) << 1) |
                                           static_cast<unsigned long long>(dir);
            best = better(best, Cand{gain, key});
          }
        }
      }
    }
  }
  best = block_best(best);
  if (threadIdx.x == 0) partial[node * gridDim.x + blockIdx.x] = best;
}

__global__ __launch_bounds__(kThreads) void k_gbdt_split_pick(const Cand* __restrict__ partial,
                                                              int64_t nparts,
                                                              int64_t* __restrict__ feature,
                                                              int32_t* __restrict__ bin,
                                                              uint8_t* __restrict__ default_left,
                                                              double* __restrict__ gain) {
  const int64_t node = blockIdx.x;
  Cand best{0.0, kNoKey};
  for (int64_t i = threadIdx.x; i < nparts; i += kThreads) {
    best = better(best, partial[node * nparts + i]);
  }
  best = block_best(best);
  if (threadIdx.x == 0) {
    const bool none = best.key == kNoKey;
    feature[node] = none ? -1 : static_cast<int64_t>(best.key >> 9);
    bin[node] = none ? 0 : static_cast<int32_t>((best.key >> 1) & 0xFFull);
    default_left[node] = none ? 0 : static_cast<uint8_t>(best.key & 1ull);
    gain[node] = none ? 0.0 : best.gain;
  }
}

// ---------------------------------------------------------------- GB5
__global__ __launch_bounds__(kThreads) void k_gbdt_advance_rows(
    const int32_t* __restrict__ pos_in, int64_t rows, const int64_t* __restrict__ feature,
    const uint8_t* __restrict__ default_left, const int32_t* __restrict__ left,
    const int32_t* __restrict__ right, int32_t first_node, int32_t num_nodes,
    int32_t* __restrict__ pos_out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; r < rows; r += stride) {
    const int32_t p = pos_in[r];
    const int64_t n = static_cast<int64_t>(p) - first_node;
    int32_t out = p;
    if (n >= 0 && n < num_nodes) {
      out = (feature[n] < 0 || default_left[n] != 0) ? left[n] : right[n];
    }
    pos_out[r] = out;
  }
}

__global__ __launch_bounds__(kThreads) void k_gbdt_advance_columns(
    const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row,
    const uint8_t* __restrict__ bin, int64_t nnz, int64_t nfeat, const int32_t* __restrict__ pos_in,
    int64_t rows, const int64_t* __restrict__ feature, const int32_t* __restrict__ split_bin,
    const int32_t* __restrict__ left, const int32_t* __restrict__ right, int32_t first_node,
    int32_t* __restrict__ pos_out) {
  const int64_t n = blockIdx.y;
  const int64_t f = feature[n];
  if (f < 0 || f >= nfeat) return;
  int64_t e0 = col_ptr[f], e1 = col_ptr[f + 1];
  if (e0 < 0) e0 = 0;
  if (e1 > nnz) e1 = nnz;
  const int32_t here = first_node + static_cast<int32_t>(n);
  const int32_t t = split_bin[n], to_left = left[n], to_right = right[n];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t j = e0 + static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < e1;
       j += stride) {
    const uint64_t r = static_cast<uint32_t>(row[j]);
    if (r >= static_cast<uint64_t>(rows) || pos_in[r] != here) continue;
    pos_out[r] = static_cast<int32_t>(bin[j]) <= t ? to_left : to_right;
  }
}

int SegmentsOf(uint64_t nnz) { return static_cast<int>((nnz + kSeg - 1) / kSeg); }

void CheckBinned(const char* op, uint64_t nnz, uint64_t num_features) {
  CHECK(num_features >= 1 && num_features <= CSRTransposeMaxFeatures())
      << op << ": num_features must be in [1, " << CSRTransposeMaxFeatures() << "]";
  CHECK_LT(nnz, (1ull << 31) * kSeg) << op << ": too many entries";
}
}  // namespace

uint64_t GbdtSegmentEntries() { return kGbdtSegmentEntries; }

void LaunchGbdtCutCount(const int64_t* keys, const CsrView& columns, uint64_t nnz, uint32_t max_bins,
                        int64_t* counts, uint32_t* error, hipStream_t stream) {
  CheckBinned("gbdt cuts", nnz, columns.nrows);
  CHECK(max_bins >= 2 && max_bins <= kGbdtMaxBins) << "gbdt cuts: max_bins must be in [2, 256]";
  hipLaunchKernelGGL(k_gbdt_cuts<false>, dim3(GridFor(columns.nrows, kWaves)), dim3(kThreads), 0,
                     stream, keys, reinterpret_cast<const int64_t*>(columns.offset),
                     static_cast<int64_t>(columns.nrows), static_cast<int64_t>(nnz), max_bins, counts,
                     nullptr, nullptr, int64_t{0}, error);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchGbdtCutEmit(const int64_t* keys, const CsrView& columns, uint64_t nnz, uint32_t max_bins,
                       const int64_t* cut_ptr, float* cut, uint64_t capacity, hipStream_t stream) {
  CheckBinned("gbdt cuts", nnz, columns.nrows);
  CHECK(max_bins >= 2 && max_bins <= kGbdtMaxBins) << "gbdt cuts: max_bins must be in [2, 256]";
  if (capacity == 0) return;
  hipLaunchKernelGGL(k_gbdt_cuts<true>, dim3(GridFor(columns.nrows, kWaves)), dim3(kThreads), 0,
                     stream, keys, reinterpret_cast<const int64_t*>(columns.offset),
                     static_cast<int64_t>(columns.nrows), static_cast<int64_t>(nnz), max_bins, nullptr,
                     cut_ptr, cut, static_cast<int64_t>(capacity), nullptr);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchGbdtBin(const CsrView& columns, uint64_t nnz, const int64_t* cut_ptr, const float* cut,
                   int32_t* row_out, uint8_t* bin_out, uint32_t* error, hipStream_t stream) {
  CheckView("gbdt bin", columns, true);
  CheckBinned("gbdt bin", nnz, columns.nrows);
  CHECK(!columns.index64) << "gbdt bin: a transpose has 32-bit row ids";
  if (nnz == 0) return;
  hipLaunchKernelGGL(k_gbdt_bin, dim3(SegmentsOf(nnz)), dim3(kThreads), 0, stream,
                     reinterpret_cast<const int64_t*>(columns.offset),
                     static_cast<const uint32_t*>(columns.index), columns.value,
                     int64_t{columns.paired ? 2 : 1}, static_cast<int64_t>(nnz),
                     static_cast<int64_t>(columns.nrows), cut_ptr, cut, row_out, bin_out, error);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchGbdtHistogram(const GbdtBinned& m, const float* grad, const float* hess,
                         const int32_t* pos, int32_t first_node, uint32_t num_nodes, double scale,
                         int64_t* hist, hipStream_t stream) {
  CheckBinned("gbdt histogram", m.nnz, m.num_features);
  CHECK(num_nodes >= 1 && num_nodes <= kGbdtMaxNodes) << "gbdt histogram: num_nodes out of range";
  if (m.nnz == 0 || m.total_bins == 0 || m.rows == 0) return;
  hipLaunchKernelGGL(k_gbdt_hist, dim3(SegmentsOf(m.nnz)), dim3(kThreads), 0, stream, m.offset, m.row,
                     m.bin, static_cast<int64_t>(m.nnz), static_cast<int64_t>(m.num_features),
                     m.cut_ptr, static_cast<int64_t>(m.total_bins), grad, hess, pos,
                     static_cast<int64_t>(m.rows), first_node, static_cast<int32_t>(num_nodes), scale,
                     reinterpret_cast<unsigned long long*>(hist));
  DMLC_HIP_CHECK_LAUNCH();
}

size_t GbdtSplitScratchBytes(uint64_t num_nodes, uint64_t num_features) {
  return sizeof(Cand) * num_nodes * ((num_features + kThreads - 1) / kThreads);
}

void LaunchGbdtBestSplits(const int64_t* hist, const int64_t* node_sum, const int64_t* cut_ptr,
                          uint64_t num_features, uint64_t total_bins, uint32_t num_nodes, double scale,
                          double reg_lambda, double gamma, double min_child_weight, void* scratch,
                          int64_t* feature, int32_t* bin, uint8_t* default_left, double* gain,
                          hipStream_t stream) {
  CheckBinned("gbdt best splits", 0, num_features);
  CHECK(num_nodes <= kGbdtMaxNodes) << "gbdt best splits: num_nodes out of range";
  CHECK(reg_lambda > 0.0 && scale > 0.0) << "gbdt best splits: reg_lambda and scale must be > 0";
  CHECK(Aligned16(scratch)) << "gbdt best splits: scratch must be 16-byte aligned";
  if (num_nodes == 0) return;
  const uint32_t parts = static_cast<uint32_t>((num_features + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(k_gbdt_split_scan, dim3(parts, num_nodes), dim3(kThreads), 0, stream,
                     reinterpret_cast<const long long*>(hist),
                     reinterpret_cast<const long long*>(node_sum), cut_ptr,
                     static_cast<int64_t>(num_features), static_cast<int64_t>(total_bins), scale,
                     reg_lambda, gamma, min_child_weight, static_cast<Cand*>(scratch));
  DMLC_HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gbdt_split_pick, dim3(num_nodes), dim3(kThreads), 0, stream,
                     static_cast<const Cand*>(scratch), static_cast<int64_t>(parts), feature, bin,
                     default_left, gain);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchGbdtAdvance(const GbdtBinned& m, const int32_t* pos_in, const int64_t* feature,
                       const int32_t* split_bin, const uint8_t* default_left, const int32_t* left,
                       const int32_t* right, int32_t first_node, uint32_t num_nodes, int32_t* pos_out,
                       hipStream_t stream) {
  CheckBinned("gbdt advance", m.nnz, m.num_features);
  CHECK(num_nodes <= kGbdtMaxNodes) << "gbdt advance: num_nodes out of range";
  CHECK(pos_in != pos_out) << "gbdt advance: pos is not updated in place";
  if (m.rows == 0) return;
  hipLaunchKernelGGL(k_gbdt_advance_rows, dim3(GridFor(m.rows, kThreads)), dim3(kThreads), 0, stream,
                     pos_in, static_cast<int64_t>(m.rows), feature, default_left, left, right,
                     first_node, static_cast<int32_t>(num_nodes), pos_out);
  DMLC_HIP_CHECK_LAUNCH();
  if (num_nodes == 0 || m.nnz == 0) return;
  // a node's column is walked by up to 64 workgroups: a hot split feature is not one workgroup's
  int blocks = SegmentsOf(m.nnz);
  if (blocks > 64) blocks = 64;
  hipLaunchKernelGGL(k_gbdt_advance_columns, dim3(blocks, num_nodes), dim3(kThreads), 0, stream,
                     m.offset, m.row, m.bin, static_cast<int64_t>(m.nnz),
                     static_cast<int64_t>(m.num_features), pos_in, static_cast<int64_t>(m.rows),
                     feature, split_bin, left, right, first_node, pos_out);
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
