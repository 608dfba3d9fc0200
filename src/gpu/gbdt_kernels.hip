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
 *  GB3m k_gbdt_hist_multi, GB4m k_gbdt_split_scan_multi: GB3 / GB4 for trees
 *                      with K values per leaf (K gradients per row): a group of
 *                      lanes per entry / per (node, feature), one lane per
 *                      output; described at the kernels.  Each pair has one
 *                      launcher, which picks the kernel by its num_outputs
 *                      (kGbdtScalar: GB3 / GB4), and shares its cell arithmetic
 *                      (add_to_cell, flush_cell) and candidate key (split_key).
 *  GB9 k_gbdt_level_*  GB3 and GB4 of one level fused: a workgroup owns whole columns,
 *                      sums them in LDS and scans the sums there for the best
 *                      thresholds, so no node histogram is written; columns
 *                      longer than a segment go through a small spill histogram.
 *                      Described at the kernels; the answer is GB4's, bit for bit.
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

/*! \brief GB3 / GB3m: the quantised (g, h) of an entry's row added to cell `at` of the LDS table */
__device__ __forceinline__ void add_to_cell(unsigned long long* table, int64_t at, float g, float h,
                                            double scale) {
  const long long qg = __double2ll_rn(static_cast<double>(g) * scale);
  const long long qh = __double2ll_rn(static_cast<double>(h) * scale);
  unsigned long long* const cell = table + 2 * at;
  atomicAdd(cell, static_cast<unsigned long long>(qg));
  atomicAdd(cell + 1, static_cast<unsigned long long>(qh));
}

/*! \brief GB3 / GB3m: a finished cell to the histogram: plain stores where this segment owns the
 *  bin's column, else one 64-bit atomic per non-zero value */
__device__ __forceinline__ void flush_cell(unsigned long long* dst, unsigned long long g,
                                           unsigned long long h, bool owned) {
  if (owned) {
    dst[0] = g;
    dst[1] = h;
  } else {
    if (g != 0ull) atomicAdd(dst, g);
    if (h != 0ull) atomicAdd(dst + 1, h);
  }
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
          add_to_cell(s_acc, node * width + cl + b, grad[r], hess[r], scale);
        }
        __syncthreads();
        const uint32_t width32 = static_cast<uint32_t>(width);  // cells <= kGbdtCells
        for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(cells); i += kThreads) {
          const int64_t node = i / width32, gb = c0 + i % width32;
          const unsigned long long g = s_acc[2 * i], h = s_acc[2 * i + 1];
          unsigned long long* const dst = hist + 2 * ((n0 + node) * total_bins + gb);
          flush_cell(dst, g, h, gb >= head_end && gb < tail_begin);
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

/*! \brief GB4 / GB4m: Cand::key of feature f, bin t and missing-left dir */
__device__ __forceinline__ unsigned long long split_key(int64_t f, int64_t t, int dir) {
  return (static_cast<unsigned long long>(f) << 9) | (static_cast<unsigned long long>(t) << 1) |
         static_cast<unsigned long long>(dir);
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
          if (gain > 0.0) best = better(best, Cand{gain, split_key(f, t, dir)});
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

// ---------------------------------------------------------------- GB9
/*! \brief the first k in [0, n] with ptr[k] >= x; ptr [n + 1] ascends from ptr[0] >= 0 */
__device__ __forceinline__ int64_t first_ge(const int64_t* __restrict__ ptr, int64_t n, int64_t x) {
  if (x <= ptr[0]) return 0;
  return last_le(ptr, 0, n, x - 1) + 1;
}

/*! \brief stage_columns for GB9: col_ptr[f_lo .. f_end] - base clamped to [0, 2 kSeg], the span of
 *  the entries a workgroup owns (short columns that start inside one segment) */
__device__ __forceinline__ bool stage_owned_columns(const int64_t* __restrict__ col_ptr, int64_t f_lo,
                                                    int64_t f_end, int64_t base, uint32_t* s_col) {
  const int64_t n = f_end - f_lo + 1;
  if (n > kColsLds) return false;
  for (int64_t k = threadIdx.x; k < n; k += kThreads) {
    const int64_t d = col_ptr[f_lo + k] - base;
    s_col[k] = static_cast<uint32_t>(d < 0 ? 0 : (d > 2 * kSeg ? 2 * kSeg : d));
  }
  __syncthreads();
  return true;
}

/*! \brief k_gbdt_split_scan's walk over the nc (g, h) cells at h (LDS or global) of feature f
 *  under the node sums (ng, nh): the same statements, so the same bits in every gain */
__device__ __forceinline__ Cand scan_cells(const long long* h, int64_t nc, int64_t f, long long ng,
                                           long long nh, double scale, double reg_lambda,
                                           double gamma, double min_child_weight) {
  Cand best{0.0, kNoKey};
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
      if (gain > 0.0) best = better(best, Cand{gain, split_key(f, t, dir)});
    }
  }
  return best;
}

/*! \brief the level's constants of the split search */
struct LevelGain {
  const long long* node_sum;
  double scale, reg_lambda, gamma, min_child_weight;
};

/*!
 * \brief GB9, the short columns: histogram and split search of a level in one launch, without
 *  the node histogram.
 *
 *  Ownership.  Workgroup s owns the columns of 1 .. kSeg entries (and the empty ones) whose
 *  first entry lies in [s S, (s + 1) S): whole columns, so their (node, bin) sums are complete
 *  in its LDS.  It streams them to their end, fewer than 2 S entries; a longer column that
 *  starts there is the last of the range and belongs to the spill kernels below.  The grid has
 *  nnz / S + 1 workgroups, so that empty columns behind the last entry have an owner too.
 *
 *  Passes.  As GB3: groups of consecutive columns whose W cells fit the table, and passes of
 *  as many nodes as fit.  The cells of a node lie W | 1 apart, an odd number of 16-byte cells.
 *
 *  Scan.  After a pass one lane per (node of the pass, column of the group) walks the column's
 *  cells in LDS.  A wave takes a contiguous quarter of the pass's nodes; within it the lanes run
 *  over the columns first and the nodes second (lane = node x ncol + column), a whole number of
 *  nodes per step.  Lanes on neighbouring columns of a node read cells that lie the columns' cut
 *  counts apart, and lanes on neighbouring nodes cells that lie W | 1 apart: with the node stride
 *  W itself, every W that is a multiple of 16 cells (256 bytes, all 64 banks) would put the lanes
 *  of one column, one per node, on the same banks at every step -- 21 ways for three 16-bin
 *  columns.  The odd stride spreads 16 neighbouring nodes over all banks, at the price of one
 *  cell per node (14 instead of 15 nodes of a 256-cut column per pass).  The candidates of a node
 *  meet by a segmented shuffle reduction under better(), and the segment's first lane folds the
 *  result into partial[node, s] by a plain load and store: the workgroup is the only writer of
 *  its slots, and its own accesses are ordered by the barriers between the passes.
 */
__global__ __launch_bounds__(kThreads) void k_gbdt_level_short(
    const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row,
    const uint8_t* __restrict__ bin, int64_t nnz, int64_t nfeat, const int64_t* __restrict__ cut_ptr,
    int64_t total_bins, const float* __restrict__ grad, const float* __restrict__ hess,
    const int32_t* __restrict__ pos, int64_t rows, int32_t first_node, int32_t num_nodes,
    LevelGain lg, Cand* partial, int64_t nparts) {
  __shared__ unsigned long long s_acc[2 * kGbdtCells];
  __shared__ uint32_t s_col[kColsLds];
  __shared__ int64_t s_slot;
  const Cand none{0.0, kNoKey};
  for (int64_t n = threadIdx.x; n < num_nodes; n += kThreads) partial[n * nparts + blockIdx.x] = none;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSeg;
  int64_t a = 0, b = 0;
  if (threadIdx.x == 0) {
    a = first_ge(col_ptr, nfeat, base);
    b = first_ge(col_ptr, nfeat, base + kSeg);
    if (b > a && col_ptr[b] - col_ptr[b - 1] > kSeg) --b;  // a long column: the spill path's
  }
  const int64_t f_lo = block_bcast(a, &s_slot);
  const int64_t f_end = block_bcast(b, &s_slot);
  if (f_lo >= f_end) return;  // no short column starts here
  const int64_t e_first = col_ptr[f_lo];
  const bool staged = stage_owned_columns(col_ptr, f_lo, f_end, e_first, s_col);
  int64_t room = kGbdtCells / num_nodes - 1;  // W <= room: every node in one pass
  if (room < static_cast<int64_t>(kGbdtMaxBins)) room = kGbdtMaxBins;
  const int lane = dev::lane_id(), wave = threadIdx.x / dev::kWave;
  for (int64_t fa = f_lo; fa < f_end;) {
    const int64_t fb = group_end(cut_ptr, fa, f_end, room, &s_slot);
    const int64_t c0 = cut_ptr[fa];
    const int64_t width = cut_ptr[fb] - c0;
    const int64_t e0 = col_ptr[fa] > 0 ? col_ptr[fa] : 0;
    const int64_t e1 = col_ptr[fb] < nnz ? col_ptr[fb] : nnz;
    if (width > 0 && width < kGbdtCells && c0 >= 0 && c0 + width <= total_bins) {
      const int64_t stride = width | 1;
      int64_t per_pass = kGbdtCells / stride;
      if (per_pass > num_nodes) per_pass = num_nodes;
      const int64_t ncol = fb - fa;
      for (int64_t n0 = 0; n0 < num_nodes; n0 += per_pass) {
        const int64_t nn = n0 + per_pass <= num_nodes ? per_pass : num_nodes - n0;
        for (int64_t i = threadIdx.x; i < 2 * nn * stride; i += kThreads) s_acc[i] = 0ull;
        __syncthreads();
        for (int64_t j = e0 + threadIdx.x; j < e1; j += kThreads) {
          const int64_t f = column_of(staged, s_col, col_ptr, f_lo, fa, fb, e_first, j);
          const int64_t cl = cut_ptr[f] - c0;
          const int64_t nc = cut_ptr[f + 1] - cut_ptr[f];
          const int64_t bj = bin[j];
          const uint64_t r = static_cast<uint32_t>(row[j]);
          if (cl < 0 || bj >= nc || cl + bj >= width || r >= static_cast<uint64_t>(rows)) continue;
          const int64_t node = static_cast<int64_t>(pos[r]) - first_node - n0;
          if (node < 0 || node >= nn) continue;
          add_to_cell(s_acc, node * stride + cl + bj, grad[r], hess[r], lg.scale);
        }
        __syncthreads();
        // the scan: this wave's nodes [w_lo, w_hi) of the pass
        const int64_t share = (nn + kWaves - 1) / kWaves;
        const int64_t w_lo = wave * share;
        const int64_t w_hi = w_lo + share < nn ? w_lo + share : nn;
        auto scan = [&](int64_t ln, int64_t f) -> Cand {
          const int64_t cl = cut_ptr[f] - c0;
          const int64_t nc = cut_ptr[f + 1] - cut_ptr[f];
          if (cl < 0 || nc <= 0 || nc > static_cast<int64_t>(kGbdtMaxBins) || cl + nc > width) {
            return none;
          }
          const long long* const cells = reinterpret_cast<const long long*>(s_acc);
          return scan_cells(cells + 2 * (ln * stride + cl), nc, f, lg.node_sum[2 * (n0 + ln)],
                            lg.node_sum[2 * (n0 + ln) + 1], lg.scale, lg.reg_lambda, lg.gamma,
                            lg.min_child_weight);
        };
        auto keep = [&](int64_t ln, const Cand& c) {
          if (c.key == kNoKey) return;
          Cand* const slot = partial + (n0 + ln) * nparts + blockIdx.x;
          *slot = better(*slot, c);
        };
        if (ncol <= dev::kWave) {
          const int nc_lanes = static_cast<int>(ncol);
          const int per_step = dev::kWave / nc_lanes;  // whole nodes per step of the wave
          const int sub = lane / nc_lanes, col = lane % nc_lanes;
          for (int64_t k0 = w_lo; k0 < w_hi; k0 += per_step) {
            const int64_t ln = k0 + sub;
            const bool active = sub < per_step && ln < w_hi;
            Cand c = active ? scan(ln, fa + col) : none;
            for (int d = 1; d < nc_lanes; d <<= 1) {
              Cand o;
              o.gain = __shfl_down(c.gain, d, dev::kWave);
              o.key = __shfl_down(c.key, d, dev::kWave);
              if (col + d < nc_lanes) c = better(c, o);
            }
            if (active && col == 0) keep(ln, c);
          }
        } else {
          for (int64_t ln = w_lo; ln < w_hi; ++ln) {
            Cand c = none;
            for (int64_t col = lane; col < ncol; col += dev::kWave) c = better(c, scan(ln, fa + col));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
              Cand o;
              o.gain = __shfl_xor(c.gain, d, dev::kWave);
              o.key = __shfl_xor(c.key, d, dev::kWave);
              c = better(c, o);
            }
            if (lane == 0) keep(ln, c);
          }
        }
        __syncthreads();
      }
    }
    fa = fb;
  }
}

/*!
 * \brief GB9, the list of the long columns (more than kSeg entries), made once per matrix by one
 *  workgroup: column[i], and the running sums bin_ptr[i] of their cut counts and piece_ptr[i] of
 *  their pieces of kSeg entries, i < capacity; totals = (columns, bins, pieces).  The waves flag
 *  256 columns at a time by ballot and thread 0 appends the flagged ones in order.
 */
__global__ __launch_bounds__(kThreads) void k_gbdt_long_columns(
    const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ cut_ptr, int64_t nfeat,
    int64_t capacity, int64_t* __restrict__ column, int64_t* __restrict__ bin_ptr,
    int64_t* __restrict__ piece_ptr, int64_t* __restrict__ totals) {
  __shared__ unsigned long long s_mask[kWaves];
  int64_t count = 0, bins = 0, pieces = 0;  // thread 0's
  for (int64_t f0 = 0; f0 < nfeat; f0 += kThreads) {
    const int64_t f = f0 + threadIdx.x;
    const unsigned long long mask = __ballot(f < nfeat && col_ptr[f + 1] - col_ptr[f] > kSeg);
    if (dev::lane_id() == 0) s_mask[threadIdx.x / dev::kWave] = mask;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < kWaves; ++w) {
        for (unsigned long long m = s_mask[w]; m != 0ull && count < capacity; m &= m - 1ull) {
          const int64_t g = f0 + w * dev::kWave + __builtin_ctzll(m);
          int64_t nc = cut_ptr[g + 1] - cut_ptr[g];
          if (nc < 0 || nc > static_cast<int64_t>(kGbdtMaxBins)) nc = 0;
          column[count] = g;
          bin_ptr[count] = bins;
          piece_ptr[count] = pieces;
          ++count;
          bins += nc;
          pieces += (col_ptr[g + 1] - col_ptr[g] + kSeg - 1) / kSeg;
        }
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    bin_ptr[count] = bins;
    piece_ptr[count] = pieces;
    totals[0] = count;
    totals[1] = bins;
    totals[2] = pieces;
  }
}

/*! \brief GB9: clears the spill histogram */
__global__ __launch_bounds__(kThreads) void k_gbdt_level_clear(unsigned long long* __restrict__ p,
                                                               int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    p[i] = 0ull;
  }
}

/*!
 * \brief GB9, the long columns' sums: workgroup p takes piece p (kSeg entries of one long
 *  column), sums it as GB3 does and adds its non-zero cells to spill [N x spill_bins x 2], where
 *  the column's bins start at bin_ptr[i], with one 64-bit atomic each
 */
__global__ __launch_bounds__(kThreads) void k_gbdt_level_long_hist(
    const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row,
    const uint8_t* __restrict__ bin, int64_t nnz, const int64_t* __restrict__ cut_ptr,
    int64_t total_bins, const float* __restrict__ grad, const float* __restrict__ hess,
    const int32_t* __restrict__ pos, int64_t rows, int32_t first_node, int32_t num_nodes, double scale,
    const int64_t* __restrict__ column, const int64_t* __restrict__ bin_ptr,
    const int64_t* __restrict__ piece_ptr, int64_t count, int64_t spill_bins,
    unsigned long long* __restrict__ spill) {
  __shared__ unsigned long long s_acc[2 * kGbdtCells];
  __shared__ int64_t s_slot;
  const int64_t piece = blockIdx.x;
  const int64_t li =
      block_bcast(threadIdx.x == 0 ? last_le(piece_ptr, 0, count, piece) : 0, &s_slot);
  const int64_t f = column[li];
  const int64_t c0 = cut_ptr[f], width = cut_ptr[f + 1] - c0, sb = bin_ptr[li];
  if (width <= 0 || width > static_cast<int64_t>(kGbdtMaxBins) || c0 < 0 ||
      c0 + width > total_bins || sb < 0 || sb + width > spill_bins) {
    return;
  }
  int64_t e0 = col_ptr[f] + (piece - piece_ptr[li]) * kSeg;
  int64_t e1 = e0 + kSeg < col_ptr[f + 1] ? e0 + kSeg : col_ptr[f + 1];
  if (e0 < 0) e0 = 0;
  if (e1 > nnz) e1 = nnz;
  int64_t per_pass = kGbdtCells / width;
  if (per_pass > num_nodes) per_pass = num_nodes;
  for (int64_t n0 = 0; n0 < num_nodes; n0 += per_pass) {
    const int64_t nn = n0 + per_pass <= num_nodes ? per_pass : num_nodes - n0;
    const int64_t cells = nn * width;
    for (int64_t i = threadIdx.x; i < 2 * cells; i += kThreads) s_acc[i] = 0ull;
    __syncthreads();
    for (int64_t j = e0 + threadIdx.x; j < e1; j += kThreads) {
      const int64_t bj = bin[j];
      const uint64_t r = static_cast<uint32_t>(row[j]);
      if (bj >= width || r >= static_cast<uint64_t>(rows)) continue;
      const int64_t node = static_cast<int64_t>(pos[r]) - first_node - n0;
      if (node < 0 || node >= nn) continue;
      add_to_cell(s_acc, node * width + bj, grad[r], hess[r], scale);
    }
    __syncthreads();
    const uint32_t width32 = static_cast<uint32_t>(width);
    for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(cells); i += kThreads) {
      const int64_t node = i / width32, lb = i % width32;
      flush_cell(spill + 2 * ((n0 + node) * spill_bins + sb + lb), s_acc[2 * i], s_acc[2 * i + 1],
                 false);
    }
    __syncthreads();
  }
}

/*! \brief GB9, the long columns' candidates: GB4's lane per (node, column) over the spill
 *  histogram, keyed by the true feature id, to the slots behind the short columns' */
__global__ __launch_bounds__(kThreads) void k_gbdt_level_long_scan(
    const long long* __restrict__ spill, const int64_t* __restrict__ cut_ptr, int64_t total_bins,
    const int64_t* __restrict__ column, const int64_t* __restrict__ bin_ptr, int64_t count,
    int64_t spill_bins, LevelGain lg, Cand* __restrict__ partial, int64_t nparts, int64_t part0) {
  const int64_t li = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t node = blockIdx.y;
  Cand best{0.0, kNoKey};
  if (li < count) {
    const int64_t f = column[li];
    const int64_t c0 = cut_ptr[f], sb = bin_ptr[li];
    int64_t nc = cut_ptr[f + 1] - c0;
    if (c0 < 0 || c0 + nc > total_bins || nc > static_cast<int64_t>(kGbdtMaxBins) || sb < 0 ||
        sb + nc > spill_bins) {
      nc = 0;
    }
    if (nc > 0) {
      best = scan_cells(spill + 2 * (node * spill_bins + sb), nc, f, lg.node_sum[2 * node],
                        lg.node_sum[2 * node + 1], lg.scale, lg.reg_lambda, lg.gamma,
                        lg.min_child_weight);
    }
  }
  best = block_best(best);
  if (threadIdx.x == 0) partial[node * nparts + part0 + blockIdx.x] = best;
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

// ---------------------------------------------------------------- GB3m
/*!
 * \brief GB3 with K gradients per row (vector-leaf trees).  The segment scheme is GB3's; the
 *  lanes and the table are laid out for the [rows x K] gradients.  A group of Kp = 2^shift lanes
 *  owns one entry: row[j], bin[j] and pos[r] are one address for the group and g[r, k0 + lane]
 *  is one contiguous read of 4 kk bytes.  The table is [node][bin][k][g, h], so a group's
 *  atomics fall on consecutive banks and a flush writes 16 kk contiguous bytes per (node, bin).
 *  A pass holds nn nodes x kk outputs x the group's W bins, nn kk W <= kGbdtCells: all K outputs
 *  and as many nodes as fit, or -- when W K alone is too much (a 256-cut column with K >= 16) --
 *  one node and an even share kk of the outputs (kGbdtCells / 256 = 15 at least fit).  Unlike
 *  GB3, a group of columns is no wider than the bins that fit with every node and output (or
 *  one column), so only a single wide column tiles the nodes or the outputs.
 */
__global__ __launch_bounds__(kThreads) void k_gbdt_hist_multi(
    const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row,
    const uint8_t* __restrict__ bin, int64_t nnz, int64_t nfeat, const int64_t* __restrict__ cut_ptr,
    int64_t total_bins, const float* __restrict__ grad, const float* __restrict__ hess,
    const int32_t* __restrict__ pos, int64_t rows, int32_t first_node, int32_t num_nodes,
    int32_t num_out, double scale, unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long s_acc[2 * kGbdtCells];
  __shared__ uint32_t s_col[kColsLds];
  __shared__ int64_t s_slot;
  const int64_t K = num_out;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSeg;
  const int64_t end = base + kSeg < nnz ? base + kSeg : nnz;
  int64_t f_lo, f_hi;
  segment_columns(col_ptr, nfeat, base, end, &s_slot, &f_lo, &f_hi);
  const bool staged = stage_columns(col_ptr, f_lo, f_hi, base, s_col);
  const int64_t head_end = col_ptr[f_lo] < base ? cut_ptr[f_lo + 1] : -1;
  const int64_t tail_begin = col_ptr[f_hi + 1] > end ? cut_ptr[f_hi] : total_bins;
  // the bins whose num_nodes x K cells fill the table once (group_end takes one column at least):
  // a group's entries are streamed once per pass and a pass rejects, a whole lane group at a
  // time, the entries of other nodes, so wider groups only add passes over more entries
  int64_t room = kGbdtCells / (K * num_nodes);
  if (room < 1) room = 1;
  for (int64_t fa = f_lo; fa <= f_hi;) {
    const int64_t fb = group_end(cut_ptr, fa, f_hi + 1, room, &s_slot);
    const int64_t c0 = cut_ptr[fa];
    int64_t width = cut_ptr[fb] - c0;
    if (width > kGbdtCells) width = kGbdtCells;
    const int64_t e0 = col_ptr[fa] > base ? col_ptr[fa] : base;
    const int64_t e1 = col_ptr[fb] < end ? col_ptr[fb] : end;
    if (width > 0 && c0 + width <= total_bins) {
      int64_t kmax = kGbdtCells / width;  // >= 1
      if (kmax > K) kmax = K;
      const int64_t kpasses = (K + kmax - 1) / kmax;
      const int64_t kper = (K + kpasses - 1) / kpasses;  // <= kmax: an even share of the outputs
      int shift = 0;
      while ((int64_t{1} << shift) < kper) ++shift;  // kper <= kGbdtMaxOutputs: shift <= 5
      const int64_t lane = threadIdx.x & ((1 << shift) - 1);
      const int64_t first_entry = threadIdx.x >> shift, step = kThreads >> shift;
      int64_t per_pass = kGbdtCells / (width * kper);  // >= 1
      if (per_pass > num_nodes) per_pass = num_nodes;
      for (int64_t n0 = 0; n0 < num_nodes; n0 += per_pass) {
        const int64_t nn = n0 + per_pass <= num_nodes ? per_pass : num_nodes - n0;
        for (int64_t k0 = 0; k0 < K; k0 += kper) {
          const int64_t kk = k0 + kper <= K ? kper : K - k0;
          const int64_t cells = nn * width * kk;  // <= kGbdtCells
          for (int64_t i = threadIdx.x; i < 2 * cells; i += kThreads) s_acc[i] = 0ull;
          __syncthreads();
          if (lane < kk) {
            for (int64_t j = e0 + first_entry; j < e1; j += step) {
              const int64_t f = column_of(staged, s_col, col_ptr, f_lo, fa, fb, base, j);
              const int64_t cl = cut_ptr[f] - c0;
              const int64_t nc = cut_ptr[f + 1] - cut_ptr[f];
              const int64_t b = bin[j];
              const uint64_t r = static_cast<uint32_t>(row[j]);
              if (cl < 0 || b >= nc || cl + b >= width || r >= static_cast<uint64_t>(rows)) continue;
              const int64_t node = static_cast<int64_t>(pos[r]) - first_node - n0;
              if (node < 0 || node >= nn) continue;
              const int64_t at = static_cast<int64_t>(r) * K + k0 + lane;
              add_to_cell(s_acc, (node * width + cl + b) * kk + lane, grad[at], hess[at], scale);
            }
          }
          __syncthreads();
          const uint32_t kk32 = static_cast<uint32_t>(kk);
          const uint32_t width32 = static_cast<uint32_t>(width);
          for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(cells); i += kThreads) {
            const uint32_t k = i % kk32, nb = i / kk32;
            const int64_t node = nb / width32, gb = c0 + nb % width32;
            const unsigned long long g = s_acc[2 * i], h = s_acc[2 * i + 1];
            unsigned long long* const dst =
                hist + 2 * (((n0 + node) * total_bins + gb) * K + k0 + k);
            flush_cell(dst, g, h, gb >= head_end && gb < tail_begin);
          }
          __syncthreads();
        }
      }
    }
    fa = fb;
  }
}

// ---------------------------------------------------------------- GB4m
/*! \brief v summed over the aligned group of kKp lanes, in every lane: a butterfly of
 *  xor-shuffles, widest first.  Both partners add the same pair, so the (float64) sum is one
 *  value for the group and a pure function of the inputs. */
template <int kKp, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int d = kKp >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, dev::kWave);
  return v;
}

/*!
 * \brief GB4 with K outputs.  A group of kKp lanes (the power of two >= K) owns one (node,
 *  feature) and lane k output k's running left sums; per bin the group reads 16 K contiguous
 *  bytes of hist [N x bins x K x 2].  A workgroup walks the 256 features of its scalar
 *  counterpart in kKp rounds of 256 / kKp groups, so the partials (and the scratch) are GB4's.
 *  gain = 1/2 sum_k (GL_k^2 / (HL_k + l) + GR_k^2 / (HR_k + l) - G_k^2 / (H_k + l)) - gamma,
 *  valid with sum_k HL_k and sum_k HR_k >= min_hess = K min_child_weight scale on the integer
 *  sums.  The bin loop runs to the wave's longest column so that every shuffle has all of its
 *  lanes; a group past its own column only idles.
 */
template <int kKp>
__global__ __launch_bounds__(kThreads) void k_gbdt_split_scan_multi(
    const long long* __restrict__ hist, const long long* __restrict__ node_sum,
    const int64_t* __restrict__ cut_ptr, int64_t nfeat, int64_t total_bins, int32_t num_out,
    double scale, double reg_lambda, double gamma, double min_hess, Cand* __restrict__ partial) {
  constexpr int kGroups = kThreads / kKp;
  const int lane = threadIdx.x % kKp, group = threadIdx.x / kKp;
  const int64_t node = blockIdx.y, K = num_out;
  const bool on = lane < K;  // lanes past K carry zeros
  long long ng = 0, nh = 0;
  if (on) {
    ng = node_sum[2 * (node * K + lane)];
    nh = node_sum[2 * (node * K + lane) + 1];
  }
  const double g_all = static_cast<double>(ng) / scale, h_all = static_cast<double>(nh) / scale;
  const double parent = on ? g_all * g_all / (h_all + reg_lambda) : 0.0;
  const long long nh_all = group_sum<kKp>(nh);
  // GL^2 / (HL + l) + GR^2 / (HR + l) - G^2 / (H + l) of this lane's output
  auto term = [&](long long qgl, long long qhl) -> double {
    const double gl = static_cast<double>(qgl) / scale, hl = static_cast<double>(qhl) / scale;
    const double gr = static_cast<double>(ng - qgl) / scale;
    const double hr = static_cast<double>(nh - qhl) / scale;
    return on ? gl * gl / (hl + reg_lambda) + gr * gr / (hr + reg_lambda) - parent : 0.0;
  };
  Cand best{0.0, kNoKey};
  for (int round = 0; round < kKp; ++round) {
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + round * kGroups + group;
    int64_t c0 = 0, nc = 0;
    if (f < nfeat) {
      c0 = cut_ptr[f];
      nc = cut_ptr[f + 1] - c0;
      if (c0 < 0 || c0 + nc > total_bins || nc > static_cast<int64_t>(kGbdtMaxBins)) nc = 0;
    }
    int nc_wave = static_cast<int>(nc);
#pragma unroll
    for (int d = dev::kWave >> 1; d >= 1; d >>= 1) {
      const int o = __shfl_xor(nc_wave, d, dev::kWave);
      nc_wave = o > nc_wave ? o : nc_wave;
    }
    // read only by a lane with an output, below its column's nc
    const long long* const h = hist + 2 * ((node * total_bins + c0) * K + lane);
    long long tg = 0, th = 0;
    if (on) {
      for (int64_t t = 0; t < nc; ++t) {
        tg += h[2 * t * K];
        th += h[2 * t * K + 1];
      }
    }
    const long long miss_g = ng - tg, miss_h = nh - th;  // rows without an entry in f
    const long long miss_h_all = group_sum<kKp>(miss_h);
    long long lg = 0, lh = 0;
    for (int t = 0; t < nc_wave; ++t) {
      const bool live = t < nc;
      if (live && on) {
        lg += h[2 * t * K];
        lh += h[2 * t * K + 1];
      }
      const double sum_right = group_sum<kKp>(term(lg, lh));  // missing goes right
      const double sum_left = group_sum<kKp>(term(lg + miss_g, lh + miss_h));
      const long long hl_right = group_sum<kKp>(lh);
      if (!live || lane != 0) continue;
      for (int dir = 0; dir < 2; ++dir) {
        const long long hl = hl_right + (dir != 0 ? miss_h_all : 0ll);
        if (!(static_cast<double>(hl) >= min_hess && static_cast<double>(nh_all - hl) >= min_hess))
          continue;
        const double gain = 0.5 * (dir != 0 ? sum_left : sum_right) - gamma;
        if (gain > 0.0) best = better(best, Cand{gain, split_key(f, t, dir)});
      }
    }
  }
  best = block_best(best);
  if (threadIdx.x == 0) partial[node * gridDim.x + blockIdx.x] = best;
}

int SegmentsOf(uint64_t nnz) { return static_cast<int>((nnz + kSeg - 1) / kSeg); }

void CheckBinned(const char* op, uint64_t nnz, uint64_t num_features) {
  CHECK(num_features >= 1 && num_features <= CSRTransposeMaxFeatures())
      << op << ": num_features must be in [1, " << CSRTransposeMaxFeatures() << "]";
  CHECK_LT(nnz, (1ull << 31) * kSeg) << op << ": too many entries";
}

/*! \brief what the histogram and the split search check alike, in either layout */
void CheckLevel(const char* op, uint64_t nnz, uint64_t num_features, bool nodes_in_range,
                uint32_t num_outputs) {
  CheckBinned(op, nnz, num_features);
  CHECK(nodes_in_range) << op << ": num_nodes out of range";
  CHECK(num_outputs == kGbdtScalar || num_outputs <= kGbdtMaxOutputs)
      << op << ": num_outputs must be in [1, " << kGbdtMaxOutputs << "]";
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
                         const int32_t* pos, int32_t first_node, uint32_t num_nodes,
                         uint32_t num_outputs, double scale, int64_t* hist, hipStream_t stream) {
  const bool scalar = num_outputs == kGbdtScalar;
  CheckLevel(scalar ? "gbdt histogram" : "gbdt histogram multi", m.nnz, m.num_features,
             num_nodes >= 1 && num_nodes <= kGbdtMaxNodes, num_outputs);
  if (m.nnz == 0 || m.total_bins == 0 || m.rows == 0) return;
  const dim3 grid(SegmentsOf(m.nnz)), block(kThreads);
  const int64_t nnz = static_cast<int64_t>(m.nnz), nfeat = static_cast<int64_t>(m.num_features);
  const int64_t total = static_cast<int64_t>(m.total_bins), rows = static_cast<int64_t>(m.rows);
  const int32_t nodes = static_cast<int32_t>(num_nodes);
  unsigned long long* const out = reinterpret_cast<unsigned long long*>(hist);
  if (scalar) {
    hipLaunchKernelGGL(k_gbdt_hist, grid, block, 0, stream, m.offset, m.row, m.bin, nnz, nfeat,
                       m.cut_ptr, total, grad, hess, pos, rows, first_node, nodes, scale, out);
  } else {
    hipLaunchKernelGGL(k_gbdt_hist_multi, grid, block, 0, stream, m.offset, m.row, m.bin, nnz, nfeat,
                       m.cut_ptr, total, grad, hess, pos, rows, first_node, nodes,
                       static_cast<int32_t>(num_outputs), scale, out);
  }
  DMLC_HIP_CHECK_LAUNCH();
}

size_t GbdtSplitScratchBytes(uint64_t num_nodes, uint64_t num_features) {
  return sizeof(Cand) * num_nodes * ((num_features + kThreads - 1) / kThreads);
}

void LaunchGbdtBestSplits(const int64_t* hist, const int64_t* node_sum, const int64_t* cut_ptr,
                          uint64_t num_features, uint64_t total_bins, uint32_t num_nodes,
                          uint32_t num_outputs, double scale, double reg_lambda, double gamma,
                          double min_child_weight, void* scratch, int64_t* feature, int32_t* bin,
                          uint8_t* default_left, double* gain, hipStream_t stream) {
  const bool scalar = num_outputs == kGbdtScalar;
  const char* const op = scalar ? "gbdt best splits" : "gbdt best splits multi";
  CheckLevel(op, 0, num_features, num_nodes <= kGbdtMaxNodes, num_outputs);
  CHECK(reg_lambda > 0.0 && scale > 0.0) << op << ": reg_lambda and scale must be > 0";
  CHECK(Aligned16(scratch)) << op << ": scratch must be 16-byte aligned";
  if (num_nodes == 0) return;
  const uint32_t parts = static_cast<uint32_t>((num_features + kThreads - 1) / kThreads);
  const dim3 grid(parts, num_nodes), block(kThreads);
  const long long* const h = reinterpret_cast<const long long*>(hist);
  const long long* const sums = reinterpret_cast<const long long*>(node_sum);
  const int64_t nfeat = static_cast<int64_t>(num_features), total = static_cast<int64_t>(total_bins);
  Cand* const partial = static_cast<Cand*>(scratch);
  if (scalar) {
    hipLaunchKernelGGL(k_gbdt_split_scan, grid, block, 0, stream, h, sums, cut_ptr, nfeat, total,
                       scale, reg_lambda, gamma, min_child_weight, partial);
  } else {
    static_assert(kGbdtMaxOutputs <= 32, "a group of lanes per (node, feature) is at most half a wave");
    auto scan = num_outputs <= 1    ? k_gbdt_split_scan_multi<1>
                : num_outputs <= 2  ? k_gbdt_split_scan_multi<2>
                : num_outputs <= 4  ? k_gbdt_split_scan_multi<4>
                : num_outputs <= 8  ? k_gbdt_split_scan_multi<8>
                : num_outputs <= 16 ? k_gbdt_split_scan_multi<16>
                                    : k_gbdt_split_scan_multi<32>;
    const double min_hess = static_cast<double>(num_outputs) * min_child_weight * scale;
    hipLaunchKernelGGL(scan, grid, block, 0, stream, h, sums, cut_ptr, nfeat, total,
                       static_cast<int32_t>(num_outputs), scale, reg_lambda, gamma, min_hess, partial);
  }
  DMLC_HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gbdt_split_pick, dim3(num_nodes), block, 0, stream, partial,
                     static_cast<int64_t>(parts), feature, bin, default_left, gain);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchGbdtLongColumns(const GbdtBinned& m, uint64_t capacity, int64_t* column, int64_t* bin_ptr,
                           int64_t* piece_ptr, int64_t* totals, hipStream_t stream) {
  CheckBinned("gbdt long columns", m.nnz, m.num_features);
  CHECK_GE(capacity, m.nnz / kSeg) << "gbdt long columns: capacity below nnz / segment entries";
  hipLaunchKernelGGL(k_gbdt_long_columns, dim3(1), dim3(kThreads), 0, stream, m.offset, m.cut_ptr,
                     static_cast<int64_t>(m.num_features), static_cast<int64_t>(capacity), column,
                     bin_ptr, piece_ptr, totals);
  DMLC_HIP_CHECK_LAUNCH();
}

namespace {
/*! \brief slots of `partial` per node: the short columns' workgroups, then the long columns' */
uint64_t LevelParts(uint64_t nnz, uint64_t long_count) {
  return nnz / kSeg + 1 + (long_count + kThreads - 1) / kThreads;
}
}  // namespace

uint32_t GbdtLevelWindowNodes(uint64_t num_nodes, uint64_t nnz, const GbdtLongColumns& lc) {
  const uint64_t per_node = sizeof(Cand) * (LevelParts(nnz, lc.count) + lc.bins);
  uint64_t window = kGbdtLevelScratchBudget / per_node;
  if (window < 1) window = 1;
  return static_cast<uint32_t>(window < num_nodes ? window : num_nodes);
}

size_t GbdtLevelScratchBytes(uint64_t num_nodes, uint64_t nnz, const GbdtLongColumns& lc) {
  return sizeof(Cand) * (LevelParts(nnz, lc.count) + lc.bins) *
         GbdtLevelWindowNodes(num_nodes, nnz, lc);
}

void LaunchGbdtLevelSplits(const GbdtBinned& m, const GbdtLongColumns& lc, const float* grad,
                           const float* hess, const int32_t* pos, int32_t first_node,
                           uint32_t num_nodes, const int64_t* node_sum, double scale,
                           double reg_lambda, double gamma, double min_child_weight, void* scratch,
                           int64_t* feature, int32_t* bin, uint8_t* default_left, double* gain,
                           hipStream_t stream) {
  const char* const op = "gbdt level splits";
  CheckLevel(op, m.nnz, m.num_features, num_nodes >= 1 && num_nodes <= kGbdtMaxNodes, kGbdtScalar);
  CHECK(reg_lambda > 0.0 && scale > 0.0) << op << ": reg_lambda and scale must be > 0";
  CHECK(Aligned16(scratch)) << op << ": scratch must be 16-byte aligned";
  CHECK(m.nnz > 0 && m.rows > 0) << op << ": an empty matrix has no splits to search";
  CHECK(lc.count <= m.nnz / kSeg && lc.pieces <= m.nnz / kSeg + lc.count &&
        lc.bins <= lc.count * kGbdtMaxBins)
      << op << ": not the long columns of this matrix";
  const int64_t nnz = static_cast<int64_t>(m.nnz), nfeat = static_cast<int64_t>(m.num_features);
  const int64_t total = static_cast<int64_t>(m.total_bins), rows = static_cast<int64_t>(m.rows);
  const int64_t count = static_cast<int64_t>(lc.count), spill_bins = static_cast<int64_t>(lc.bins);
  const uint32_t segs = static_cast<uint32_t>(m.nnz / kSeg + 1);
  const uint32_t long_parts = static_cast<uint32_t>((lc.count + kThreads - 1) / kThreads);
  const int64_t parts = static_cast<int64_t>(LevelParts(m.nnz, lc.count));
  const uint32_t window = GbdtLevelWindowNodes(num_nodes, m.nnz, lc);
  const dim3 block(kThreads);
  Cand* const partial = static_cast<Cand*>(scratch);
  for (uint32_t w0 = 0; w0 < num_nodes; w0 += window) {
    const uint32_t nw = num_nodes - w0 < window ? num_nodes - w0 : window;
    const int32_t first = first_node + static_cast<int32_t>(w0), nodes = static_cast<int32_t>(nw);
    const LevelGain lg{reinterpret_cast<const long long*>(node_sum) + 2 * w0, scale, reg_lambda,
                       gamma, min_child_weight};
    hipLaunchKernelGGL(k_gbdt_level_short, dim3(segs), block, 0, stream, m.offset, m.row, m.bin, nnz,
                       nfeat, m.cut_ptr, total, grad, hess, pos, rows, first, nodes, lg, partial,
                       parts);
    DMLC_HIP_CHECK_LAUNCH();
    if (count > 0 && lc.pieces > 0 && spill_bins > 0) {
      unsigned long long* const spill = reinterpret_cast<unsigned long long*>(partial + nw * parts);
      const int64_t words = 2 * static_cast<int64_t>(nw) * spill_bins;
      hipLaunchKernelGGL(k_gbdt_level_clear, dim3(GridFor(static_cast<uint64_t>(words), kThreads)),
                         block, 0, stream, spill, words);
      DMLC_HIP_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_gbdt_level_long_hist, dim3(static_cast<uint32_t>(lc.pieces)), block, 0,
                         stream, m.offset, m.row, m.bin, nnz, m.cut_ptr, total, grad, hess, pos, rows,
                         first, nodes, scale, lc.column, lc.bin_ptr, lc.piece_ptr, count, spill_bins,
                         spill);
      DMLC_HIP_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_gbdt_level_long_scan, dim3(long_parts, nw), block, 0, stream,
                         reinterpret_cast<const long long*>(spill), m.cut_ptr, total, lc.column,
                         lc.bin_ptr, count, spill_bins, lg, partial, parts,
                         static_cast<int64_t>(segs));
      DMLC_HIP_CHECK_LAUNCH();
    } else if (long_parts > 0) {
      // long columns without cuts: their slots hold no candidate
      hipLaunchKernelGGL(k_gbdt_level_long_scan, dim3(long_parts, nw), block, 0, stream,
                         static_cast<const long long*>(nullptr), m.cut_ptr, total, lc.column,
                         lc.bin_ptr, count, spill_bins, lg, partial, parts,
                         static_cast<int64_t>(segs));
      DMLC_HIP_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_gbdt_split_pick, dim3(nw), block, 0, stream, partial, parts, feature + w0,
                       bin + w0, default_left + w0, gain + w0);
    DMLC_HIP_CHECK_LAUNCH();
  }
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
