/*!
 * \file src/gpu/rowsort_kernels.hip
 * \brief SR0 - SR3, SD1 / SD2: canonical CSR rows -- every row's entries sorted
 *  by (index, field) or (field, index), stable, and optionally one entry per
 *  run of equal keys (scipy's sort_indices / sum_duplicates).
 *
 *  The sort is a segmented one: rows are short, so a row is sorted where it
 *  fits -- in a wave's registers, in a workgroup's LDS -- and never through a
 *  global radix sort of (row, key) pairs.  What is sorted is the element
 *  (key, position in the row): positions are distinct, so the order is total
 *  and the result stable, and values / fields / indices are moved once, at the
 *  end, through the sorted positions (out[i] = in[pos[i]]).
 *
 *  SR0 k_sort_prepare  the output row pointer (offset[r] - offset[0]) and zeros
 *                      for the entries of the outputs past the last row.
 *  SR1 k_sort_wave     one wave per row of up to kSortWaveRowEntries (256)
 *                      entries, 4 per lane.  The keys are staged coalesced in
 *                      the wave's LDS slice and read back blocked (lane l holds
 *                      elements 4l .. 4l + 3).  A bitonic network over the
 *                      padded power of two: strides 1 and 2 are compare-
 *                      exchanges between a lane's own registers, strides 4 ..
 *                      128 exchange with lane ^ (stride / 4) by shuffles.
 *                      The sorted positions go back to the slice and the
 *                      payload is moved with coalesced stores.  Rows of 0 or 1
 *                      entries copy through.
 *  SR2 k_sort_block    one workgroup per row of up to kSortBlockRowEntries
 *                      (4096) entries, whole in LDS (up to 80 KiB with 64-bit
 *                      ids and fields: the launch opts in).  Every wave sorts
 *                      256-entry chunks with SR1's register network; the merge
 *                      phases above 256 run their strides >= 256 as compare-
 *                      exchanges in LDS and finish every chunk's strides 128 ..
 *                      1 in registers again.
 *  SR3 k_sort_long     one workgroup per longer row: tiles of 4096 sorted as
 *                      SR2 does, their sorted positions written out; then the
 *                      same workgroup merges runs pairwise, ping-pong between a
 *                      scratch buffer and the row's slice of out_index (used
 *                      as u32 words), each pass split into kSortMergeTile-entry
 *                      output segments by merge-path searches.  The first
 *                      buffer is chosen by the parity of the passes, so the
 *                      positions always end in the scratch and the payload
 *                      move then fills the outputs.
 *  All three run over all rows and each skips the others' rows, so the host
 *  needs no row length and the launch sequence no read-back.
 *
 *  SD1 k_row_runs      per sorted row, the number of runs of equal keys (the
 *                      row's distinct keys), by ballot and popcount; without a
 *                      write target it is ops.row_order's kernel: whether any
 *                      entry is below its predecessor, and the adjacent repeats.
 *  K3                  scans the counts into the new row pointer.
 *  SD2 k_row_heads     every run's head to offset'[r] + rank, the rank from the
 *                      ballot below the lane plus a carry over the row's
 *                      64-entry steps; "sum" adds the run's values one by one
 *                      in input order.
 *
 *  A row whose pointers descend, start before offset[0] or end past the entry
 *  arrays is skipped and sets an error bit; no address is formed from it.  No
 *  atomics touch the outputs: their bytes are a pure function of the inputs.
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
/*! \brief entries a lane holds in registers */
constexpr int kPerLane = 4;
/*! \brief entries a wave sorts in registers: SR1's cap and SR2's chunk */
constexpr uint32_t kChunk = kPerLane * dev::kWave;
constexpr uint32_t kBlockCap = kSortBlockRowEntries;
/*! \brief rows a workgroup of SR2 / SR3 classifies at once */
constexpr uint32_t kRowGroup = dev::kWave;
static_assert(kSortWaveRowEntries == kChunk, "SR1 sorts one register chunk");
static_assert(kBlockCap % kChunk == 0 && (kBlockCap & (kBlockCap - 1)) == 0, "tile of chunks");
static_assert((2 * kBlockCap) % kSortMergeTile == 0, "a merge segment stays inside one run pair");

/*! \brief the sorted element: key (hi, lo) and the entry's position in its row */
template <typename T, bool kField>
struct Elem {
  T hi;
  T lo;  // unused without a second key column
  uint32_t pos;
};

template <typename T, bool kField>
__device__ __forceinline__ bool key_less(const Elem<T, kField>& a, const Elem<T, kField>& b) {
  if (a.hi != b.hi) return a.hi < b.hi;
  if constexpr (kField) return a.lo < b.lo;
  return false;
}
template <typename T, bool kField>
__device__ __forceinline__ bool key_equal(const Elem<T, kField>& a, const Elem<T, kField>& b) {
  if constexpr (kField) return a.hi == b.hi && a.lo == b.lo;
  return a.hi == b.hi;
}
/*! \brief the strict total order of the sort: key, then position */
template <typename T, bool kField>
__device__ __forceinline__ bool elem_less(const Elem<T, kField>& a, const Elem<T, kField>& b) {
  if (!key_equal(a, b)) return key_less(a, b);
  return a.pos < b.pos;
}

/*! \brief what the kernels share: the source CSR, its key columns, the outputs */
template <typename T>
struct SortArgs {
  const uint64_t* offset;
  uint64_t nrows;
  uint64_t entries;  // of index / value / field, source and output
  const T* kp;       // primary key column
  const T* ks;       // secondary key column (null: none)
  const T* index;
  const float* value;  // may be null
  const T* field;      // may be null
  T* oindex;
  float* ovalue;
  T* ofield;
  uint32_t* scratch;  // `entries` words (SR3)
  uint32_t* error;
};

template <typename T, bool kField>
__device__ __forceinline__ Elem<T, kField> load_elem(const SortArgs<T>& a, uint64_t src,
                                                     uint32_t pos) {
  Elem<T, kField> e;
  e.hi = a.kp[src];
  if constexpr (kField) {
    e.lo = a.ks[src];
  } else {
    e.lo = T(0);
  }
  e.pos = pos;
  return e;
}

template <typename T>
__device__ __forceinline__ void move_entry(const SortArgs<T>& a, uint64_t src, uint64_t dst) {
  a.oindex[dst] = a.index[src];
  if (a.value != nullptr) a.ovalue[dst] = a.value[src];
  if (a.field != nullptr) a.ofield[dst] = a.field[src];
}

/*! \brief out[dst] = entry `pos` of the row of n entries at b; the sorted positions
 *  are a permutation of 0 .. n - 1, and nothing else is ever turned into an address */
template <typename T>
__device__ __forceinline__ void move_sorted(const SortArgs<T>& a, uint64_t b, uint32_t pos,
                                            uint32_t n, uint64_t dst) {
  if (pos < n) move_entry(a, b + pos, dst);
}

/*! \brief row r's entries [*b, *e) if its pointers can be used, else false */
template <typename T>
__device__ __forceinline__ bool row_span(const SortArgs<T>& a, uint64_t r, uint64_t base,
                                         uint64_t* b, uint64_t* e) {
  *b = a.offset[r];
  *e = a.offset[r + 1];
  return base <= *b && *b <= *e && *e <= a.entries;
}

/*! \brief which kernel sorts a row of n entries: 0 SR1, 1 SR2, 2 SR3 */
__device__ __forceinline__ int row_class(uint64_t n) {
  return n <= kChunk ? 0 : (n <= kBlockCap ? 1 : 2);
}

__device__ __forceinline__ uint32_t next_pow2(uint32_t v, uint32_t least) {
  uint32_t p = least;
  while (p < v) p <<= 1;
  return p;
}

// ------------------------------------------------------------- LDS layout
/*! \brief hi [n], lo [n] (with a second key), pos [n] of a region of n elements */
template <typename T, bool kField>
struct Lds {
  T* hi;
  T* lo;
  uint32_t* pos;
  __device__ __forceinline__ Lds(unsigned char* base, uint32_t n) {
    hi = reinterpret_cast<T*>(base);
    lo = hi + (kField ? n : 0);
    pos = reinterpret_cast<uint32_t*>(lo + n);
  }
  __device__ __forceinline__ Elem<T, kField> get(uint32_t i) const {
    Elem<T, kField> e;
    e.hi = hi[i];
    e.lo = kField ? lo[i] : T(0);
    e.pos = pos[i];
    return e;
  }
  __device__ __forceinline__ void put(uint32_t i, const Elem<T, kField>& e) const {
    hi[i] = e.hi;
    if constexpr (kField) lo[i] = e.lo;
    pos[i] = e.pos;
  }
};
template <typename T, bool kField>
constexpr size_t ElemLdsBytes() {
  return sizeof(T) * (kField ? 2 : 1) + sizeof(uint32_t);
}

/*! \brief element i of the padded row: the entry, or past n a sentinel that
 *  sorts after every entry (the largest key with a position >= n) */
template <typename T, bool kField>
__device__ __forceinline__ void stage(const Lds<T, kField>& l, const SortArgs<T>& a, uint64_t b,
                                      uint32_t n, uint32_t i) {
  Elem<T, kField> e;
  if (i < n) {
    e = load_elem<T, kField>(a, b + i, i);
  } else {
    e.hi = ~T(0);
    e.lo = ~T(0);
    e.pos = i;
  }
  l.put(i, e);
}

// ------------------------------------------------- the register network
__device__ __forceinline__ uint32_t shfl_xor_bits(uint32_t x, int m) {
  return static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), m, dev::kWave));
}
__device__ __forceinline__ uint64_t shfl_xor_bits(uint64_t x, int m) {
  const uint32_t lo = shfl_xor_bits(static_cast<uint32_t>(x), m);
  const uint32_t hi = shfl_xor_bits(static_cast<uint32_t>(x >> 32), m);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

/*! \brief compare-exchange of two registers, a at the lower element index */
template <typename T, bool kField>
__device__ __forceinline__ void cx(Elem<T, kField>& a, Elem<T, kField>& b, bool asc) {
  if (elem_less(b, a) == asc) {
    const Elem<T, kField> t = a;
    a = b;
    b = t;
  }
}

/*!
 * \brief the compare-exchange stages of strides jfrom, jfrom / 2, .. 1 (jfrom <=
 *  128) of the bitonic phase k on a chunk held blocked in registers: e[a] is
 *  element i0 + a, i0 = chunk base + 4 lane.  Element i pairs with i ^ j and
 *  the pair ascends when (i & k) == 0.
 */
template <typename T, bool kField>
__device__ __forceinline__ void wave_stages(Elem<T, kField> (&e)[kPerLane], uint32_t i0, uint32_t k,
                                            uint32_t jfrom) {
  for (uint32_t j = jfrom; j >= 1; j >>= 1) {
    if (j >= kPerLane) {
      // cross-lane: the partner element sits in lane ^ (j / 4), same register
      const int m = static_cast<int>(j / kPerLane);
      const bool asc = (i0 & k) == 0;      // k >= 8: the same for the lane's 4 elements
      const bool keep_min = ((i0 & j) == 0) == asc;
#pragma unroll
      for (int a = 0; a < kPerLane; ++a) {
        Elem<T, kField> o;
        o.hi = shfl_xor_bits(e[a].hi, m);
        if constexpr (kField) {
          o.lo = shfl_xor_bits(e[a].lo, m);
        } else {
          o.lo = T(0);
        }
        o.pos = shfl_xor_bits(e[a].pos, m);
        if (elem_less(o, e[a]) == keep_min) e[a] = o;
      }
    } else if (j == 2) {
      cx(e[0], e[2], (i0 & k) == 0);
      cx(e[1], e[3], (i0 & k) == 0);
    } else {
      cx(e[0], e[1], (i0 & k) == 0);
      cx(e[2], e[3], ((i0 + 2) & k) == 0);
    }
  }
}

template <typename T, bool kField>
__device__ __forceinline__ void load_chunk(const Lds<T, kField>& l, uint32_t i0,
                                           Elem<T, kField> (&e)[kPerLane]) {
#pragma unroll
  for (int a = 0; a < kPerLane; ++a) e[a] = l.get(i0 + a);
}
template <typename T, bool kField>
__device__ __forceinline__ void store_chunk(const Lds<T, kField>& l, uint32_t i0,
                                            const Elem<T, kField> (&e)[kPerLane]) {
#pragma unroll
  for (int a = 0; a < kPerLane; ++a) l.put(i0 + a, e[a]);
}

/*! \brief sort elements [0, n2) of an LDS region with the whole workgroup (n2 a
 *  power of two, kChunk .. kBlockCap; every thread calls it; the region is
 *  staged and a barrier passed) */
template <typename T, bool kField>
__device__ void block_sort(const Lds<T, kField>& l, uint32_t n2) {
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  const uint32_t lane = static_cast<uint32_t>(dev::lane_id());
  const uint32_t nchunks = n2 / kChunk;
  Elem<T, kField> e[kPerLane];
  for (uint32_t c = wave; c < nchunks; c += kWaves) {
    const uint32_t i0 = c * kChunk + lane * kPerLane;
    load_chunk(l, i0, e);
    for (uint32_t k = 2; k <= kChunk; k <<= 1) wave_stages(e, i0, k, k / 2);
    store_chunk(l, i0, e);
  }
  __syncthreads();
  for (uint32_t k = 2 * kChunk; k <= n2; k <<= 1) {
    for (uint32_t j = k / 2; j >= kChunk; j >>= 1) {
      for (uint32_t p = threadIdx.x; p < n2 / 2; p += kThreads) {
        const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        Elem<T, kField> x = l.get(i), y = l.get(i | j);
        if (elem_less(y, x) == ((i & k) == 0)) {
          l.put(i, y);
          l.put(i | j, x);
        }
      }
      __syncthreads();
    }
    for (uint32_t c = wave; c < nchunks; c += kWaves) {
      const uint32_t i0 = c * kChunk + lane * kPerLane;
      load_chunk(l, i0, e);
      wave_stages(e, i0, k, kChunk / 2);
      store_chunk(l, i0, e);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------- SR0
template <typename T>
__global__ __launch_bounds__(kThreads) void k_sort_prepare(SortArgs<T> a, uint64_t* out_offset) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  const uint64_t base = a.offset[0], last = a.offset[a.nrows];
  for (uint64_t r = tid; r <= a.nrows; r += step) out_offset[r] = a.offset[r] - base;
  // entries past the last row (the source's unused tail, or all of them behind
  // a row pointer that cannot be used) hold zeros
  const uint64_t total = (base <= last && last <= a.entries) ? last - base : 0;
  for (uint64_t p = total + tid; p < a.entries; p += step) {
    a.oindex[p] = T(0);
    if (a.value != nullptr) a.ovalue[p] = 0.0f;
    if (a.field != nullptr) a.ofield[p] = T(0);
  }
}

// ------------------------------------------------------------------- SR1
template <typename T, bool kField>
__global__ __launch_bounds__(kThreads) void k_sort_wave(SortArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  const uint32_t lane = static_cast<uint32_t>(dev::lane_id());
  const Lds<T, kField> l(s_raw + wave * (kChunk * ElemLdsBytes<T, kField>()), kChunk);
  const uint64_t base = a.offset[0];
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; r < a.nrows; r += nwaves) {
    uint64_t b, e;
    if (!row_span(a, r, base, &b, &e)) {
      if (lane == 0) atomicOr(a.error, kSortErrOffset);  // the status word, not an output
      continue;
    }
    if (row_class(e - b) != 0) continue;
    const uint32_t n = static_cast<uint32_t>(e - b);
    const uint64_t ob = b - base;
    if (n <= 1) {
      if (n == 1 && lane == 0) move_entry(a, b, ob);
      continue;
    }
    const uint32_t n2 = next_pow2(n, kPerLane);
    for (uint32_t i = lane; i < kChunk; i += dev::kWave) stage(l, a, b, n, i);
    dev::wave_sync();
    Elem<T, kField> x[kPerLane];
    const uint32_t i0 = lane * kPerLane;
    load_chunk(l, i0, x);
    // elements at and past n2 are sentinels and only ever meet each other
    for (uint32_t k = 2; k <= n2; k <<= 1) wave_stages(x, i0, k, k / 2);
    dev::wave_sync();
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) l.pos[i0 + c] = x[c].pos;
    dev::wave_sync();
    for (uint32_t i = lane; i < n; i += dev::kWave) move_sorted(a, b, l.pos[i], n, ob + i);
    dev::wave_sync();  // the slice is read before the next row is staged
  }
}

/*! \brief SR2 / SR3: the rows of class `cls` among rows [g0, g0 + 64), as a
 *  mask every thread of the workgroup holds (two barriers) */
template <typename T>
__device__ __forceinline__ uint64_t class_mask(const SortArgs<T>& a, uint64_t g0, uint64_t base,
                                               int cls, uint64_t* s_mask) {
  __syncthreads();  // the previous group's mask has been read
  if (threadIdx.x < kRowGroup) {
    const uint64_t r = g0 + threadIdx.x;
    uint64_t b = 0, e = 0;
    const bool mine = r < a.nrows && row_span(a, r, base, &b, &e) && row_class(e - b) == cls;
    const uint64_t m = __ballot(mine);
    if (threadIdx.x == 0) *s_mask = m;
  }
  __syncthreads();
  return *s_mask;
}

// ------------------------------------------------------------------- SR2
template <typename T, bool kField>
__global__ __launch_bounds__(kThreads) void k_sort_block(SortArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ uint64_t s_mask;
  const Lds<T, kField> l(s_raw, kBlockCap);
  const uint64_t base = a.offset[0];
  for (uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kRowGroup; g0 < a.nrows;
       g0 += static_cast<uint64_t>(gridDim.x) * kRowGroup) {
    uint64_t mask = class_mask(a, g0, base, 1, &s_mask);
    while (mask != 0) {
      const uint64_t r = g0 + static_cast<uint64_t>(__builtin_ctzll(mask));
      mask &= mask - 1;
      const uint64_t b = a.offset[r];
      const uint32_t n = static_cast<uint32_t>(a.offset[r + 1] - b);
      const uint32_t n2 = next_pow2(n, kChunk);
      for (uint32_t i = threadIdx.x; i < n2; i += kThreads) stage(l, a, b, n, i);
      __syncthreads();
      block_sort(l, n2);
      for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
        move_sorted(a, b, l.pos[i], n, b - base + i);
      }
      __syncthreads();  // the region is read before the next row is staged
    }
  }
}

// ------------------------------------------------------------------- SR3
/*!
 * \brief one merge pass of the row at entries b ..: runs of w sorted positions
 *  in src are merged pairwise into dst (n positions each).  Output segment s =
 *  [s kSortMergeTile, ..) lies inside one pair of runs; its start on the merge
 *  path is found by a binary search on the segment's diagonal, then the
 *  segment is merged serially.  Equal keys cannot meet: positions differ.
 */
template <typename T, bool kField>
__device__ void merge_pass(const SortArgs<T>& a, uint64_t b, const uint32_t* src, uint32_t* dst,
                           uint32_t n, uint64_t w) {
  const uint32_t nseg = (n + kSortMergeTile - 1) / kSortMergeTile;
  for (uint32_t s = threadIdx.x; s < nseg; s += kThreads) {
    const uint64_t o0 = static_cast<uint64_t>(s) * kSortMergeTile;
    const uint64_t o1 = o0 + kSortMergeTile < n ? o0 + kSortMergeTile : n;
    const uint64_t pl = o0 / (2 * w) * (2 * w);
    const uint64_t a1 = pl + w < n ? pl + w : n;          // run A: [pl, a1)
    const uint64_t b1 = pl + 2 * w < n ? pl + 2 * w : n;  // run B: [a1, b1)
    const uint64_t la = a1 - pl, lb = b1 - a1, d = o0 - pl;
    auto at = [&](uint64_t i) {
      const uint32_t p = src[i] < n ? src[i] : n - 1;  // a position of the row, whatever src holds
      return load_elem<T, kField>(a, b + p, p);
    };
    // x: how many of the first d merged elements come from A
    uint64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (!elem_less(at(a1 + (d - 1 - mid)), at(pl + mid))) {
        lo = mid + 1;  // A[mid] comes before B[d - 1 - mid]: it is among the first d
      } else {
        hi = mid;
      }
    }
    uint64_t x = lo, y = d - lo;
    Elem<T, kField> ea{}, eb{};
    if (x < la) ea = at(pl + x);
    if (y < lb) eb = at(a1 + y);
    for (uint64_t o = o0; o < o1; ++o) {
      const bool take_a = y >= lb || (x < la && !elem_less(eb, ea));
      if (take_a) {
        dst[o] = ea.pos;
        if (++x < la) ea = at(pl + x);
      } else {
        dst[o] = eb.pos;
        if (++y < lb) eb = at(a1 + y);
      }
    }
  }
}

template <typename T, bool kField>
__global__ __launch_bounds__(kThreads) void k_sort_long(SortArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ uint64_t s_mask;
  const Lds<T, kField> l(s_raw, kBlockCap);
  const uint64_t base = a.offset[0];
  for (uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kRowGroup; g0 < a.nrows;
       g0 += static_cast<uint64_t>(gridDim.x) * kRowGroup) {
    uint64_t mask = class_mask(a, g0, base, 2, &s_mask);
    while (mask != 0) {
      const uint64_t r = g0 + static_cast<uint64_t>(__builtin_ctzll(mask));
      mask &= mask - 1;
      const uint64_t b = a.offset[r], len = a.offset[r + 1] - b, ob = b - base;
      if (len >= (1ull << 32)) {  // positions are 32-bit
        if (threadIdx.x == 0) atomicOr(a.error, kSortErrRowLength);
        continue;
      }
      const uint32_t n = static_cast<uint32_t>(len);
      int passes = 0;
      for (uint64_t w = kBlockCap; w < n; w <<= 1) ++passes;
      // the two position buffers of the row: its words of the scratch and of
      // out_index (sizeof(T) >= 4 bytes per entry).  After `passes` swaps the
      // positions are in the scratch.
      uint32_t* const in_scratch = a.scratch + ob;
      uint32_t* const in_output = reinterpret_cast<uint32_t*>(a.oindex + ob);
      uint32_t* cur = (passes & 1) ? in_output : in_scratch;
      for (uint32_t tb = 0; tb < n; tb += kBlockCap) {
        const uint32_t tn = n - tb < kBlockCap ? n - tb : kBlockCap;
        const uint32_t n2 = next_pow2(tn, kChunk);
        for (uint32_t i = threadIdx.x; i < n2; i += kThreads) stage(l, a, b + tb, tn, i);
        __syncthreads();
        block_sort(l, n2);
        for (uint32_t i = threadIdx.x; i < tn; i += kThreads) cur[tb + i] = tb + l.pos[i];
        __syncthreads();
      }
      for (uint64_t w = kBlockCap; w < n; w <<= 1) {
        uint32_t* const dst = cur == in_scratch ? in_output : in_scratch;
        merge_pass<T, kField>(a, b, cur, dst, n, w);
        __syncthreads();  // the pass's stores are visible to the workgroup
        cur = dst;
      }
      for (uint32_t i = threadIdx.x; i < n; i += kThreads) move_sorted(a, b, in_scratch[i], n, ob + i);
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------- SD1 / SD2
/*! \brief the heads of row entries s .. s + 63 (lane i - s): an entry whose key
 *  differs from its predecessor's, and the row's first.  *below: the entry's
 *  key is less than its predecessor's */
template <typename T, bool kField>
__device__ __forceinline__ bool is_head(const SortArgs<T>& a, uint64_t b, uint64_t n, uint64_t i,
                                        Elem<T, kField>* cur, bool* below) {
  *below = false;
  if (i >= n) return false;
  *cur = load_elem<T, kField>(a, b + i, 0);
  if (i == 0) return true;
  const Elem<T, kField> prev = load_elem<T, kField>(a, b + i - 1, 0);
  *below = key_less(*cur, prev);
  return !key_equal(prev, *cur);
}

template <typename T, bool kField>
__global__ __launch_bounds__(kThreads) void k_row_runs(SortArgs<T> a, uint64_t* counts,
                                                       unsigned long long* status) {
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  const uint32_t lane = static_cast<uint32_t>(dev::lane_id());
  const uint64_t base = a.offset[0];
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWaves;
  uint64_t repeats = 0;
  bool unsorted = false;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; r < a.nrows; r += nwaves) {
    uint64_t b, e, heads = 0;
    if (!row_span(a, r, base, &b, &e)) {
      if (lane == 0) atomicOr(a.error, kSortErrOffset);
      e = b;
    }
    const uint64_t n = e - b;
    for (uint64_t s = 0; s < n; s += dev::kWave) {
      Elem<T, kField> cur;
      bool below;
      const bool head = is_head(a, b, n, s + lane, &cur, &below);
      heads += static_cast<uint64_t>(__popcll(__ballot(head)));
      unsorted |= __ballot(below) != 0;
    }
    if (counts != nullptr && lane == 0) counts[r] = heads;
    repeats += n - heads;
  }
  // the status words of ops.row_order, not outputs
  if (status != nullptr && lane == 0) {
    if (unsorted) atomicOr(&status[0], 1ull);
    if (repeats != 0) atomicAdd(&status[1], static_cast<unsigned long long>(repeats));
  }
}

template <typename T, bool kField>
__global__ __launch_bounds__(kThreads) void k_row_heads(SortArgs<T> a, bool sum,
                                                        uint64_t* out_offset,
                                                        const uint64_t* total,
                                                        uint64_t out_capacity) {
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  const uint32_t lane = static_cast<uint32_t>(dev::lane_id());
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out_offset[a.nrows] = *total;  // the closing row pointer (single writer)
    if (*total > out_capacity) atomicOr(a.error, kSortErrCapacity);
  }
  const uint64_t base = a.offset[0];
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; r < a.nrows; r += nwaves) {
    uint64_t b, e;
    if (!row_span(a, r, base, &b, &e)) continue;  // SD1 flagged it and counted 0
    const uint64_t n = e - b;
    uint64_t carry = out_offset[r];
    for (uint64_t s = 0; s < n; s += dev::kWave) {
      const uint64_t i = s + lane;
      Elem<T, kField> cur;
      bool below;
      const bool head = is_head(a, b, n, i, &cur, &below);
      const uint64_t m = __ballot(head);
      const uint64_t dst = carry + static_cast<uint64_t>(__popcll(m & ((1ull << lane) - 1ull)));
      if (head && dst < out_capacity) {
        a.oindex[dst] = a.index[b + i];
        if (a.field != nullptr) a.ofield[dst] = a.field[b + i];
        if (a.value != nullptr) {
          float v = a.value[b + i];
          if (sum) {
            // the run's values one by one, in input order (the sort is stable)
            for (uint64_t j = i + 1; j < n; ++j) {
              if (!key_equal(cur, load_elem<T, kField>(a, b + j, 0))) break;
              v += a.value[b + j];
            }
          }
          a.ovalue[dst] = v;
        }
      }
      carry += static_cast<uint64_t>(__popcll(m));
    }
  }
}

// --------------------------------------------------------------- launchers
template <typename T>
SortArgs<T> MakeArgs(const CsrView& src, uint64_t entries, bool by_field, void* out_index,
                     float* out_value, void* out_field, uint32_t* scratch, uint32_t* error) {
  const T* index = IndexOf<T>(src);
  const T* field = FieldOf<T>(src);
  SortArgs<T> a;
  a.offset = src.offset;
  a.nrows = src.nrows;
  a.entries = entries;
  a.kp = by_field ? field : index;
  a.ks = field == nullptr ? nullptr : (by_field ? index : field);
  a.index = index;
  a.value = src.value;
  a.field = field;
  a.oindex = static_cast<T*>(out_index);
  a.ovalue = out_value;
  a.ofield = static_cast<T*>(out_field);
  a.scratch = scratch;
  a.error = error;
  return a;
}

/*! \brief f(IndexType{}, whether the key has a second column) */
template <typename F>
void DispatchKey(const char* op, const CsrView& src, bool by_field, F&& f) {
  CheckView(op, src, false);
  CHECK(!by_field || src.field != nullptr) << op << ": by field needs a field column";
  DispatchIndex(src, [&](auto tag) {
    if (src.field != nullptr) {
      f(tag, std::true_type{});
    } else {
      f(tag, std::false_type{});
    }
  });
}
}  // namespace

void LaunchSortRows(const CsrView& src, uint64_t src_entries, bool by_field, uint64_t* out_offset,
                    void* out_index, float* out_value, void* out_field, uint32_t* scratch,
                    uint32_t* error, hipStream_t stream) {
  DispatchKey("sort_rows", src, by_field, [&](auto tag, auto has_field) {
    using T = decltype(tag);
    constexpr bool kField = decltype(has_field)::value;
    if (src.nrows == 0) return;
    const SortArgs<T> a =
        MakeArgs<T>(src, src_entries, by_field, out_index, out_value, out_field, scratch, error);
    hipLaunchKernelGGL(k_sort_prepare<T>, dim3(GridFor(src.nrows + 1, kThreads)), dim3(kThreads), 0,
                       stream, a, out_offset);
    DMLC_HIP_CHECK_LAUNCH();
    constexpr size_t kWaveLds = kWaves * kChunk * ElemLdsBytes<T, kField>();
    hipLaunchKernelGGL((k_sort_wave<T, kField>), dim3(GridFor(src.nrows, kWaves)), dim3(kThreads),
                       kWaveLds, stream, a);
    DMLC_HIP_CHECK_LAUNCH();
    // up to 80 KiB (64-bit ids and fields): above 64 KiB the launch opts in
    constexpr size_t kBlockLds = kBlockCap * ElemLdsBytes<T, kField>();
    const int groups = GridFor((src.nrows + kRowGroup - 1) / kRowGroup, 1);
    PrepareLdsLaunch(k_sort_block<T, kField>, kBlockLds);
    hipLaunchKernelGGL((k_sort_block<T, kField>), dim3(groups), dim3(kThreads), kBlockLds, stream,
                       a);
    DMLC_HIP_CHECK_LAUNCH();
    PrepareLdsLaunch(k_sort_long<T, kField>, kBlockLds);
    hipLaunchKernelGGL((k_sort_long<T, kField>), dim3(groups), dim3(kThreads), kBlockLds, stream,
                       a);
    DMLC_HIP_CHECK_LAUNCH();
  });
}

void LaunchRowRuns(const CsrView& sorted, uint64_t src_entries, bool by_field, uint64_t* counts,
                   uint64_t* status, uint32_t* error, hipStream_t stream) {
  DispatchKey("row_order", sorted, by_field, [&](auto tag, auto has_field) {
    using T = decltype(tag);
    constexpr bool kField = decltype(has_field)::value;
    if (sorted.nrows == 0) return;
    const SortArgs<T> a =
        MakeArgs<T>(sorted, src_entries, by_field, nullptr, nullptr, nullptr, nullptr, error);
    hipLaunchKernelGGL((k_row_runs<T, kField>), dim3(GridFor(sorted.nrows, kWaves)),
                       dim3(kThreads), 0, stream, a, counts,
                       reinterpret_cast<unsigned long long*>(status));
    DMLC_HIP_CHECK_LAUNCH();
  });
}

void LaunchRowHeads(const CsrView& sorted, uint64_t src_entries, bool by_field, bool sum,
                    uint64_t* out_offset, const uint64_t* total, void* out_index, float* out_value,
                    void* out_field, uint64_t out_capacity, uint32_t* error, hipStream_t stream) {
  DispatchKey("sort_rows", sorted, by_field, [&](auto tag, auto has_field) {
    using T = decltype(tag);
    constexpr bool kField = decltype(has_field)::value;
    if (sorted.nrows == 0) return;
    const SortArgs<T> a = MakeArgs<T>(sorted, src_entries, by_field, out_index, out_value,
                                      out_field, nullptr, error);
    hipLaunchKernelGGL((k_row_heads<T, kField>), dim3(GridFor(sorted.nrows, kWaves)),
                       dim3(kThreads), 0, stream, a, sum, out_offset, total, out_capacity);
    DMLC_HIP_CHECK_LAUNCH();
  });
}

}  // namespace gpu
}  // namespace dmlc
