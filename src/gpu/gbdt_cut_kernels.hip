/*!
 * \file src/gpu/gbdt_cut_kernels.hip
 * \brief GB1w: the weighted quantile cuts of every column of a transpose,
 *  without a global sort.  A column is sorted by value where it lies -- in a
 *  wave's registers, in a workgroup's LDS -- its integer weights are scanned
 *  in sorted order and the cuts are picked from the scan.
 *
 *  The rule.  An entry of row r weighs q = llrint(double(w[r]) * scale), scale
 *  a power of two chosen by the host so that a column's total W stays near
 *  2^52.  With C(v) the sum of q over the column's entries of value <= v and
 *  T(c) = floor(c B / W), B = max_bins, the distinct value v_k is a cut iff
 *  W > 0 and T(C(v_k)) > T(C(v_{k-1})) (C(v_0) = 0).  All of it is integer
 *  arithmetic below 2^62: no order of evaluation changes a bit.
 *
 *  The sorted element is (ordered u32 of the value) << 32 | position in the
 *  column: positions are distinct, so the order is total and only these 8
 *  bytes move; q is read through the sorted position, w[row[pos]].
 *
 *  GB1w-a k_cutw_wave   one wave per column of up to kGbdtCutWaveEntries (256)
 *                       entries, 4 per lane, blocked: a bitonic network whose
 *                       strides 1 and 2 are compare-exchanges between a lane's
 *                       registers and strides 4 .. 128 shuffles with lane ^
 *                       (stride / 4).  The sorted keys and their q go to the
 *                       wave's 4 KiB LDS slice for the pick.
 *  GB1w-b k_cutw_block  one workgroup per column of up to kGbdtCutFusedEntries
 *                       (4096) entries: 64 KiB of LDS (8-byte element + 8-byte
 *                       q).  Waves sort 256-entry chunks in registers; merge
 *                       phases above run strides >= 256 in LDS and finish in
 *                       registers.
 *  GB1w-c k_cutw_long_prepare / LaunchSortRows / k_cutw_long_pick
 *                       columns above the fused limit: their (ordered value,
 *                       w[row]) go to a side CSR that SR1 - SR3 sort by key,
 *                       stably; one workgroup per column then streams the
 *                       sorted run in tiles of 4096 through the same pick, the
 *                       carries (c, the last run end's t, the cuts so far) held
 *                       across tiles.
 *  The pick (pick_tile), on a sorted tile in LDS, blocked (a thread owns
 *  consecutive entries): an inclusive int64 scan of q (thread sums, a shuffle
 *  scan over the wave, the waves' totals through LDS), t = c B / W per entry
 *  (one 64-bit division), a run-end flag from the next key, an exclusive
 *  max-scan of the run ends' t -- t ascends, so this is the previous run end's
 *  t -- and a run end is a cut where its t exceeds that.  The cuts' ranks come
 *  from a scan of the per-thread counts; they are written to a scratch at
 *  bound[f] (bound: the scan of min(n_f, B)) and their number to counts[f].
 *  GB1w-d k_cutw_compact  behind the scan of the counts:
 *                       scratch[bound[f] + k] -> cut[cut_ptr[f] + k].
 *  k_cutw_weights flags a NaN, infinite or negative weight of any row.
 *
 *  Every kernel runs over all columns and skips the others' columns, so the
 *  launch sequence needs no column list.  A column whose pointers cannot be
 *  used counts 0; no address is formed from a row id >= rows, a sorted position
 *  >= n or a scratch slot outside the column's min(n, B).  No atomics touch an
 *  output (only the error word).
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
/*! \brief entries a wave sorts in registers */
constexpr uint32_t kChunk = kPerLane * dev::kWave;
/*! \brief entries of the fused path's LDS region, and of a tile of the long path */
constexpr uint32_t kTile = kGbdtCutFusedEntries;
/*! \brief columns a workgroup of GB1w-b / -c classifies at once */
constexpr uint32_t kColGroup = kThreads;
/*! \brief the padding element: sorts after every entry (a position >= n) */
constexpr uint64_t kPad = ~0ull;
static_assert(kGbdtCutWaveEntries == kChunk, "GB1w-a sorts one register chunk");
static_assert(kTile % kChunk == 0 && (kTile & (kTile - 1)) == 0, "a tile of chunks");
static_assert(kTile == kSortBlockRowEntries, "the long path's columns are SR3's rows");
/*! \brief the tile's elements and q, the waves' scan totals and column masks: just above
 *  64 KiB, so the launch opts in */
constexpr size_t kTileLdsBytes =
    kTile * (sizeof(uint64_t) + sizeof(int64_t)) + kWaves * (sizeof(int64_t) + sizeof(uint64_t));

/*! \brief what the kernels share: the transpose, the weights, the outputs */
struct CutArgs {
  const int64_t* col_ptr;  // nfeat + 1, from 0
  int64_t nfeat;
  int64_t nnz;
  const uint32_t* row;  // row id of entry j at row[j * stride]
  const float* val;     // value at val[j * stride]; null: 1.0
  int64_t stride;       // 2 for a transpose's interleaved pairs
  const float* weight;  // rows
  int64_t rows;
  double scale;
  uint32_t max_bins;
  const int64_t* bound;  // nfeat + 1: scan of min(n_f, max_bins)
  float* scratch;
  int64_t scratch_entries;
  int64_t* counts;  // nfeat
  uint32_t* error;
};

/*! \brief the carries of a column's pick across its tiles (uniform in the group) */
struct Carry {
  int64_t c;        // sum of q so far
  int64_t t_prev;   // t of the last run end so far
  int64_t ncut;     // cuts so far
};

/*! \brief one thread ORs the wave's error into the status word (not an output) */
__device__ __forceinline__ void report(bool bad, uint32_t bit, uint32_t* error) {
  const uint64_t m = __ballot(bad);
  if (m != 0 && dev::lane_id() == __builtin_ctzll(m)) atomicOr(error, bit);
}

/*! \brief order-preserving u32 of a float; -0.0 is +0.0.  NaNs land past +-inf */
__device__ __forceinline__ uint32_t ordered_of(float v, bool* nan) {
  *nan |= v != v;
  uint32_t b = __float_as_uint(v);
  if ((b << 1) == 0u) b = 0u;
  return (b & 0x80000000u) != 0u ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_float(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) != 0u ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ uint32_t hi_of(uint64_t e) { return static_cast<uint32_t>(e >> 32); }

__device__ __forceinline__ int64_t quantise(float w, double scale) {
  return static_cast<int64_t>(__double2ll_rn(static_cast<double>(w) * scale));
}

/*! \brief entries [*lo, *lo + n) of column f if its pointers can be used, else n = 0 */
__device__ __forceinline__ int64_t column_span(const CutArgs& a, int64_t f, int64_t* lo) {
  *lo = a.col_ptr[f];
  const int64_t n = a.col_ptr[f + 1] - *lo;
  return (*lo < 0 || n < 0 || *lo + n > a.nnz) ? 0 : n;
}
/*! \brief which kernel takes a column of n entries: 0 wave, 1 block, 2 long */
__device__ __forceinline__ int column_class(int64_t n) {
  return n <= static_cast<int64_t>(kChunk) ? 0 : (n <= static_cast<int64_t>(kTile) ? 1 : 2);
}

/*! \brief the sort element of entry i of the column at lo */
__device__ __forceinline__ uint64_t load_elem(const CutArgs& a, int64_t lo, uint32_t i, bool* nan) {
  const float v = a.val != nullptr ? a.val[(lo + i) * a.stride] : 1.0f;
  return (static_cast<uint64_t>(ordered_of(v, nan)) << 32) | i;
}
/*! \brief q of the entry at position pos of the column of n entries at lo */
__device__ __forceinline__ int64_t load_q(const CutArgs& a, int64_t lo, uint32_t pos, uint32_t n) {
  if (pos >= n) return 0;
  const uint32_t r = a.row[(lo + pos) * a.stride];
  return r < static_cast<uint64_t>(a.rows) ? quantise(a.weight[r], a.scale) : 0;
}

/*! \brief where column f's cuts go, and how many fit: min(n, B) inside the scratch */
__device__ __forceinline__ float* column_out(const CutArgs& a, int64_t f, int64_t n, int64_t* room) {
  const int64_t b = a.bound[f];
  *room = n < static_cast<int64_t>(a.max_bins) ? n : static_cast<int64_t>(a.max_bins);
  if (b < 0 || b + *room > a.scratch_entries) *room = 0;
  return a.scratch + (*room > 0 ? b : 0);
}

__device__ __forceinline__ uint32_t next_pow2(uint32_t v, uint32_t least) {
  uint32_t p = least;
  while (p < v) p <<= 1;
  return p;
}

// ------------------------------------------------- the register network
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t x, int m) {
  const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), m, dev::kWave));
  const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(x >> 32), m, dev::kWave));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ int64_t shfl_up_i64(int64_t x, int d) {
  const uint64_t u = static_cast<uint64_t>(x);
  const uint32_t lo = static_cast<uint32_t>(__shfl_up(static_cast<int>(u), d, dev::kWave));
  const uint32_t hi = static_cast<uint32_t>(__shfl_up(static_cast<int>(u >> 32), d, dev::kWave));
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}
__device__ __forceinline__ int64_t shfl_i64(int64_t x, int src) {
  const uint64_t u = static_cast<uint64_t>(x);
  const uint32_t lo = static_cast<uint32_t>(__shfl(static_cast<int>(u), src, dev::kWave));
  const uint32_t hi = static_cast<uint32_t>(__shfl(static_cast<int>(u >> 32), src, dev::kWave));
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

/*! \brief compare-exchange of two registers, x at the lower element index */
__device__ __forceinline__ void cx(uint64_t& x, uint64_t& y, bool asc) {
  if ((y < x) == asc) {
    const uint64_t t = x;
    x = y;
    y = t;
  }
}

/*!
 * \brief the stages of strides jfrom, jfrom / 2, .. 1 (jfrom <= 128) of the
 *  bitonic phase k on a chunk held blocked in registers: e[c] is element i0 +
 *  c, i0 = chunk base + 4 lane.  Element i pairs with i ^ j; the pair ascends
 *  when (i & k) == 0.
 */
__device__ __forceinline__ void wave_stages(uint64_t (&e)[kPerLane], uint32_t i0, uint32_t k,
                                            uint32_t jfrom) {
  for (uint32_t j = jfrom; j >= 1; j >>= 1) {
    if (j >= kPerLane) {
      // the partner element sits in lane ^ (j / 4), same register
      const int m = static_cast<int>(j / kPerLane);
      const bool asc = (i0 & k) == 0;  // k >= 8: the same for the lane's 4 elements
      const bool keep_min = ((i0 & j) == 0) == asc;
#pragma unroll
      for (int c = 0; c < kPerLane; ++c) {
        const uint64_t o = shfl_xor_u64(e[c], m);
        if ((o < e[c]) == keep_min) e[c] = o;
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

/*! \brief sort elements [0, n2) of an LDS region with the whole workgroup (n2 a
 *  power of two, kChunk .. kTile; the region is staged and a barrier passed;
 *  ends with a barrier) */
__device__ void block_sort(uint64_t* s_key, uint32_t n2) {
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  const uint32_t lane = static_cast<uint32_t>(dev::lane_id());
  const uint32_t nchunks = n2 / kChunk;
  uint64_t e[kPerLane];
  for (uint32_t c = wave; c < nchunks; c += kWaves) {
    const uint32_t i0 = c * kChunk + lane * kPerLane;
#pragma unroll
    for (int x = 0; x < kPerLane; ++x) e[x] = s_key[i0 + x];
    for (uint32_t k = 2; k <= kChunk; k <<= 1) wave_stages(e, i0, k, k / 2);
#pragma unroll
    for (int x = 0; x < kPerLane; ++x) s_key[i0 + x] = e[x];
  }
  __syncthreads();
  for (uint32_t k = 2 * kChunk; k <= n2; k <<= 1) {
    for (uint32_t j = k / 2; j >= kChunk; j >>= 1) {
      for (uint32_t p = threadIdx.x; p < n2 / 2; p += kThreads) {
        const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const uint64_t x = s_key[i], y = s_key[i | j];
        if ((y < x) == ((i & k) == 0)) {
          s_key[i] = y;
          s_key[i | j] = x;
        }
      }
      __syncthreads();
    }
    for (uint32_t c = wave; c < nchunks; c += kWaves) {
      const uint32_t i0 = c * kChunk + lane * kPerLane;
#pragma unroll
      for (int x = 0; x < kPerLane; ++x) e[x] = s_key[i0 + x];
      wave_stages(e, i0, k, kChunk / 2);
#pragma unroll
      for (int x = 0; x < kPerLane; ++x) s_key[i0 + x] = e[x];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------ scans of a group
/*! \brief a group is a wave (its LDS slice) or the workgroup */
template <bool kBlock>
__device__ __forceinline__ void group_sync() {
  if constexpr (kBlock) {
    __syncthreads();
  } else {
    dev::wave_sync();
  }
}

/*!
 * \brief exclusive scan of v >= 0 over the group's threads, a sum or (kMax) a
 *  maximum; *total: over all of them.  A shuffle ladder over the wave; a
 *  workgroup combines its waves' totals through s_part [kWaves] (two barriers).
 */
template <bool kBlock, bool kMax>
__device__ __forceinline__ int64_t group_excl_scan(int64_t v, int64_t* s_part, int64_t* total) {
  auto op = [](int64_t x, int64_t y) { return kMax ? (x > y ? x : y) : x + y; };
  const int lane = dev::lane_id();
  int64_t x = v;
#pragma unroll
  for (int d = 1; d < dev::kWave; d <<= 1) {
    const int64_t y = shfl_up_i64(x, d);
    if (lane >= d) x = op(y, x);
  }
  int64_t excl = shfl_up_i64(x, 1);
  if (lane == 0) excl = 0;
  const int64_t wtotal = shfl_i64(x, dev::kWave - 1);
  if constexpr (!kBlock) {
    *total = wtotal;
    return excl;
  } else {
    const int wid = threadIdx.x / dev::kWave;
    __syncthreads();  // the previous scan's totals have been read
    if (lane == 0) s_part[wid] = wtotal;
    __syncthreads();
    int64_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int64_t t = s_part[w];
      if (w < wid) base = op(base, t);
      all = op(all, t);
    }
    *total = all;
    return op(base, excl);
  }
}

// ---------------------------------------------------------------- the pick
/*!
 * \brief the cuts among entries [0, m) of a sorted tile: s_key[i] >> 32 is the
 *  ordered value, s_q[i] the entry's q (overwritten).  more / next_hi: the
 *  column goes on behind the tile, with that key.  W > 0: the column's total.
 *  Cuts of rank < room go to out[rank].  The group's threads call it together,
 *  behind a group_sync that made the tile visible; the caller syncs again
 *  before it restages the tile.
 */
template <bool kBlock>
__device__ __forceinline__ void pick_tile(const uint64_t* s_key, int64_t* s_q, uint32_t m, bool more,
                                          uint32_t next_hi, int64_t W, uint32_t B, Carry* carry,
                                          float* out, int64_t room, int64_t* s_part) {
  constexpr uint32_t kGroup = kBlock ? kThreads : dev::kWave;
  const uint32_t g = kBlock ? threadIdx.x : static_cast<uint32_t>(dev::lane_id());
  const uint32_t per = (m + kGroup - 1) / kGroup;  // at most kTile / kThreads = 16 (a wave: 4)
  const uint32_t i0 = g * per < m ? g * per : m;
  const uint32_t i1 = i0 + per < m ? i0 + per : m;
  // the inclusive scan of q: c at the thread's first entry
  int64_t sum = 0;
  for (uint32_t i = i0; i < i1; ++i) sum += s_q[i];
  int64_t tile_sum;
  int64_t c = carry->c + group_excl_scan<kBlock, false>(sum, s_part, &tile_sum);
  // t of every run end (0 elsewhere: a t of 0 is never a cut)
  int64_t tmax = 0;
  for (uint32_t i = i0; i < i1; ++i) {
    c += s_q[i];
    const uint32_t key = hi_of(s_key[i]);
    const bool end = i + 1 < m ? hi_of(s_key[i + 1]) != key : (!more || next_hi != key);
    const int64_t t =
        end ? static_cast<int64_t>(static_cast<uint64_t>(c) * B / static_cast<uint64_t>(W)) : 0;
    s_q[i] = t;
    tmax = t > tmax ? t : tmax;
  }
  int64_t tile_max;
  int64_t prev = group_excl_scan<kBlock, true>(tmax, s_part, &tile_max);
  prev = prev > carry->t_prev ? prev : carry->t_prev;
  // a run end is a cut where its t exceeds the previous run end's
  uint32_t bits = 0;
  for (uint32_t i = i0; i < i1; ++i) {
    const int64_t t = s_q[i];
    if (t > prev) {
      bits |= 1u << (i - i0);
      prev = t;
    }
  }
  int64_t tile_cuts;
  int64_t rank = carry->ncut +
                 group_excl_scan<kBlock, false>(static_cast<int64_t>(__popc(bits)), s_part, &tile_cuts);
  for (; bits != 0; bits &= bits - 1) {
    const uint32_t i = i0 + static_cast<uint32_t>(__builtin_ctz(bits));
    if (rank < room) out[rank] = ordered_to_float(hi_of(s_key[i]));
    ++rank;
  }
  carry->c += tile_sum;
  carry->t_prev = tile_max > carry->t_prev ? tile_max : carry->t_prev;
  carry->ncut += tile_cuts;
}

// ------------------------------------------------------------ the weights
__global__ __launch_bounds__(kThreads) void k_cutw_weights(const float* __restrict__ weight,
                                                           int64_t rows, uint32_t* error) {
  bool bad = false;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; r < rows;
       r += static_cast<int64_t>(gridDim.x) * kThreads) {
    const float w = weight[r];
    bad |= !(w >= 0.0f) || w == __builtin_inff();
  }
  report(bad, kGbdtErrWeight, error);
}

// ----------------------------------------------------------------- GB1w-a
__global__ __launch_bounds__(kThreads) void k_cutw_wave(CutArgs a) {
  __shared__ uint64_t s_keys[kWaves][kChunk];
  __shared__ int64_t s_qs[kWaves][kChunk];
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  const uint32_t lane = static_cast<uint32_t>(dev::lane_id());
  uint64_t* const s_key = s_keys[wave];
  int64_t* const s_q = s_qs[wave];
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWaves;
  bool nan = false;
  for (int64_t f = static_cast<int64_t>(blockIdx.x) * kWaves + wave; f < a.nfeat; f += nwaves) {
    int64_t lo;
    const int64_t len = column_span(a, f, &lo);
    if (column_class(len) != 0) continue;
    if (len == 0) {
      if (lane == 0) a.counts[f] = 0;
      continue;
    }
    const uint32_t n = static_cast<uint32_t>(len);
    const uint32_t i0 = lane * kPerLane;
    uint64_t e[kPerLane];
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) e[c] = i0 + c < n ? load_elem(a, lo, i0 + c, &nan) : kPad;
    // elements at and past n2 are padding and only ever meet each other
    const uint32_t n2 = next_pow2(n, kPerLane);
    for (uint32_t k = 2; k <= n2; k <<= 1) wave_stages(e, i0, k, k / 2);
    int64_t sum = 0;
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
      const int64_t q = load_q(a, lo, static_cast<uint32_t>(e[c]), n);
      s_key[i0 + c] = e[c];
      s_q[i0 + c] = q;
      sum += q;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += shfl_i64(sum, static_cast<int>(lane) ^ d);
    const int64_t W = sum;
    dev::wave_sync();
    Carry carry{0, 0, 0};
    int64_t room;
    float* const out = column_out(a, f, len, &room);
    if (W > 0) pick_tile<false>(s_key, s_q, n, false, 0u, W, a.max_bins, &carry, out, room, nullptr);
    if (lane == 0) a.counts[f] = carry.ncut < room ? carry.ncut : room;
    dev::wave_sync();  // the slice is read before the next column is staged
  }
  report(nan, kGbdtErrNaN, a.error);
}

/*! \brief GB1w-b / -c: the columns of class `cls` among [g0, g0 + kColGroup), a
 *  mask per wave of the workgroup in s_mask [kWaves] (two barriers) */
__device__ __forceinline__ void class_masks(const CutArgs& a, int64_t g0, int cls, uint64_t* s_mask) {
  __syncthreads();  // the previous group's masks have been read
  const int64_t f = g0 + threadIdx.x;
  int64_t lo;
  const bool mine = f < a.nfeat && column_class(column_span(a, f, &lo)) == cls;
  const uint64_t m = __ballot(mine);
  if (dev::lane_id() == 0) s_mask[threadIdx.x / dev::kWave] = m;
  __syncthreads();
}

// ----------------------------------------------------------------- GB1w-b
__global__ __launch_bounds__(kThreads) void k_cutw_block(CutArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint64_t* const s_key = reinterpret_cast<uint64_t*>(s_raw);
  int64_t* const s_q = reinterpret_cast<int64_t*>(s_key + kTile);
  int64_t* const s_part = s_q + kTile;
  uint64_t* const s_mask = reinterpret_cast<uint64_t*>(s_part + kWaves);
  bool nan = false;
  for (int64_t g0 = static_cast<int64_t>(blockIdx.x) * kColGroup; g0 < a.nfeat;
       g0 += static_cast<int64_t>(gridDim.x) * kColGroup) {
    class_masks(a, g0, 1, s_mask);
    for (int w = 0; w < kWaves; ++w) {
      uint64_t mask = s_mask[w];
      while (mask != 0) {
        const int64_t f = g0 + w * dev::kWave + __builtin_ctzll(mask);
        mask &= mask - 1;
        const int64_t lo = a.col_ptr[f];
        const uint32_t n = static_cast<uint32_t>(a.col_ptr[f + 1] - lo);
        const uint32_t n2 = next_pow2(n, kChunk);
        for (uint32_t i = threadIdx.x; i < n2; i += kThreads) {
          s_key[i] = i < n ? load_elem(a, lo, i, &nan) : kPad;
        }
        __syncthreads();
        block_sort(s_key, n2);
        int64_t sum = 0;
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
          const int64_t q = load_q(a, lo, static_cast<uint32_t>(s_key[i]), n);
          s_q[i] = q;
          sum += q;
        }
        int64_t W;
        (void)group_excl_scan<true, false>(sum, s_part, &W);
        __syncthreads();
        Carry carry{0, 0, 0};
        int64_t room;
        float* const out = column_out(a, f, n, &room);
        if (W > 0) pick_tile<true>(s_key, s_q, n, false, 0u, W, a.max_bins, &carry, out, room, s_part);
        if (threadIdx.x == 0) a.counts[f] = carry.ncut < room ? carry.ncut : room;
        __syncthreads();  // the region is read before the next column is staged
      }
    }
  }
  report(nan, kGbdtErrNaN, a.error);
}

// ----------------------------------------------------------------- GB1w-c
/*! \brief the side CSR of the long columns: side_ptr [nfeat + 1] (the scan of
 *  their lengths, 0 for the others), keys / weights [side_entries] */
struct SideArgs {
  const int64_t* side_ptr;
  int64_t side_entries;
  uint32_t* key;
  float* w;
};

/*! \brief the long column f's slice [*b, *b + n) of the side CSR, or false */
__device__ __forceinline__ bool side_span(const SideArgs& s, int64_t f, int64_t n, int64_t* b) {
  *b = s.side_ptr[f];
  return *b >= 0 && s.side_ptr[f + 1] - *b == n && *b + n <= s.side_entries;
}

__global__ __launch_bounds__(kThreads) void k_cutw_long_prepare(CutArgs a, SideArgs s) {
  __shared__ uint64_t s_mask[kWaves];
  bool nan = false;
  for (int64_t g0 = static_cast<int64_t>(blockIdx.x) * kColGroup; g0 < a.nfeat;
       g0 += static_cast<int64_t>(gridDim.x) * kColGroup) {
    class_masks(a, g0, 2, s_mask);
    for (int w = 0; w < kWaves; ++w) {
      uint64_t mask = s_mask[w];
      while (mask != 0) {
        const int64_t f = g0 + w * dev::kWave + __builtin_ctzll(mask);
        mask &= mask - 1;
        const int64_t lo = a.col_ptr[f], n = a.col_ptr[f + 1] - lo;
        int64_t b;
        if (!side_span(s, f, n, &b)) continue;
        for (int64_t i = threadIdx.x; i < n; i += kThreads) {
          const float v = a.val != nullptr ? a.val[(lo + i) * a.stride] : 1.0f;
          const uint32_t r = a.row[(lo + i) * a.stride];
          s.key[b + i] = ordered_of(v, &nan);
          s.w[b + i] = r < static_cast<uint64_t>(a.rows) ? a.weight[r] : 0.0f;
        }
      }
    }
  }
  report(nan, kGbdtErrNaN, a.error);
}

/*! \brief s: the side CSR sorted by key within every column */
__global__ __launch_bounds__(kThreads) void k_cutw_long_pick(CutArgs a, SideArgs s) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint64_t* const s_key = reinterpret_cast<uint64_t*>(s_raw);
  int64_t* const s_q = reinterpret_cast<int64_t*>(s_key + kTile);
  int64_t* const s_part = s_q + kTile;
  uint64_t* const s_mask = reinterpret_cast<uint64_t*>(s_part + kWaves);
  for (int64_t g0 = static_cast<int64_t>(blockIdx.x) * kColGroup; g0 < a.nfeat;
       g0 += static_cast<int64_t>(gridDim.x) * kColGroup) {
    class_masks(a, g0, 2, s_mask);
    for (int w = 0; w < kWaves; ++w) {
      uint64_t mask = s_mask[w];
      while (mask != 0) {
        const int64_t f = g0 + w * dev::kWave + __builtin_ctzll(mask);
        mask &= mask - 1;
        const int64_t n = a.col_ptr[f + 1] - a.col_ptr[f];
        int64_t b;
        if (!side_span(s, f, n, &b)) {
          if (threadIdx.x == 0) a.counts[f] = 0;
          continue;
        }
        int64_t sum = 0;
        for (int64_t i = threadIdx.x; i < n; i += kThreads) sum += quantise(s.w[b + i], a.scale);
        int64_t W;
        (void)group_excl_scan<true, false>(sum, s_part, &W);
        Carry carry{0, 0, 0};
        int64_t room;
        float* const out = column_out(a, f, n, &room);
        for (int64_t tb = 0; W > 0 && tb < n; tb += kTile) {
          const uint32_t tn = static_cast<uint32_t>(n - tb < kTile ? n - tb : kTile);
          __syncthreads();  // the previous tile has been read
          for (uint32_t i = threadIdx.x; i < tn; i += kThreads) {
            s_key[i] = static_cast<uint64_t>(s.key[b + tb + i]) << 32;
            s_q[i] = quantise(s.w[b + tb + i], a.scale);
          }
          __syncthreads();
          const bool more = tb + tn < n;
          const uint32_t next_hi = more ? s.key[b + tb + tn] : 0u;
          pick_tile<true>(s_key, s_q, tn, more, next_hi, W, a.max_bins, &carry, out, room, s_part);
        }
        if (threadIdx.x == 0) a.counts[f] = carry.ncut < room ? carry.ncut : room;
      }
    }
  }
}

// ----------------------------------------------------------------- GB1w-d
__global__ __launch_bounds__(kThreads) void k_cutw_compact(const int64_t* __restrict__ bound,
                                                           const int64_t* __restrict__ cut_ptr,
                                                           const float* __restrict__ scratch,
                                                           int64_t scratch_entries, int64_t nfeat,
                                                           float* __restrict__ cut, int64_t capacity) {
  const int lane = dev::lane_id();
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWaves;
  for (int64_t f = static_cast<int64_t>(blockIdx.x) * kWaves + threadIdx.x / dev::kWave; f < nfeat;
       f += nwaves) {
    const int64_t src = bound[f], dst = cut_ptr[f];
    int64_t n = cut_ptr[f + 1] - dst;
    if (src < 0 || dst < 0 || n < 0 || src + n > scratch_entries || dst + n > capacity) n = 0;
    for (int64_t k = lane; k < n; k += dev::kWave) cut[dst + k] = scratch[src + k];
  }
}

CutArgs MakeArgs(const char* op, const CsrView& columns, uint64_t nnz, const GbdtCutWeights& w,
                 uint32_t max_bins, const int64_t* bound, float* scratch, uint64_t scratch_entries,
                 int64_t* counts, uint32_t* error) {
  CheckView(op, columns, true);
  CHECK(columns.nrows >= 1 && columns.nrows <= CSRTransposeMaxFeatures())
      << op << ": num_features must be in [1, " << CSRTransposeMaxFeatures() << "]";
  CHECK(!columns.index64) << op << ": a transpose has 32-bit row ids";
  CHECK(max_bins >= 2 && max_bins <= kGbdtMaxBins) << op << ": max_bins must be in [2, 256]";
  CHECK_LT(nnz, 1ull << 62) << op << ": too many entries";
  CHECK(w.weight != nullptr && w.scale > 0.0) << op << ": needs weights and a positive scale";
  CutArgs a;
  a.col_ptr = reinterpret_cast<const int64_t*>(columns.offset);
  a.nfeat = static_cast<int64_t>(columns.nrows);
  a.nnz = static_cast<int64_t>(nnz);
  a.row = static_cast<const uint32_t*>(columns.index);
  a.val = columns.value;
  a.stride = columns.paired ? 2 : 1;
  a.weight = w.weight;
  a.rows = static_cast<int64_t>(w.rows);
  a.scale = w.scale;
  a.max_bins = max_bins;
  a.bound = bound;
  a.scratch = scratch;
  a.scratch_entries = static_cast<int64_t>(scratch_entries);
  a.counts = counts;
  a.error = error;
  return a;
}
}  // namespace

void LaunchGbdtCutFused(const CsrView& columns, uint64_t nnz, const GbdtCutWeights& weights,
                        uint32_t max_bins, const int64_t* bound, float* scratch,
                        uint64_t scratch_entries, int64_t* counts, uint32_t* error,
                        hipStream_t stream) {
  const CutArgs a = MakeArgs("gbdt weighted cuts", columns, nnz, weights, max_bins, bound, scratch,
                             scratch_entries, counts, error);
  if (weights.rows > 0) {
    hipLaunchKernelGGL(k_cutw_weights, dim3(GridFor(weights.rows, kThreads)), dim3(kThreads), 0,
                       stream, weights.weight, a.rows, error);
    DMLC_HIP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_cutw_wave, dim3(GridFor(columns.nrows, kWaves)), dim3(kThreads), 0, stream, a);
  DMLC_HIP_CHECK_LAUNCH();
  PrepareLdsLaunch(k_cutw_block, kTileLdsBytes);
  hipLaunchKernelGGL(k_cutw_block, dim3(GridFor(columns.nrows, kColGroup)), dim3(kThreads),
                     kTileLdsBytes, stream, a);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchGbdtCutLong(const CsrView& columns, uint64_t nnz, const GbdtCutWeights& weights,
                       uint32_t max_bins, const int64_t* bound, float* scratch,
                       uint64_t scratch_entries, int64_t* counts, const GbdtCutSide& side,
                       uint32_t* error, hipStream_t stream) {
  const CutArgs a = MakeArgs("gbdt weighted cuts, long columns", columns, nnz, weights, max_bins,
                             bound, scratch, scratch_entries, counts, error);
  if (side.entries == 0) return;
  const int groups = GridFor(columns.nrows, kColGroup);
  const SideArgs raw{side.ptr, static_cast<int64_t>(side.entries), side.key, side.weight};
  hipLaunchKernelGGL(k_cutw_long_prepare, dim3(groups), dim3(kThreads), 0, stream, a, raw);
  DMLC_HIP_CHECK_LAUNCH();
  // the side CSR's rows are the columns: SR1 - SR3 order every long one by key, stably
  const CsrView rows{reinterpret_cast<const uint64_t*>(side.ptr), side.key, side.weight, nullptr,
                     columns.nrows, false, false};
  LaunchSortRows(rows, side.entries, false, side.sorted_ptr, side.sorted_key, side.sorted_weight,
                 nullptr, side.sort_scratch, error + 1, stream);
  const SideArgs sorted{side.ptr, static_cast<int64_t>(side.entries), side.sorted_key,
                        side.sorted_weight};
  PrepareLdsLaunch(k_cutw_long_pick, kTileLdsBytes);
  hipLaunchKernelGGL(k_cutw_long_pick, dim3(groups), dim3(kThreads), kTileLdsBytes, stream, a,
                     sorted);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchGbdtCutCompact(const int64_t* bound, const int64_t* cut_ptr, const float* scratch,
                          uint64_t scratch_entries, uint64_t num_features, float* cut,
                          uint64_t capacity, hipStream_t stream) {
  if (capacity == 0 || num_features == 0) return;
  hipLaunchKernelGGL(k_cutw_compact, dim3(GridFor(num_features, kWaves)), dim3(kThreads), 0, stream,
                     bound, cut_ptr, scratch, static_cast<int64_t>(scratch_entries),
                     static_cast<int64_t>(num_features), cut, static_cast<int64_t>(capacity));
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
