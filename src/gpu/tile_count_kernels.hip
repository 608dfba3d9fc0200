/*!
 * \file src/gpu/tile_count_kernels.hip
 * \brief the tile parser's C1 count, C2 scan and C4 fold (tile_common.h has
 *  the overview).  The CSV and RecordIO pipelines use C2 (LaunchTileScanRaw)
 *  and C4 (LaunchTileFinish) over their own per-tile counts and slots.
 *
 *  C1 k_tile_count (one wave per 8 KiB tile): SWAR byte masks of 16 B per
 *     lane, per tile (line starts << 32 | token starts) and an irregular bit (a
 *     line that starts with a blank, control bytes other than \t \n \r).
 *     Reads the chunk once.  A token that does not start with [0-9+-.] never
 *     passes the fill's register-window decoder; the fill (and the fused hash
 *     kernel) flags it irregular on that fallback path, at no fast-path cost.
 *  C2 k_tile_scan  (one 1024-lane workgroup): exclusive scan of the tile
 *     counts, OR of the flags; nlines / nrows / nnz / flags go to the
 *     ChunkMeta and to mapped pinned memory the host polls (no D2H copy).
 *  C4 k_tile_finish (one workgroup): fold the slots into the ChunkMeta and
 *     write the chunk's closing row pointer.
 */
#include <dmlc/gpu/hip_utils.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "./device_common.h"
#include "./kernels.h"
#include "./tile_common.h"

namespace dmlc {
namespace gpu {

namespace {
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ text, size_t pos, size_t n) {
  // a 16 B load that starts before n stays inside n + kTextPadBytes
  if (pos < n) return *reinterpret_cast<const uint4*>(text + pos);
  return make_uint4(0, 0, 0, 0);
}

/*!
 * \brief C1: one wave per 8 KiB tile, 8 x 16 B loads per lane all in flight,
 *  wave-level reductions only (no LDS, no barrier).
 */
__global__ __launch_bounds__(kThreads) void k_tile_count(const uint8_t* __restrict__ text,
                                                         size_t n, size_t ntiles,
                                                         uint64_t* __restrict__ counts,
                                                         uint32_t* __restrict__ flags,
                                                         uint2* __restrict__ masks) {
  const int lane = dev::lane_id();
  const size_t tile = static_cast<size_t>(blockIdx.x) * (kThreads / dev::kWave) +
                      threadIdx.x / dev::kWave;
  if (tile >= ntiles) return;  // whole waves leave; no barrier below
  const size_t base = tile * kTileBytes;
  uint4 v[kCountLoads];
#pragma unroll
  for (int j = 0; j < kCountLoads; ++j) v[j] = load16(text, base + j * 1024 + lane * 16, n);
  const uint32_t first = base == 0 ? static_cast<uint32_t>('\n') : text[base - 1];
  uint32_t lines = 0, toks = 0, qtoks = 0;
  bool bad = false;
  // the fill's masks of slices 2 s and 2 s + 1 (its step s), one 8-byte store
  // per lane per step: [tile][step][lane]
  uint2* const mrow = masks + tile * (kTileBytes / 2048) * dev::kWave + lane;
  auto count_tile = [&](auto full) {
    uint32_t m0 = 0;
#pragma unroll
    for (int j = 0; j < kCountLoads; ++j) {
      const uint32_t pc = count_prev(v, j, first, lane);
      uint32_t m;
      bad |= count16<decltype(full)::value>(v[j], pc, base + j * 1024 + lane * 16, n, &lines,
                                            &toks, &qtoks, &m);
      if (j & 1) {
        mrow[(j >> 1) * dev::kWave] = make_uint2(m0, m);
      } else {
        m0 = m;
      }
    }
  };
  if (base + kTileBytes <= n) {  // wave-uniform: every tile but a chunk's last
    count_tile(std::true_type{});
  } else {
    count_tile(std::false_type{});
  }
  lines = dev::wave_sum(lines);
  toks = dev::wave_sum(toks);
  qtoks = dev::wave_sum(qtoks);
  const bool any_bad = __any(bad);
  if (lane == 0) {
    // letter-started tokens (LibSVM `qid:`) are no CSR entries: out of the count
    counts[tile] = (static_cast<uint64_t>(lines) << 32) | (toks - qtoks);
    flags[tile] = (any_bad ? kFlagIrregular : 0u) | (qtoks != 0 ? kFlagQid : 0u);
  }
}

constexpr int kScanThreads = 1024;
constexpr int kScanPer = 8;

/*! \brief exclusive scan of ntiles counts in place (one workgroup), meta totals */
__global__ __launch_bounds__(kScanThreads) void k_tile_scan(uint64_t* __restrict__ counts,
                                                            const uint32_t* __restrict__ flags,
                                                            size_t ntiles, ChunkMeta* meta,
                                                            ChunkMeta* host_meta, int raw) {
  __shared__ uint64_t swave[kScanThreads / 64];
  __shared__ uint32_t sflag[kScanThreads / 64];
  const int wid = threadIdx.x / dev::kWave;
  uint64_t carry = 0;
  uint32_t fl = 0;
  for (size_t t0 = 0; t0 < ntiles; t0 += static_cast<size_t>(kScanThreads) * kScanPer) {
    const size_t base = t0 + static_cast<size_t>(threadIdx.x) * kScanPer;
    uint64_t v[kScanPer];
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
      v[i] = base + i < ntiles ? counts[base + i] : 0;
      if (base + i < ntiles) fl |= flags[base + i];
      s += v[i];
    }
    uint64_t wtot;
    const uint64_t wx = dev::wave_excl_scan(s, &wtot);
    if (dev::lane_id() == 0) swave[wid] = wtot;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const uint64_t t = swave[w];
      if (w < wid) before += t;
      all += t;
    }
    uint64_t x = carry + before + wx;
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
      if (base + i < ntiles) counts[base + i] = x;
      x += v[i];
    }
    carry += all;
    __syncthreads();
  }
  fl = dev::wave_or(fl);
  if (dev::lane_id() == 0) sflag[wid] = fl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t f = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) f |= sflag[w];
    const uint64_t lines = carry >> 32, toks = carry & 0xffffffffull;
    // text: (lines << 32 | tokens); raw (RecordIO): (records << 32 | bytes)
    meta->nlines = lines;
    meta->nrows = lines;
    meta->nnz = raw ? toks : toks - lines;
    meta->max_index = 0;
    meta->max_field = 0;
    meta->flags = f;
    meta->pad = 0;
    if (host_meta != nullptr) publish_host_meta(host_meta, *meta);  // no D2H blit
  }
}

/*!
 * \brief two-level scan for large chunks (a 1 GiB HBM-resident pass has 131 K
 *  tiles; one workgroup reading them all is bound by a single CU's load path).
 *  Level 1: workgroup g scans tiles [4096 g, 4096 (g+1)) in place -- coalesced
 *  loads into LDS, a blocked 4-per-lane scan, coalesced stores -- and writes
 *  its total and flag OR.  Level 2 is k_tile_scan over the block totals (it
 *  also fills the ChunkMeta).  Level 3 adds each block's prefix to its tiles.
 */
constexpr int kScanBlockPer = 4;
constexpr size_t kScanBlockTiles = static_cast<size_t>(kScanThreads) * kScanBlockPer;
__global__ __launch_bounds__(kScanThreads) void k_tile_scan_local(uint64_t* __restrict__ counts,
                                                                  const uint32_t* __restrict__ flags,
                                                                  size_t ntiles,
                                                                  uint64_t* __restrict__ bsum,
                                                                  uint32_t* __restrict__ bflag) {
  __shared__ uint64_t sbuf[kScanBlockTiles];
  __shared__ uint64_t swave[kScanThreads / 64];
  __shared__ uint32_t sfl[kScanThreads / 64];
  const int wid = threadIdx.x / dev::kWave;
  const size_t t0 = static_cast<size_t>(blockIdx.x) * kScanBlockTiles;
  uint32_t fl = 0;
#pragma unroll
  for (int k = 0; k < kScanBlockPer; ++k) {
    const size_t idx = t0 + static_cast<size_t>(k) * kScanThreads + threadIdx.x;
    uint64_t c = 0;
    if (idx < ntiles) {
      c = counts[idx];
      fl |= flags[idx];
    }
    sbuf[k * kScanThreads + threadIdx.x] = c;
  }
  __syncthreads();
  uint64_t v[kScanBlockPer];
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < kScanBlockPer; ++i) {
    v[i] = sbuf[threadIdx.x * kScanBlockPer + i];
    s += v[i];
  }
  uint64_t wtot;
  const uint64_t wx = dev::wave_excl_scan(s, &wtot);
  fl = dev::wave_or(fl);
  if (dev::lane_id() == 0) {
    swave[wid] = wtot;
    sfl[wid] = fl;
  }
  __syncthreads();
  uint64_t before = 0, all = 0;
  uint32_t f = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const uint64_t t = swave[w];
    if (w < wid) before += t;
    all += t;
    f |= sfl[w];
  }
  uint64_t x = before + wx;
#pragma unroll
  for (int i = 0; i < kScanBlockPer; ++i) {  // each lane rewrites only its own 4 entries
    sbuf[threadIdx.x * kScanBlockPer + i] = x;
    x += v[i];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kScanBlockPer; ++k) {
    const size_t idx = t0 + static_cast<size_t>(k) * kScanThreads + threadIdx.x;
    if (idx < ntiles) counts[idx] = sbuf[k * kScanThreads + threadIdx.x];
  }
  if (threadIdx.x == 0) {
    bsum[blockIdx.x] = all;
    bflag[blockIdx.x] = f;
  }
}

__global__ __launch_bounds__(kThreads) void k_tile_scan_add(uint64_t* __restrict__ counts,
                                                            size_t ntiles,
                                                            const uint64_t* __restrict__ bprefix) {
  const size_t t = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (t < ntiles) counts[t] += bprefix[t / kScanBlockTiles];
}

/*!
 * \brief fold the per-workgroup slots into meta; closing row pointer.  One
 *  1024-lane workgroup, 8 independent slot loads per lane per step (a
 *  latency-bound single-workgroup pass otherwise dominates small chunks).
 */
constexpr int kFinishThreads = 1024;
constexpr int kFinishPer = 8;
__global__ __launch_bounds__(kFinishThreads) void k_tile_finish(
    const MetaPartial* __restrict__ p, int np, ChunkMeta* meta, ChunkMeta* host_meta,
    uint64_t* offset, uint64_t row_base, uint64_t nnz_base) {
  unsigned long long mi = 0, mf = 0;
  unsigned fl = 0;
  for (int i0 = threadIdx.x; i0 < np; i0 += kFinishThreads * kFinishPer) {
    MetaPartial q[kFinishPer];
#pragma unroll
    for (int u = 0; u < kFinishPer; ++u) {
      const int i = i0 + u * kFinishThreads;
      if (i < np) {
        q[u] = p[i];
      } else {
        q[u].max_index = q[u].max_field = 0;
        q[u].flags = 0;
      }
    }
#pragma unroll
    for (int u = 0; u < kFinishPer; ++u) {
      mi = q[u].max_index > mi ? q[u].max_index : mi;
      mf = q[u].max_field > mf ? q[u].max_field : mf;
      fl |= q[u].flags;
    }
  }
  dev::block_fold_meta<kFinishThreads>(&mi, &mf, &fl);
  if (threadIdx.x == 0) {
    meta->max_index = mi;
    meta->max_field = mf;
    meta->flags |= fl;
    // (an overflowed one-pass fill's rows reach past the target: no row pointer)
    if (offset != nullptr && !(meta->flags & kFlagOverflow)) {
      offset[row_base + meta->nrows] = nnz_base + meta->nnz;
    }
    if (host_meta != nullptr) publish_host_meta(host_meta, *meta);
  }
}
/*! \brief level 1 of the finish fold: workgroup g folds slots g, g+G, ... into out[g] */
__global__ __launch_bounds__(kFinishThreads) void k_tile_finish_partial(
    const MetaPartial* __restrict__ p, size_t np, MetaPartial* __restrict__ out) {
  unsigned long long mi = 0, mf = 0;
  unsigned fl = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kFinishThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kFinishThreads + threadIdx.x; i < np;
       i += stride) {
    const MetaPartial q = p[i];
    mi = q.max_index > mi ? q.max_index : mi;
    mf = q.max_field > mf ? q.max_field : mf;
    fl |= q.flags;
  }
  dev::block_fold_meta<kFinishThreads>(&mi, &mf, &fl);
  if (threadIdx.x == 0) {
    MetaPartial r;
    r.max_index = mi;
    r.max_field = mf;
    r.flags = fl;
    r.pad = 0;
    out[blockIdx.x] = r;
  }
}

// chunks above this many tiles take the multi-workgroup scan / finish
constexpr size_t kTwoLevelTiles = 2 * kScanBlockTiles;
constexpr int kFinishGroups = 128;

void TileScan(uint64_t* tile_counts, uint32_t* tile_flags, size_t ntiles, ChunkMeta* meta,
              ChunkMeta* host_meta, int raw, hipStream_t stream) {
  if (ntiles <= kTwoLevelTiles) {
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanThreads), 0, stream, tile_counts,
                       tile_flags, ntiles, meta, host_meta, raw);
    return;
  }
  // block totals / flags live past the tiles (TileScratchWords reserves them)
  const size_t nblk = (ntiles + kScanBlockTiles - 1) / kScanBlockTiles;
  uint64_t* bsum = tile_counts + ntiles;
  uint32_t* bflag = tile_flags + ntiles;
  hipLaunchKernelGGL(k_tile_scan_local, dim3(nblk), dim3(kScanThreads), 0, stream, tile_counts,
                     tile_flags, ntiles, bsum, bflag);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanThreads), 0, stream, bsum, bflag, nblk, meta,
                     host_meta, raw);
  hipLaunchKernelGGL(k_tile_scan_add, dim3((ntiles + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, tile_counts, ntiles, bsum);
}
}  // namespace

size_t TileCount(size_t nbytes) { return (nbytes + kTileBytes - 1) / kTileBytes; }

void LaunchTileCountScan(const char* text, size_t nbytes, uint64_t* tile_counts,
                         uint32_t* tile_flags, uint32_t* tile_masks, ChunkMeta* meta,
                         ChunkMeta* host_meta, hipStream_t stream) {
  const size_t ntiles = TileCount(nbytes);
  CHECK(tile_masks != nullptr) << "LaunchTileCountScan: tile_masks (TileMaskWords) is required";
  if (ntiles != 0) {
    const size_t per_block = kThreads / dev::kWave;
    hipLaunchKernelGGL(k_tile_count, dim3((ntiles + per_block - 1) / per_block), dim3(kThreads), 0,
                       stream, reinterpret_cast<const uint8_t*>(text), nbytes, ntiles, tile_counts,
                       tile_flags, reinterpret_cast<uint2*>(tile_masks));
  }
  TileScan(tile_counts, tile_flags, ntiles, meta, host_meta, 0, stream);
}

void LaunchTileScanRaw(uint64_t* tile_counts, uint32_t* tile_flags, size_t ntiles,
                       ChunkMeta* meta, ChunkMeta* host_meta, hipStream_t stream) {
  TileScan(tile_counts, tile_flags, ntiles, meta, host_meta, 1, stream);
}

void LaunchTileFinish(MetaPartial* partials, size_t nslots, ChunkMeta* meta, ChunkMeta* host_meta,
                      uint64_t* offset, uint64_t row_base, uint64_t nnz_base, hipStream_t stream) {
  const MetaPartial* src = partials;
  int np = static_cast<int>(nslots);
  if (nslots > kTwoLevelTiles) {
    MetaPartial* folded = partials + nslots;  // TileScratchSlots(nslots) leaves room
    hipLaunchKernelGGL(k_tile_finish_partial, dim3(kFinishGroups), dim3(kFinishThreads), 0, stream,
                       partials, nslots, folded);
    src = folded;
    np = kFinishGroups;
  }
  hipLaunchKernelGGL(k_tile_finish, dim3(1), dim3(kFinishThreads), 0, stream, src, np, meta,
                     host_meta, offset, row_base, nnz_base);
}

size_t TileScratchWords(size_t ntiles) {
  return ntiles + (ntiles + kScanBlockTiles - 1) / kScanBlockTiles + 64;
}

size_t TileScratchSlots(size_t ntiles) { return ntiles + kFinishGroups; }

size_t TileMaskWords(size_t ntiles) { return ntiles * (kTileBytes / 16); }

}  // namespace gpu
}  // namespace dmlc
