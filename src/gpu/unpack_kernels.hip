/*!
 * \file src/gpu/unpack_kernels.hip
 * \brief Device side of the packed H2D transfer (text_pack.h): expand a
 *  chunk's 4-bit codes back to its n text bytes at a destination of any
 *  alignment, then overwrite the exception blocks with their raw bytes.
 *  Bytes past dst + n are never written.
 *
 * k_unpack_nibbles: one lane per 16 output bytes, grouped on the
 * destination's 16-byte grid -- two aligned 8-byte loads of codes (funnel
 * shifted when the destination is misaligned against the code stream), one
 * 16-byte store.  The groups cut by either end of the chunk store bytes.
 * k_unpack_exceptions: one workgroup per exception block, byte stores (the
 * blocks are rare: a chunk with many goes raw).
 * k_unpack_dense: the dense code of text_pack_dense.h (described at the kernel).
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "./kernels.h"
#include "./text_pack.h"
#include "./text_pack_dense.h"

namespace dmlc {
namespace gpu {

namespace {
constexpr int kThreads = 256;

struct Alphabet4 {
  uint32_t w[4];
};

__device__ __forceinline__ uint32_t decode(const Alphabet4& a, uint32_t code) {
  const uint32_t sel = code >> 2;
  const uint32_t lo = sel & 1 ? a.w[1] : a.w[0];
  const uint32_t hi = sel & 1 ? a.w[3] : a.w[2];
  const uint32_t word = sel & 2 ? hi : lo;
  return (word >> ((code & 3) * 8)) & 0xffu;
}

__global__ __launch_bounds__(kThreads) void k_unpack_nibbles(const uint64_t* __restrict__ nib,
                                                             size_t n, Alphabet4 alpha,
                                                             char* __restrict__ dst,
                                                             unsigned lead) {
  const size_t g = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  // output bytes [s, s + 16) of the chunk; dst + s is 16-byte aligned
  const long long s = static_cast<long long>(g) * 16 - static_cast<long long>(lead);
  const long long end = static_cast<long long>(n);
  if (s >= end) return;
  if (s >= 0 && s + 16 <= end) {
    const size_t w = static_cast<size_t>(s) >> 4;
    const unsigned sh = (static_cast<unsigned>(s) & 15u) * 4u;  // the same for every lane
    uint64_t v = nib[w];
    if (sh != 0) v = (v >> sh) | (nib[w + 1] << (64u - sh));
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c = static_cast<uint32_t>(v >> (16 * q)) & 0xffffu;
      o[q] = decode(alpha, c & 15u) | (decode(alpha, (c >> 4) & 15u) << 8) |
             (decode(alpha, (c >> 8) & 15u) << 16) | (decode(alpha, c >> 12) << 24);
    }
    *reinterpret_cast<uint4*>(dst + s) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(nib);
    const long long j0 = s < 0 ? 0 : s;
    const long long j1 = s + 16 < end ? s + 16 : end;
    for (long long j = j0; j < j1; ++j) {
      const uint32_t b = bytes[j >> 1];
      dst[j] = static_cast<char>(decode(alpha, (j & 1) ? b >> 4 : b & 15u));
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_unpack_exceptions(const uint32_t* __restrict__ index,
                                                                const uint8_t* __restrict__ raw,
                                                                size_t n, char* __restrict__ dst) {
  const size_t e = blockIdx.x;
  const size_t off = static_cast<size_t>(index[e]) * kPackBlockBytes + threadIdx.x;
  if (off < n) dst[off] = static_cast<char>(raw[e * kPackBlockBytes + threadIdx.x]);
}
// ------------------------------------------------------------ dense chunks
/*! \brief blocks a workgroup expands: 4 per wave, 4 KiB of text in LDS */
constexpr int kGroupBlocks = 16;
constexpr int kGroupBytes = kGroupBlocks * static_cast<int>(kPackBlockBytes);

/*! \brief payload bytes of block i of a range; a raw block before the text's
 *  last one holds kPackBlockBytes */
__device__ __forceinline__ uint32_t dense_payload(const uint8_t* meta, uint32_t i, uint32_t raw_len) {
  const uint32_t m0 = meta[2 * i], m1 = meta[2 * i + 1];
  return (m0 == kDenseRawMeta && m1 == kDenseRawMeta) ? raw_len : m0 + m1;
}

/*!
 * \brief k_unpack_dense: a workgroup expands kGroupBlocks consecutive blocks of
 *  one range into LDS and stores them as one span.  It sums the payload
 *  lengths of the range's earlier blocks to find its own; each wave then takes
 *  4 blocks, one after the other: a lane holds 4 codes of the block (<= 256:
 *  every code yields a byte), looks up their entries in LDS, and one wave scan
 *  of a packed counter (output bytes in the low half, escapes in the high
 *  half) gives every code its output position and its literal's ordinal.  The
 *  span leaves as 16-byte stores on the destination's grid, funnel shifted out
 *  of LDS words; the groups cut by either end of the span store bytes, so
 *  neighbouring workgroups never write the same byte and nothing is written
 *  past dst + n.
 */
__global__ __launch_bounds__(kThreads) void k_unpack_dense(const uint8_t* __restrict__ packed,
                                                           size_t n, uint32_t range_blocks,
                                                           uint32_t groups_per_range,
                                                           char* __restrict__ dst) {
  __shared__ uint32_t s_out[kGroupBytes / 4 + 4];
  __shared__ uint32_t s_entry[16], s_count[16];
  __shared__ uint32_t s_off[kGroupBlocks];
  __shared__ uint32_t s_base;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t r = blockIdx.x / groups_per_range, g = blockIdx.x % groups_per_range;
  const size_t total_blocks = (n + kPackBlockBytes - 1) / kPackBlockBytes;
  const size_t rb0 = static_cast<size_t>(r) * range_blocks;
  const uint32_t nblocks =
      static_cast<uint32_t>(total_blocks - rb0 < range_blocks ? total_blocks - rb0 : range_blocks);
  const uint32_t gb0 = g * kGroupBlocks;
  if (gb0 >= nblocks) return;
  const uint32_t gblocks = nblocks - gb0 < kGroupBlocks ? nblocks - gb0 : kGroupBlocks;

  const DenseHeader* h = reinterpret_cast<const DenseHeader*>(packed);
  const uint32_t entry_bytes = h->entry_bytes;
  if (tid < 16) {
    // the entries lie back to back behind the header
    uint32_t at = 0, len = 0;
    for (uint32_t c = 0; c <= tid; ++c) {
      at += len;
      len = (h->len[c / 2] >> (4 * (c & 1))) & 15u;
    }
    uint32_t e = 0;
    for (uint32_t j = 0; j < 4; ++j) {
      if (j < len && at + j < entry_bytes) {
        e |= static_cast<uint32_t>(packed[sizeof(DenseHeader) + at + j]) << (8 * j);
      }
    }
    s_entry[tid] = e;
    s_count[tid] = tid == h->escape ? 0x10001u : (len <= 4 ? len : 0u);
  }
  if (tid == 0) s_base = 0;
  const DenseDirEntry dir = reinterpret_cast<const DenseDirEntry*>(
      packed + sizeof(DenseHeader) + ((entry_bytes + 7u) & ~7u))[r];
  const uint8_t* meta = packed + dir.offset;
  const uint8_t* payload = meta + ((2u * nblocks + 15u) & ~15u);
  __syncthreads();
  // where this group's payloads begin
  uint32_t sum = 0;
  for (uint32_t i = tid; i < gb0; i += kThreads) sum += dense_payload(meta, i, kPackBlockBytes);
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
  if (lane == 0 && sum != 0) atomicAdd(&s_base, sum);
  __syncthreads();
  if (tid < gblocks) {
    uint32_t off = s_base;
    for (uint32_t j = 0; j < tid; ++j) off += dense_payload(meta, gb0 + j, kPackBlockBytes);
    s_off[tid] = off;
  }
  __syncthreads();

  uint8_t* out8 = reinterpret_cast<uint8_t*>(s_out);
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t bi = wave * 4 + k;
    if (bi >= gblocks) break;
    const size_t tb = rb0 + gb0 + bi;
    const uint32_t blen = static_cast<uint32_t>(
        n - tb * kPackBlockBytes < kPackBlockBytes ? n - tb * kPackBlockBytes : kPackBlockBytes);
    const uint8_t* p = payload + s_off[bi];
    uint8_t* o = out8 + bi * kPackBlockBytes;
    const uint32_t m0 = meta[2 * (gb0 + bi)], m1 = meta[2 * (gb0 + bi) + 1];
    if (m0 == kDenseRawMeta && m1 == kDenseRawMeta) {
      for (uint32_t j = lane; j < blen; j += 64) o[j] = p[j];
      continue;
    }
    const uint8_t* lit = p + m0;
    const uint32_t b0 = 2 * lane < m0 ? p[2 * lane] : 0u;
    const uint32_t b1 = 2 * lane + 1 < m0 ? p[2 * lane + 1] : 0u;
    const uint32_t code[4] = {b0 & 15u, b0 >> 4, b1 & 15u, b1 >> 4};
    uint32_t cnt[4], total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cnt[q] = s_count[code[q]];
      total += cnt[q];
    }
    uint32_t incl = total;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d);
      if (lane >= static_cast<uint32_t>(d)) incl += t;
    }
    uint32_t pos = (incl - total) & 0xffffu, esc = (incl - total) >> 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t len = cnt[q] & 0xffffu;
      if (cnt[q] >> 16) {
        if (pos < blen && esc < m1) o[pos] = lit[esc];
        ++esc;
      } else {
        const uint32_t e = s_entry[code[q]];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          if (j < len && pos + j < blen) o[pos + j] = static_cast<uint8_t>(e >> (8 * j));
        }
      }
      pos += len;
    }
  }
  __syncthreads();

  // the span [start, start + gbytes) of the text, in 16-byte groups of dst's grid
  const size_t start = (rb0 + gb0) * kPackBlockBytes;
  const uint32_t gbytes = static_cast<uint32_t>(
      n - start < static_cast<size_t>(gblocks) * kPackBlockBytes ? n - start
                                                                 : gblocks * kPackBlockBytes);
  char* span = dst + start;
  const uint32_t lead = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(span) & 15u);
  const uint32_t ngroups = (gbytes + lead + 15u) / 16u;
  for (uint32_t gi = tid; gi < ngroups; gi += kThreads) {
    const int s = static_cast<int>(gi * 16u) - static_cast<int>(lead);
    if (s >= 0 && s + 16 <= static_cast<int>(gbytes)) {
      const uint32_t w = static_cast<uint32_t>(s) >> 2;
      const uint32_t sh = (static_cast<uint32_t>(s) & 3u) * 8u;  // the same for every lane
      uint32_t v[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) v[q] = s_out[w + q];
      if (sh != 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (v[q] >> sh) | (v[q + 1] << (32u - sh));
      }
      *reinterpret_cast<uint4*>(span + s) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
      const int j0 = s < 0 ? 0 : s;
      const int j1 = s + 16 < static_cast<int>(gbytes) ? s + 16 : static_cast<int>(gbytes);
      for (int j = j0; j < j1; ++j) span[j] = static_cast<char>(out8[j]);
    }
  }
}
}  // namespace

void LaunchUnpackDense(const void* packed, size_t n, uint32_t nranges, uint32_t range_blocks,
                       char* dst, hipStream_t stream) {
  if (n == 0 || nranges == 0) return;
  const size_t blocks = PackBlocks(n);
  const size_t per_range = std::min<size_t>(range_blocks, blocks);
  const uint32_t groups = static_cast<uint32_t>((per_range + kGroupBlocks - 1) / kGroupBlocks);
  hipLaunchKernelGGL(k_unpack_dense, dim3(nranges * groups), dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(packed), n, range_blocks, groups, dst);
}

void LaunchUnpackText(const void* packed, size_t n, uint32_t nexc, const uint8_t alphabet[16],
                      char* dst, hipStream_t stream) {
  static_assert(kPackBlockBytes == kThreads, "one lane per byte of an exception block");
  if (n == 0) return;
  const uint8_t* base = static_cast<const uint8_t*>(packed);
  const uint8_t* nib = base + sizeof(PackedHeader);
  const uint8_t* idx = nib + NibbleAreaBytes(n);
  const uint8_t* raw = idx + ((static_cast<size_t>(nexc) * 4 + 15) & ~size_t(15));
  Alphabet4 alpha;
  for (int i = 0; i < 4; ++i) {
    alpha.w[i] = static_cast<uint32_t>(alphabet[4 * i]) | static_cast<uint32_t>(alphabet[4 * i + 1]) << 8 |
                 static_cast<uint32_t>(alphabet[4 * i + 2]) << 16 |
                 static_cast<uint32_t>(alphabet[4 * i + 3]) << 24;
  }
  const unsigned lead = static_cast<unsigned>(reinterpret_cast<uintptr_t>(dst) & 15u);
  const size_t groups = (n + lead + 15) / 16;
  hipLaunchKernelGGL(k_unpack_nibbles, dim3((groups + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, reinterpret_cast<const uint64_t*>(nib), n, alpha, dst, lead);
  if (nexc != 0) {
    hipLaunchKernelGGL(k_unpack_exceptions, dim3(nexc), dim3(kThreads), 0, stream,
                       reinterpret_cast<const uint32_t*>(idx), raw, n, dst);
  }
}

}  // namespace gpu
}  // namespace dmlc
