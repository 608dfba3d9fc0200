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
 */
#include <hip/hip_runtime.h>

#include "./kernels.h"
#include "./text_pack.h"

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
}  // namespace

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
