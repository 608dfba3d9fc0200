/*!
 * \file src/gpu/text_pack.cc
 * \brief Nibble packer of text chunks (see text_pack.h): a scalar path, an
 *  AVX2 path (per-high-nibble pshufb tables) and an AVX-512 BW+VBMI path
 *  (128-entry vpermi2b table), chosen at run time; all write the same bytes.
 *  The nibble area is written with non-temporal stores: it is read next by
 *  the DMA engine, not by this core.
 */
#include "./text_pack.h"

#include <algorithm>
#include <cstring>

#if defined(__x86_64__)
#include <immintrin.h>
#define DMLC_PACK_X86 1
#else
#define DMLC_PACK_X86 0
#endif

namespace dmlc {
namespace gpu {

namespace {

constexpr uint8_t kBad = 0x80;
constexpr size_t kBlockNibbles = kPackBlockBytes / 2;

/*! \brief codes of src[0, len) into out[0, (len+1)/2); false: a byte outside the alphabet */
bool BlockScalar(const uint8_t* src, size_t len, const uint8_t* enc, uint8_t* out) {
  uint8_t bad = 0;
  for (size_t k = 0; k < len / 2; ++k) {
    const uint8_t a = enc[src[2 * k]], b = enc[src[2 * k + 1]];
    bad |= a | b;
    out[k] = static_cast<uint8_t>((a & 15) | (b << 4));
  }
  if (len & 1) {
    const uint8_t a = enc[src[len - 1]];
    bad |= a;
    out[len / 2] = a & 15;
  }
  return !(bad & kBad);
}

#if DMLC_PACK_X86
/*! \brief codes of 32 bytes: per used high nibble, a pshufb over its 16-entry table */
__attribute__((target("avx2"))) inline __m256i LookupAvx2(__m256i x, const __m256i* table,
                                                          const bool* used) {
  const __m256i low4 = _mm256_set1_epi8(0x0f);
  const __m256i lo = _mm256_and_si256(x, low4);
  const __m256i hi = _mm256_and_si256(_mm256_srli_epi16(x, 4), low4);
  __m256i res = _mm256_setzero_si256(), matched = _mm256_setzero_si256();
  for (int h = 0; h < 8; ++h) {
    if (!used[h]) continue;
    const __m256i m = _mm256_cmpeq_epi8(hi, _mm256_set1_epi8(static_cast<char>(h)));
    res = _mm256_or_si256(res, _mm256_and_si256(_mm256_shuffle_epi8(table[h], lo), m));
    matched = _mm256_or_si256(matched, m);
  }
  return _mm256_or_si256(res,
                         _mm256_andnot_si256(matched, _mm256_set1_epi8(static_cast<char>(kBad))));
}

/*! \brief one full block, AVX2: tables of the high nibbles that hold symbols */
__attribute__((target("avx2"))) bool BlockAvx2(const uint8_t* src, const uint8_t* enc,
                                               uint8_t* out, bool aligned) {
  const __m256i low4 = _mm256_set1_epi8(0x0f);
  const __m256i k1001 = _mm256_set1_epi16(0x1001);
  __m256i table[8];
  bool used[8];
  for (int h = 0; h < 8; ++h) {
    const __m128i t = _mm_loadu_si128(reinterpret_cast<const __m128i*>(enc + 16 * h));
    table[h] = _mm256_broadcastsi128_si256(t);
    used[h] = false;
    for (int l = 0; l < 16; ++l) used[h] |= enc[16 * h + l] != kBad;
  }
  __m256i bad = _mm256_setzero_si256();
  __m256i o[4];
  for (int v = 0; v < 4; ++v) {
    const __m256i a = LookupAvx2(
        _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + 64 * v)), table, used);
    const __m256i b = LookupAvx2(
        _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + 64 * v + 32)), table, used);
    bad = _mm256_or_si256(bad, _mm256_or_si256(a, b));
    const __m256i wa = _mm256_maddubs_epi16(_mm256_and_si256(a, low4), k1001);
    const __m256i wb = _mm256_maddubs_epi16(_mm256_and_si256(b, low4), k1001);
    o[v] = _mm256_permute4x64_epi64(_mm256_packus_epi16(wa, wb), 0xD8);
  }
  const bool ok = _mm256_movemask_epi8(bad) == 0;
  if (!ok) {
    for (int v = 0; v < 4; ++v) o[v] = _mm256_setzero_si256();
  }
  for (int v = 0; v < 4; ++v) {
    if (aligned) {
      _mm256_stream_si256(reinterpret_cast<__m256i*>(out + 32 * v), o[v]);
    } else {
      _mm256_storeu_si256(reinterpret_cast<__m256i*>(out + 32 * v), o[v]);
    }
  }
  return ok;
}

/*! \brief one full block, AVX-512 BW + VBMI: one vpermi2b over enc[0, 128) */
__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi,avx2"))) bool BlockAvx512(
    const uint8_t* src, const uint8_t* enc, uint8_t* out, bool aligned) {
  const __m512i tlo = _mm512_loadu_si512(enc);
  const __m512i thi = _mm512_loadu_si512(enc + 64);
  const __m512i low4 = _mm512_set1_epi8(0x0f);
  const __m512i k1001 = _mm512_set1_epi16(0x1001);
  __mmask64 bad = 0;
  __m256i o[4];
  for (int v = 0; v < 4; ++v) {
    const __m512i x = _mm512_loadu_si512(src + 64 * v);
    const __m512i c = _mm512_permutex2var_epi8(tlo, x, thi);
    bad |= _mm512_movepi8_mask(_mm512_or_si512(c, x));  // bit 7: outside, or a byte >= 0x80
    o[v] = _mm512_cvtepi16_epi8(_mm512_maddubs_epi16(_mm512_and_si512(c, low4), k1001));
  }
  const bool ok = bad == 0;
  if (!ok) {
    for (int v = 0; v < 4; ++v) o[v] = _mm256_setzero_si256();
  }
  for (int v = 0; v < 4; ++v) {
    if (aligned) {
      _mm256_stream_si256(reinterpret_cast<__m256i*>(out + 32 * v), o[v]);
    } else {
      _mm256_storeu_si256(reinterpret_cast<__m256i*>(out + 32 * v), o[v]);
    }
  }
  return ok;
}
#endif  // DMLC_PACK_X86

PackIsa Resolve(PackIsa isa) {
  if (isa != PackIsa::kAuto) return isa;
  if (PackIsaSupported(PackIsa::kAvx512)) return PackIsa::kAvx512;
  if (PackIsaSupported(PackIsa::kAvx2)) return PackIsa::kAvx2;
  return PackIsa::kScalar;
}

}  // namespace

PackEncoder::PackEncoder(const uint8_t alphabet[16]) {
  std::memset(enc, kBad, sizeof(enc));
  for (int c = 15; c >= 0; --c) {
    if (alphabet[c] < 0x80) enc[alphabet[c]] = static_cast<uint8_t>(c);
  }
}

bool PackIsaSupported(PackIsa isa) {
  switch (isa) {
    case PackIsa::kAuto:
    case PackIsa::kScalar:
      return true;
#if DMLC_PACK_X86
    case PackIsa::kAvx2:
      return __builtin_cpu_supports("avx2");
    case PackIsa::kAvx512:
      return __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw") &&
             __builtin_cpu_supports("avx512vl") && __builtin_cpu_supports("avx512vbmi") &&
             __builtin_cpu_supports("avx2");
#endif
    default:
      return false;
  }
}

void PackAlphabet(bool csv, char delimiter, uint8_t alphabet[16]) {
  static const char kSymbols[17] = "0123456789:. \n-e";
  std::memcpy(alphabet, kSymbols, 16);
  if (csv) alphabet[10] = static_cast<uint8_t>(delimiter);
}

long PackMaxExceptions(size_t n, double ratio) {
  const size_t blocks = PackBlocks(n);
  if (ratio < 0) return static_cast<long>(blocks);
  const double limit_f = ratio * static_cast<double>(n);
  if (limit_f >= static_cast<double>(PackedBytes(n, blocks))) return static_cast<long>(blocks);
  const size_t limit = static_cast<size_t>(limit_f);
  if (PackedBytes(n, 0) > limit) return -1;
  size_t e = std::min(blocks, (limit - PackedBytes(n, 0)) / (kPackBlockBytes + 4));
  while (e > 0 && PackedBytes(n, e) > limit) --e;
  return static_cast<long>(e);
}

bool PackRange(const uint8_t* text, size_t n, size_t block_begin, size_t block_end,
               const PackEncoder& table, uint8_t* nibbles, std::vector<uint32_t>* exc,
               std::atomic<long>* exc_total, long exc_limit, PackIsa isa) {
  const PackIsa use = Resolve(isa);
  (void)use;
  long own = 0;
  bool fits = true;
  for (size_t b = block_begin; b < block_end && fits; ++b) {
    const uint8_t* src = text + b * kPackBlockBytes;
    uint8_t* out = nibbles + b * kBlockNibbles;
    const size_t len = std::min(kPackBlockBytes, n - b * kPackBlockBytes);
    bool ok = false, simd = false;
#if DMLC_PACK_X86
    const bool aligned = (reinterpret_cast<uintptr_t>(out) & 31) == 0;
    if (len == kPackBlockBytes && use == PackIsa::kAvx512) {
      ok = BlockAvx512(src, table.enc, out, aligned);
      simd = true;
    } else if (len == kPackBlockBytes && use == PackIsa::kAvx2) {
      ok = BlockAvx2(src, table.enc, out, aligned);
      simd = true;
    }
#endif
    if (!simd) {
      ok = BlockScalar(src, len, table.enc, out);
      if (!ok) std::memset(out, 0, (len + 1) / 2);
    }
    if (!ok) {
      exc->push_back(static_cast<uint32_t>(b));
      const long total = exc_total != nullptr ? exc_total->fetch_add(1) + 1 : ++own;
      if (total > exc_limit) fits = false;
    }
  }
#if DMLC_PACK_X86
  _mm_sfence();  // the streamed nibbles are visible before the range is reported done
#endif
  return fits;
}

bool PackRange(const uint8_t* text, size_t n, size_t block_begin, size_t block_end,
               const uint8_t alphabet[16], uint8_t* nibbles, std::vector<uint32_t>* exc,
               std::atomic<long>* exc_total, long exc_limit, PackIsa isa) {
  return PackRange(text, n, block_begin, block_end, PackEncoder(alphabet), nibbles, exc, exc_total,
                   exc_limit, isa);
}

size_t PackFinishHeader(size_t n, const uint8_t alphabet[16], const std::vector<uint32_t>& exc,
                        uint8_t* packed) {
  PackedHeader h;
  h.n = n;
  h.nexc = static_cast<uint32_t>(exc.size());
  h.reserved = 0;
  std::memcpy(h.alphabet, alphabet, 16);
  std::memcpy(packed, &h, sizeof(h));
  uint8_t* nib = packed + sizeof(PackedHeader);
  const size_t area = NibbleAreaBytes(n);
  std::memset(nib + (n + 1) / 2, 0, area - (n + 1) / 2);
  uint8_t* idx = nib + area;
  const size_t idx_bytes = (exc.size() * 4 + 15) & ~size_t(15);
  std::memset(idx, 0, idx_bytes);
  if (!exc.empty()) std::memcpy(idx, exc.data(), exc.size() * 4);
  return PackedBytes(n, exc.size());
}

void PackCopyExceptions(const uint8_t* text, size_t n, const std::vector<uint32_t>& exc,
                        size_t first, size_t last, uint8_t* packed) {
  uint8_t* raw = packed + sizeof(PackedHeader) + NibbleAreaBytes(n) +
                 ((exc.size() * 4 + 15) & ~size_t(15));
  for (size_t i = first; i < last; ++i) {
    const size_t off = static_cast<size_t>(exc[i]) * kPackBlockBytes;
    const size_t len = std::min(kPackBlockBytes, n - off);
    std::memcpy(raw + i * kPackBlockBytes, text + off, len);
    std::memset(raw + i * kPackBlockBytes + len, 0, kPackBlockBytes - len);
  }
}

size_t PackFinish(const uint8_t* text, size_t n, const uint8_t alphabet[16],
                  const std::vector<uint32_t>& exc, uint8_t* packed) {
  const size_t size = PackFinishHeader(n, alphabet, exc, packed);
  PackCopyExceptions(text, n, exc, 0, exc.size(), packed);
  return size;
}

bool PackText(const uint8_t* text, size_t n, const uint8_t alphabet[16], double ratio,
              std::vector<uint8_t>* packed, PackIsa isa) {
  const long limit = PackMaxExceptions(n, ratio);
  if (limit < 0) return false;
  // the nibble area sits 32 bytes into a 64-byte aligned buffer, as in a
  // pinned pack slot (aligned streaming stores)
  packed->assign(PackedBytes(n, static_cast<size_t>(limit)) + 64, 0);
  uint8_t* base = packed->data();
  const size_t shift = (64 - (reinterpret_cast<uintptr_t>(base) & 63)) & 63;
  std::vector<uint32_t> exc;
  if (!PackRange(text, n, 0, PackBlocks(n), alphabet, base + shift + sizeof(PackedHeader), &exc,
                 nullptr, limit, isa)) {
    return false;
  }
  const size_t size = PackFinish(text, n, alphabet, exc, base + shift);
  if (shift != 0) std::memmove(base, base + shift, size);
  packed->resize(size);
  return true;
}

PackedView ViewPacked(const uint8_t* packed) {
  PackedView v;
  std::memcpy(&v.header, packed, sizeof(PackedHeader));
  v.nibbles = packed + sizeof(PackedHeader);
  const uint8_t* idx = v.nibbles + NibbleAreaBytes(v.header.n);
  v.exc_index = reinterpret_cast<const uint32_t*>(idx);
  v.exc_bytes = idx + ((static_cast<size_t>(v.header.nexc) * 4 + 15) & ~size_t(15));
  v.bytes = PackedBytes(v.header.n, v.header.nexc);
  return v;
}

void UnpackReference(const uint8_t* packed, uint8_t* dst) {
  const PackedView v = ViewPacked(packed);
  const size_t n = v.header.n;
  for (size_t j = 0; j < n; ++j) {
    const uint8_t byte = v.nibbles[j / 2];
    dst[j] = v.header.alphabet[(j & 1) ? byte >> 4 : byte & 15];
  }
  for (size_t i = 0; i < v.header.nexc; ++i) {
    uint32_t b;
    std::memcpy(&b, reinterpret_cast<const uint8_t*>(v.exc_index) + 4 * i, 4);
    const size_t off = static_cast<size_t>(b) * kPackBlockBytes;
    std::memcpy(dst + off, v.exc_bytes + i * kPackBlockBytes, std::min(kPackBlockBytes, n - off));
  }
}

}  // namespace gpu
}  // namespace dmlc
