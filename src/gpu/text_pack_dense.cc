/*!
 * \file src/gpu/text_pack_dense.cc
 * \brief Dense packer of text chunks (see text_pack_dense.h): the table
 *  selector, a scalar encoder and an AVX-512 BW + VBMI + VBMI2 encoder chosen
 *  at run time (both write the same bytes), and the CPU reference decoder.
 *
 * The AVX-512 encoder works on the four 64-byte vectors of a block.  The
 * single-byte codes of a vector come from one vpermi2b, as in the nibble
 * packer; every multi-byte entry adds one compare per entry byte against the
 * vector loaded at that byte's shift.  The no-overlap rule makes the match
 * masks disjoint, so the bytes a match covers after its first are simply
 * dropped by one vpcompressb (into a register: its memory form is slow on
 * Zen), and the codes of a block, one per byte, are joined to nibbles at the
 * end.  Escaped bytes are compressed out of the text the same way, only in
 * vectors that hold one.
 */
#include "./text_pack_dense.h"

#include <dmlc/logging.h>

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

inline bool Blank(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

/*! \brief one block, scalar: payload at out, returns its length (raw: len) */
size_t BlockScalarDense(const uint8_t* src, size_t len, const DenseEncoder& e, uint8_t* out,
                        uint8_t* meta, size_t* escapes, size_t* raw_blocks) {
  uint8_t codes[kPackBlockBytes + 1];
  uint8_t lits[kPackBlockBytes];
  size_t cnt = 0, nlit = 0;
  for (size_t i = 0; i < len;) {
    int hit = -1;
    for (int m = 0; m < e.nmulti && hit < 0; ++m) {
      if (i + e.mlen[m] <= len && std::memcmp(src + i, e.mbytes[m], e.mlen[m]) == 0) hit = m;
    }
    if (hit >= 0) {
      codes[cnt++] = e.mcode[hit];
      i += e.mlen[hit];
      continue;
    }
    const uint8_t c = e.enc[src[i]];
    if (c & kBad) {
      codes[cnt++] = e.table.escape;
      lits[nlit++] = src[i];
    } else {
      codes[cnt++] = c;
    }
    ++i;
  }
  codes[cnt] = 0;
  const size_t nb = (cnt + 1) / 2;
  if (nb + nlit > kDenseMaxPayload) {
    std::memcpy(out, src, len);
    meta[0] = meta[1] = kDenseRawMeta;
    if (raw_blocks != nullptr) ++*raw_blocks;
    return len;
  }
  for (size_t k = 0; k < nb; ++k) {
    out[k] = static_cast<uint8_t>(codes[2 * k] | (codes[2 * k + 1] << 4));
  }
  std::memcpy(out + nb, lits, nlit);
  meta[0] = static_cast<uint8_t>(nb);
  meta[1] = static_cast<uint8_t>(nlit);
  if (escapes != nullptr) *escapes += nlit;
  return nb + nlit;
}

#if DMLC_PACK_X86
#define DMLC_DENSE_TARGET \
  __attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi,avx512vbmi2,avx2,popcnt")))

/*! \brief the codes (one per byte) and the escaped bytes of a block, and where
 *  its payload goes */
struct DenseBlock {
  alignas(64) uint8_t codes[kPackBlockBytes + 64];
  alignas(64) uint8_t lits[kPackBlockBytes + 64];
  const uint8_t* src;
  uint8_t* out;
  size_t cnt, nlit;
  bool raw;
};

/*! \brief second half of a block: join the codes to nibbles and append the
 *  literals, or copy a raw block.  It runs one block late, when the codes have
 *  left the store buffer (a load over several pending stores stalls), and in
 *  block order: its whole-vector stores run up to 63 bytes past the payload,
 *  into the place of the next block's, which is written after it */
DMLC_DENSE_TARGET inline void BlockPayloadAvx512(const DenseBlock* blk) {
  uint8_t* out = blk->out;
  if (blk->raw) {
    for (int v = 0; v < 4; ++v) {
      _mm512_storeu_si512(out + 64 * v, _mm512_loadu_si512(blk->src + 64 * v));
    }
    return;
  }
  const __m512i k1001 = _mm512_set1_epi16(0x1001);
  const size_t cnt = blk->cnt, nlit = blk->nlit;
  for (size_t k = 0; k < cnt; k += 64) {
    const __m512i a = _mm512_load_si512(blk->codes + k);
    _mm256_storeu_si256(reinterpret_cast<__m256i*>(out + k / 2),
                        _mm512_cvtepi16_epi8(_mm512_maddubs_epi16(a, k1001)));
  }
  if (nlit != 0) {
    uint8_t* lit = out + (cnt + 1) / 2;
    if (nlit <= 64) {
      _mm512_storeu_si512(lit, _mm512_load_si512(blk->lits));
    } else {
      std::memcpy(lit, blk->lits, nlit);
    }
  }
}

/*!
 * \brief the blocks of a range, AVX-512, for a table of NM multi-byte entries
 *  (the loops over them unroll and the table stays in registers: the byte
 *  stores below may alias anything that lives in memory).  A full block whose
 *  3 following bytes are readable is coded here, the text's last one by the
 *  scalar encoder.
 */
template <int NM>
DMLC_DENSE_TARGET void RangeAvx512Dense(const uint8_t* text, size_t n, size_t block_begin,
                                        size_t block_end, const DenseEncoder& e, uint8_t* meta,
                                        uint8_t* payload, size_t* pos, size_t* escapes,
                                        size_t* raw_blocks) {
  constexpr int kM = NM > 0 ? NM : 1;
  const __m512i tlo = _mm512_loadu_si512(e.enc);
  const __m512i thi = _mm512_loadu_si512(e.enc + 64);
  const __m512i vesc = _mm512_set1_epi8(static_cast<char>(e.table.escape));
  __m512i mcode[kM], mb[kM][4];
  int mlen[kM];
  int maxlen = 1;
  for (int m = 0; m < NM; ++m) {
    mcode[m] = _mm512_set1_epi8(static_cast<char>(e.mcode[m]));
    mlen[m] = e.mlen[m];
    maxlen = std::max(maxlen, mlen[m]);
    for (int k = 0; k < 4; ++k) mb[m][k] = _mm512_set1_epi8(static_cast<char>(e.mbytes[m][k]));
  }
  DenseBlock blocks[2];
  DenseBlock* blk = &blocks[0];
  DenseBlock* prev = nullptr;  // coded, its payload not yet written
  size_t at = *pos, nesc = 0, nraw = 0;
  for (size_t b = block_begin; b < block_end; ++b) {
    const size_t off = b * kPackBlockBytes;
    uint8_t* mt = meta + 2 * (b - block_begin);
    if (off + kPackBlockBytes + 3 > n) {
      if (prev != nullptr) BlockPayloadAvx512(prev);
      prev = nullptr;
      at += BlockScalarDense(text + off, std::min(kPackBlockBytes, n - off), e, payload + at, mt,
                             &nesc, &nraw);
      continue;
    }
    const uint8_t* src = text + off;
    uint8_t* codes = blk->codes;
    uint8_t* lits = blk->lits;
    size_t cnt = 0, nlit = 0;
    uint64_t carry = 0;  // bytes at the next vector's start that a match covers
#pragma GCC unroll 4
    for (int v = 0; v < 4; ++v) {
      const uint8_t* p = src + 64 * v;
      const __m512i x0 = _mm512_loadu_si512(p);
      __m512i code = _mm512_permutex2var_epi8(tlo, x0, thi);
      // bit 7: outside the table, or a byte >= 0x80
      uint64_t esc = _mm512_movepi8_mask(_mm512_or_si512(code, x0));
      uint64_t cover = carry, start = 0;
      carry = 0;
      if (NM != 0) {
        const __m512i x1 = _mm512_loadu_si512(p + 1);
        const __m512i x2 = maxlen > 2 ? _mm512_loadu_si512(p + 2) : x1;
        const __m512i x3 = maxlen > 3 ? _mm512_loadu_si512(p + 3) : x1;
#pragma GCC unroll 4
        for (int m = 0; m < NM; ++m) {
          const int len = mlen[m];
          __mmask64 k = _mm512_cmpeq_epi8_mask(x0, mb[m][0]);
          k = _mm512_mask_cmpeq_epi8_mask(k, x1, mb[m][1]);
          if (len > 2) k = _mm512_mask_cmpeq_epi8_mask(k, x2, mb[m][2]);
          if (len > 3) k = _mm512_mask_cmpeq_epi8_mask(k, x3, mb[m][3]);
          uint64_t mk = k;
          // a match never extends past the block's end
          if (v == 3) mk &= ~uint64_t(0) >> (len - 1);
          // (no branch on mk: whether a vector holds a rare entry is a coin toss)
          code = _mm512_mask_mov_epi8(code, mk, mcode[m]);
          start |= mk;
          cover |= mk << 1;
          carry |= mk >> 63;
          if (len > 2) {
            cover |= mk << 2;
            carry |= mk >> 62;
          }
          if (len > 3) {
            cover |= mk << 3;
            carry |= mk >> 61;
          }
        }
      }
      const uint64_t keep = ~cover;
      esc &= keep & ~start;
      code = _mm512_mask_mov_epi8(code, esc, vesc);
      _mm512_storeu_si512(codes + cnt, _mm512_maskz_compress_epi8(keep, code));
      cnt += static_cast<size_t>(_mm_popcnt_u64(keep));
      if (esc != 0) {
        _mm512_storeu_si512(lits + nlit, _mm512_maskz_compress_epi8(esc, x0));
        nlit += static_cast<size_t>(_mm_popcnt_u64(esc));
      }
    }
    codes[cnt] = 0;  // the pad nibble of an odd count
    const size_t nb = (cnt + 1) / 2;
    const bool raw = nb + nlit > kDenseMaxPayload;
    blk->src = src;
    blk->out = payload + at;
    blk->cnt = cnt;
    blk->nlit = nlit;
    blk->raw = raw;
    if (raw) {
      mt[0] = mt[1] = kDenseRawMeta;
      ++nraw;
      at += kPackBlockBytes;
    } else {
      mt[0] = static_cast<uint8_t>(nb);
      mt[1] = static_cast<uint8_t>(nlit);
      nesc += nlit;
      at += nb + nlit;
    }
    if (prev != nullptr) BlockPayloadAvx512(prev);
    prev = blk;
    blk = blk == &blocks[0] ? &blocks[1] : &blocks[0];
  }
  if (prev != nullptr) BlockPayloadAvx512(prev);
  *pos = at;
  if (escapes != nullptr) *escapes += nesc;
  if (raw_blocks != nullptr) *raw_blocks += nraw;
}

/*! \brief 16-byte streaming stores up to dst's next 64-byte boundary and for
 *  the tail, 64-byte ones in between */
DMLC_DENSE_TARGET void CopyOutAvx512(const uint8_t* src, size_t bytes, uint8_t* dst) {
  size_t k = 0;
  for (; k < bytes && ((reinterpret_cast<uintptr_t>(dst + k) & 63) != 0); k += 16) {
    _mm_stream_si128(reinterpret_cast<__m128i*>(dst + k),
                     _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + k)));
  }
  for (; k + 64 <= bytes; k += 64) {
    _mm512_stream_si512(reinterpret_cast<__m512i*>(dst + k), _mm512_loadu_si512(src + k));
  }
  for (; k < bytes; k += 16) {
    _mm_stream_si128(reinterpret_cast<__m128i*>(dst + k),
                     _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + k)));
  }
}
#endif  // DMLC_PACK_X86

struct Candidate {
  uint64_t score;
  int len;
  uint8_t bytes[4];
};

bool CandidateBefore(const Candidate& a, const Candidate& b) {
  if (a.score != b.score) return a.score > b.score;
  if (a.len != b.len) return a.len < b.len;
  return std::memcmp(a.bytes, b.bytes, 4) < 0;
}

}  // namespace

bool DenseCompatible(const uint8_t* a, int alen, const uint8_t* b, int blen) {
  const bool same = alen == blen && std::memcmp(a, b, alen) == 0;
  // b laid at shift s over a, and a at shift s over b
  for (int pass = 0; pass < 2; ++pass) {
    const uint8_t* x = pass == 0 ? a : b;
    const uint8_t* y = pass == 0 ? b : a;
    const int xl = pass == 0 ? alen : blen, yl = pass == 0 ? blen : alen;
    for (int s = (same || pass == 1) ? 1 : 0; s < xl; ++s) {
      const int shared = std::min(xl - s, yl);
      if (std::memcmp(x + s, y, shared) == 0) return false;
    }
  }
  return true;
}

bool DenseTableValid(const DenseTable& t) {
  if (t.escape > 15 || t.len[t.escape] != 0) return false;
  bool single[256] = {false};
  for (int c = 0; c < 16; ++c) {
    if (t.len[c] > 4) return false;
    if (t.len[c] == 1) {
      if (single[t.bytes[c][0]]) return false;
      single[t.bytes[c][0]] = true;
    }
    if (t.len[c] < 2) continue;
    for (int d = 0; d <= c; ++d) {
      if (t.len[d] >= 2 && !DenseCompatible(t.bytes[c], t.len[c], t.bytes[d], t.len[d])) {
        return false;
      }
    }
  }
  return true;
}

bool DenseMakeTable(const std::vector<std::vector<uint8_t>>& entries, DenseTable* out) {
  if (entries.size() > 15) return false;
  std::memset(out, 0, sizeof(*out));
  for (size_t c = 0; c < entries.size(); ++c) {
    if (entries[c].empty() || entries[c].size() > 4) return false;
    out->len[c] = static_cast<uint8_t>(entries[c].size());
    std::memcpy(out->bytes[c], entries[c].data(), entries[c].size());
  }
  out->escape = static_cast<uint8_t>(entries.size());
  return DenseTableValid(*out);
}

DenseTable DenseDefaultTable(bool csv, char delimiter) {
  uint8_t alphabet[16];
  PackAlphabet(csv, delimiter, alphabet);
  DenseTable t;
  std::memset(&t, 0, sizeof(t));
  for (int c = 0; c < 15; ++c) {
    t.bytes[c][0] = alphabet[c];
    t.len[c] = 1;
  }
  t.escape = 15;
  return t;
}

DenseTable DenseSelectTable(const uint8_t* text, size_t n, bool csv, char delimiter) {
  uint8_t alphabet[16];
  PackAlphabet(csv, delimiter, alphabet);
  bool format[256] = {false};
  for (int c = 0; c < 16; ++c) format[alphabet[c]] = true;

  // the sample's windows
  struct Window {
    size_t begin, end;
  };
  std::vector<Window> windows;
  for (size_t at = 0; at < n; at += kDenseSampleStride) {
    windows.push_back(Window{at, std::min(n, at + kDenseSampleBytes)});
  }
  uint32_t count[256] = {0};
  size_t sampled = 0;
  for (const Window& w : windows) {
    for (size_t i = w.begin; i < w.end; ++i) ++count[text[i]];
    sampled += w.end - w.begin;
  }
  // classes 1-15: the most frequent bytes that can be part of an n-gram
  int order[256];
  for (int b = 0; b < 256; ++b) order[b] = b;
  std::stable_sort(order, order + 256, [&](int a, int b) { return count[a] > count[b]; });
  uint8_t cls[256] = {0}, cls_byte[16] = {0};
  int ncls = 0;
  for (int k = 0; k < 256 && ncls < 15; ++k) {
    const int b = order[k];
    if (count[b] == 0) break;
    if (Blank(static_cast<uint8_t>(b))) continue;
    cls[b] = static_cast<uint8_t>(++ncls);
    cls_byte[ncls] = static_cast<uint8_t>(b);
  }
  uint32_t c2[256] = {0};
  std::vector<uint32_t> c3(4096, 0);
  for (const Window& w : windows) {
    unsigned h = 0, run = 0;
    for (size_t i = w.begin; i < w.end; ++i) {
      const unsigned c = cls[text[i]];
      h = ((h << 4) | c) & 0xfffu;
      run = c != 0 ? run + 1 : 0;
      c2[h & 0xffu] += run >= 2;
      c3[h] += run >= 3;
    }
  }
  // n-grams worth an entry, best first
  std::vector<Candidate> cand;
  auto add = [&](unsigned h, int len, uint32_t cnt) {
    const uint64_t score = static_cast<uint64_t>(len - 1) * cnt;
    if (cnt == 0 || score * 256 < sampled) return;
    Candidate c;
    c.score = score;
    c.len = len;
    std::memset(c.bytes, 0, 4);
    for (int k = 0; k < len; ++k) c.bytes[k] = cls_byte[(h >> (4 * (len - 1 - k))) & 15u];
    cand.push_back(c);
  };
  for (unsigned h = 0; h < 256; ++h) add(h, 2, c2[h]);
  for (unsigned h = 0; h < 4096; ++h) add(h, 3, c3[h]);
  std::sort(cand.begin(), cand.end(), CandidateBefore);
  // taken greedily: an n-gram has to save more than the escapes of the single
  // byte it pushes out of the table cost, and 1/256 of the sample on top
  // (left[b]: occurrences of byte b that no chosen n-gram covers)
  std::vector<int64_t> left(count, count + 256);
  auto loss = [](const std::vector<int64_t>& a, size_t slots) {
    std::vector<int64_t> v(a);
    std::sort(v.begin(), v.end(), [](int64_t x, int64_t y) { return x > y; });
    int64_t sum = 0;
    for (size_t k = slots; k < v.size(); ++k) sum += 2 * v[k];
    return sum;
  };
  std::vector<Candidate> multi;
  int64_t cur_loss = loss(left, 15);
  const size_t tries = std::min<size_t>(cand.size(), 64);
  for (size_t i = 0; i < tries && static_cast<int>(multi.size()) < kDenseMaxMulti; ++i) {
    const Candidate& c = cand[i];
    bool ok = DenseCompatible(c.bytes, c.len, c.bytes, c.len);
    for (size_t k = 0; k < multi.size() && ok; ++k) {
      ok = DenseCompatible(c.bytes, c.len, multi[k].bytes, multi[k].len);
    }
    if (!ok) continue;
    std::vector<int64_t> after(left);
    const int64_t cnt = static_cast<int64_t>(c.score) / (c.len - 1);
    for (int k = 0; k < c.len; ++k) after[c.bytes[k]] = std::max<int64_t>(0, after[c.bytes[k]] - cnt);
    const int64_t new_loss = loss(after, 15 - multi.size() - 1);
    if (static_cast<int64_t>(c.score) <= new_loss - cur_loss + static_cast<int64_t>(sampled / 256)) {
      continue;
    }
    multi.push_back(c);
    left.swap(after);
    cur_loss = new_loss;
  }
  // single bytes for the other codes: by what is left of them, then by count,
  // the format's symbols first among equals (they fill the table where the
  // sample holds fewer bytes)
  std::stable_sort(order, order + 256, [&](int a, int b) {
    if (left[a] != left[b]) return left[a] > left[b];
    if (count[a] != count[b]) return count[a] > count[b];
    return format[a] && !format[b];
  });
  const size_t nsingle = 15 - multi.size();
  std::vector<uint8_t> singles;
  for (int k = 0; k < 256 && singles.size() < nsingle; ++k) {
    if (count[order[k]] == 0 && !format[order[k]]) break;
    singles.push_back(static_cast<uint8_t>(order[k]));
  }
  std::sort(singles.begin(), singles.end());
  DenseTable t;
  std::memset(&t, 0, sizeof(t));
  int code = 0;
  for (uint8_t b : singles) {
    t.bytes[code][0] = b;
    t.len[code++] = 1;
  }
  for (const Candidate& c : multi) {
    std::memcpy(t.bytes[code], c.bytes, 4);
    t.len[code++] = static_cast<uint8_t>(c.len);
  }
  t.escape = static_cast<uint8_t>(code);
  return t;
}

DenseEncoder::DenseEncoder(const DenseTable& t) : table(t), nmulti(0) {
  CHECK(DenseTableValid(t)) << "dense pack: the table breaks the no-overlap rule";
  std::memset(enc, kBad, sizeof(enc));
  for (int c = 0; c < 16; ++c) {
    if (t.len[c] == 1 && t.bytes[c][0] < 0x80) enc[t.bytes[c][0]] = static_cast<uint8_t>(c);
    if (t.len[c] >= 2) {
      mcode[nmulti] = static_cast<uint8_t>(c);
      mlen[nmulti] = t.len[c];
      std::memcpy(mbytes[nmulti], t.bytes[c], 4);
      ++nmulti;
    }
  }
}

bool PackIsaSupportedDense(PackIsa isa) {
#if DMLC_PACK_X86
  if (isa == PackIsa::kAvx512) {
    return PackIsaSupported(isa) && __builtin_cpu_supports("avx512vbmi2") &&
           __builtin_cpu_supports("popcnt");
  }
#endif
  return PackIsaSupported(isa);
}

size_t PackRangeDense(const uint8_t* text, size_t n, size_t block_begin, size_t block_end,
                      const DenseEncoder& e, uint8_t* out, size_t* escapes, size_t* raw_blocks,
                      PackIsa isa) {
  const size_t nblocks = block_end - block_begin;
  const size_t meta_bytes = DenseMetaBytes(nblocks);
  std::memset(out + 2 * nblocks, 0, meta_bytes - 2 * nblocks);
  uint8_t* payload = out + meta_bytes;
  size_t pos = 0;
  bool simd = false;
#if DMLC_PACK_X86
  // (more multi-byte entries than the SIMD encoder holds in registers: scalar)
  static const bool have512 = PackIsaSupportedDense(PackIsa::kAvx512);
  if ((isa == PackIsa::kAvx512 || (isa == PackIsa::kAuto && have512)) &&
      e.nmulti <= kDenseMaxMulti) {
    switch (e.nmulti) {
#define DMLC_DENSE_CASE(NM)                                                                \
  case NM:                                                                                 \
    RangeAvx512Dense<NM>(text, n, block_begin, block_end, e, out, payload, &pos, escapes, \
                         raw_blocks);                                                      \
    break;
      DMLC_DENSE_CASE(0)
      DMLC_DENSE_CASE(1)
      default:
        static_assert(kDenseMaxMulti == 2, "a case per count of multi-byte entries");
        DMLC_DENSE_CASE(2)
#undef DMLC_DENSE_CASE
    }
    simd = true;
  }
#endif
  if (!simd) {
    for (size_t b = block_begin; b < block_end; ++b) {
      const size_t off = b * kPackBlockBytes;
      pos += BlockScalarDense(text + off, std::min(kPackBlockBytes, n - off), e, payload + pos,
                              out + 2 * (b - block_begin), escapes, raw_blocks);
    }
  }
  const size_t used = meta_bytes + pos;
  const size_t length = DenseAlign(used, kDenseRangeAlign);
  std::memset(out + used, 0, length - used);
  return length;
}

void DenseWriteHeader(size_t n, size_t range_blocks, const DenseTable& table,
                      const std::vector<DenseDirEntry>& dir, uint8_t* packed) {
  DenseHeader h;
  std::memset(&h, 0, sizeof(h));
  h.n = n;
  h.nranges = static_cast<uint32_t>(dir.size());
  h.magic = kDenseMagic;
  h.range_blocks = static_cast<uint32_t>(range_blocks);
  h.escape = table.escape;
  const size_t entry_bytes = DenseEntryBytes(table);
  h.entry_bytes = static_cast<uint8_t>(entry_bytes);
  const size_t total = DenseHeaderBytes(dir.size(), entry_bytes);
  std::memset(packed + sizeof(h), 0, total - sizeof(h));
  uint8_t* at = packed + sizeof(h);
  for (int c = 0; c < 16; ++c) {
    h.len[c / 2] |= static_cast<uint8_t>(table.len[c] << (4 * (c & 1)));
    std::memcpy(at, table.bytes[c], table.len[c]);
    at += table.len[c];
  }
  std::memcpy(packed, &h, sizeof(h));
  if (!dir.empty()) {
    std::memcpy(packed + DenseDirOffset(entry_bytes), dir.data(),
                dir.size() * sizeof(DenseDirEntry));
  }
}

void DenseCopyOut(const uint8_t* src, size_t bytes, uint8_t* dst) {
#if DMLC_PACK_X86
  static const bool have512 = __builtin_cpu_supports("avx512f");
  if (have512 && bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    CopyOutAvx512(src, bytes, dst);
    _mm_sfence();  // the streamed bytes are visible before the range is reported done
    return;
  }
#endif
  std::memcpy(dst, src, bytes);
}

bool PackTextDense(const uint8_t* text, size_t n, const DenseTable& table, size_t range_blocks,
                   double ratio, std::vector<uint8_t>* packed, PackIsa isa, size_t* escapes,
                   size_t* raw_blocks) {
  CHECK_GE(range_blocks, 1u);
  const DenseEncoder encoder(table);
  const size_t nranges = DenseRanges(n, range_blocks);
  const size_t limit = ratio < 0 ? DenseMaxBytes(n, range_blocks)
                                 : static_cast<size_t>(ratio * static_cast<double>(n));
  std::vector<uint8_t> range(DenseRangeCapacity(range_blocks));
  std::vector<DenseDirEntry> dir(nranges);
  packed->assign(DenseHeaderBytes(nranges, DenseEntryBytes(table)), 0);
  for (size_t r = 0; r < nranges; ++r) {
    const size_t b0 = r * range_blocks, b1 = std::min(PackBlocks(n), b0 + range_blocks);
    const size_t len =
        PackRangeDense(text, n, b0, b1, encoder, range.data(), escapes, raw_blocks, isa);
    dir[r].offset = static_cast<uint32_t>(packed->size());
    dir[r].length = static_cast<uint32_t>(len);
    packed->insert(packed->end(), range.begin(), range.begin() + len);
    if (packed->size() > limit) return false;
  }
  if (packed->size() > limit) return false;
  DenseWriteHeader(n, range_blocks, table, dir, packed->data());
  return true;
}

bool IsDenseChunk(const uint8_t* packed, size_t bytes) {
  if (bytes < sizeof(DenseHeader)) return false;
  DenseHeader h;
  std::memcpy(&h, packed, sizeof(h));
  return h.magic == kDenseMagic;
}

namespace {
/*! \brief header, table and directory of a chunk */
struct DenseView {
  DenseHeader h;
  DenseTable table;
  const uint8_t* dir;
};

DenseView ViewDense(const uint8_t* packed) {
  DenseView v;
  std::memcpy(&v.h, packed, sizeof(v.h));
  std::memset(&v.table, 0, sizeof(v.table));
  v.table.escape = v.h.escape;
  const uint8_t* at = packed + sizeof(DenseHeader);
  size_t left = v.h.entry_bytes;
  for (int c = 0; c < 16; ++c) {
    // (a length that is out of bounds is kept for DenseTableValid to refuse)
    const uint8_t len = (v.h.len[c / 2] >> (4 * (c & 1))) & 15u;
    v.table.len[c] = len;
    if (len <= 4 && len <= left) {
      std::memcpy(v.table.bytes[c], at, len);
      at += len;
      left -= len;
    } else {
      v.table.len[c] = 15;
    }
  }
  v.dir = packed + DenseDirOffset(v.h.entry_bytes);
  return v;
}

inline DenseDirEntry DirEntry(const DenseView& v, size_t r) {
  DenseDirEntry e;
  std::memcpy(&e, v.dir + r * sizeof(e), sizeof(e));
  return e;
}
}  // namespace

size_t DenseCheck(const uint8_t* packed, size_t bytes) {
  CHECK_GE(bytes, sizeof(DenseHeader)) << "not a dense chunk";
  const DenseView v = ViewDense(packed);
  CHECK_EQ(v.h.magic, kDenseMagic) << "not a dense chunk";
  CHECK_LT(v.h.escape, 16u) << "dense chunk: escape code";
  CHECK_LE(DenseDirOffset(v.h.entry_bytes), bytes) << "dense chunk: entries";
  CHECK(DenseTableValid(v.table) && DenseEntryBytes(v.table) == v.h.entry_bytes)
      << "dense chunk: table";
  const size_t header_bytes = DenseHeaderBytes(v.h.nranges, v.h.entry_bytes);
  const size_t n = v.h.n;
  if (n == 0) {
    CHECK_EQ(v.h.nranges, 0u);
    return 0;
  }
  CHECK_GE(v.h.range_blocks, 1u) << "dense chunk: range_blocks";
  CHECK_EQ(DenseRanges(n, v.h.range_blocks), v.h.nranges) << "dense chunk: range count";
  CHECK_LE(header_bytes, bytes) << "dense chunk: directory";
  for (size_t r = 0; r < v.h.nranges; ++r) {
    const DenseDirEntry e = DirEntry(v, r);
    CHECK(e.offset >= header_bytes &&
          static_cast<size_t>(e.offset) + e.length <= bytes)
        << "dense chunk: range " << r << " outside the chunk";
    const size_t b0 = r * v.h.range_blocks;
    const size_t nblocks = std::min<size_t>(v.h.range_blocks, PackBlocks(n) - b0);
    size_t used = DenseMetaBytes(nblocks);
    CHECK_LE(used, e.length) << "dense chunk: metadata of range " << r;
    const uint8_t* meta = packed + e.offset;
    for (size_t b = 0; b < nblocks; ++b) {
      const size_t len = std::min(kPackBlockBytes, n - (b0 + b) * kPackBlockBytes);
      const bool raw = meta[2 * b] == kDenseRawMeta && meta[2 * b + 1] == kDenseRawMeta;
      if (!raw) {
        CHECK(meta[2 * b] <= kPackBlockBytes / 2 &&
              static_cast<size_t>(meta[2 * b]) + meta[2 * b + 1] <= kDenseMaxPayload)
            << "dense chunk: metadata of block " << b0 + b;
      }
      used += raw ? len : static_cast<size_t>(meta[2 * b]) + meta[2 * b + 1];
    }
    CHECK_LE(used, e.length) << "dense chunk: payloads of range " << r;
  }
  return n;
}

DenseDirEntry DenseDirectory(const uint8_t* packed, size_t r) {
  return DirEntry(ViewDense(packed), r);
}

void UnpackDenseReference(const uint8_t* packed, uint8_t* dst) {
  const DenseView v = ViewDense(packed);
  const size_t n = v.h.n;
  for (size_t r = 0; r < v.h.nranges; ++r) {
    const DenseDirEntry e = DirEntry(v, r);
    const size_t b0 = r * v.h.range_blocks;
    const size_t nblocks = std::min<size_t>(v.h.range_blocks, PackBlocks(n) - b0);
    const uint8_t* meta = packed + e.offset;
    const uint8_t* p = meta + DenseMetaBytes(nblocks);
    for (size_t b = 0; b < nblocks; ++b) {
      uint8_t* o = dst + (b0 + b) * kPackBlockBytes;
      const size_t len = std::min(kPackBlockBytes, n - (b0 + b) * kPackBlockBytes);
      if (meta[2 * b] == kDenseRawMeta && meta[2 * b + 1] == kDenseRawMeta) {
        std::memcpy(o, p, len);
        p += len;
        continue;
      }
      const size_t nb = meta[2 * b], nlit = meta[2 * b + 1];
      const uint8_t* lit = p + nb;
      size_t at = 0;
      for (size_t k = 0; k < 2 * nb && at < len; ++k) {
        const unsigned c = (k & 1) ? p[k / 2] >> 4 : p[k / 2] & 15u;
        if (c == v.table.escape) {
          o[at++] = *lit++;
        } else {
          for (int j = 0; j < v.table.len[c] && at < len; ++j) o[at++] = v.table.bytes[c][j];
        }
      }
      p += nb + nlit;
    }
  }
}

}  // namespace gpu
}  // namespace dmlc
