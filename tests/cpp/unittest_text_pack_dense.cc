/*!
 * \file tests/cpp/unittest_text_pack_dense.cc
 * \brief The dense code of the packed H2D transfer (src/gpu/text_pack_dense.h):
 *  table rules and selection, the scalar and AVX-512 encoders against the CPU
 *  reference decoder on every edge of a vector and of a block, and the pack
 *  pool's ranges of variable size.  Part of the sanitizer runs of the suite.
 */
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../src/gpu/pack_pool.h"
#include "../../src/gpu/text_pack_codec.h"
#include "../../src/gpu/text_pack_dense.h"
#include "./testing.h"

namespace {

using namespace dmlc::gpu;  // NOLINT

typedef std::vector<std::vector<uint8_t>> Entries;

Entries Singles(const char* symbols) {
  Entries e;
  for (const char* c = symbols; *c; ++c) e.push_back({static_cast<uint8_t>(*c)});
  return e;
}
std::vector<uint8_t> Bytes(const char* s) {
  return std::vector<uint8_t>(s, s + std::strlen(s));
}

/*! \brief 14 symbols and `:0.` */
DenseTable BenchTable() {
  Entries e = Singles("0123456789:. \n");
  e.push_back(Bytes(":0."));
  DenseTable t;
  EXPECT_TRUE(DenseMakeTable(e, &t));
  return t;
}

/*! \brief rows of tokens ` iiiiii:0.dddddd` (value "0.dddddd") or ` iiiiii:1` */
std::string TokenText(size_t n, unsigned seed, bool binary) {
  std::string s;
  unsigned x = seed * 2654435761u + 7u;
  auto digits = [&](int k) {
    for (int i = 0; i < k; ++i) {
      x = x * 1664525u + 1013904223u;
      s.push_back(static_cast<char>('0' + (x >> 24) % 10));
    }
  };
  while (s.size() < n) {
    s.push_back('1');
    for (int t = 0; t < 30; ++t) {
      s.push_back(' ');
      digits(6);
      s += binary ? ":1" : ":0.";
      if (!binary) digits(6);
    }
    s.push_back('\n');
  }
  s.resize(n);
  return s;
}

const uint8_t* U8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

/*! \brief pack with every encoder this CPU runs (equal bytes), check the
 *  chunk and decode it; returns the packed chunk */
std::vector<uint8_t> RoundTrip(const std::string& text, const DenseTable& table,
                               size_t range_blocks = 4, size_t* escapes = nullptr,
                               size_t* raw_blocks = nullptr) {
  std::vector<uint8_t> packed;
  EXPECT_TRUE(PackTextDense(U8(text), text.size(), table, range_blocks, -1.0, &packed,
                            PackIsa::kScalar, escapes, raw_blocks));
  if (PackIsaSupportedDense(PackIsa::kAvx512)) {
    std::vector<uint8_t> simd;
    EXPECT_TRUE(PackTextDense(U8(text), text.size(), table, range_blocks, -1.0, &simd,
                              PackIsa::kAvx512));
    EXPECT_TRUE(simd == packed);
  }
  EXPECT_TRUE(IsDenseChunk(packed.data(), packed.size()));
  EXPECT_EQ(DenseCheck(packed.data(), packed.size()), text.size());
  std::string out(text.size() + 8, '#');
  UnpackDenseReference(packed.data(), reinterpret_cast<uint8_t*>(&out[0]));
  EXPECT_TRUE(out.compare(0, text.size(), text) == 0);
  EXPECT_TRUE(out.compare(text.size(), 8, "########") == 0);  // nothing past n
  return packed;
}

/*! \brief the two metadata bytes of block b (ranges of range_blocks blocks) */
std::pair<int, int> Meta(const std::vector<uint8_t>& packed, size_t b, size_t range_blocks) {
  const DenseDirEntry e = DenseDirectory(packed.data(), b / range_blocks);
  const uint8_t* m = packed.data() + e.offset + 2 * (b % range_blocks);
  return {m[0], m[1]};
}

bool Has(const DenseTable& t, const char* entry) {
  const size_t len = std::strlen(entry);
  for (int c = 0; c < 16; ++c) {
    if (t.len[c] == len && std::memcmp(t.bytes[c], entry, len) == 0) return true;
  }
  return false;
}

}  // namespace

TEST(TextPackDense, RoundTripEverySmallSize) {
  const DenseTable table = BenchTable();
  const std::string all = TokenText(600, 1, false);
  for (size_t n = 0; n <= 600; ++n) RoundTrip(all.substr(0, n), table, 1 + n % 3);
  for (size_t n : {255, 256, 257, 511, 512, 513}) {
    std::string t = TokenText(n, static_cast<unsigned>(n), false);
    RoundTrip(t, DenseSelectTable(U8(t), t.size(), false, ','));
    t[n / 2] = '\r';
    t[n - 1] = static_cast<char>(0xC3);
    RoundTrip(t, table);
  }
}

TEST(TextPackDense, EncodersAgreePerRange) {
  const std::string text = TokenText(9000, 5, false);
  const DenseEncoder enc(BenchTable());
  if (!PackIsaSupportedDense(PackIsa::kAvx512)) return;
  for (size_t rb : {1, 3, 8}) {
    for (size_t b0 = 0; b0 < PackBlocks(text.size()); b0 += rb) {
      const size_t b1 = std::min(PackBlocks(text.size()), b0 + rb);
      std::vector<uint8_t> a(DenseRangeCapacity(rb), 0x11), b(DenseRangeCapacity(rb), 0x22);
      size_t ea = 0, eb = 0;
      const size_t la = PackRangeDense(U8(text), text.size(), b0, b1, enc, a.data(), &ea, nullptr,
                                       PackIsa::kScalar);
      const size_t lb = PackRangeDense(U8(text), text.size(), b0, b1, enc, b.data(), &eb, nullptr,
                                       PackIsa::kAvx512);
      ASSERT_EQ(la, lb);
      EXPECT_EQ(la % kDenseRangeAlign, 0u);
      EXPECT_EQ(ea, eb);
      EXPECT_TRUE(std::equal(a.begin(), a.begin() + la, b.begin()));
    }
  }
}

TEST(TextPackDense, TrigramAtVectorAndBlockEdges) {
  const DenseTable table = BenchTable();
  // every offset around the end of a 64-byte vector: one code for three bytes
  for (size_t at = 60; at <= 66; ++at) {
    std::string t(515, '7');
    t.replace(at, 3, ":0.");
    const std::vector<uint8_t> packed = RoundTrip(t, table);
    EXPECT_EQ(Meta(packed, 0, 4).first, 127);  // 254 codes
  }
  // around the end of a block: a match never extends past it
  const int codes0[4] = {254, 256, 256, 256}, codes1[4] = {256, 256, 256, 254};
  for (int k = 0; k < 4; ++k) {
    std::string t(515, '7');
    t.replace(253 + k, 3, ":0.");
    const std::vector<uint8_t> packed = RoundTrip(t, table);
    EXPECT_EQ(Meta(packed, 0, 4).first, codes0[k] / 2);
    EXPECT_EQ(Meta(packed, 1, 4).first, codes1[k] / 2);
    EXPECT_EQ(Meta(packed, 0, 4).second, 0);
  }
  // at the very end of the text, and cut by it
  std::string t(512, '7');
  t.replace(509, 3, ":0.");
  EXPECT_EQ(Meta(RoundTrip(t, table), 1, 4).first, 127);
  t = std::string(511, '7');
  t.replace(509, 2, ":0");
  EXPECT_EQ(Meta(RoundTrip(t, table), 1, 4).first, 128);  // 255 codes and the pad
}

TEST(TextPackDense, LiteralAsLastByteOfBlock) {
  std::string t = TokenText(700, 3, false);
  t[255] = '\r';
  t[511] = 'x';
  size_t escapes = 0;
  const std::vector<uint8_t> packed = RoundTrip(t, BenchTable(), 4, &escapes);
  EXPECT_EQ(escapes, 2u);
  EXPECT_EQ(Meta(packed, 0, 4).second, 1);
  EXPECT_EQ(Meta(packed, 1, 4).second, 1);
  EXPECT_EQ(Meta(packed, 2, 4).second, 0);
}

TEST(TextPackDense, BlockOutsideTableIsRaw) {
  std::string t = TokenText(768, 4, false);
  for (size_t i = 256; i < 512; ++i) t[i] = 'x';
  size_t escapes = 0, raw = 0;
  const std::vector<uint8_t> packed = RoundTrip(t, BenchTable(), 4, &escapes, &raw);
  EXPECT_EQ(raw, 1u);
  EXPECT_EQ(escapes, 0u);
  EXPECT_EQ(Meta(packed, 1, 4).first, static_cast<int>(kDenseRawMeta));
  EXPECT_EQ(Meta(packed, 1, 4).second, static_cast<int>(kDenseRawMeta));
  EXPECT_NE(Meta(packed, 0, 4).first, static_cast<int>(kDenseRawMeta));
  // a short last block, raw
  t = TokenText(456, 4, false);
  for (size_t i = 256; i < 456; ++i) t[i] = 'x';
  raw = 0;
  RoundTrip(t, BenchTable(), 4, nullptr, &raw);
  EXPECT_EQ(raw, 1u);
}

TEST(TextPackDense, PayloadLimit) {
  // 256 single-byte codes are 128 nibble bytes: 64 literals reach the limit
  for (size_t nlit : {64, 65}) {
    std::string t(512, '3');
    for (size_t i = 0; i < nlit; ++i) t[3 * i + 1] = 'x';
    size_t raw = 0;
    const std::vector<uint8_t> packed = RoundTrip(t, BenchTable(), 4, nullptr, &raw);
    if (nlit == 64) {
      EXPECT_EQ(raw, 0u);
      EXPECT_EQ(Meta(packed, 0, 4).first + Meta(packed, 0, 4).second,
                static_cast<int>(kDenseMaxPayload));
    } else {
      EXPECT_EQ(raw, 1u);
      EXPECT_EQ(Meta(packed, 0, 4).first, static_cast<int>(kDenseRawMeta));
    }
  }
}

TEST(TextPackDense, EntriesOfEveryLength) {
  Entries e = Singles("0123 \n");
  e.push_back(Bytes("ab"));
  e.push_back(Bytes("cde"));
  e.push_back(Bytes("fghi"));
  DenseTable table;
  ASSERT_TRUE(DenseMakeTable(e, &table));
  std::string unit = "0ab1cde2fghi3 ab\ncdefghi";
  std::string t;
  while (t.size() < 1500) t += unit;
  size_t escapes = 0;
  const std::vector<uint8_t> packed = RoundTrip(t, table, 2, &escapes);
  EXPECT_LT(packed.size(), t.size() / 2);
  // (a, c, ... on their own are outside the table)
  t[700] = 'a';
  t[701] = '0';
  RoundTrip(t, table, 2);
  // two entries, of 3 and 4 bytes: the SIMD encoder's widest loads
  Entries e2 = Singles("0123 \n");
  e2.push_back(Bytes("cde"));
  e2.push_back(Bytes("fghi"));
  ASSERT_TRUE(DenseMakeTable(e2, &table));
  for (size_t shift = 0; shift < 8; ++shift) RoundTrip(t.substr(shift), table, 3);
}

TEST(TextPackDense, NoOverlapRule) {
  auto ok = [](const char* a, const char* b) {
    return DenseCompatible(reinterpret_cast<const uint8_t*>(a), static_cast<int>(std::strlen(a)),
                           reinterpret_cast<const uint8_t*>(b), static_cast<int>(std::strlen(b)));
  };
  EXPECT_FALSE(ok("0.", ":0."));   // a suffix of one is a prefix of the other
  EXPECT_FALSE(ok(":0.", "0."));
  EXPECT_FALSE(ok(":0", ":0."));   // one begins the other
  EXPECT_FALSE(ok("abcd", "bc"));  // one lies inside the other
  EXPECT_FALSE(ok("11", "11"));    // overlaps itself
  EXPECT_FALSE(ok("aba", "aba"));
  EXPECT_TRUE(ok(":0.", ":0."));
  EXPECT_TRUE(ok(":0.", ":1"));
  EXPECT_TRUE(ok("12", "34"));
  Entries e = Singles("0123456789: \n");
  e.push_back(Bytes(":0."));
  e.push_back(Bytes("0."));
  DenseTable t;
  EXPECT_FALSE(DenseMakeTable(e, &t));
  e.back() = Bytes(":1");
  EXPECT_TRUE(DenseMakeTable(e, &t));
}

TEST(TextPackDense, SelectorPicksTheFormatsConstants) {
  const std::string values = TokenText(64 << 10, 9, false);
  const DenseTable a = DenseSelectTable(U8(values), values.size(), false, ',');
  EXPECT_TRUE(DenseTableValid(a));
  EXPECT_TRUE(Has(a, ":0."));
  EXPECT_FALSE(Has(a, "0."));
  const std::string binary = TokenText(64 << 10, 9, true);
  const DenseTable b = DenseSelectTable(U8(binary), binary.size(), false, ',');
  EXPECT_TRUE(DenseTableValid(b));
  EXPECT_TRUE(Has(b, ":1"));
  // the same text, the same table; an empty text gets the format's symbols
  const DenseTable a2 = DenseSelectTable(U8(values), values.size(), false, ',');
  EXPECT_TRUE(std::memcmp(&a, &a2, sizeof(a)) == 0);
  const DenseTable empty = DenseSelectTable(nullptr, 0, true, ';');
  EXPECT_TRUE(DenseTableValid(empty));
  EXPECT_TRUE(Has(empty, ";"));
  RoundTrip(values.substr(0, 5000), a);
  RoundTrip(binary.substr(0, 5000), b);
}

TEST(TextPackDense, PoolRangesInAnyOrder) {
  std::string text = TokenText(2048, 11, false);
  text[300] = '\r';
  uint8_t alphabet[16];
  PackAlphabet(false, ',', alphabet);
  for (size_t rb : {1, 2}) {
    std::vector<std::vector<uint8_t>> ranges[2];
    size_t bytes[2] = {0, 0};
    int k = 0;
    for (int threads : {1, 4}) {
      std::vector<uint8_t> out(DenseMaxBytes(text.size(), rb) + 64, 0xEE);
      PackJob job;
      job.ptr = text.data();
      job.size = text.size();
      job.ratio = -1.0;
      job.out = out.data() + ((64 - (reinterpret_cast<uintptr_t>(out.data()) & 63)) & 63);
      {
        PackPool pool(threads, MakePackCodec(PackCode::kDense, false, ','), 0, rb);
        pool.Push(&job);
        pool.Wait(&job);
      }
      ASSERT_EQ(job.state.load(), static_cast<int>(PackJob::kPacked));
      EXPECT_TRUE(job.dense);
      EXPECT_GE(job.escape_bytes, 1u);  // the carriage return, and what the table left out
      EXPECT_EQ(DenseCheck(job.out, job.packed_bytes), text.size());
      std::string decoded(text.size(), '#');
      UnpackDenseReference(job.out, reinterpret_cast<uint8_t*>(&decoded[0]));
      EXPECT_TRUE(decoded == text);
      const size_t nranges = DenseRanges(text.size(), rb);
      size_t payload = 0;
      for (size_t r = 0; r < nranges; ++r) {
        const DenseDirEntry e = DenseDirectory(job.out, r);
        ranges[k].emplace_back(job.out + e.offset, job.out + e.offset + e.length);
        payload += e.length;
      }
      EXPECT_EQ(DenseHeaderBytes(nranges, DenseEntryBytes(job.table)) + payload,
                job.packed_bytes);
      bytes[k++] = job.packed_bytes;
    }
    // range r holds the same bytes wherever it landed
    EXPECT_EQ(bytes[0], bytes[1]);
    EXPECT_TRUE(ranges[0] == ranges[1]);
  }
}

TEST(TextPackDense, PoolThreeQuarterRule) {
  // text outside every table: all blocks raw, the job does not fit 3/4
  std::string text(8192, 'x');
  for (size_t i = 0; i < text.size(); ++i) text[i] = static_cast<char>('A' + (i * 7) % 50);
  uint8_t alphabet[16];
  PackAlphabet(false, ',', alphabet);
  std::vector<uint8_t> out(DenseMaxBytes(text.size(), 4) + 64, 0);
  PackJob job;
  job.ptr = text.data();
  job.size = text.size();
  job.out = out.data() + ((64 - (reinterpret_cast<uintptr_t>(out.data()) & 63)) & 63);
  PackPool pool(2, MakePackCodec(PackCode::kDense, false, ','), 0, 4);
  pool.Push(&job);
  pool.Wait(&job);
  EXPECT_EQ(job.state.load(), static_cast<int>(PackJob::kRejected));
}
