/*!
 * \file tests/cpp/unittest_text_pack.cc
 * \brief The host nibble packer of the packed H2D transfer (src/gpu/text_pack.h):
 *  pack -> reference unpack round trips, every SIMD path the host supports
 *  against the scalar path byte for byte, exception blocks, misaligned input,
 *  and the 3/4 size rule on both sides of its threshold.
 */
#include <cstring>
#include <string>
#include <vector>

#include "../../src/gpu/text_pack.h"
#include "./testing.h"

namespace {

using dmlc::gpu::PackIsa;

const double kForce = -1;  // ratio that packs whatever the size

/*! \brief LibSVM-like text of n bytes, all inside the alphabet */
std::string CleanText(size_t n, unsigned seed = 1) {
  static const char kSym[] = "0123456789:. \n-e";
  std::string s(n, '0');
  unsigned x = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    s[i] = kSym[(x >> 24) % 16];
  }
  return s;
}

std::vector<PackIsa> Paths() {
  std::vector<PackIsa> p;
  for (PackIsa isa : {PackIsa::kScalar, PackIsa::kAvx2, PackIsa::kAvx512, PackIsa::kAuto}) {
    if (dmlc::gpu::PackIsaSupported(isa)) p.push_back(isa);
  }
  return p;
}

/*! \brief pack on every path: identical bytes, and the round trip gives text back */
void CheckAllPaths(const char* text, size_t n, size_t want_exc, bool csv = false, char delim = ',') {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(csv, delim, alphabet);
  const uint8_t* src = reinterpret_cast<const uint8_t*>(text);
  std::vector<uint8_t> scalar;
  ASSERT_TRUE(dmlc::gpu::PackText(src, n, alphabet, kForce, &scalar, PackIsa::kScalar));
  const dmlc::gpu::PackedView v = dmlc::gpu::ViewPacked(scalar.data());
  EXPECT_EQ(v.header.n, n);
  EXPECT_EQ(static_cast<size_t>(v.header.nexc), want_exc);
  EXPECT_EQ(v.bytes, scalar.size());
  EXPECT_EQ(scalar.size(), dmlc::gpu::PackedBytes(n, want_exc));
  std::string back(n + 8, '#');
  dmlc::gpu::UnpackReference(scalar.data(), reinterpret_cast<uint8_t*>(&back[0]));
  EXPECT_TRUE(std::memcmp(back.data(), text, n) == 0);
  EXPECT_EQ(back.substr(n), std::string(8, '#'));  // nothing past n is written
  for (PackIsa isa : Paths()) {
    std::vector<uint8_t> other;
    ASSERT_TRUE(dmlc::gpu::PackText(src, n, alphabet, kForce, &other, isa));
    EXPECT_TRUE(other == scalar);
  }
}

const size_t kSizes[] = {0, 1, 2, 255, 256, 257, 511, 513, 5003};

}  // namespace

TEST(TextPack, RoundTripNoExceptions) {
  for (size_t n : kSizes) {
    const std::string s = CleanText(n, static_cast<unsigned>(n));
    CheckAllPaths(s.data(), n, 0);
  }
}

TEST(TextPack, EveryBlockAnException) {
  for (size_t n : kSizes) {
    std::string s = CleanText(n, 7);
    for (size_t b = 0; b * 256 < n; ++b) s[std::min(n - 1, b * 256 + (b * 37) % 256)] = 'q';
    CheckAllPaths(s.data(), n, (n + 255) / 256);
  }
}

TEST(TextPack, ExceptionOnlyInShortLastBlock) {
  for (size_t n : {size_t(1), size_t(257), size_t(511), size_t(513), size_t(5003)}) {
    std::string s = CleanText(n, 9);
    s[n - 1] = '\t';
    CheckAllPaths(s.data(), n, 1);
  }
}

TEST(TextPack, HighBytesCarriageReturnAndNul) {
  const char kExotic[] = {'\x80', '\xff', '\xb0', '\r', '\0', '\t', 'q', 'E', '+', ','};
  for (char c : kExotic) {
    for (size_t pos : {size_t(0), size_t(63), size_t(64), size_t(255), size_t(300), size_t(767)}) {
      std::string s = CleanText(1024, 11);
      s[pos] = c;
      CheckAllPaths(s.data(), s.size(), 1);
    }
  }
  // 0xb0 must not alias '0' (0x30) through a 7-bit table index
  std::string s = CleanText(512, 3);
  s[100] = '\xb0';
  s[400] = '\xba';
  CheckAllPaths(s.data(), s.size(), 2);
}

TEST(TextPack, MisalignedInput) {
  const std::string base = CleanText(5003 + 64, 13);
  for (size_t shift = 1; shift < 64; shift += 6) {
    CheckAllPaths(base.data() + shift, 5003, 0);
    std::string s = base;
    s[shift + 300] = '\r';
    CheckAllPaths(s.data() + shift, 5003, 1);
  }
}

TEST(TextPack, CsvDelimiterReplacesColon) {
  std::string s = CleanText(2048, 17);
  for (char& c : s) {
    if (c == ':') c = ',';
  }
  CheckAllPaths(s.data(), s.size(), 0, /*csv=*/true, ',');
  s[5] = ':';  // not in the CSV alphabet
  CheckAllPaths(s.data(), s.size(), 1, /*csv=*/true, ',');
  for (char& c : s) {
    if (c == ',' || c == ':') c = '|';
  }
  CheckAllPaths(s.data(), s.size(), 0, /*csv=*/true, '|');
}

TEST(TextPack, ThreeQuarterRule) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  const size_t n = 64 * 1024;
  const long limit = dmlc::gpu::PackMaxExceptions(n);
  ASSERT_GT(limit, 0L);
  EXPECT_LE(dmlc::gpu::PackedBytes(n, static_cast<size_t>(limit)), n * 3 / 4);
  EXPECT_GT(dmlc::gpu::PackedBytes(n, static_cast<size_t>(limit) + 1), n * 3 / 4);
  for (PackIsa isa : Paths()) {
    for (long nexc : {limit, limit + 1}) {
      std::string s = CleanText(n, 19);
      for (long b = 0; b < nexc; ++b) s[static_cast<size_t>(b) * 256 + 5] = 'x';
      std::vector<uint8_t> packed;
      const bool ok = dmlc::gpu::PackText(reinterpret_cast<const uint8_t*>(s.data()), n, alphabet,
                                          dmlc::gpu::kPackMaxRatio, &packed, isa);
      EXPECT_EQ(ok, nexc == limit);
      if (ok) {
        EXPECT_LE(packed.size(), n * 3 / 4);
        std::string back(n, '#');
        dmlc::gpu::UnpackReference(packed.data(), reinterpret_cast<uint8_t*>(&back[0]));
        EXPECT_TRUE(back == s);
      }
    }
  }
  // too small for the header and the nibble slack: raw
  std::vector<uint8_t> packed;
  const std::string tiny = CleanText(64);
  EXPECT_FALSE(dmlc::gpu::PackText(reinterpret_cast<const uint8_t*>(tiny.data()), tiny.size(),
                                   alphabet, dmlc::gpu::kPackMaxRatio, &packed));
  EXPECT_EQ(dmlc::gpu::PackMaxExceptions(0), -1L);
}

TEST(TextPack, CooperativeRangesMatchOneCall) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  const size_t n = 40 * 256 + 77;
  std::string s = CleanText(n, 23);
  for (size_t b : {size_t(0), size_t(13), size_t(14), size_t(39), size_t(40)}) s[b * 256 + 9] = 'z';
  const uint8_t* src = reinterpret_cast<const uint8_t*>(s.data());
  std::vector<uint8_t> whole;
  ASSERT_TRUE(dmlc::gpu::PackText(src, n, alphabet, kForce, &whole));
  // three ranges as three pool threads would take them, lists concatenated
  std::vector<uint8_t> coop(dmlc::gpu::PackedBytes(n, 5), 0xEE);
  std::atomic<long> total{0};
  std::vector<uint32_t> all;
  const size_t cuts[] = {0, 14, 27, dmlc::gpu::PackBlocks(n)};
  for (int p = 2; p >= 0; --p) {  // any completion order
    std::vector<uint32_t> part;
    ASSERT_TRUE(dmlc::gpu::PackRange(src, n, cuts[p], cuts[p + 1], alphabet,
                                     coop.data() + sizeof(dmlc::gpu::PackedHeader), &part, &total,
                                     1000));
    all.insert(all.begin(), part.begin(), part.end());
  }
  EXPECT_EQ(total.load(), 5L);
  EXPECT_EQ(dmlc::gpu::PackFinish(src, n, alphabet, all, coop.data()), coop.size());
  EXPECT_TRUE(coop == whole);
}
