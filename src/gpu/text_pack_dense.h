/*!
 * \file src/gpu/text_pack_dense.h
 * \brief The dense code of the packed H2D transfer: a 4-bit code whose 16
 *  entries may be strings of 1-4 bytes, chosen per job from a sample of the
 *  job's own text.  A token ` iiiiii:0.dddddd` then crosses the link as 13.9
 *  nibbles where the nibble code (text_pack.h) takes 15.9.  Plain C++, no HIP.
 *
 * Table.  15 entries and one escape code.  The escape stands for one raw byte,
 * taken in order from the block's literal tail (12 bits for a byte outside the
 * table; there are no exception blocks).  Multi-byte entries obey the
 * no-overlap rule (DenseCompatible): wherever two of them are laid over each
 * other at a shift of 0-3 bytes they disagree in a byte they share, so the
 * matches in a text never overlap and an encoder needs no sequential greedy
 * step.  This covers "no proper suffix of an entry is a prefix of an entry"
 * and also an entry lying inside a longer one.
 *
 * Blocks.  Text is coded in the 256-byte blocks of text_pack.h; a match never
 * extends past its block's end.  A block's payload is its nibble bytes (code
 * k of the block in bits 4 * (k & 1) of byte k / 2, an odd count padded with a
 * zero nibble) followed by its literal bytes.  Its two metadata bytes are the
 * count of nibble bytes (<= 128: every code yields a byte) and the count of
 * literals.  A block whose payload would exceed kDenseMaxPayload (192) bytes
 * is stored raw, metadata 0xff 0xff.
 *
 * Range.  A job is cut into ranges of `range_blocks` blocks (the pack pool's
 * unit of work).  A packed range is
 *   metadata, 2 bytes per block, padded to 16 bytes
 *   the blocks' payloads back to back, no alignment
 * padded with zeros to a multiple of kDenseRangeAlign (16) bytes: the decoder
 * reads single bytes, the 16 are for the pool's streaming stores.
 *
 * Chunk.
 *   DenseHeader           n, the range geometry, the escape code, the entries'
 *                         lengths (32 bytes)
 *   entry bytes           the entries back to back, in code order (padded to 8)
 *   directory             per range: offset from the chunk's start, length
 *   (padded to 16 bytes)
 *   packed ranges         each at a multiple of 16, in any order: the
 *                         directory says where range r is
 * Header and directory take 64 bytes for a typical table and one range, so
 * that chunks of a few KiB still gain.
 * DenseHeader.magic sits where PackedHeader.reserved (always 0) does, so the
 * two kinds of chunk are told apart by that word.
 */
#ifndef DMLC_SRC_GPU_TEXT_PACK_DENSE_H_
#define DMLC_SRC_GPU_TEXT_PACK_DENSE_H_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "./text_pack.h"

namespace dmlc {
namespace gpu {

constexpr uint32_t kDenseMagic = 0x45534e44u;  // "DNSE"
constexpr size_t kDenseMaxPayload = 192;
constexpr size_t kDenseRangeAlign = 16;
constexpr uint8_t kDenseRawMeta = 0xff;
/*! \brief multi-byte entries the selector picks at most (each costs the SIMD
 *  encoder a few compares per vector) */
constexpr int kDenseMaxMulti = 2;

/*! \brief the 16 codes: entry c is bytes[c][0, len[c]); len[escape] is 0 */
struct DenseTable {
  uint8_t bytes[16][4];
  uint8_t len[16];
  uint8_t escape;
};

struct DenseHeader {
  uint64_t n;
  uint32_t nranges;
  uint32_t magic;
  uint32_t range_blocks;
  uint8_t escape;
  /*! \brief sum of the entries' lengths */
  uint8_t entry_bytes;
  uint16_t reserved;
  /*! \brief length of entry c in bits 4 * (c & 1) of byte c / 2 */
  uint8_t len[8];
};
static_assert(sizeof(DenseHeader) == 32, "DenseHeader is 32 bytes");

struct DenseDirEntry {
  uint32_t offset;
  uint32_t length;
};

inline size_t DenseAlign(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline size_t DenseRanges(size_t n, size_t range_blocks) {
  return (PackBlocks(n) + range_blocks - 1) / range_blocks;
}
/*! \brief where the directory starts in a chunk whose entries take entry_bytes */
inline size_t DenseDirOffset(size_t entry_bytes) {
  return sizeof(DenseHeader) + DenseAlign(entry_bytes, 8);
}
/*! \brief header, entries and directory: where the first packed range may start */
inline size_t DenseHeaderBytes(size_t nranges, size_t entry_bytes) {
  return DenseAlign(DenseDirOffset(entry_bytes) + nranges * sizeof(DenseDirEntry),
                    kDenseRangeAlign);
}
inline size_t DenseMetaBytes(size_t nblocks) { return DenseAlign(2 * nblocks, 16); }
/*! \brief the most a packed range of nblocks takes (every block raw), plus
 *  the slack the SIMD encoder's whole-vector stores write past a payload */
inline size_t DenseRangeCapacity(size_t nblocks) {
  return DenseAlign(DenseMetaBytes(nblocks) + nblocks * kPackBlockBytes, kDenseRangeAlign) + 128;
}
/*! \brief the most a packed chunk takes */
inline size_t DenseMaxBytes(size_t n, size_t range_blocks) {
  const size_t nranges = DenseRanges(n, range_blocks);
  return DenseHeaderBytes(nranges, 60) + nranges * DenseRangeCapacity(range_blocks);
}

/*! \brief the no-overlap rule for two multi-byte entries (a may equal b): laid
 *  over each other at any shift that makes them share a byte (shift 0 only for
 *  distinct entries), they disagree in a shared byte */
bool DenseCompatible(const uint8_t* a, int alen, const uint8_t* b, int blen);
/*! \brief a table is well formed: one escape, lengths 1-4, distinct
 *  single-byte entries, multi-byte entries pairwise (and each with itself)
 *  compatible */
bool DenseTableValid(const DenseTable& t);
inline size_t DenseEntryBytes(const DenseTable& t) {
  size_t sum = 0;
  for (int c = 0; c < 16; ++c) sum += t.len[c];
  return sum;
}
/*! \brief directory entry r of a packed chunk */
DenseDirEntry DenseDirectory(const uint8_t* packed, size_t r);
/*! \brief the table of a format with no multi-byte entry: PackAlphabet's first
 *  15 symbols and the escape */
DenseTable DenseDefaultTable(bool csv, char delimiter);
/*! \brief table from explicit entries (tests): entries.size() <= 15, the
 *  escape takes the next code, codes after it stay unused (length 0); false
 *  when the result is not valid */
bool DenseMakeTable(const std::vector<std::vector<uint8_t>>& entries, DenseTable* out);

/*!
 * \brief choose the table of a job from a sample of its text: kDenseSampleBytes
 *  at every kDenseSampleStride (about 0.1 %; a text shorter than one stride is
 *  sampled from its start).  Bytes, bigrams and trigrams are counted; an
 *  n-gram is a candidate when it lies inside a token (no blank, tab, CR or LF)
 *  and its bytes are among the 15 most frequent such bytes.  A single byte
 *  costs 2 nibbles more per occurrence when it is left to the escape, an n-gram
 *  saves its length - 1 nibbles per occurrence.  N-grams are tried best first
 *  under the no-overlap rule, at most kDenseMaxMulti of them; one is taken
 *  when it saves more than the single byte it pushes out of the table costs,
 *  by at least 1/256 of the sample.  Single bytes fill the other codes by the
 *  occurrences no chosen n-gram covers, the format's symbols first among
 *  equals, so that clean text costs what the nibble code does plus the
 *  metadata.  A pure function of the
 *  text.
 */
DenseTable DenseSelectTable(const uint8_t* text, size_t n, bool csv, char delimiter);
constexpr size_t kDenseSampleBytes = 4096;
constexpr size_t kDenseSampleStride = size_t(4) << 20;

/*! \brief a table prepared for the encoders */
struct DenseEncoder {
  DenseTable table;
  /*! \brief byte -> code of its single-byte entry, 0x80 outside the table */
  uint8_t enc[256];
  /*! \brief the multi-byte entries */
  int nmulti;
  uint8_t mcode[15], mlen[15];
  uint8_t mbytes[15][4];
  explicit DenseEncoder(const DenseTable& t);
};

/*!
 * \brief pack blocks [block_begin, block_end) of text[0, n) as one range into
 *  out (DenseRangeCapacity(block_end - block_begin) bytes); returns the packed
 *  range's length, a multiple of kDenseRangeAlign.  kAvx512 needs BW, VBMI and
 *  VBMI2 (PackIsaSupportedDense); kAvx2 runs the scalar encoder.  All produce
 *  identical bytes.
 * \param escapes, raw_blocks counters to add to (may be null)
 */
size_t PackRangeDense(const uint8_t* text, size_t n, size_t block_begin, size_t block_end,
                      const DenseEncoder& encoder, uint8_t* out, size_t* escapes,
                      size_t* raw_blocks, PackIsa isa = PackIsa::kAuto);
bool PackIsaSupportedDense(PackIsa isa);

/*! \brief write header, entries and directory
 *  (DenseHeaderBytes(dir.size(), DenseEntryBytes(table)) bytes) */
void DenseWriteHeader(size_t n, size_t range_blocks, const DenseTable& table,
                      const std::vector<DenseDirEntry>& dir, uint8_t* packed);
/*! \brief copy of a packed range into the chunk (dst 16-byte aligned, bytes a
 *  multiple of 16): streaming stores, fenced before it returns */
void DenseCopyOut(const uint8_t* src, size_t bytes, uint8_t* dst);

/*! \brief one-call pack, ranges in order; false when the chunk goes raw
 *  (packed size above ratio * n; a negative ratio lifts the bound) */
bool PackTextDense(const uint8_t* text, size_t n, const DenseTable& table, size_t range_blocks,
                   double ratio, std::vector<uint8_t>* packed, PackIsa isa = PackIsa::kAuto,
                   size_t* escapes = nullptr, size_t* raw_blocks = nullptr);

/*! \brief whether a packed chunk is a dense one */
bool IsDenseChunk(const uint8_t* packed, size_t bytes);
/*! \brief check a dense chunk of `bytes` bytes: header, table, directory and
 *  every block's payload inside its range; returns n, throws dmlc::Error */
size_t DenseCheck(const uint8_t* packed, size_t bytes);
/*! \brief CPU reference of the device unpack: exactly header.n bytes at dst */
void UnpackDenseReference(const uint8_t* packed, uint8_t* dst);

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_TEXT_PACK_DENSE_H_
