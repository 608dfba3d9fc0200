/*!
 * \file src/gpu/text_pack.h
 * \brief Host side of the packed H2D transfer: LibSVM / LibFM / CSV text draws
 *  almost every byte from ~15 symbols, so a chunk crosses the PCIe link as
 *  4-bit codes and is expanded back to the same bytes in HBM
 *  (unpack_kernels.hip).  Plain C++, no HIP.
 *
 * Packed form of a chunk of n text bytes, in blocks of kPackBlockBytes input
 * bytes:
 *   PackedHeader                       n, exception count, the 16-symbol alphabet
 *   nibble area, NibbleAreaBytes(n)    byte k = code(text[2k]) | code(text[2k+1]) << 4
 *                                      ((n+1)/2 bytes, zero padded; block b at 128 * b)
 *   exception indices, u32 each        blocks holding a byte outside the alphabet
 *                                      (padded to 16 bytes)
 *   exception bytes, 256 per block     those blocks' raw bytes (the last short
 *                                      block zero padded); their nibbles are zero
 * A chunk is sent packed only when the packed size is at most
 * kPackMaxRatio (3/4) of n.
 */
#ifndef DMLC_SRC_GPU_TEXT_PACK_H_
#define DMLC_SRC_GPU_TEXT_PACK_H_

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dmlc {
namespace gpu {

constexpr size_t kPackBlockBytes = 256;
constexpr double kPackMaxRatio = 0.75;

struct PackedHeader {
  uint64_t n;
  uint32_t nexc;
  uint32_t reserved;
  uint8_t alphabet[16];
};
static_assert(sizeof(PackedHeader) == 32, "PackedHeader is 32 bytes");

/*! \brief instruction sets of the packer; all produce identical bytes */
enum class PackIsa : int { kAuto = 0, kScalar = 1, kAvx2 = 2, kAvx512 = 3 };
/*! \brief whether this CPU runs `isa` (kAuto and kScalar: always) */
bool PackIsaSupported(PackIsa isa);

/*! \brief the 16 symbols of a format: digits : . space \n - e (LibSVM, LibFM),
 *  CSV with its delimiter in place of ':' */
void PackAlphabet(bool csv, char delimiter, uint8_t alphabet[16]);

inline size_t PackBlocks(size_t n) { return (n + kPackBlockBytes - 1) / kPackBlockBytes; }
/*! \brief (n+1)/2 rounded up to 16, plus 16: the device reads aligned 8-byte
 *  pairs up to one word past the last code */
inline size_t NibbleAreaBytes(size_t n) { return (((n + 1) / 2 + 15) & ~size_t(15)) + 16; }
inline size_t PackedBytes(size_t n, size_t nexc) {
  return sizeof(PackedHeader) + NibbleAreaBytes(n) + ((nexc * 4 + 15) & ~size_t(15)) +
         nexc * kPackBlockBytes;
}
/*! \brief the most exception blocks with PackedBytes <= ratio * n; -1: none
 *  fits.  A negative ratio lifts the bound (every chunk packs; the tests) */
long PackMaxExceptions(size_t n, double ratio = kPackMaxRatio);

/*! \brief byte -> code table of an alphabet, 0x80 outside it (symbols >= 0x80
 *  never encode); built once by a caller that packs many ranges */
struct PackEncoder {
  uint8_t enc[256];
  explicit PackEncoder(const uint8_t alphabet[16]);
};

/*!
 * \brief pack blocks [block_begin, block_end) of text[0, n): nibbles go to
 *  their fixed position in `nibbles` (the chunk's nibble area), the indices of
 *  exception blocks are appended to `exc` in order.
 * \param exc_total shared exception counter of a cooperative pack (may be null)
 * \param exc_limit stop, returning false, once more than this many were counted
 */
bool PackRange(const uint8_t* text, size_t n, size_t block_begin, size_t block_end,
               const PackEncoder& encoder, uint8_t* nibbles, std::vector<uint32_t>* exc,
               std::atomic<long>* exc_total, long exc_limit, PackIsa isa = PackIsa::kAuto);
/*! \brief the same, building the alphabet's table for this call */
bool PackRange(const uint8_t* text, size_t n, size_t block_begin, size_t block_end,
               const uint8_t alphabet[16], uint8_t* nibbles, std::vector<uint32_t>* exc,
               std::atomic<long>* exc_total, long exc_limit, PackIsa isa = PackIsa::kAuto);

/*! \brief the parts of PackFinish, for a caller that shares the copy of the
 *  exception blocks among threads: the header, the nibble area's zero tail and
 *  the exception indices (returns the packed size), then the raw bytes of
 *  exception blocks [first, last) of `exc` */
size_t PackFinishHeader(size_t n, const uint8_t alphabet[16], const std::vector<uint32_t>& exc,
                        uint8_t* packed);
void PackCopyExceptions(const uint8_t* text, size_t n, const std::vector<uint32_t>& exc,
                        size_t first, size_t last, uint8_t* packed);

/*! \brief write the header, the nibble area's zero tail and the exception
 *  lists around an already packed nibble area; returns the packed size */
size_t PackFinish(const uint8_t* text, size_t n, const uint8_t alphabet[16],
                  const std::vector<uint32_t>& exc, uint8_t* packed);

/*! \brief one-call pack; false when the chunk goes raw (packed size above ratio * n) */
bool PackText(const uint8_t* text, size_t n, const uint8_t alphabet[16], double ratio,
              std::vector<uint8_t>* packed, PackIsa isa = PackIsa::kAuto);

/*! \brief sections of a packed chunk */
struct PackedView {
  PackedHeader header;
  const uint8_t* nibbles;
  const uint32_t* exc_index;
  const uint8_t* exc_bytes;
  size_t bytes;
};
PackedView ViewPacked(const uint8_t* packed);

/*! \brief CPU reference of the device unpack: exactly header.n bytes at dst */
void UnpackReference(const uint8_t* packed, uint8_t* dst);

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_TEXT_PACK_H_
