/*!
 * \file src/gpu/tile_common.h
 * \brief LDS-staged tile parser: the LibSVM / LibFM fast path in three launches
 *  and one host wait (mapped pinned memory) for the chunk sizes.  What the
 *  stages share: tile constants, byte-class masks, text / mask loads, token
 *  list entries and the generic-token and `qid:` fallbacks.  Device-only;
 *  included by tile_count_kernels.hip and tile_fill_kernels.hip alone.
 *
 *  Every row of a regular chunk is one line whose first byte starts its label
 *  token, so with L(p) = line starts at or before byte p and T(p) = tokens
 *  before p, the CSR position of a token follows from two prefix counts:
 *      row(label token k of line l)   = l,        offset[l] = k - l
 *      nnz(feature token k of line l) = k - l - 1
 *  No per-line or per-token index arrays are materialised.
 *
 *  C1 k_tile_count (tile_count_kernels.hip): per tile (line starts << 32 |
 *     token starts), an irregular bit and the per-16-byte start masks.  Reads
 *     the chunk once.
 *  C2 k_tile_scan  (tile_count_kernels.hip): exclusive scan of the tile
 *     counts, OR of the flags; the chunk sizes go to the ChunkMeta and to
 *     mapped pinned memory the host polls.
 *  C3 k_tile_fill  (tile_fill_kernels.hip): one wave per tile decodes every
 *     token and stores index / value / label / offset directly; or
 *     k_tile_hash (the same file): tokenize -> hash -> dense rows, no CSR.
 *  (C2 and C4 become two-level -- many workgroups, then one -- above 8192
 *  tiles, i.e. for the 1 GiB passes over HBM-resident text.)
 *  C4 k_tile_finish (tile_count_kernels.hip): fold the per-wave slots into the
 *     ChunkMeta and write the chunk's closing row pointer.
 *  Traffic per chunk: text read twice (C1, C3) + the CSR written once.
 */
#ifndef DMLC_GPU_TILE_COMMON_H_
#define DMLC_GPU_TILE_COMMON_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../data/strtonum.h"
#include "./device_common.h"
#include "./kernels.h"
#include "./token_decode.h"

namespace dmlc {
namespace gpu {

namespace {
constexpr int kThreads = 256;
static_assert(kTileBytes == 8192, "entry packing assumes 8 KiB tiles");

constexpr int kCountLoads = static_cast<int>(kTileBytes / 1024);  // 16 B loads per lane and tile
constexpr int kFillWaves = kThreads / 64;
constexpr uint32_t kDecodeCarry = 64;  // tokens a step may leave for the next one's rounds
#ifndef DMLC_FILL_WAVES
#define DMLC_FILL_WAVES 4  // measured best (profiles/r03_fill_ablation)
#endif
constexpr uint32_t kStepBytes = 2048;
constexpr int kSteps = static_cast<int>(kTileBytes / kStepBytes);
constexpr uint32_t kSlotBytes = kStepBytes + 64;           // a step + 64 B of the next
constexpr uint32_t kStageVecs = 2 * kSlotBytes / 16;       // two slots: step s and s - 1
constexpr uint32_t kListCap = kDecodeCarry + kStepBytes / 2;  // carried + a step's tokens
// deferred-token ring: < 64 left after a queue round + 128 from a pair round
constexpr uint32_t kQueueCap = 256;
// k_tile_hash: the tokens after a step's last whole round (< 64) are carried
// into the next step's rounds; their text moves with them into a 1 KiB carry
// area in front of the staged step (the window stays contiguous), so no step
// pays a mostly idle last round.  A step of more tokens than the list holds
// is listed in two halves.  LDS per workgroup at dim 1024: 4 x (3136 B text +
// 428 x 4 B list + 64 dummy slots) + 16 KiB rows: 4 workgroups per CU
constexpr uint32_t kHashListCap = 428;
constexpr uint32_t kHashCarry = 1024;  // carry area ahead of the staged step
constexpr uint32_t kHashText = kHashCarry + kSlotBytes;

/*! \brief the high bit of each byte of z (z & 0x80808080) as a 4-bit mask:
 *  one byte dot product (v_dot4_u32_u8, full rate), not the quarter-rate
 *  v_mul_lo_u32 of the multiply-gather */
__device__ __forceinline__ uint32_t gather_hi(uint32_t z) {
  return __builtin_amdgcn_udot4(z, 0x08040201u, 0u, false) >> 7;
}

/*!
 * \brief byte classes of 16 bytes, branch-free SWAR (no cross-byte carries):
 *  sep = byte <= 0x20, eol = sep with (byte & 6) != 0, ctl = byte < 0x20.
 *  On text whose control bytes are only \t \n \r (verified per chunk by
 *  k_tile_count through `ctl`), sep is exactly {' ', \t, \n, \r} and eol
 *  exactly {\n, \r}.
 */
__device__ __forceinline__ void classify16(uint4 v, uint32_t* sep, uint32_t* eol, uint32_t* ctl) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t s = 0, e = 0, c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t x = w[i];
    const uint32_t lo7 = x & 0x7F7F7F7Fu;
    const uint32_t le20 = ~((lo7 + 0x5F5F5F5Fu) | x) & 0x80808080u;    // <= 0x20
    const uint32_t lt20 = ~((lo7 + 0x60606060u) | x) & 0x80808080u;    // <  0x20
    const uint32_t b6 = ((x & 0x06060606u) + 0x7E7E7E7Eu) & 0x80808080u;  // (b & 6) != 0
    s |= gather_hi(le20) << (4 * i);
    e |= gather_hi(le20 & b6) << (4 * i);
    c |= gather_hi(lt20) << (4 * i);
  }
  *sep = s;
  *eol = e;
  *ctl = c;
}

/*! \brief bytes of v with bit 6 set (letters and the like: no number starts
 *  so), as a 16-bit mask -- the C1 test of letter-started tokens */
__device__ __forceinline__ uint32_t letter_mask(uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) m |= gather_hi((w[i] << 1) & 0x80808080u) << (4 * i);
  return m;
}

__device__ __forceinline__ bool num_start(uint32_t c) {
  return (c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.';
}

/*!
 * \brief line-start / token-start masks of the 16 bytes v at chunk offset pos;
 *  pc = the byte before pos ('\n' at 0).  Bytes at or past n are invalid.
 *  kCheck: also return true when the lane saw an irregular construct (a
 *  control byte other than \t \n \r, a line starting with a blank, a token
 *  starting outside [0-9+-.]).
 */
template <bool kCheck, bool kFull = false, bool kCheckTokens = true>
__device__ __forceinline__ bool lane_masks(uint4 v, uint32_t pc, size_t pos, size_t n,
                                           uint32_t* lm, uint32_t* tm) {
  uint32_t sep, eol, ctl;
  classify16(v, &sep, &eol, &ctl);
  const uint32_t prev_eol = (pc == '\n' || pc == '\r') ? 1u : 0u;
  const uint32_t prev_sep = (prev_eol || pc == ' ' || pc == '\t') ? 1u : 0u;
  uint32_t valid = 0xFFFFu;  // kFull: all 16 bytes are before n (no 64-bit compares)
  if (kFull) {
  } else if (pos >= n) {
    valid = 0;
  } else if (n - pos < 16) {
    valid = (1u << (n - pos)) - 1u;
  }
  *lm = ~eol & ((eol << 1) | prev_eol) & valid & 0xFFFFu;
  *tm = ~sep & ((sep << 1) | prev_sep) & valid & 0xFFFFu;
  if (!kCheck) return false;
  bool bad = (*lm & ~*tm) != 0;  // a line that starts with a blank
  uint32_t t = kCheckTokens ? *tm : 0u;  // (else: the decoder's fallback flags them)
  while (t != 0) {
    const int j = __ffs(t) - 1;
    t &= t - 1;
    bad |= !num_start(dev::vec_byte(v, j));
  }
  uint32_t c = ctl & valid;
  while (c != 0) {
    const int j = __ffs(c) - 1;
    c &= c - 1;
    bad |= !((0x2600u >> dev::vec_byte(v, j)) & 1u);  // only \t \n \r
  }
  return bad;
}

/*! \brief the byte before this lane's 16 bytes of load j of a tile held in
 *  v[]: lane - 1's last byte, for lane 0 lane 63's of load j - 1 (`first`, the
 *  byte before the tile, for load 0).  Every lane calls it (cross-lane reads) */
__device__ __forceinline__ uint32_t count_prev(const uint4* v, int j, uint32_t first, int lane) {
  const uint32_t left = dev::lane_shr1(v[j].w >> 24);
  const uint32_t wrap = j == 0 ? first : dev::lane63(v[j - 1].w >> 24);
  return lane == 0 ? wrap : left;
}

/*!
 * \brief C1 lane step: line / token starts of 16 bytes as per-byte high-bit
 *  masks (bit 7 of byte j), gathered into 16-bit masks by byte dot products
 *  and popcounted once per 16 bytes, plus the irregular checks of
 *  lane_masks<true>.  pc: the byte before the 16.
 */
template <bool kFull>
__device__ __forceinline__ bool count16(uint4 v, uint32_t pc, size_t pos, size_t n,
                                        uint32_t* lines, uint32_t* toks, uint32_t* qtoks,
                                        uint32_t* packed) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  // the token / line start masks in the fill's form (bit j = byte j of the 16,
  // token starts in bits 0..15, line starts in 16..31): byte dot products
  // gather the per-byte high bits (0x80 = 128 x the weight), two words per
  // accumulator
  uint32_t acc_t[2] = {0u, 0u}, acc_l[2] = {0u, 0u};
  // bytes at or past n are "separators" (no starts there); kFull: the whole
  // tile lies before n (every tile but a chunk's last), no per-word masks
  const size_t room = kFull ? 16 : (pos >= n ? 0 : (n - pos < 16 ? n - pos : 16));
  uint32_t prev_sep = (pc <= 0x20u) ? 0x80u : 0u;  // sep bit of the byte before, at bit 7
  uint32_t prev_eol = (pc == '\n' || pc == '\r') ? 0x80u : 0u;
  bool bad = false;
  uint32_t blank = 0;  // line starts that are no token starts (a line starting with a blank)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t x = w[i];
    const uint32_t lo7 = x & 0x7F7F7F7Fu;
    const uint32_t le20 = ~((lo7 + 0x5F5F5F5Fu) | x) & 0x80808080u;
    const uint32_t lt20 = ~((lo7 + 0x60606060u) | x) & 0x80808080u;
    const uint32_t b6 = ((x & 0x06060606u) + 0x7E7E7E7Eu) & 0x80808080u;
    const int valid_bytes = static_cast<int>(room) - 4 * i;
    const uint32_t valid = valid_bytes >= 4 ? 0x80808080u
                           : (valid_bytes <= 0 ? 0u : (0x80808080u >> (8 * (4 - valid_bytes))));
    const uint32_t sep = le20 | (~valid & 0x80808080u);
    const uint32_t eol = le20 & b6;
    const uint32_t sep_before = (sep << 8) | prev_sep;
    const uint32_t eol_before = (eol << 8) | prev_eol;
    const uint32_t tm = ~sep & sep_before & 0x80808080u;
    const uint32_t lm = ~eol & eol_before & valid & 0x80808080u;
    // tokens starting with a letter (byte bit 6 set; digits, signs and '.'
    // have it clear) are no entries of the CSR: LibSVM `qid:` tokens, which
    // the fill decodes beside its list, or junk that sends the chunk to the
    // exact kernels.  Bit 6 of each byte, moved to bit 7: x << 1.
    *qtoks += __popc(tm & (x << 1));
    // the starts gathered into the 16-bit masks by byte dot products (0x80 =
    // 128 x the weight, two words per accumulator); the token / line counts
    // are their popcounts, once per 16 bytes
    const uint32_t wgt = (i & 1) ? 0x80402010u : 0x08040201u;
    acc_t[i >> 1] = __builtin_amdgcn_udot4(tm, wgt, acc_t[i >> 1], false);
    acc_l[i >> 1] = __builtin_amdgcn_udot4(lm, wgt, acc_l[i >> 1], false);
    blank |= lm & ~tm;
    // (token starts outside [0-9+-.] are flagged by the fill / hash kernels:
    // such a token never passes the register-window decoder, so the check
    // costs nothing on the fast path -- here it was ~40% of the count's VALU)
    // control bytes other than \t \n \r: rare (line ends), a short loop is cheaper
    // than three more byte tests per word (measured: 88.5 vs 103.5 us per call)
    uint32_t c = lt20 & valid;
    while (c != 0) {
      const int j = (__ffs(c) - 1) >> 3;
      c &= c - 1;
      bad |= !((0x2600u >> ((x >> (8 * j)) & 0xFFu)) & 1u);
    }
    prev_sep = (sep >> 24) & 0x80u;
    prev_eol = (eol >> 24) & 0x80u;
  }
  const uint32_t pt = (acc_t[0] >> 7) | (acc_t[1] << 1);  // token starts, bit j = byte j
  const uint32_t pl = (acc_l[0] >> 7) | (acc_l[1] << 1);  // line starts
  *toks += __popc(pt);
  *lines += __popc(pl);
  bad |= blank != 0;
  if (packed != nullptr) *packed = pt | (pl << 16);
  return bad;
}

/*! \brief line starts of 16 bytes (the lm of count16 alone); room: bytes before n */
template <bool kFull>
__device__ __forceinline__ uint32_t lines16(uint4 v, uint32_t pc, int room) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t prev_eol = (pc == '\n' || pc == '\r') ? 0x80u : 0u;
  uint32_t lines = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t x = w[i];
    const uint32_t lo7 = x & 0x7F7F7F7Fu;
    const uint32_t le20 = ~((lo7 + 0x5F5F5F5Fu) | x) & 0x80808080u;
    const uint32_t b6 = ((x & 0x06060606u) + 0x7E7E7E7Eu) & 0x80808080u;
    const uint32_t eol = le20 & b6;
    const int valid_bytes = room - 4 * i;
    const uint32_t valid = kFull || valid_bytes >= 4
                               ? 0x80808080u
                               : (valid_bytes <= 0 ? 0u : (0x80808080u >> (8 * (4 - valid_bytes))));
    lines += __popc(~eol & ((eol << 8) | prev_eol) & valid);
    prev_eol = (eol >> 24) & 0x80u;
  }
  return lines;
}

/*!
 * \brief copy the ChunkMeta to mapped pinned host memory, then raise its
 *  `pad` word (after a system-scope fence) so the host can poll for it
 *  instead of a blocking stream synchronise (DeviceParser::WaitMapped)
 */
__device__ __forceinline__ void publish_host_meta(ChunkMeta* host_meta, ChunkMeta m) {
  m.pad = 0;
  *host_meta = m;
  __threadfence_system();
  *reinterpret_cast<volatile unsigned*>(&host_meta->pad) = 1u;
}

/*! \brief the chunk's sizes as the last tile of a one-pass launch writes them
 *  (k_tile_finish, stream-ordered, adds the flags and maxima, writes the
 *  closing row pointer and publishes the meta) */
__device__ __forceinline__ ChunkMeta one_pass_meta(uint64_t nlines, uint64_t nnz) {
  ChunkMeta m;
  m.nlines = m.nrows = nlines;
  m.nnz = nnz;
  m.max_index = m.max_field = 0;
  m.flags = 0;
  m.pad = 0;
  return m;
}

/*!
 * \brief byte iterator whose end is "the next separator" (blank / EOL) or a
 *  hard limit.  strtonum.h's ParsePair / ParseTriple compare against an end
 *  iterator; a `sentinel` end makes them stop at the token's own end without
 *  knowing its length, so a token is parsed with one pass of byte loads
 *  (ds_read_u8 from the LDS tile, or global loads for the last token of a
 *  tile) instead of locating its end first.
 */
template <typename Ptr>
struct SepIter {
  Ptr p;
  Ptr limit;
  bool sentinel;
  __device__ __forceinline__ char operator*() const { return static_cast<char>(*p); }
  __device__ __forceinline__ SepIter& operator++() {
    ++p;
    return *this;
  }
  __device__ __forceinline__ bool at_end() const {
    if (p >= limit) return true;
    const uint8_t c = *p;
    return c == ' ' || c == '\t' || c == '\n' || c == '\r';
  }
  __device__ __forceinline__ bool operator!=(const SepIter& o) const {
    return o.sentinel ? !at_end() : p != o.p;
  }
  __device__ __forceinline__ bool operator==(const SepIter& o) const { return !(*this != o); }
};

template <typename Ptr>
__device__ __forceinline__ SepIter<Ptr> sep_begin(Ptr p, Ptr limit) {
  return SepIter<Ptr>{p, limit, false};
}
template <typename Ptr>
__device__ __forceinline__ SepIter<Ptr> sep_end(Ptr limit) {
  return SepIter<Ptr>{limit, limit, true};
}

/*!
 * \brief generic (strtonum.h ParsePair / ParseTriple) parse of the token at
 *  global offset gpos: tokens the register-window decoder does not cover.
 *  Out of line: it is rare, and inlined it would raise the register
 *  allocation of the whole fill kernel.
 */
struct GenericResult {
  tok::Token t;
  bool bad;
};

template <TextFormat F, typename IndexType>
__device__ __noinline__ GenericResult generic_token(const uint8_t* __restrict__ text, size_t n,
                                                    size_t gpos, bool is_label) {
  GenericResult res;
  tok::Token* const t = &res.t;
  bool* const bad = &res.bad;
  t->u0 = t->u1 = t->u0_hi = t->u1_hi = 0;
  t->f0 = t->f1 = 0.0f;
  const uint8_t* lim = text + n;
  auto beg = sep_begin(text + gpos, lim);
  auto end = sep_end(lim);
  float f0 = 0.0f, f1 = 0.0f;
  *bad = false;
  if (is_label) {
    t->r = data::ParsePair<float, float>(beg, end, &f0, &f1, bad);
    t->f0 = f0;
    t->f1 = f1;
  } else if constexpr (F == TextFormat::kLibSVM) {
    IndexType idx = 0;
    t->r = data::ParsePair<IndexType, float>(beg, end, &idx, &f0, bad);
    t->u0 = static_cast<uint32_t>(idx);
    t->u0_hi = static_cast<uint32_t>(static_cast<uint64_t>(idx) >> 32);
    t->f0 = f0;
  } else {
    IndexType fid = 0, idx = 0;
    t->r = data::ParseTriple<IndexType, IndexType, float>(beg, end, &fid, &idx, &f0, bad);
    t->u0 = static_cast<uint32_t>(fid);
    t->u0_hi = static_cast<uint32_t>(static_cast<uint64_t>(fid) >> 32);
    t->u1 = static_cast<uint32_t>(idx);
    t->u1_hi = static_cast<uint32_t>(static_cast<uint64_t>(idx) >> 32);
    t->f0 = f0;
  }
  return res;
}

/*!
 * \brief a letter-started token at chunk offset gp: true when it is the
 *  row's `qid:` token -- the second token of its line (only blanks and one
 *  token, the label, between the line start and it) spelled `qid:` + integer
 *  (the CPU parser's grammar, src/data/libsvm_parser.h) -- and *qid its
 *  value.  Anything else is for the exact kernels.  Rare path: byte loads from
 *  global memory (L2-resident text).
 */
struct QidResult {
  uint64_t value;
  bool ok;
};

__device__ __noinline__ QidResult qid_token(const uint8_t* __restrict__ text, size_t n, size_t gp) {
  QidResult r{0, false};
  auto blank = [](uint32_t c) { return c == ' ' || c == '\t'; };
  auto eol = [](uint32_t c) { return c == '\n' || c == '\r'; };
  if (gp + 4 > n || text[gp] != 'q' || text[gp + 1] != 'i' || text[gp + 2] != 'd' ||
      text[gp + 3] != ':') {
    return r;
  }
  // backward: blanks, then the label token, then the line start
  size_t p = gp;
  while (p > 0 && blank(text[p - 1])) --p;
  if (p == 0 || p == gp || eol(text[p - 1])) return r;  // no label before it
  while (p > 0 && !blank(text[p - 1]) && !eol(text[p - 1])) --p;
  if (p != 0 && !eol(text[p - 1])) return r;  // another token before the label
  // the value: StrToInt<int64_t> over the token's bytes after "qid:"
  size_t q = gp + 4;
  bool neg = false;
  if (q < n && (text[q] == '-' || text[q] == '+')) {
    neg = text[q] == '-';
    ++q;
  }
  uint64_t v = 0;
  for (int k = 0; k < 20 && q < n && text[q] >= '0' && text[q] <= '9'; ++k, ++q) {
    v = v * 10 + (text[q] - '0');
  }
  if (q < n && !blank(text[q]) && !eol(text[q])) return r;  // junk after the digits
  r.value = neg ? 0 - v : v;
  r.ok = true;
  return r;
}

/*!
 * \brief the `qid:` token at staged LDS byte a (the 32 bytes from a are
 *  staged: a step slot holds 64 bytes past the step), same grammar as
 *  qid_token; a zero byte (past the text end) ends the digits like the end of
 *  the text does.
 */
__device__ __forceinline__ QidResult qid_lds(const uint4* lds, uint32_t a) {
  QidResult r{0, false};
  const uint3 g = tok::ext12(lds, a);
  if (g.x != 0x3A646971u) return r;  // "qid:"
  const uint32_t c0 = g.y & 0xFFu;
  const bool neg = c0 == '-';
  const uint32_t s = (neg || c0 == '+') ? 1u : 0u;
  // the digits 8 at a time (digit_run8); 16 or more: the byte loop below
  const uint3 d1 = tok::ext12(lds, a + 4u + s);
  const tok::Run8 r1 = tok::digit_run8(d1.x, d1.y, d1.z & 0xFFu);
  uint64_t v = r1.val;
  uint32_t term = r1.term;
  if (r1.k == 8u) {
    const uint3 d2 = tok::ext12(lds, a + 12u + s);
    const tok::Run8 r2 = tok::digit_run8(d2.x, d2.y, d2.z & 0xFFu);
    if (r2.k == 8u) {
      // 16+ digits (StrToInt over up to 20, wrapping): byte by byte
      const uint4 g0 = tok::ext16(lds, a), g1 = tok::ext16(lds, a + 16);
      uint32_t i = 4u + s;
      v = 0;
      for (int k = 0; k < 20; ++k, ++i) {
        const uint32_t c = tok::win_byte(g0, g1, i);
        if (c - '0' > 9u) break;
        v = v * 10 + (c - '0');
      }
      term = tok::win_byte(g0, g1, i);
    } else {
      v = v * tok::pow10_u(r2.k) + r2.val;
      term = r2.term;
    }
  }
  if (term != ' ' && term != '\t' && term != '\n' && term != '\r' && term != 0) return r;
  r.value = neg ? 0 - v : v;
  r.ok = true;
  return r;
}

/*! \brief status of the last token start of a 16-byte slice: 0 none, 2 a token
 *  that does not start a line, 3 one that does (a label) */
__device__ __forceinline__ uint32_t slice_last(uint32_t tm, uint32_t lm) {
  return tm != 0 ? 2u | ((lm >> (31 - __builtin_clz(tm))) & 1u) : 0u;
}

/*!
 * \brief for a `qid:` token start: the status of the token start before it --
 *  a `qid:` is the line's second token iff that one starts the line (3).
 *  Slices of a step in text order are all lanes' a slices, then the b slices;
 *  `carried` is the status at the step start (0: no token yet in this tile,
 *  then the global-memory check decides).  Wave-uniform call.
 */
struct PrevTok {
  uint32_t a, b;
};
__device__ __forceinline__ PrevTok prev_token_status(uint32_t tm_a, uint32_t lm_a, uint32_t tm_b,
                                                     uint32_t lm_b, uint32_t carried, int lane) {
  // inclusive max over lanes <= lane: the DPP ladder (no LDS round trips)
  auto scan = [](uint32_t v) {
    return dev::wave_incl_scan_op(v, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
  };
  const uint32_t ia = scan(tm_a != 0 ? ((lane + 1u) << 2) | slice_last(tm_a, lm_a) : 0u);
  const uint32_t ib = scan(tm_b != 0 ? ((lane + 1u) << 2) | slice_last(tm_b, lm_b) : 0u);
  const uint32_t xa = dev::lane_shr1(ia), xb = dev::lane_shr1(ib);  // lane 0: 0
  const uint32_t ta = dev::lane63(ia);
  PrevTok r;
  r.a = xa != 0 ? (xa & 3u) : carried;
  r.b = xb != 0 ? (xb & 3u) : (ta != 0 ? (ta & 3u) : carried);
  return r;
}

/*! \brief the status after a step (its last token start's), or `carried` */
__device__ __forceinline__ uint32_t step_last_status(uint32_t tm_a, uint32_t lm_a, uint32_t tm_b,
                                                     uint32_t lm_b, uint32_t carried) {
  const uint64_t bb = __ballot(tm_b != 0), ba = __ballot(tm_a != 0);
  const uint32_t sb = __builtin_amdgcn_readlane(slice_last(tm_b, lm_b),
                                                bb ? 63 - __builtin_clzll(bb) : 0);
  const uint32_t sa = __builtin_amdgcn_readlane(slice_last(tm_a, lm_a),
                                                ba ? 63 - __builtin_clzll(ba) : 0);
  // wave-uniform: kept in a scalar register
  return __builtin_amdgcn_readfirstlane(bb ? sb : (ba ? sa : carried));
}

/*! \brief status of the token start before bit j of a slice, given the status
 *  before the slice */
__device__ __forceinline__ uint32_t status_before(uint32_t tm, uint32_t lm, uint32_t j,
                                                  uint32_t before_slice) {
  const uint32_t inside = tm & ((1u << j) - 1u);
  return inside != 0 ? slice_last(inside, lm) : before_slice;
}

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

/*! \brief a buffer resource over the text from base on (raw, gfx9 dword3):
 *  the address lives in scalar registers, loads take a 32-bit lane offset.
 *  The range check zeroes whole dwords past num_records, so the record count
 *  is the text rounded up to 16 bytes (every 16-byte load that starts inside
 *  the text returns all its bytes; text buffers carry kTextPadBytes of
 *  padding) and the caller zeroes the bytes past the text (clip16). */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t text_rsrc(const uint8_t* base, size_t avail) {
  const size_t up = (avail + 15) & ~static_cast<size_t>(15);
  const uint32_t nr = up > 0xFFFFFFF0ull ? 0xFFFFFFF0u : static_cast<uint32_t>(up);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, nr, 0x00020000);
}

/*! \brief the 16 bytes at byte voff of a text_rsrc (zeros past its records).
 *  The whole offset goes in voffset: the range check does not cover soffset */
__device__ __forceinline__ uint4 bload16(__amdgpu_buffer_rsrc_t r, uint32_t voff) {
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

/*! \brief the published start masks from tile `tile` on (C1's [tile][step][lane]
 *  uint2 words), as a buffer resource: per step one 8-byte load whose lane
 *  offset is fixed and whose step offset is scalar (no address VALU) */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mask_rsrc(const uint32_t* masks, size_t tile,
                                                            size_t ntiles) {
  const size_t words = (ntiles - tile) * (kTileBytes / 16);
  const size_t bytes = words * 4 > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : words * 4;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(masks) + tile * (kTileBytes / 16),
                                           0, static_cast<uint32_t>(bytes), 0x00020000);
}

/*! \brief step s's two slice masks of this lane (x: slice a, y: slice b) */
__device__ __forceinline__ uint2 load_masks(__amdgpu_buffer_rsrc_t r, uint32_t lane_off, int s) {
  const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(r, lane_off, s * dev::kWave * 8, 0);
  return make_uint2(v.x, v.y);
}

/*! \brief v (the 16 bytes at pos) with the bytes at or past n zeroed */
__device__ __forceinline__ uint4 clip16(uint4 v, size_t pos, size_t n) {
  const uint32_t keep = pos < n ? static_cast<uint32_t>(n - pos < 16 ? n - pos : 16) : 0u;
  const uint64_t m_lo = keep >= 8 ? ~0ull : ((1ull << (8 * keep)) - 1ull);
  const uint64_t m_hi = keep >= 16 ? ~0ull : (keep <= 8 ? 0ull : ((1ull << (8 * (keep - 8))) - 1ull));
  return make_uint4(v.x & static_cast<uint32_t>(m_lo), v.y & static_cast<uint32_t>(m_lo >> 32),
                    v.z & static_cast<uint32_t>(m_hi), v.w & static_cast<uint32_t>(m_hi >> 32));
}

/*!
 * \brief append the token starts of one lane's 16 B slice to the wave's list
 *  (`at` = its first list position; `line0` = line starts of the tile before
 *  this slice).  An entry is  staging offset (13 bits: slot * kSlotBytes +
 *  byte in the step) | line start (bit 13) | line ordinal in the tile, this
 *  token's line included (bits 14..26), so a round can take the entries in
 *  any lane order and a token can be decoded a step after it was listed.
 *  The first two starts are written unconditionally -- a lane with fewer
 *  writes a private dummy slot past kListCap -- so the common case has no
 *  per-lane loop; slices with more starts (tokens shorter than 8 B) take the
 *  loop.
 */
__device__ __forceinline__ uint32_t list_entry(uint32_t tm_bit_j, uint32_t lm, uint32_t base,
                                               uint32_t line0) {
  const uint32_t j = tm_bit_j;
  const uint32_t upto = lm & ((2u << j) - 1u);  // line starts up to byte j of the slice
  return (base + j) | (((lm >> j) & 1u) << 13) | ((line0 + __popc(upto)) << 14);
}

template <uint32_t kCap = kListCap>
__device__ __forceinline__ void list_slice(uint32_t* sl, uint32_t tm, uint32_t lm, uint32_t at,
                                           uint32_t base, uint32_t line0, int lane) {
  uint32_t m = tm;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t j = static_cast<uint32_t>(__builtin_ctz(m | 0x10000u));
    const bool has = m != 0;
    sl[has ? at : kCap + lane] = list_entry(j & 15u, lm, base, line0);  // (the list holds kCap + 64)
    at += has ? 1u : 0u;
    m &= m - 1;
  }
  if (__any(m != 0)) {
    for (; m != 0; m &= m - 1) {
      sl[at++] = list_entry(static_cast<uint32_t>(__builtin_ctz(m)), lm, base, line0);
    }
  }
}

/*!
 * \brief token slot of `lane` in a decode round: the four 16-lane groups of a
 *  ds_read_b128 ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32)
 *  take 16 consecutive tokens each, which start ~16 B apart -- distinct bank
 *  quads, where lane-ordered slots put tokens 256 B apart into one group
 */
__device__ __forceinline__ uint32_t round_slot(int lane) {
  // rank within its group + 16 * group, for lanes 0..31 (4 bits per entry)
  const uint32_t l = static_cast<uint32_t>(lane) & 31u;
  uint32_t k;
  if (l < 4) {
    k = l;
  } else if (l < 12) {
    k = 16u + (l - 4u);
  } else if (l < 16) {
    k = 4u + (l - 12u);
  } else if (l < 20) {
    k = 24u + (l - 16u);
  } else if (l < 28) {
    k = 8u + (l - 20u);
  } else {
    k = 28u + (l - 28u);
  }
  return (static_cast<uint32_t>(lane) & 32u) + k;
}
}  // namespace

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_GPU_TILE_COMMON_H_
