/*!
 * \file src/gpu/tile_fill_kernels.hip
 * \brief the tile parser's C3 in both forms: k_tile_fill, text tiles to CSR,
 *  and k_tile_hash, text tiles to hashed dense rows (tile_common.h has the
 *  overview).  The two stay in one translation unit: they share the
 *  out-of-line tok::decode_ext, qid_token and generic_token, and the compiler
 *  shapes those bodies (constant arguments, unused results) by the callers it
 *  sees -- alone, k_tile_hash gets other callees and another register
 *  allocation (profiles/tile_split).
 *
 *  C3 k_tile_fill  (one wave per tile, no workgroup barrier): streams the tile
 *     in 2 KiB steps through two LDS slots (step s and s - 1) with the next
 *     step prefetched in registers, lists every token (staging offset, line
 *     start bit, tile line ordinal) in a wave-private LDS list, and decodes
 *     whole 64-token rounds only -- a step's remainder waits for the next
 *     step's rounds.  Lane i decodes token i from two aligned ds_read_b128 in
 *     registers (token_decode.h: integer fields with parse_int, values with
 *     parse_num; anything else through strtonum.h's ParsePair / ParseTriple
 *     from global memory, bit-identical to the CPU parser) and stores index /
 *     value / label / offset directly.  K8 (max index / field, flags) is a
 *     per-wave slot.
 */
#include <dmlc/gpu/hip_utils.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "./device_common.h"
#include "./kernels.h"
#include "./tile_common.h"
#include "./token_decode.h"

namespace dmlc {
namespace gpu {

namespace {
/*! \brief the one-pass fill's look-back state (kOnePass) */
struct FillPass {
  LookBack lb;                  // status: zeroed before the launch
  ChunkMeta* meta;              // nlines / nrows / nnz of the chunk (the last tile writes them)
  uint32_t exp;                 // pricing experiments (DMLC_FILL_EXP in a DMLC_PRICING build):
                                // 1 no CSR stores, 2 no token decode (outputs are wrong)
  const uint32_t* masks;        // counted path: C1's start masks (TileMaskWords)
};

/*!
 * \brief C3: wave-autonomous tile fill.  Each wave of the workgroup owns one
 *  8 KiB tile and never synchronises with the others (no __syncthreads):
 *   1. all 8 KiB (+ the 64 bytes after it) are loaded into registers at once;
 *   2. per 2 KiB step the step is staged in the wave's LDS region, the
 *      line / token start masks of each lane's two 16 B slices come from the
 *      same registers, and a wave scan (DPP) places each token's LDS offset
 *      (and its line-start bit) in a wave-private list, in text order;
 *   3. 64 list entries at a time, lane i decodes token i from the LDS text in
 *      registers (token_decode.h: two aligned ds_read_b128 per number), its
 *      line ordinal comes from a ballot of the line-start bits, and it writes
 *      index / value (consecutive lanes -> consecutive nnz slots) or label /
 *      offset / weight directly.
 *  Tokens the fast decoder does not take use the generic strtonum.h parser
 *  from global memory (bit-identical by construction).
 */
// kLean: a target without qid / weight columns (the common case) compiled on
// its own -- no qid pass, no weight stores, one flag for "weights seen": the
// scalar registers those held are what the kernel spilled to VGPR lanes (it
// sits at the SGPR limit)
template <TextFormat F, typename IndexType, bool kOnePass, bool kLean = false>
__global__ __launch_bounds__(kThreads, DMLC_FILL_WAVES) void k_tile_fill(
    const uint8_t* __restrict__ text, size_t n, size_t ntiles, const uint64_t* __restrict__ prefix,
    FillTarget<IndexType> out, MetaPartial* __restrict__ partials, FillPass op) {
  __shared__ uint4 s_text[kFillWaves][kStageVecs];
  __shared__ uint32_t s_list[kFillWaves][kListCap + 64];  // + a dummy slot per lane
  __shared__ uint32_t s_dq[kFillWaves][kQueueCap];  // deferred tokens: list index ring
  // wave-uniform in a scalar register: the tile's buffer resource stays scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / dev::kWave);
  const int lane = dev::lane_id();
  size_t group = blockIdx.x;
  if constexpr (kOnePass) group = dev::ticket_group(op.lb.ticket, op.lb.ticket0);  // tiles in ticket order
  const size_t tile = group * kFillWaves + wave;
  if (tile >= ntiles) return;  // whole waves leave; nothing below synchronises waves
  uint4* const st = s_text[wave];
  uint32_t* const sl = s_list[wave];
  uint32_t* const dq = s_dq[wave];
  uint32_t qh = 0, qn = 0;  // queue head, queued tokens
  const uint32_t slot = round_slot(lane);
  const size_t tile0 = tile * kTileBytes;

  // ---- 1. the first step in flight.  Each step's loads go into the previous
  // step's registers once its masks are built (no register copies of loads
  // in flight, so no wait right behind the load), and the tail a step stages
  // -- the next step's first 64 B -- is loaded one step ahead in `t`.  Bytes
  // at or past n are zeroed where a step is staged (buffer loads past the
  // resource return zeros; clip16 handles the last partial dword).
  const __amdgpu_buffer_rsrc_t trs = text_rsrc(text + tile0, n - tile0);
  const uint32_t loff = static_cast<uint32_t>(lane) * 16;
  uint4 a = bload16(trs, loff);
  uint4 b = bload16(trs, loff + 1024);
  uint4 t = make_uint4(0, 0, 0, 0);
  if (!kOnePass && lane < 4) t = bload16(trs, loff + kStepBytes);
  // counted path: the step's start masks come from C1 (published per 16 B),
  // not from classifying the bytes again; one pass classifies here
  __amdgpu_buffer_rsrc_t mrs;
  const uint32_t moff = static_cast<uint32_t>(lane) * 8;
  uint2 mk = make_uint2(0, 0);
  if constexpr (!kOnePass) {
    mrs = mask_rsrc(op.masks, tile, ntiles);
    mk = load_masks(mrs, moff, 0);
  }
  uint32_t carry_pc = 0;
  if constexpr (kOnePass) carry_pc = tile0 == 0 ? static_cast<uint32_t>('\n') : text[tile0 - 1];
  uint64_t line_base, tok_base;
  unsigned count_flags = 0;  // one pass: what C1 would have flagged for this tile
  if constexpr (kOnePass) {
    // C1 in the fill: the tile's 8 KiB in flight at once (the steps below
    // re-read 2 KiB at a time, from L2), line / entry starts and the
    // irregular checks counted, then the look-back for the tiles before it
    uint4 v[kCountLoads];
    v[0] = a;
    v[1] = b;
#pragma unroll
    for (int j = 2; j < kCountLoads; ++j) v[j] = bload16(trs, loff + j * 1024);
    if (lane < 4) t = v[2];  // step 0's tail (the 64 B after it) is already here
    uint32_t lines = 0, toks = 0, qtoks = 0;
    bool bad = false;
    auto count_tile = [&](auto full) {
#pragma unroll
      for (int j = 0; j < kCountLoads; ++j) {
        const uint32_t pc = count_prev(v, j, carry_pc, lane);
        // (C1's packed masks, unused here.  Passed all the same: with only null
        // callers in this file count16 is specialised before it is inlined and
        // the kernel's register allocation moves)
        uint32_t m;
        bad |= count16<decltype(full)::value>(v[j], pc, tile0 + j * 1024 + lane * 16, n, &lines,
                                              &toks, &qtoks, &m);
      }
    };
    if (tile0 + kTileBytes <= n) {  // wave-uniform: every tile but a chunk's last
      count_tile(std::true_type{});
    } else {
      count_tile(std::false_type{});
    }
    lines = dev::wave_sum(lines);
    const uint32_t ent = dev::wave_sum(toks - qtoks);  // letter tokens are no entries
    qtoks = dev::wave_sum(qtoks);
    count_flags = (__any(bad) ? kFlagIrregular : 0u) | (qtoks != 0 ? kFlagQid : 0u);
    const uint64_t own = (static_cast<uint64_t>(lines) << 31) | ent;
    // (lines, entries) as a 31 / 31-bit pair: a chunk is < 2 GiB, so both are
    // <= bytes / 2 and the packed sums never carry
    const uint64_t excl = dev::lookback_pairs<31>(op.lb.status, tile, own, lane);
    line_base = excl >> 31;
    tok_base = excl & 0x7FFFFFFFull;
    if (tile + 1 == ntiles && lane == 0) {
      *op.meta = one_pass_meta(line_base + lines, tok_base + ent - (line_base + lines));
    }
  } else {
    const uint64_t pre = prefix[tile];
    line_base = pre >> 32;
    tok_base = pre & 0xffffffffull;
  }
  // token k = tok_base + i of line l = line_base + lcnt - 1 goes to nnz
  // position C + (i - lcnt); its row is R + lcnt - 1 (as k_tile_scan defines)
  const uint64_t C = out.nnz_base + tok_base - line_base;
  const uint64_t R = out.row_base + line_base;
  // rooms clamped to int32 (a tile's ordinals are < 2^13): 32-bit compares per token
  auto clamp32 = [](int64_t v) {
    return static_cast<int32_t>(v > INT32_MAX ? INT32_MAX : (v < INT32_MIN ? INT32_MIN : v));
  };
  const int32_t nnz_room =
      clamp32(static_cast<int64_t>(out.nnz_limit) - static_cast<int64_t>(C));
  const int32_t row_room =
      clamp32(static_cast<int64_t>(out.row_limit) - static_cast<int64_t>(R));
  const uint32_t nnz_room_u = nnz_room > 0 ? static_cast<uint32_t>(nnz_room) : 0u;
  IndexType* const idx_at = out.index + C;
  float* const val_at = out.value + C;
  IndexType* const fld_at = out.field != nullptr ? out.field + C : nullptr;
  float* const lab_at = out.label + R - 1;
  uint64_t* const off_at = out.offset + R - 1;
  float* const wgt_at = !kLean && out.weight != nullptr ? out.weight + R - 1 : nullptr;
  uint64_t* const qid_at = !kLean && out.qid != nullptr ? out.qid + R - 1 : nullptr;
  // the count pass saw 'q' token starts in this chunk (the host then enables
  // the qid column): only such chunks look for `qid:` tokens
  const bool qid_chunk = !kLean && F == TextFormat::kLibSVM && out.qid != nullptr;

  uint32_t tok0 = 0;   // tile token ordinal of list position 0
  uint32_t lcnt = 0;   // line starts of this tile so far
  uint32_t carry = 0;  // list entries left for the next step's rounds (listed, not decoded)
  uint32_t qid_prev = 0;  // status of the last token start so far (prev_token_status)
  // maxima in the index width (32-bit compares for u32 indices)
  using MaxT = typename std::conditional<sizeof(IndexType) == 4, uint32_t, uint64_t>::type;
  MaxT mx_index = 0, mx_field = 0;
  bool any_value = false, any_weight = false, irregular = false, neg = false, need_w = false;
  bool over = false;
  uint32_t sink = 0;  // pricing experiments only

#pragma unroll 1
  for (int s = 0; s < kSteps; ++s) {
    const bool last = s + 1 == kSteps;
    const size_t pos_a = tile0 + s * kStepBytes + lane * 16;
    if (tile0 + static_cast<size_t>(s + 1) * kStepBytes + 64 > n) {  // wave-uniform: the text ends here
      a = clip16(a, pos_a, n);
      b = clip16(b, pos_a + 1024, n);
      t = clip16(t, pos_a + kStepBytes, n);
    }
    // ---- 2. stage the step (+ the next 64 B) in slot s & 1 -- the other slot
    // still holds step s - 1 for the tokens carried from it -- and list its tokens
    const uint32_t sbase = (static_cast<uint32_t>(s) & 1u) * kSlotBytes;
    uint4* const ss = st + sbase / 16;
    ss[lane] = a;
    ss[64 + lane] = b;
    if (lane < 4) ss[128 + lane] = t;
    uint32_t lm_a, tm_a, lm_b, tm_b;
    if constexpr (kOnePass) {
      const uint32_t left_a = dev::lane_shr1(a.w >> 24);
      const uint32_t pc_a = lane == 0 ? carry_pc : left_a;
      const uint32_t left_b = dev::lane_shr1(b.w >> 24);
      // cross-lane reads run in every lane (a shuffle inside `lane == 0 ? :`
      // would execute with only lane 0 active and read an inactive lane)
      const uint32_t last_a = dev::lane63(a.w >> 24);
      const uint32_t pc_b = lane == 0 ? last_a : left_b;
      carry_pc = dev::lane63(b.w >> 24);
      if (tile0 + static_cast<size_t>(s + 1) * kStepBytes <= n) {  // wave-uniform: a full step
        (void)lane_masks<false, true>(a, pc_a, pos_a, n, &lm_a, &tm_a);
        (void)lane_masks<false, true>(b, pc_b, pos_a + 1024, n, &lm_b, &tm_b);
      } else {
        (void)lane_masks<false>(a, pc_a, pos_a, n, &lm_a, &tm_a);
        (void)lane_masks<false>(b, pc_b, pos_a + 1024, n, &lm_b, &tm_b);
      }
    } else {
      // C1's masks: the same starts (its blank / control checks passed)
      tm_a = mk.x & 0xFFFFu;
      lm_a = mk.x >> 16;
      tm_b = mk.y & 0xFFFFu;
      lm_b = mk.y >> 16;
    }
    // `qid:` tokens (C1 left them out of the entry counts): taken out of the
    // list here, decoded by their lane after the scan (wave-uniform test:
    // only chunks that have them pay)
    uint32_t qa = 0, qb = 0;
    if (qid_chunk) {
      qa = tm_a & letter_mask(a);
      qb = tm_b & letter_mask(b);
      tm_a &= ~qa;
      tm_b &= ~qb;
    }
    // a, b, t (and the masks) are consumed: the next step's loads go straight into them
    if (!last) {
      const uint32_t so = static_cast<uint32_t>(s + 1) * kStepBytes;
      a = bload16(trs, loff + so);
      b = bload16(trs, loff + so + 1024);
      if (lane < 4) t = bload16(trs, loff + so + kStepBytes);
      if constexpr (!kOnePass) mk = load_masks(mrs, moff, s + 1);
    }
    // one 64-bit scan of four 16-bit counts: tokens / lines of both slices
    const uint64_t cnt = static_cast<uint64_t>(__popc(tm_a)) |
                         (static_cast<uint64_t>(__popc(tm_b)) << 16) |
                         (static_cast<uint64_t>(__popc(lm_a)) << 32) |
                         (static_cast<uint64_t>(__popc(lm_b)) << 48);
    uint64_t tot;
    const uint64_t before = dev::wave_excl_scan_2x32(cnt, &tot);  // 16-bit fields: no carries
    const uint32_t ntok_a = static_cast<uint32_t>(tot & 0xFFFFu);
    const uint32_t ntok = ntok_a + static_cast<uint32_t>((tot >> 16) & 0xFFFFu);
    const uint32_t nline_a = static_cast<uint32_t>((tot >> 32) & 0xFFFFu);
    const uint32_t nline = nline_a + static_cast<uint32_t>(tot >> 48);
    list_slice(sl, tm_a, lm_a, carry + static_cast<uint32_t>(before & 0xFFFFu), sbase + lane * 16,
               lcnt + static_cast<uint32_t>((before >> 32) & 0xFFFFu), lane);
    list_slice(sl, tm_b, lm_b, carry + ntok_a + static_cast<uint32_t>((before >> 16) & 0xFFFFu),
               sbase + 1024 + lane * 16, lcnt + nline_a + static_cast<uint32_t>(before >> 48), lane);
    dev::wave_sync();  // the staged text and the list are visible to every lane
    if (qid_chunk) {
      if (__any((qa | qb) != 0)) {
        const PrevTok pv = prev_token_status(tm_a | qa, lm_a, tm_b | qb, lm_b, qid_prev, lane);
        const uint32_t lbase[2] = {lcnt + static_cast<uint32_t>((before >> 32) & 0xFFFFu),
                                   lcnt + nline_a + static_cast<uint32_t>(before >> 48)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          // token starts with the letter ones: a `qid:` after another letter
          // token is not the second token
          const uint32_t lmh = h == 0 ? lm_a : lm_b, tmh = h == 0 ? tm_a | qa : tm_b | qb;
          for (uint32_t m = h == 0 ? qa : qb; m != 0; m &= m - 1) {
            const uint32_t j = static_cast<uint32_t>(__builtin_ctz(m));
            // its row: the tile's line starts up to this byte (a line that
            // starts with 'q' has no label: exact kernels)
            const uint32_t lc = lbase[h] + static_cast<uint32_t>(__popc(lmh & ((2u << j) - 1u)));
            // the second token of its line: the token start before it is the
            // line's label (from the masks; the tile's first token: global check)
            const uint32_t prev = status_before(tmh, lmh, j, h == 0 ? pv.a : pv.b);
            QidResult q{0, false};
            if (prev == 3u) {
              q = qid_lds(st, sbase + static_cast<uint32_t>(h) * 1024 + lane * 16 + j);
            } else if (prev == 0u) {
              q = qid_token(text, n, pos_a + static_cast<size_t>(h) * 1024 + j);
            }
            // (lc 0: the tile's first, unfinished line -- the row before R)
            const bool ok = q.ok && ((lmh >> j) & 1u) == 0 &&
                            static_cast<int32_t>(lc) - 1 < row_room && qid_at != nullptr;
            if (ok) qid_at[lc] = q.value;
            irregular |= !ok;
          }
        }
      }
      qid_prev = step_last_status(tm_a | qa, lm_a, tm_b | qb, lm_b, qid_prev);
    }

    // ---- 3. decode 64 listed tokens per round.  Only whole rounds run: the
    // rest of this step's tokens (< 64) wait for the next step's rounds, so a
    // step does not pay a mostly idle last round; every older token is
    // decoded now (its slot is restaged next step), and the last step takes all
    const uint32_t total = carry + ntok;
    const uint32_t rest = total % dev::kWave < ntok ? total % dev::kWave : ntok;
    const uint32_t ndec = last ? total : total - rest;
    // a decoded token's outputs (every write is at a position derived from
    // the token / line ordinals, so deferred tokens may write later)
    auto emit = [&](bool active, uint32_t e, uint32_t i, const tok::Token& t, bool bad) {
      const bool is_label = active && ((e >> 13) & 1u) != 0;
      const uint32_t lc = e >> 14;
      const int32_t rel = static_cast<int32_t>(i) - static_cast<int32_t>(lc);
      const bool row_ok = static_cast<int32_t>(lc) - 1 < row_room;
      // rel < 0: the tile opens with a line that counts while its first token
      // does not start it -- a letter token taken out of the list (qid chunk),
      // or, in one pass (where no count pass has turned the chunk away), a
      // blank-started or blank-only line.  Both are flagged irregular; the
      // feature must not be stored, its unsigned byte offset below would
      // wrap.  One unsigned compare covers 0 <= rel < room.
      const bool nnz_ok = static_cast<uint32_t>(rel) < nnz_room_u;
      bool field_ok = true;
      if (F == TextFormat::kLibFM) field_ok = is_label || t.r >= 2;
      // past the target's rows / entries: with sizes from C1 + C2 that is a
      // C1 / C3 disagreement (irregular); one pass writes into the capacity
      // the host has and asks for more (kFlagOverflow: grow, run again)
      const bool room_ok = is_label ? row_ok : nnz_ok;
      irregular |= active & !is_label & !field_ok;
      if constexpr (kOnePass) {
        over |= active & !room_ok;
      } else {
        irregular |= active & !room_ok;
      }
      if (dev::pricing_exp(op.exp) & 1u) {
        // pricing: everything but the stores (the values stay live)
        sink ^= (active ? __float_as_uint(t.f0) ^ t.u0 ^ t.u1 : 0u) + static_cast<uint32_t>(i);
        return;
      }
      if (active & is_label & row_ok) {
        lab_at[lc] = t.f0;
        off_at[lc] = C + 1 + (static_cast<int64_t>(i) - static_cast<int64_t>(lc));
        if (wgt_at != nullptr) wgt_at[lc] = t.r == 2 ? t.f1 : 1.0f;
        // (qid: zero-filled by the host, the qid token's lane writes it)
      }
      if constexpr (!kLean) need_w |= active & is_label & (wgt_at == nullptr) & (t.r == 2);
      any_weight |= active & is_label & (t.r == 2);
      const bool feat = active & !is_label & nnz_ok & field_ok;
      const uint64_t u0 = (static_cast<uint64_t>(t.u0_hi) << 32) | t.u0;
      // (a feature's rel = i - lc is >= 0 and < 2^13: a 32-bit byte offset
      // from the SGPR base, no 64-bit address arithmetic per store)
      const uint32_t boff = static_cast<uint32_t>(rel) * static_cast<uint32_t>(sizeof(IndexType));
      const uint32_t voff = static_cast<uint32_t>(rel) * 4u;
      auto at = [](auto* base, uint32_t off) {
        using T = typename std::remove_pointer<decltype(base)>::type;
        return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off);
      };
      if constexpr (F == TextFormat::kLibSVM) {
        if (feat) {
          *at(idx_at, boff) = static_cast<IndexType>(u0);
          *at(val_at, voff) = t.r == 2 ? t.f0 : 1.0f;
        }
        any_value |= feat && t.r == 2;
        const MaxT iu = static_cast<MaxT>(static_cast<IndexType>(u0));
        mx_index = feat && iu > mx_index ? iu : mx_index;
      } else {
        const uint64_t u1 = (static_cast<uint64_t>(t.u1_hi) << 32) | t.u1;
        if (feat) {
          *at(fld_at, boff) = static_cast<IndexType>(u0);
          *at(idx_at, boff) = static_cast<IndexType>(u1);
          *at(val_at, voff) = t.r == 3 ? t.f0 : 1.0f;
        }
        any_value |= feat && t.r == 3;
        const MaxT iu = static_cast<MaxT>(static_cast<IndexType>(u1));
        const MaxT fu = static_cast<MaxT>(static_cast<IndexType>(u0));
        mx_index = feat && iu > mx_index ? iu : mx_index;
        mx_field = feat && fu > mx_field ? fu : mx_field;
      }
      neg |= active && bad;
    };
    // tokens the register-window decoder declines (exponents, long fractions,
    // anything for the generic parser) are queued (their list index, in a
    // ring) and decoded 64 at a time in rounds of their own, so a round with
    // one such token does not pay the long decoder for all 64 lanes; the
    // queue is drained before the slots it points into are restaged (by the
    // end of every step).  While 128 listed tokens remain a round decodes two
    // per lane (tok::decode2: two independent dependency chains per lane).
    auto enqueue = [&](bool defer, uint32_t li) {
      const uint64_t dm = __ballot(defer);
      if (dm != 0) {
        const uint32_t rank = static_cast<uint32_t>(__popcll(dm & ((1ull << lane) - 1ull)));
        if (defer) dq[(qh + qn + rank) & (kQueueCap - 1)] = li;
        qn += static_cast<uint32_t>(__popcll(dm));
      }
    };
    for (uint32_t r0 = 0;;) {
      const bool qround = qn >= static_cast<uint32_t>(dev::kWave) || (r0 >= ndec && qn != 0);
      if (!qround && r0 >= ndec) break;
      if (!qround && r0 + 2 * dev::kWave <= ndec) {  // wave-uniform: a pair round
        const uint32_t la = r0 + slot, lb = la + dev::kWave;
        const uint32_t ea = sl[la], eb = sl[lb];
        tok::Token ta, tb;
        ta.u0_hi = ta.u1_hi = tb.u0_hi = tb.u1_hi = 0;
        ta.u1 = tb.u1 = 0;
        bool oka, okb;
        if (dev::pricing_exp(op.exp) & 2u) {  // pricing: no decode
          ta.u0 = ea;
          tb.u0 = eb;
          ta.f0 = ta.f1 = tb.f0 = tb.f1 = 1.0f;
          ta.r = tb.r = 2;
          oka = okb = true;
        } else {
          tok::decode2<F>(st, ea & 0x1FFFu, eb & 0x1FFFu, ((ea >> 13) & 1u) != 0,
                          ((eb >> 13) & 1u) != 0, &ta, &tb, &oka, &okb);
        }
        enqueue(!oka, la);
        enqueue(!okb, lb);
        emit(oka, ea, tok0 + la, ta, false);
        emit(okb, eb, tok0 + lb, tb, false);
        r0 += 2 * dev::kWave;
        continue;
      }
      bool active;
      uint32_t e, i;
      tok::Token t;
      t.u0_hi = t.u1_hi = 0;
      t.u1 = 0;
      bool bad = false;
      if (!qround) {
        const uint32_t li = r0 + slot;
        active = li < ndec;
        e = active ? sl[li] : 0u;
        i = tok0 + li;
        const bool is_label = active && ((e >> 13) & 1u) != 0;
        // 0 in idle lanes: they decode harmless bytes
        const bool ok = tok::decode<F>(st, e & 0x1FFFu, is_label, &t);
        enqueue(active & !ok, li);
        active = active & ok;
        r0 += dev::kWave;
      } else {
        dev::wave_sync();  // queue entries visible
        const uint32_t cnt = qn < static_cast<uint32_t>(dev::kWave) ? qn : dev::kWave;
        active = slot < cnt;
        const uint32_t li = active ? dq[(qh + slot) & (kQueueCap - 1)] : 0u;
        qh += cnt;
        qn -= cnt;
        e = active ? sl[li] : 0u;
        i = tok0 + li;
        const bool is_label = active && ((e >> 13) & 1u) != 0;
        const uint32_t off = e & 0x1FFFu;
        bool ok = false;
        if (active) {
          const tok::ExtToken x = tok::decode_ext<F>(
              st, off, is_label, off >= kSlotBytes ? 2 * kSlotBytes : kSlotBytes);
          t = x.t;
          ok = x.ok;
        }
        if (active & !ok) {
          // the step a slot holds: s, or s - 1 for a carried token
          const uint32_t in_slot = off >= kSlotBytes ? 1u : 0u;
          const int step = in_slot == (static_cast<uint32_t>(s) & 1u) ? s : s - 1;
          // by value: result pointers into this frame would put t / bad on the
          // stack, with a scratch store + load (and a vmcnt(0) wait) every round
          const size_t gpos =
              tile0 + static_cast<size_t>(step) * kStepBytes + off - in_slot * kSlotBytes;
          const GenericResult g = generic_token<F, IndexType>(text, n, gpos, is_label);
          t = g.t;
          bad = g.bad;
          // qid:, comments, junk: the exact kernels own the reference semantics
          irregular |= !num_start(text[gpos]);
        }
      }
      emit(active, e, i, t, bad);
    }
    // the undecoded rest moves to the front of the list (all lanes read before any writes)
    const uint32_t left = total - ndec;
    const uint32_t moved = lane < static_cast<int>(left) ? sl[ndec + lane] : 0u;
    dev::wave_sync();
    if (lane < static_cast<int>(left)) sl[lane] = moved;
    tok0 += ndec;
    carry = left;
    lcnt += nline;
    dev::wave_sync();  // every lane is done with this step's text and list
  }
  unsigned fl = count_flags;
  if (sink == 0x9E3779B9u) fl |= kFlagIrregular;  // keeps a pricing run's values live
  if (any_value) fl |= kFlagValue;
  if (any_weight) fl |= kFlagWeight;
  if (irregular) fl |= kFlagIrregular;
  if (neg) fl |= kFlagNegIndex;
  if (kLean ? any_weight : need_w) fl |= kFlagNeedWeight;  // (lean: no weight column)
  if (over) fl |= kFlagOverflow;
  if (F == TextFormat::kLibFM) fl |= kFlagField;
  const unsigned long long mi = dev::wave_max(static_cast<unsigned long long>(mx_index));
  const unsigned long long mf = dev::wave_max(static_cast<unsigned long long>(mx_field));
  fl = dev::wave_or(fl);
  if (lane == 0) {
    MetaPartial p;
    p.max_index = mi;
    p.max_field = mf;
    p.flags = fl;
    p.pad = 0;
    partials[tile] = p;
  }
}
}  // namespace

template <typename IndexType>
size_t LaunchTileFill(const char* text, size_t nbytes, TextFormat format,
                      const uint64_t* tile_prefix, const uint32_t* tile_masks,
                      const FillTarget<IndexType>& out, MetaPartial* partials, ChunkMeta* meta,
                      ChunkMeta* host_meta, hipStream_t stream, const FillOnePass* one_pass) {
  const size_t ntiles = TileCount(nbytes);
  const uint8_t* t = reinterpret_cast<const uint8_t*>(text);
  const size_t groups = (ntiles + kFillWaves - 1) / kFillWaves;
  static const uint32_t exp = dev::pricing_env("DMLC_FILL_EXP");
  FillPass op{LookBack{nullptr, nullptr, 0ull}, meta, exp, tile_masks};
  CHECK(one_pass != nullptr || tile_masks != nullptr || ntiles == 0)
      << "LaunchTileFill: the counted path needs C1's tile_masks";
  if (one_pass != nullptr) {
    op.lb = *one_pass;
    // every look-back word starts "not yet" (cdna_hip_programming.md G16:
    // zero every polled word before every launch)
    DMLC_HIP_CHECK(hipMemsetAsync(op.lb.status, 0, ntiles * sizeof(uint64_t), stream));
  }
  if (ntiles != 0) {
    const dim3 grid(static_cast<unsigned>(groups));
#define DMLC_TILE_FILL(FMT, ONE, LEAN)                                                       \
  hipLaunchKernelGGL((k_tile_fill<FMT, IndexType, ONE, LEAN>), grid, dim3(kThreads), 0, stream, t, \
                     nbytes, ntiles, tile_prefix, out, partials, op)
    // counted path without qid / weight columns: the lean instantiation
    const bool lean = one_pass == nullptr && out.qid == nullptr && out.weight == nullptr;
    if (format == TextFormat::kLibFM) {
      if (one_pass != nullptr) {
        DMLC_TILE_FILL(TextFormat::kLibFM, true, false);
      } else if (lean) {
        DMLC_TILE_FILL(TextFormat::kLibFM, false, true);
      } else {
        DMLC_TILE_FILL(TextFormat::kLibFM, false, false);
      }
    } else if (one_pass != nullptr) {
      DMLC_TILE_FILL(TextFormat::kLibSVM, true, false);
    } else if (lean) {
      DMLC_TILE_FILL(TextFormat::kLibSVM, false, true);
    } else {
      DMLC_TILE_FILL(TextFormat::kLibSVM, false, false);
    }
#undef DMLC_TILE_FILL
  }
  LaunchTileFinish(partials, ntiles, meta, host_meta, out.offset, out.row_base, out.nnz_base, stream);
  return ntiles != 0 ? groups : 0;
}

template size_t LaunchTileFill<uint32_t>(const char*, size_t, TextFormat, const uint64_t*,
                                         const uint32_t*, const FillTarget<uint32_t>&, MetaPartial*,
                                         ChunkMeta*, ChunkMeta*, hipStream_t, const FillOnePass*);
template size_t LaunchTileFill<uint64_t>(const char*, size_t, TextFormat, const uint64_t*,
                                         const uint32_t*, const FillTarget<uint64_t>&, MetaPartial*,
                                         ChunkMeta*, ChunkMeta*, hipStream_t, const FillOnePass*);

// ---------------- the fused form: tokenize -> hash -> dense rows ----------------
namespace {
/*!
 * \brief decoupled look-back over per-tile line counts (one wave per tile):
 *  publish this tile's count, sum the predecessors' counts back to the first
 *  inclusive prefix (64 tiles per probe), publish the inclusive prefix, return
 *  the exclusive one.  Status word: tag (30 bits, one per launch, so the array
 *  needs no reset) << 34 | state (1: count, 2: inclusive) << 32 | value.
 *  Tiles run in ticket order (k_tile_hash), so every tile waited on is resident
 *  or done and the wait ends.
 */
__device__ __forceinline__ uint64_t lookback_lines(uint64_t* st, size_t tile, uint32_t own,
                                                   uint32_t tag, int lane) {
  const uint64_t tg = static_cast<uint64_t>(tag) << 34;
  if (lane == 0) {
    __hip_atomic_store(&st[tile], tg | ((tile == 0 ? 2ull : 1ull) << 32) | own, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tile == 0) return 0;
  uint64_t excl = 0;
  int64_t j = static_cast<int64_t>(tile) - 1;  // the nearest predecessor not summed yet
  for (;;) {
    const int64_t k = j - lane;
    const uint64_t v = k >= 0 ? __hip_atomic_load(&st[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : (tg | (2ull << 32));  // before the chunk: inclusive 0
    const uint32_t state = static_cast<uint32_t>(v >> 32) & 3u;
    const bool ready = (v >> 34) == tag && state != 0;
    const uint64_t inc = __ballot(ready && state == 2u);
    const uint64_t waiting = __ballot(!ready);
    const int first = inc != 0 ? __builtin_ctzll(inc) : dev::kWave - 1;
    const uint64_t need = first >= dev::kWave - 1 ? ~0ull : ((2ull << first) - 1ull);
    if ((waiting & need) != 0) {
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    excl += dev::wave_sum(lane <= first ? static_cast<uint32_t>(v) : 0u);
    if (inc != 0) break;
    j -= dev::kWave;
  }
  if (lane == 0) {
    __hip_atomic_store(&st[tile], tg | (2ull << 32) | (excl + own), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  return excl;
}

/*!
 * \brief fused tokenize -> hash -> dense row (BASELINE config 5) on the fill
 *  kernel's wave-autonomous pipeline.  Wave w OWNS the lines that start in its
 *  8 KiB tile (`own` of them, from the C2 prefix -- no per-tile host data):
 *   1. the tile streams through the two LDS slots in 2 KiB steps exactly as in
 *      k_tile_fill (register prefetch, SWAR masks, DPP scan, wave-private token
 *      list, 64-token decode rounds through tok::decode).  Only owned tokens
 *      are listed: the head of the tile (the rest of the previous tile's last
 *      line) and everything after the owned lines are masked out before the
 *      scan, in the first / last step only (wave-uniform test);
 *   2. the last owned line is followed past the tile end step by step until
 *      the next line start (or the end of the text) -- no extension cap and
 *      no fallback for long lines; steps after the first extension step
 *      prefetch only the 64 B tail (lines > 2 KiB past the tile are rare);
 *   3. every decoded feature adds +-value at bucket hash % dim of ONE f32 row
 *      in the wave's LDS (ds_add_f32); when a round moves past a line, that row
 *      is flushed: each lane reads a float4 per 256 columns (lane-interleaved,
 *      conflict-free), zeroes it, converts to OCP fp8 e4m3 (v_cvt_pk_fp8_f32)
 *      and stores 4 B -- 256 contiguous bytes per wave store, zero spans
 *      included, no separate memset pass.
 *  The label token's lane writes the label.  No CSR, no per-row LDS buffers
 *  per workgroup, no barrier.  Hash and bucket are K9's (dev::hash_u64), so
 *  the fp8 bytes equal tile CSR + K9.  Reference token loop:
 *  src/data/libfm_parser.h:36-93, libsvm_parser.h:36-99 (strtonum.h:266-303).
 */
struct HashTarget {
  void* x;            // [row_limit, dim] fp8 bytes or f32
  float* label;
  uint64_t row_base;  // global row of the chunk's first line
  uint64_t nlines;    // lines of the chunk (the C2 total; one-pass: unused)
  int dim;
  float scale;
  uint32_t seed;
  // one pass (no C1 / C2): line counts by look-back, rows checked against row_cap
  uint32_t tag;                 // this launch's status tag (!= 0)
  LookBack lb;                  // status: tagged words, never reset
  uint64_t row_cap;             // rows of x / label
  ChunkMeta* meta;              // nlines / nrows of the chunk (the last tile writes them)
  const uint32_t* masks;        // counted path: C1's start masks (TileMaskWords)
};

/*! \brief keep the token starts of a slice whose line ordinals are in [1, own];
 *  L0 = ordinal at the slice start (line starts before it, this tile) */
__device__ __forceinline__ uint32_t owned_tokens(uint32_t tm, uint32_t lm, uint32_t L0,
                                                 uint32_t own) {
  uint32_t m = tm;
  if (L0 == 0) m &= lm != 0 ? ~((lm & (0u - lm)) - 1u) : 0u;  // from the first line start on
  const uint32_t nl = static_cast<uint32_t>(__popc(lm));
  if (L0 + nl > own) {
    if (L0 > own) return 0u;
    uint32_t x = lm;
    for (uint32_t k = own - L0; k != 0; --k) x &= x - 1u;  // drop the starts still owned
    m &= (x & (0u - x)) - 1u;  // bytes before the first line start past `own`
  }
  return m;
}

template <TextFormat F, typename IndexType, bool kFP8, bool kOnePass>
__global__ __launch_bounds__(kThreads, DMLC_FILL_WAVES) void k_tile_hash(
    const uint8_t* __restrict__ text, size_t n, size_t ntiles,
    const uint64_t* __restrict__ prefix, HashTarget out, MetaPartial* __restrict__ partials) {
  // one staging slot and a list without carried entries: every step decodes
  // all its tokens, so the LDS per wave (+ the dim-wide f32 row) leaves room
  // for 4 workgroups per CU up to dim 1024
  __shared__ uint4 s_text[kFillWaves][kHashText / 16];
  __shared__ uint32_t s_list[kFillWaves][kHashListCap + 64];
  extern __shared__ __attribute__((aligned(16))) float s_hrow[];  // kFillWaves x dim
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / dev::kWave);
  const int lane = dev::lane_id();
  size_t group = blockIdx.x;
  if constexpr (kOnePass) group = dev::ticket_group(out.lb.ticket, out.lb.ticket0);  // tiles in ticket order
  const size_t tile = group * kFillWaves + wave;
  if (tile >= ntiles) return;  // whole waves leave; nothing below synchronises waves
  uint4* const st = s_text[wave];
  uint32_t* const sl = s_list[wave];
  const int dim = out.dim;
  float* const row = s_hrow + static_cast<size_t>(wave) * dim;
  const uint32_t slot = round_slot(lane);
  const size_t tile0 = tile * kTileBytes;
  const __amdgpu_buffer_rsrc_t trs = text_rsrc(text + tile0, n - tile0);
  const uint32_t loff = static_cast<uint32_t>(lane) * 16;
  uint4 a = bload16(trs, loff);
  uint4 b = bload16(trs, loff + 1024);
  // counted path: C1's start masks per step (steps past the tile read the
  // next tiles' words: the layout is contiguous over the chunk)
  __amdgpu_buffer_rsrc_t mrs;
  const uint32_t moff = static_cast<uint32_t>(lane) * 8;
  uint2 mk = make_uint2(0, 0);
  if constexpr (!kOnePass) {
    mrs = mask_rsrc(out.masks, tile, ntiles);
    mk = load_masks(mrs, moff, 0);
  }
  uint32_t carry_pc = 0;
  if constexpr (kOnePass) carry_pc = tile0 == 0 ? static_cast<uint32_t>('\n') : text[tile0 - 1];
  uint64_t line_base;
  uint32_t own;
  if constexpr (kOnePass) {
    // the C1 line count of this tile (its other 6 KiB come into L2 for the
    // steps), then the look-back for the lines before it
    uint4 v[kCountLoads];
    v[0] = a;
    v[1] = b;
#pragma unroll
    for (int j = 2; j < kCountLoads; ++j) v[j] = bload16(trs, loff + j * 1024);
    const bool full = tile0 + kTileBytes <= n;
    uint32_t lines = 0;
#pragma unroll
    for (int j = 0; j < kCountLoads; ++j) {
      const uint32_t pc = count_prev(v, j, carry_pc, lane);
      if (full) {
        lines += lines16<true>(v[j], pc, 16);
      } else {
        const size_t pos = tile0 + j * 1024 + lane * 16;
        const int room = pos >= n ? 0 : (n - pos < 16 ? static_cast<int>(n - pos) : 16);
        lines += lines16<false>(v[j], pc, room);
      }
    }
    own = dev::wave_sum(lines);
    line_base = lookback_lines(out.lb.status, tile, own, out.tag, lane);
    if (tile + 1 == ntiles && lane == 0) {
      *out.meta = one_pass_meta(line_base + own, 0);
    }
  } else {
    line_base = prefix[tile] >> 32;
    const uint64_t line_next = tile + 1 < ntiles ? prefix[tile + 1] >> 32 : out.nlines;
    own = static_cast<uint32_t>(line_next - line_base);
  }
  const uint64_t row_cap = kOnePass ? out.row_cap : ~0ull;
  bool irregular = false, neg = false, over = false;
  if (own != 0) {
    const uint64_t R = out.row_base + line_base;  // global row of tile line ordinal 1
    float* const lab_at = out.label + R - 1;      // labels by tile line ordinal
    const bool pow2 = (dim & (dim - 1)) == 0;
    const uint32_t dmask = static_cast<uint32_t>(dim - 1);
    for (int c = lane * 4; c < dim; c += dev::kWave * 4) {
      *reinterpret_cast<float4*>(row + c) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    // one row out: read + zero this lane's columns, convert, store
    auto flush = [&](uint32_t lc) {
      dev::wave_sync();  // the row's adds are done
      const uint64_t g = R + lc - 1;
      const bool ok = lc <= own && g < row_cap;
      over |= lc <= own && g >= row_cap;
      if constexpr (kFP8) {
        // lane-interleaved float4s (consecutive lanes, consecutive 16 B: no
        // bank conflicts on the b128 read / zero), 4 fp8 bytes per lane store
        uint8_t* o = static_cast<uint8_t*>(out.x) + g * static_cast<uint64_t>(dim);
#pragma unroll 4
        for (int c0 = 0; c0 < dim; c0 += dev::kWave * 4) {  // uniform trip count
          const int c = c0 + lane * 4;
          if (c < dim) {  // (no break: the loop exit stays uniform)
            float4* r4 = reinterpret_cast<float4*>(row + c);
            const float4 x = *r4;
            *r4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            int pk = __builtin_amdgcn_cvt_pk_fp8_f32(x.x * out.scale, x.y * out.scale, 0, false);
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(x.z * out.scale, x.w * out.scale, pk, true);
            if (ok) *reinterpret_cast<uint32_t*>(o + c) = static_cast<uint32_t>(pk);
          }
        }
      } else {
        float* o = static_cast<float*>(out.x) + g * static_cast<uint64_t>(dim);
        for (int c0 = 0; c0 < dim; c0 += dev::kWave * 4) {
          const int c = c0 + lane * 4;
          if (c < dim) {
            float4* r4 = reinterpret_cast<float4*>(row + c);
            const float4 x = *r4;
            *r4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ok) *reinterpret_cast<float4*>(o + c) = make_float4(x.x, x.y, x.z, x.w);
          }
        }
      }
      dev::wave_sync();  // zeros land before the next row's adds
    };

    // loads as in k_tile_fill: the next step's go into a / b / t once they are
    // consumed (no copies of loads in flight), clipped where staged
    uint4 t = make_uint4(0, 0, 0, 0);
    if (lane < 4) t = bload16(trs, loff + kStepBytes);
    uint32_t lcnt = 0;   // line starts seen so far (this tile's ordinals)
    uint32_t open = 0;   // ordinal of the row being accumulated (0: none yet)
    uint32_t carry = 0;  // list entries carried from the previous step (listed, not decoded)
    uint32_t qid_prev = 0;  // LibSVM: status of the last token start (prev_token_status)
#pragma unroll 1
    for (int s = 0;; ++s) {
      const size_t cur = tile0 + static_cast<size_t>(s) * kStepBytes;
      const size_t nxt = cur + kStepBytes;
      const size_t pos_a = cur + lane * 16;
      if (nxt + 64 > n) {  // wave-uniform: the text ends here
        a = clip16(a, pos_a, n);
        b = clip16(b, pos_a + 1024, n);
        t = clip16(t, pos_a + kStepBytes, n);
      }
      // the step at [kHashCarry, kHashText); carried tokens' text before it
      constexpr uint32_t sbase = kHashCarry;
      st[sbase / 16 + lane] = a;
      st[sbase / 16 + 64 + lane] = b;
      if (lane < 4) st[sbase / 16 + 128 + lane] = t;
      uint32_t lm_a, tm_a, lm_b, tm_b;
      if constexpr (kOnePass) {
        const uint32_t left_a = dev::lane_shr1(a.w >> 24);
        const uint32_t pc_a = lane == 0 ? carry_pc : left_a;
        const uint32_t left_b = dev::lane_shr1(b.w >> 24);
        const uint32_t last_a = dev::lane63(a.w >> 24);
        const uint32_t pc_b = lane == 0 ? last_a : left_b;
        // one pass: C1's checks of blank-started lines and control bytes here
        // (token starts outside [0-9+-.] fail the decoder and are flagged there)
        if (nxt <= n) {  // wave-uniform: a full step
          irregular |= lane_masks<true, true, false>(a, pc_a, pos_a, n, &lm_a, &tm_a);
          irregular |= lane_masks<true, true, false>(b, pc_b, pos_a + 1024, n, &lm_b, &tm_b);
        } else {
          irregular |= lane_masks<true, false, false>(a, pc_a, pos_a, n, &lm_a, &tm_a);
          irregular |= lane_masks<true, false, false>(b, pc_b, pos_a + 1024, n, &lm_b, &tm_b);
        }
      } else {
        tm_a = mk.x & 0xFFFFu;
        lm_a = mk.x >> 16;
        tm_b = mk.y & 0xFFFFu;
        lm_b = mk.y >> 16;
      }
      carry_pc = dev::lane63(b.w >> 24);  // the step's last byte (a line end?)
      if (F == TextFormat::kLibSVM) {
        // `qid:` tokens are no features of the batch: dropped (checked as in
        // the fill, from the staged text; any other letter token sends the
        // chunk to the exact kernels)
        const uint32_t qa = tm_a & letter_mask(a), qb = tm_b & letter_mask(b);
        if (__any((qa | qb) != 0)) {
          const PrevTok pv = prev_token_status(tm_a, lm_a, tm_b, lm_b, qid_prev, lane);
          dev::wave_sync();  // the staged step is visible to every lane
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const uint32_t lmh = h == 0 ? lm_a : lm_b, tmh = h == 0 ? tm_a : tm_b;
            for (uint32_t m = h == 0 ? qa : qb; m != 0; m &= m - 1) {
              const uint32_t j = static_cast<uint32_t>(__builtin_ctz(m));
              const uint32_t prev = status_before(tmh, lmh, j, h == 0 ? pv.a : pv.b);
              bool ok = false;
              if (prev == 3u) {
                ok = qid_lds(st, sbase + static_cast<uint32_t>(h) * 1024 + lane * 16 + j).ok;
              } else if (prev == 0u) {
                ok = qid_token(text, n, pos_a + static_cast<size_t>(h) * 1024 + j).ok;
              }
              irregular |= ((lmh >> j) & 1u) != 0 || !ok;
            }
          }
        }
        qid_prev = step_last_status(tm_a, lm_a, tm_b, lm_b, qid_prev);
        tm_a &= ~qa;
        tm_b &= ~qb;
      }
      uint64_t cnt = static_cast<uint64_t>(__popc(tm_a)) |
                     (static_cast<uint64_t>(__popc(tm_b)) << 16) |
                     (static_cast<uint64_t>(__popc(lm_a)) << 32) |
                     (static_cast<uint64_t>(__popc(lm_b)) << 48);
      uint64_t tot;
      uint64_t before = dev::wave_excl_scan_2x32(cnt, &tot);  // 16-bit fields: no carries
      const uint32_t nline_a = static_cast<uint32_t>((tot >> 32) & 0xFFFFu);
      const uint32_t nline = nline_a + static_cast<uint32_t>(tot >> 48);
      const uint32_t la0 = lcnt + static_cast<uint32_t>((before >> 32) & 0xFFFFu);
      const uint32_t lb0 = lcnt + nline_a + static_cast<uint32_t>(before >> 48);
      if (lcnt == 0 || lcnt + nline > own) {
        // wave-uniform (first / last step): drop tokens outside the owned lines
        tm_a = owned_tokens(tm_a, lm_a, la0, own);
        tm_b = owned_tokens(tm_b, lm_b, lb0, own);
        cnt = static_cast<uint64_t>(__popc(tm_a)) | (static_cast<uint64_t>(__popc(tm_b)) << 16);
        uint32_t t32;
        const uint32_t b32 = dev::wave_excl_scan<uint32_t>(static_cast<uint32_t>(cnt), &t32);
        before = (before & ~0xFFFFFFFFull) | b32;
        tot = (tot & ~0xFFFFFFFFull) | t32;
      }
      const uint32_t ntok_a = static_cast<uint32_t>(tot & 0xFFFFu);
      const uint32_t ntok = ntok_a + static_cast<uint32_t>((tot >> 16) & 0xFFFFu);
      // a step of more tokens than the list holds is listed and decoded in
      // its two 1 KiB halves (a half of more: the exact kernels)
      const uint32_t ntok_b = ntok - ntok_a;
      const bool split = carry + ntok > kHashListCap;
      if (split && (carry + ntok_a > kHashListCap || ntok_b > kHashListCap)) {
        irregular = true;
        break;
      }
      lcnt += nline;
      const bool eol_end = carry_pc == '\n' || carry_pc == '\r';
      const bool last = nxt >= n || lcnt > own || (s + 1 >= kSteps && lcnt == own && eol_end);
      // a, b, t are consumed (staged, masks taken): the next step's loads go
      // straight into them (in flight during this step's rounds)
      if (!last) {
        const uint32_t so = static_cast<uint32_t>(s + 1) * kStepBytes;
        a = bload16(trs, loff + so);
        b = bload16(trs, loff + so + 1024);
        if (lane < 4) t = bload16(trs, loff + so + kStepBytes);
        if constexpr (!kOnePass) mk = load_masks(mrs, moff, s + 1);
      }

      list_slice<kHashListCap>(sl, tm_a, lm_a, carry + static_cast<uint32_t>(before & 0xFFFFu),
                               sbase + lane * 16, la0, lane);
      // split: the b half is listed after the a half's rounds, from two packed
      // registers (few live across the rounds)
      const uint32_t pk_m = tm_b | (lm_b << 16);
      const uint32_t pk_o = static_cast<uint32_t>((before >> 16) & 0xFFFFu) | (lb0 << 16);
      if (!split) {
        list_slice<kHashListCap>(sl, tm_b, lm_b,
                                 carry + ntok_a + static_cast<uint32_t>((before >> 16) & 0xFFFFu),
                                 sbase + 1024 + lane * 16, lb0, lane);
      }
      dev::wave_sync();
      uint32_t total = 0, ndec = 0;
#pragma unroll 1
      for (int part = 0;; ++part) {
        // the list: carried tokens, then this step's (or its halves'); only
        // whole rounds run unless this is the wave's last step, or the first
        // left-over token starts before the part of the step a carry keeps
        // (its text would not fit the carry area: decode it all now).  The
        // a half of a split step is decoded whole.
        total = !split ? carry + ntok : (part == 0 ? carry + ntok_a : ntok_b);
        uint32_t rest = (last || (split && part == 0)) ? 0u : total % dev::kWave;
        if (rest != 0 && (dev::uniform(sl[total - rest]) & 0x1FFFu) < kHashText - kHashCarry - 64u) {
          rest = 0;
        }
        ndec = total - rest;
        for (uint32_t r0 = 0; r0 < ndec; r0 += dev::kWave) {
          const uint32_t li = r0 + slot;
          const bool active = li < ndec;
          const uint32_t e = active ? sl[li] : 0u;
          const bool is_label = active && ((e >> 13) & 1u) != 0;
          const uint32_t off = e & 0x1FFFu;
          const uint32_t lc = e >> 14;
          tok::Token t;
          t.u0_hi = t.u1_hi = 0;
          t.u1 = 0;
          bool bad = false;
          bool ok = tok::decode<F>(st, off, is_label, &t);
          if (__any(active & !ok)) {
            if (active & !ok) {
              const tok::ExtToken x = tok::decode_ext<F>(st, off, is_label, kHashText);
              if (x.ok) t = x.t;
              ok = x.ok;
            }
          }
          if (active & !ok) {
            const size_t gpos = cur + off - sbase;  // (carried tokens: before cur)
            const GenericResult gr = generic_token<F, IndexType>(text, n, gpos, is_label);
            t = gr.t;
            bad = gr.bad;
            irregular |= !num_start(text[gpos]);  // qid:, comments, junk: the exact kernels
          }
          // (counted path: C2 sized the target, no row check)
          if (active & is_label && (!kOnePass || R + lc - 1 < row_cap)) lab_at[lc] = t.f0;
          bool feat = active & !is_label;
          uint64_t key;
          float val;
          const uint64_t u0 = (static_cast<uint64_t>(t.u0_hi) << 32) | t.u0;
          if constexpr (F == TextFormat::kLibSVM) {
            key = static_cast<uint64_t>(static_cast<IndexType>(u0));
            val = t.r == 2 ? t.f0 : 1.0f;
          } else {
            const uint64_t u1 = (static_cast<uint64_t>(t.u1_hi) << 32) | t.u1;
            feat &= t.r >= 2;  // not field:index: the CPU parser skips it too
            key = dev::hash_key(static_cast<uint64_t>(static_cast<IndexType>(u1)),
                                static_cast<uint64_t>(static_cast<IndexType>(u0)), true);
            val = t.r == 3 ? t.f0 : 1.0f;
          }
          neg |= active && bad;
          const uint32_t h = dev::hash_u64(key, out.seed);
          uint32_t bucket;
          if (pow2) {
            bucket = h & dmask;
          } else {
            bucket = h % static_cast<uint32_t>(dim);
          }
          const float sv = (h & 0x80000000u) ? -val : val;
          // the round's rows, in text order: list entries r0 .. r0 + 63
          const uint32_t lo = dev::uniform(sl[r0] >> 14);
          const uint32_t hi =
              dev::uniform(sl[r0 + dev::kWave - 1 < ndec ? r0 + dev::kWave - 1 : ndec - 1] >> 14);
          for (uint32_t rr = lo; rr <= hi; ++rr) {
            if (rr != open) {
              if (open != 0) flush(open);
              open = rr;
            }
            if (feat && lc == rr) atomicAdd(&row[bucket], sv);
          }
        }
        if (!split || part == 1) break;
        carry = 0;  // the a half's list (carried tokens included) is done
        dev::wave_sync();  // the a half's rounds are done with the list
        list_slice<kHashListCap>(sl, pk_m & 0xFFFFu, pk_m >> 16, pk_o & 0xFFFFu,
                                 sbase + 1024 + lane * 16, pk_o >> 16, lane);
        dev::wave_sync();
      }  // part
      if (last) break;
      // carry the rest: the step's last 1 KiB of text into the carry area (the
      // next step restages the 64 B after it), its entries to the list front
      // with offsets moved down by the 2 KiB the text shifts
      const uint32_t left = total - ndec;
      dev::wave_sync();  // every lane is done with this step's rounds
      if (left != 0) {
        const uint4 keep = st[(kHashText - kHashCarry - 64) / 16 + lane];
        const uint32_t moved = lane < static_cast<int>(left) ? sl[ndec + lane] : 0u;
        dev::wave_sync();
        st[lane] = keep;
        if (lane < static_cast<int>(left)) sl[lane] = moved - kStepBytes;
      }
      carry = left;
      dev::wave_sync();  // every lane is done with this step's text and list
    }
    if (open != 0) flush(open);
  }
  unsigned fl = 0;
  if (irregular) fl |= kFlagIrregular;
  if (neg) fl |= kFlagNegIndex;
  if (over) fl |= kFlagOverflow;
  fl = dev::wave_or(fl);
  if (lane == 0) {
    MetaPartial p;
    p.max_index = 0;
    p.max_field = 0;
    p.flags = fl;
    p.pad = 0;
    partials[tile] = p;
  }
}
}  // namespace

template <typename IndexType>
size_t LaunchTileHashed(const char* text, size_t nbytes, TextFormat format,
                        const uint64_t* tile_prefix, const uint32_t* tile_masks,
                        uint64_t row_base, uint64_t nlines, int dim,
                        float scale, uint32_t seed, bool fp8, void* out, float* labels,
                        MetaPartial* partials, ChunkMeta* meta, ChunkMeta* host_meta,
                        hipStream_t stream, const HashOnePass* one_pass) {
  const size_t ntiles = TileCount(nbytes);
  const uint8_t* t = reinterpret_cast<const uint8_t*>(text);
  const size_t smem = static_cast<size_t>(kFillWaves) * dim * sizeof(float);
  HashTarget tgt{out, labels, row_base, nlines, dim, scale, seed, 0u, LookBack{nullptr, nullptr, 0ull},
                 0ull, meta, tile_masks};
  CHECK(one_pass != nullptr || tile_masks != nullptr || ntiles == 0)
      << "LaunchTileHashed: the counted path needs C1's tile_masks";
  const size_t groups = (ntiles + kFillWaves - 1) / kFillWaves;
  if (one_pass != nullptr) {
    tgt.tag = one_pass->tag;
    tgt.lb = *one_pass;
    tgt.row_cap = one_pass->row_cap;
  }
  if (ntiles != 0) {
    const dim3 grid(static_cast<unsigned>(groups));
#define DMLC_TILE_HASH(FMT, FP8, ONE)                                                          \
  PrepareLdsLaunch(k_tile_hash<FMT, IndexType, FP8, ONE>, smem);                                \
  hipLaunchKernelGGL((k_tile_hash<FMT, IndexType, FP8, ONE>), grid, dim3(kThreads), smem, stream, \
                     t, nbytes, ntiles, tile_prefix, tgt, partials);                            \
  DMLC_HIP_CHECK_LAUNCH()
#define DMLC_TILE_HASH_FMT(FMT)             \
  if (one_pass != nullptr) {                \
    if (fp8) {                              \
      DMLC_TILE_HASH(FMT, true, true);      \
    } else {                                \
      DMLC_TILE_HASH(FMT, false, true);     \
    }                                       \
  } else if (fp8) {                         \
    DMLC_TILE_HASH(FMT, true, false);       \
  } else {                                  \
    DMLC_TILE_HASH(FMT, false, false);      \
  }
    if (format == TextFormat::kLibFM) {
      DMLC_TILE_HASH_FMT(TextFormat::kLibFM)
    } else {
      DMLC_TILE_HASH_FMT(TextFormat::kLibSVM)
    }
#undef DMLC_TILE_HASH_FMT
#undef DMLC_TILE_HASH
  }
  LaunchTileFinish(partials, ntiles, meta, host_meta, nullptr, 0ull, 0ull, stream);
  return ntiles != 0 ? groups : 0;
}

template size_t LaunchTileHashed<uint32_t>(const char*, size_t, TextFormat, const uint64_t*,
                                           const uint32_t*, uint64_t, uint64_t, int, float, uint32_t,
                                           bool, void*, float*, MetaPartial*, ChunkMeta*, ChunkMeta*,
                                           hipStream_t, const HashOnePass*);
template size_t LaunchTileHashed<uint64_t>(const char*, size_t, TextFormat, const uint64_t*,
                                           const uint32_t*, uint64_t, uint64_t, int, float, uint32_t,
                                           bool, void*, float*, MetaPartial*, ChunkMeta*, ChunkMeta*,
                                           hipStream_t, const HashOnePass*);

}  // namespace gpu
}  // namespace dmlc
