/*!
 * \file src/gpu/kernels.h
 * \brief Host-callable launchers of the CDNA4 (gfx950) ingestion kernels.
 *
 * Kernel inventory:
 *   K1 line index        LaunchLineIndex          (text_kernels.hip)
 *   K2 per-line count    LaunchTextCount          (text_kernels.hip)
 *   K3 offsets scan      LaunchScanU64            (scan_kernels.hip)
 *   K4 per-line fill     LaunchTextFill           (text_kernels.hip)
 *   K5 CSV / K6 LibFM    same launchers, TextFormat::kCSV / kLibFM
 *   K7 recordio decode   LaunchRecordIOTileCount / LaunchRecordIOTileFill, LaunchRecordIOGather
 *                        (recordio_kernels.hip)
 *   C1 + C2 tile count   LaunchTileCountScan, LaunchTileScanRaw (tile_count_kernels.hip)
 *   C3 tile fill / hash  LaunchTileFill, LaunchTileHashed (tile_fill_kernels.hip)
 *   C4 tile finish       LaunchTileFinish         (tile_count_kernels.hip)
 *   K8 max reduce        fused into K4 (wave max + one atomicMax per wave)
 *   K9 fp8 pack / hash   LaunchHashedDenseFP8     (feature_kernels.hip)
 *   K10 csr concat       LaunchCSRAppend          (feature_kernels.hip)
 *   K11 spmv / sdot      LaunchCSRSpMV, LaunchCSRSpMVT (feature_kernels.hip)
 *   M1 spmm              LaunchCSRSpMM            (spmm_kernels.hip)
 *   M1p spmm over pairs  LaunchCSRSpMM, CsrView::paired
 *   M2 spmm transposed   LaunchCSRSpMMT           (spmm_kernels.hip)
 *   FF1 ffm forward      LaunchFFMForward         (ffm_kernels.hip)
 *   FF2 ffm backward     LaunchFFMBackward        (ffm_kernels.hip)
 *   Q1 qid run flags     LaunchQidFlags           (rank_kernels.hip)
 *   Q2 qid group pointer LaunchQidGroupPtr        (rank_kernels.hip)
 *   RK1 rank, wave/group LaunchRankLoss, LaunchRankNdcg (rank_kernels.hip)
 *   RK2 rank, block/group the same launchers, groups above kRankWaveGroupRows
 *   G1 row gather count  LaunchCSRGatherCount     (gather_kernels.hip)
 *   G2 row gather fill   LaunchCSRGatherFill      (gather_kernels.hip)
 *   CSR -> CSC           LaunchCSRTranspose       (transpose_kernels.hip)
 *   U1 compact mark      LaunchCompactMark        (compact_kernels.hip)
 *   U2 compact count     LaunchCompactCount       (compact_kernels.hip; + K3)
 *   U3 compact emit      LaunchCompactEmit        (compact_kernels.hip)
 *   U4 compact remap     LaunchCompactRemap       (compact_kernels.hip)
 *   L1 lazy row update   LaunchLazyUpdate         (optim_kernels.hip)
 *   GB1 quantile cuts    LaunchGbdtCutCount, LaunchGbdtCutEmit (gbdt_kernels.hip)
 *   GB2 bin features     LaunchGbdtBin            (gbdt_kernels.hip)
 *   GB3 grad histogram   LaunchGbdtHistogram      (gbdt_kernels.hip)
 *   GB4 best splits      LaunchGbdtBestSplits     (gbdt_kernels.hip)
 *   GB5 advance rows     LaunchGbdtAdvance        (gbdt_kernels.hip)
 * The launchers of K9, K11, M1 / M2, FF1 / FF2, G2 and the transpose take
 * their CSR operand as one CsrView and pick the kernel for its index width
 * (and pair layout) themselves; launch_common.h holds what they share.
 * All launchers are asynchronous on `stream` and never allocate or
 * synchronise (graph-capture safe, cdna_hip_programming.md Guideline 9).
 */
#ifndef DMLC_GPU_KERNELS_H_
#define DMLC_GPU_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace dmlc {
namespace gpu {

/*! \brief padding (bytes) every device text buffer must have past its end */
constexpr size_t kTextPadBytes = 4096;
/*! \brief bytes per workgroup tile of the line-index kernels (256 lanes x 16 B) */
constexpr size_t kLineTileBytes = 4096;

enum class TextFormat : int { kLibSVM = 0, kLibFM = 1, kCSV = 2 };

/*! \brief per-format knobs passed by value to the kernels */
struct TextParseConfig {
  TextFormat format{TextFormat::kLibSVM};
  int label_column{-1};   // CSV
  int weight_column{-1};  // CSV
  char delimiter{','};    // CSV
};

/*! \brief per-chunk results written by the device */
struct ChunkMeta {
  unsigned long long nlines;     // candidate lines (K1)
  unsigned long long nrows;      // valid rows (K3 total >> 32)
  unsigned long long nnz;        // entries (K3 total & 0xffffffff)
  unsigned long long max_index;  // K8
  unsigned long long max_field;  // K8 (LibFM)
  unsigned int flags;            // kFlag* bits
  unsigned int pad;
};
constexpr unsigned kFlagWeight = 1u;
constexpr unsigned kFlagQid = 2u;
constexpr unsigned kFlagValue = 4u;
constexpr unsigned kFlagField = 8u;
constexpr unsigned kFlagNegIndex = 256u;
constexpr unsigned kFlagOverflow = 512u;

/*!
 * \brief per-workgroup reduction slot.  Kernels never hit one global word from
 *  every wave (same-address atomics serialise at the memory side, ~10 ns each:
 *  62k waves x 3 atomics cost 1.5 ms per chunk); each workgroup reduces in
 *  LDS and writes its slot, then k_reduce_partials folds the slots into the
 *  ChunkMeta with one workgroup.
 */
struct MetaPartial {
  unsigned long long max_index;
  unsigned long long max_field;
  unsigned int flags;
  unsigned int pad;
};
/*! \brief max workgroups of any kernel that writes MetaPartial slots */
constexpr int kMaxPartialBlocks = 8192;
/*! \brief fold nblocks MetaPartial slots into meta (max / or) with one workgroup */
void LaunchReducePartials(const MetaPartial* partials, int nblocks, ChunkMeta* meta,
                          hipStream_t stream);

/*!
 * \brief the device CSR operand of the op launchers (K9, K11, M1 / M2, FF1 /
 *  FF2, G2, transpose).  Every launcher checks its view before anything else,
 *  an empty one included: `paired` needs !index64, value == (float*)index + 1
 *  and 8-byte aligned pairs, and only LaunchCSRSpMV / LaunchCSRSpMM take it.
 */
struct CsrView {
  const uint64_t* offset;  // nrows + 1, may be a slice (offset[0] != 0)
  const void* index;       // u32 or u64 per index64
  const float* value;      // may be null (1.0 per entry)
  const void* field;       // may be null; index's type
  size_t nrows;
  bool index64;
  bool paired;             // index/value are the interleaved (u32, f32) pairs of a transpose
};

/*! \brief destination arrays of the fill pass (device pointers) */
template <typename IndexType>
struct FillTarget {
  uint64_t* offset;  // row pointer (global)
  float* label;
  float* weight;
  uint64_t* qid;
  IndexType* field;  // may be null unless LibFM
  IndexType* index;
  float* value;
  uint64_t row_base;   // first row written by this chunk
  uint64_t nnz_base;   // first entry written by this chunk
  uint64_t row_limit;  // rows [row_base, row_limit) may be written
  uint64_t nnz_limit;  // entries [nnz_base, nnz_limit) may be written
};

/*! \brief scratch sizes for a chunk of `nbytes` */
size_t LineIndexTiles(size_t nbytes);
size_t ScanPartials(size_t n);

/*!
 * \brief K1a: count line starts per 4 KiB tile and scan the tile counts.
 * \param tile_scratch >= LineIndexTiles(nbytes) u64
 * \param meta meta->nlines receives the number of lines
 */
void LaunchLineCount(const char* text, size_t nbytes, uint64_t* tile_scratch, ChunkMeta* meta,
                     hipStream_t stream);
/*!
 * \brief K1b: write the line start offsets (needs LaunchLineCount's scanned
 *  tile_scratch); line_starts needs meta->nlines entries.
 */
void LaunchLineEmit(const char* text, size_t nbytes, const uint64_t* tile_scratch,
                    uint32_t* line_starts, hipStream_t stream);

/*!
 * \brief K2: per-line (row_valid << 32 | nnz) into line_info[nlines]; sets
 *  weight/qid flags in meta.
 */
void LaunchTextCount(const char* text, size_t nbytes, const uint32_t* line_starts,
                     size_t nlines, const TextParseConfig& cfg, uint64_t* line_info,
                     MetaPartial* partials, ChunkMeta* meta, hipStream_t stream);

/*!
 * \brief K3: exclusive scan of n u64 values in place (mod 2^64); *total
 *  receives the sum.
 *
 *  Alignment: `data` must be 16-byte aligned -- the reduce and down-sweep
 *  passes read and write it as 16-byte pairs.  `partials` and `total` need
 *  only the 8 bytes of a u64: every access to them is a single word, so a
 *  caller may place them straight behind an array of any length.
 * \param partials >= ScanPartials(n) + 1 u64
 */
void LaunchScanU64(uint64_t* data, size_t n, uint64_t* partials, uint64_t* total,
                   hipStream_t stream);

/*! \brief split the scan total into meta->nrows / meta->nnz */
void LaunchMetaFromTotal(const uint64_t* total, ChunkMeta* meta, hipStream_t stream);

/*!
 * \brief K4 (+K5/K6/K8): parse every line into the CSR target. line_info must
 *  hold the exclusive scan produced by K3.  Also writes the closing offset.
 */
template <typename IndexType>
void LaunchTextFill(const char* text, size_t nbytes, const uint32_t* line_starts,
                    size_t nlines, const TextParseConfig& cfg, const uint64_t* line_info,
                    const FillTarget<IndexType>& out, uint64_t nrows, uint64_t nnz,
                    MetaPartial* partials, ChunkMeta* meta, hipStream_t stream);

/*! \brief offset[row_end] = nnz_end (closing row pointer of a chunk) */
void LaunchCloseOffsets(uint64_t* offset, uint64_t row_end, uint64_t nnz_end, hipStream_t stream);

/*! \brief a chunk the tile parser cannot take (the exact per-line kernels re-parse it) */
constexpr unsigned kFlagIrregular = 1024u;

// --------------- LDS-staged tile parser (LibSVM/LibFM fast path) ---------------
/*! \brief decoupled look-back state of a one-pass launch (tile, hash and
 *  RecordIO fills): one status word per tile and the workgroup ticket counter */
struct LookBack {
  uint64_t* status;            // one word per tile of the chunk
  unsigned long long* ticket;  // counter, zeroed once
  unsigned long long ticket0;  // the counter's value before this launch
};
/*! \brief bytes of text per workgroup of the tile kernels */
constexpr size_t kTileBytes = 8192;
/*! \brief a weighted row met a FillTarget without a weight column (re-run with one) */
constexpr unsigned kFlagNeedWeight = 2048u;
/*! \brief tiles of a chunk (size of the tile count / flag scratch and MetaPartial slots) */
size_t TileCount(size_t nbytes);
/*! \brief u64 tile_counts / u32 tile_flags entries to reserve for ntiles tiles (scan scratch) */
size_t TileScratchWords(size_t ntiles);
/*! \brief MetaPartial slots to reserve for ntiles tiles (finish-fold scratch) */
size_t TileScratchSlots(size_t ntiles);
/*!
 * \brief C1 + C2: per-tile (line starts << 32 | token starts) and irregular
 *  flags, exclusive-scanned in place; meta receives nlines, nrows = nlines,
 *  nnz = tokens - lines, flags (kFlagIrregular) and zeroed maxima; host_meta
 *  (mapped pinned memory, may be null) receives a copy the host reads after
 *  synchronising the stream, without a device-to-host copy.
 *  tile_counts / tile_flags need TileCount(nbytes) entries; tile_masks
 *  (TileMaskWords) receives the per-16-byte start masks the fill reads.
 */
void LaunchTileCountScan(const char* text, size_t nbytes, uint64_t* tile_counts,
                         uint32_t* tile_flags, uint32_t* tile_masks, ChunkMeta* meta,
                         ChunkMeta* host_meta, hipStream_t stream);
/*!
 * \brief u32 words of C1's published token / line start masks for ntiles
 *  tiles (one word per 16 text bytes: the fill and the fused hash kernel take
 *  them instead of classifying every byte a second time)
 */
size_t TileMaskWords(size_t ntiles);
/*!
 * \brief C3 + C4: parse every token of a regular chunk into out using the
 *  scanned tile prefixes; merges max index / field and flags into meta and
 *  writes offset[row_base + nrows].  partials needs TileCount(nbytes) slots.
 *  Sets kFlagNeedWeight if a row is weighted and out.weight is null.
 *
 *  One pass (one_pass != nullptr; tile_prefix unused, nbytes > 0): no C1 / C2
 *  -- each wave counts its tile's lines and entries itself (with C1's
 *  irregular checks) and takes the counts before it by decoupled look-back
 *  over one_pass->status (zeroed here, in the stream, before the launch).
 *  The chunk's nlines / nrows / nnz land in meta (and host_meta) with the
 *  flags.  out.row_limit / nnz_limit are the target's capacities: rows or
 *  entries past them are not written and set kFlagOverflow (grow the target
 *  to meta's sizes and run the chunk again; no closing row pointer is
 *  written).  kFlagQid: the chunk has `qid:` tokens, which only the counted
 *  path (LaunchTileCountScan first, qid column zeroed) writes -- run it so.
 *  Returns the workgroups launched: advance ticket0 by it.
 */
struct FillOnePass : LookBack {};  // status: >= TileCount(nbytes) words
template <typename IndexType>
size_t LaunchTileFill(const char* text, size_t nbytes, TextFormat format,
                      const uint64_t* tile_prefix, const uint32_t* tile_masks,
                      const FillTarget<IndexType>& out, MetaPartial* partials, ChunkMeta* meta,
                      ChunkMeta* host_meta, hipStream_t stream,
                      const FillOnePass* one_pass = nullptr);

/*!
 * \brief fused tokenize -> hash -> dense rows on the tile parser (config 5):
 *  rows = the `nlines` lines of a regular chunk (tile_prefix from
 *  LaunchTileCountScan), row row_base + line of a [rows x dim] fp8 (x scale)
 *  or f32 batch, labels alongside; no CSR is written.  One wave per tile, the
 *  lines that start in it (followed past the tile end, any length).  Sets
 *  kFlagIrregular for tokens only the exact kernels parse (qid:, junk; re-run
 *  the chunk with LaunchTextHashed), merges kFlagNegIndex.  dim: multiple of
 *  16, 16 .. 4096 (16 x dim bytes of dynamic LDS next to ~20 KiB of static
 *  staging; checked launch as for K9; the same fp8 conversion).
 */
/*!
 *  One pass (one_pass != nullptr; tile_prefix / nlines unused): no C1 / C2 --
 *  each wave counts its tile's lines itself and takes the lines before it by
 *  decoupled look-back; the chunk's nlines / nrows land in meta (and
 *  host_meta) with the flags.  Rows at or past row_cap are not written and set
 *  kFlagOverflow (grow the batch to meta->nrows and run the chunk again).
 *  nbytes > 0 (an empty chunk has no tile to write the sizes).
 *  Also sets kFlagIrregular for what C1 would have (blank-started lines,
 *  control bytes other than \t \n \r).  Returns the workgroups launched:
 *  advance ticket0 by it for the next launch on the same counter.
 */
struct HashOnePass : LookBack {  // status: >= TileCount(nbytes) words, zeroed once at allocation
  uint32_t tag;                // distinct per launch on the same status array, 1..2^30-1
  uint64_t row_cap;            // rows of out / labels
};
template <typename IndexType>
size_t LaunchTileHashed(const char* text, size_t nbytes, TextFormat format,
                        const uint64_t* tile_prefix, const uint32_t* tile_masks,
                        uint64_t row_base, uint64_t nlines, int dim,
                        float scale, uint32_t seed, bool fp8, void* out, float* labels,
                        MetaPartial* partials, ChunkMeta* meta, ChunkMeta* host_meta,
                        hipStream_t stream, const HashOnePass* one_pass = nullptr);

/*!
 * \brief C2 alone over caller-filled per-tile u64 counts (hi 32 bits: items,
 *  lo 32 bits: bytes): exclusive scan in place, meta->nrows = items,
 *  meta->nnz = bytes, OR of tile_flags into meta->flags, published to
 *  host_meta.  Scratch sizes as for LaunchTileCountScan (TileScratchWords).
 */
void LaunchTileScanRaw(uint64_t* tile_counts, uint32_t* tile_flags, size_t ntiles,
                       ChunkMeta* meta, ChunkMeta* host_meta, hipStream_t stream);
/*!
 * \brief C4 alone: fold nslots MetaPartial slots into meta (max / or), write
 *  offset[row_base + meta->nrows] = nnz_base + meta->nnz (offset may be null)
 *  and publish meta to host_meta.  partials needs TileScratchSlots(nslots).
 */
void LaunchTileFinish(MetaPartial* partials, size_t nslots, ChunkMeta* meta, ChunkMeta* host_meta,
                      uint64_t* offset, uint64_t row_base, uint64_t nnz_base, hipStream_t stream);

// ------------------------- CSV on the tile pipeline -------------------------
/*!
 * \brief S1: per 8 KiB tile (rows starting in it << 32 | their entries) and
 *  kFlagIrregular (a row running > 4 KiB past its tile, control bytes); scan
 *  them with LaunchTileScanRaw.  tile_counts / tile_flags: TileScratchWords.
 *  With label / weight columns of at most 0 the counts are positional (S1p:
 *  row starts and entries whose first byte is in the tile, no flags) and the
 *  fill flags irregular chunks; LaunchCsvTileFill takes the same columns, so
 *  both pick the same mode.  The positional count also publishes every 16
 *  bytes' line-end / delimiter masks into tile_masks (TileMaskWords) and
 *  flags control bytes; the fill then reads the masks instead of classifying.
 */
void LaunchCsvTileCount(const char* text, size_t nbytes, int label_column, int weight_column,
                        char delimiter, uint64_t* tile_counts, uint32_t* tile_flags,
                        uint32_t* tile_masks, hipStream_t stream);
/*!
 * \brief S2: every row of a regular chunk into out (index / value / label /
 *  weight / offset) from the scanned S1 prefixes; one MetaPartial per tile
 *  (max index, kFlagValue / kFlagWeight), folded by LaunchTileFinish.
 */
template <typename IndexType>
void LaunchCsvTileFill(const char* text, size_t nbytes, int label_column, int weight_column,
                       char delimiter, const uint64_t* tile_prefix, const uint32_t* tile_masks,
                       const FillTarget<IndexType>& out, MetaPartial* partials,
                       hipStream_t stream);

// ----------------------------- RecordIO (K7) -----------------------------
/*! \brief error bits reported by the RecordIO kernels */
constexpr uint32_t kRecErrTruncated = 1;   // a part runs past the chunk end
constexpr uint32_t kRecErrBadPart = 2;     // continuation part without its head
/*! \brief 2048-word tiles of a chunk of `nwords` words (scan scratch: TileScratchWords) */
size_t RecordIOTiles(size_t nwords);
/*!
 * \brief R1: per tile (record heads << 32 | output bytes) and error bits
 *  (kRecErr*); scan them with LaunchTileScanRaw.  The chunk must start at a
 *  record head and be < 4 GiB.
 */
void LaunchRecordIOTileCount(const uint32_t* words, size_t nwords, uint64_t* tile_counts,
                             uint32_t* tile_flags, hipStream_t stream);
/*!
 * \brief R2: decode every record of the chunk: record r (chunk-relative) gets
 *  offset[rec_base + r] = byte_base + its output position and its payload
 *  (multi-part records reassembled, escaped magic words re-inserted) at
 *  data + that position.  tile_prefix: the scanned R1 counts; partials: one
 *  MetaPartial per tile (error bits), folded by LaunchTileFinish, which also
 *  writes the closing offset.
 */
/*!
 *  One pass (one_pass != nullptr; tile_prefix unused, nwords > 0): R1 runs
 *  inside the fill (decoupled look-back over one_pass->status, zeroed here
 *  before the launch); the chunk's records / bytes land in one_pass->meta
 *  (nrows / nnz), for LaunchTileFinish.  Records at or past rec_cap (offset
 *  slots; the closing one needs one more) and bytes past byte_cap are not
 *  written and set kFlagOverflow: grow to rec_base + nrows / byte_base + nnz
 *  and run the chunk again.  Returns the workgroups launched (advance
 *  ticket0 by it).
 */
struct RecordIOOnePass : LookBack {  // status: >= RecordIOTiles(nwords) words
  ChunkMeta* meta;
  uint64_t rec_cap;            // offset slots - 1
  uint64_t byte_cap;           // data bytes
};
/*!
 * \brief counted fill's guards: writes past (rec_cap offset slots, byte_cap
 *  data bytes) are dropped, and each tile checks that its parts end at the
 *  next tile's prefix (the last one: meta's totals); either miss is
 *  kRecErrBadPart (a count that disagrees with the fill's header view)
 */
struct RecordIOCaps {
  ChunkMeta* meta;
  uint64_t rec_cap;
  uint64_t byte_cap;
};
size_t LaunchRecordIOTileFill(const uint32_t* words, size_t nwords, const uint64_t* tile_prefix,
                              uint64_t* offset, uint64_t rec_base, uint8_t* data,
                              uint64_t byte_base, MetaPartial* partials, hipStream_t stream,
                              const RecordIOOnePass* one_pass = nullptr,
                              const RecordIOCaps* caps = nullptr);
/*!
 * \brief R1c: LaunchRecordIOTileCount's per-tile counts by following part
 *  chains (one 8-byte read per part after each tile's first-header search):
 *  the same counts on a well-formed chunk for ~2 % of its reads at 512-byte
 *  records; latency-bound, for chunks of parts >= ~128 bytes
 */
void LaunchRecordIOTileCountChain(const uint32_t* words, size_t nwords, uint64_t* tile_counts,
                                  uint32_t* tile_flags, hipStream_t stream);
/*!
 * \brief R3: gather nrec whole records (src + src_off[k], len[k] bytes, 4-byte
 *  multiples) to dst + dst_off[k]
 */
void LaunchRecordIOGather(const uint8_t* src, const uint64_t* src_off, const uint32_t* len,
                          const uint64_t* dst_off, size_t nrec, uint8_t* dst, hipStream_t stream);

// --------------------------- features (K9-K11) ---------------------------
/*!
 * \brief K9: hashed dense batch in OCP fp8 e4m3: out[r, h(index) % dim] +=
 *  value * scale, accumulated in f32 in LDS and converted with gfx950
 *  v_cvt_pk_fp8_f32.  rows = nrows; dim: multiple of 4, 4 .. 8192 (16 x dim
 *  bytes of dynamic LDS per workgroup, up to 128 KiB: the launch opts in to
 *  it and is checked, a refused launch throws).  A wave takes rows r, r +
 *  4 x grid, ...: its LDS row is zeroed again by each readout.
 *  Conversion: round to nearest even of sum * scale (f32), subnormals
 *  included; |x| <= 464 gives a finite code (464 -> 448).  Out of range, as
 *  produced by gfx950's conversion: finite |x| > 464 and +-inf give the NaN
 *  code with the value's sign (0x7F / 0xFF, no saturation; the same bytes as
 *  torch's float8_e4m3fn cast), a NaN gives 0xFF whatever its sign (torch:
 *  0x7F for a positive NaN).
 */
void LaunchHashedDenseFP8(const CsrView& csr, int dim, float scale, uint32_t seed, uint8_t* out,
                          hipStream_t stream);
/*! \brief same but f32 output (reference for the fp8 path / bf16 consumers) */
void LaunchHashedDenseF32(const CsrView& csr, int dim, uint32_t seed, float* out,
                          hipStream_t stream);
/*!
 * \brief K9 fused with the text walk (BASELINE config 5): every valid line of a
 *  LibSVM / LibFM chunk becomes row row_base + (line_info >> 32) of a dense
 *  [rows x dim] batch -- OCP fp8 e4m3 (x scale) or f32 -- with features
 *  hashed exactly as LaunchHashedDense* does, plus its label; no CSR is
 *  written.  line_starts / line_info as for LaunchTextFill (K1, K2 + K3).
 *  dim: multiple of 4, 4 .. 4096 (LDS row per wave, 16 x dim bytes of dynamic
 *  LDS; checked launch as for K9; the same fp8 conversion).  Merges
 *  kFlagNegIndex.
 */
template <typename IndexType>
void LaunchTextHashed(const char* text, size_t nbytes, const uint32_t* line_starts, size_t nlines,
                      TextFormat format, const uint64_t* line_info, uint64_t row_base, int dim,
                      float scale, uint32_t seed, bool fp8, void* out, float* labels,
                      MetaPartial* partials, ChunkMeta* meta, hipStream_t stream);
/*! \brief K11: y[r] = sum_j value * w[index] (+ bias), 16 lanes per row; a
 *  paired view is read as interleaved (index, value) pairs */
void LaunchCSRSpMV(const CsrView& csr, const float* w, float bias, float* y, hipStream_t stream);
/*! \brief K11^T: g[index] += value * d[r] (f32 atomics) */
void LaunchCSRSpMVT(const CsrView& csr, const float* d, float* g, hipStream_t stream);
// ------------------------- SpMM (spmm_kernels.hip) -------------------------
/*! \brief widest dense operand (columns) of M1 / M1p / M2 */
constexpr int kSpMMMaxCols = 256;
/*!
 * \brief M1: y[r, :] = sum_j value[j] * w[index[j], :] (+ bias[:]) for row-major
 *  contiguous f32 w [features x k], y [nrows x k], bias [k] or nullptr; k in
 *  1 .. kSpMMMaxCols.  The CSR shapes of K11: value may be nullptr (1.0 per
 *  entry, a compile-time variant), offset may be a slice of a larger row
 *  pointer, empty rows give bias or 0.  k % 4 == 0 with 16-byte aligned w, y
 *  and bias takes 16-byte loads, anything else 4-byte loads.  No atomics and a
 *  summation order fixed by k: the output bytes are a pure function of the
 *  inputs.  Feature ids must be < features (not checked on the device).
 *  M1p (a paired view): M1 over the interleaved (u32 index, f32 value) pairs
 *  of a transpose, one 8-byte load per entry; the same summation order as M1.
 *  A row of any length runs on one lane group of one wave.
 */
void LaunchCSRSpMM(const CsrView& csr, const float* w, const float* bias, int k, float* y,
                   hipStream_t stream);
/*! \brief M2: g[index[j], :] += value[j] * d[r, :] with no-return f32 atomics
 *  into a zeroed g [features x k]; the lanes of one entry cover one contiguous
 *  4 * min(k, 64)-byte segment of a g row per wave-instruction */
void LaunchCSRSpMMT(const CsrView& csr, const float* d, int k, float* g, hipStream_t stream);
// -------------------- field-aware FM (ffm_kernels.hip) ---------------------
/*! \brief largest factor rank k of FF1 / FF2 (k: a multiple of 4 from 4) */
constexpr int kFFMMaxRank = 32;
/*! \brief entries of a row FF1 / FF2 stage in LDS; longer rows re-read global memory */
constexpr uint32_t kFFMStagedRowEntries = 128;
/*! \brief bits FF1 ORs into its error word: an id >= features, a field >= num_fields */
constexpr uint32_t kFFMErrIndex = 1, kFFMErrField = 2;
/*!
 * \brief FF1: y[r] = sum_{a < b} x_a x_b sum_c v[i_a, f_b, c] v[i_b, f_a, c] over
 *  the entries (i, f, x) of row r, for a row-major contiguous, 16-byte aligned
 *  f32 v [features x num_fields x k].  Pairs run over entries, not distinct
 *  ids; rows of 0 or 1 entries give 0.  The CSR shapes of K11 (value may be
 *  nullptr, offset a slice of a larger row pointer, no rows) with a field per
 *  entry, of the index's type.  An entry with id >= features or field >=
 *  num_fields takes part in no pair, is never turned into an address, and ORs
 *  kFFMErrIndex / kFFMErrField into *error (an int32 the caller zeroed).  No
 *  atomics on y; the summation order depends on the row's length and k alone.
 */
void LaunchFFMForward(const CsrView& csr, const float* v, uint64_t features, int num_fields, int k,
                      float* y, int* error, hipStream_t stream);
/*!
 * \brief FF2: dv[i_a, f_b, :] += g[r] x_a x_b v[i_b, f_a, :] for every ordered
 *  pair a != b of every row, with no-return f32 atomics into a zeroed dv shaped
 *  as v.  One wave per row, a fixed per wave-instruction, the lanes over (b, c)
 *  with c fastest: for entries in field order one instruction's targets are one
 *  contiguous stretch of dv[i_a, :, :].  Rows with g[r] == +-0 are skipped;
 *  out-of-range entries are skipped as in FF1 (nothing is reported here).
 */
void LaunchFFMBackward(const CsrView& csr, const float* g, const float* v, uint64_t features,
                       int num_fields, int k, float* dv, hipStream_t stream);
// --------------------- ranking on qid groups (rank_kernels.hip) ---------------------
/*! \brief largest label of RK1 / RK2 (labels are integers from 0; gain 2^label - 1) */
constexpr uint32_t kRankMaxLabel = 31;
/*! \brief rows of a group RK1 takes (one wave, the group staged in LDS); longer groups are RK2's */
constexpr uint32_t kRankWaveGroupRows = 256;
/*! \brief rows of the tiles RK2 passes a group through LDS in */
constexpr uint32_t kRankTileRows = 256;
/*! \brief bits RK1 / RK2 OR into their error word: a group whose pointers descend, end past
 *  `rows` or span >= 2^31 rows; a label that is no integer in [0, kRankMaxLabel] */
constexpr uint32_t kRankErrGroup = 1, kRankErrLabel = 2;
/*!
 * \brief Q1: flag[r] = (r == 0 || qid[r] != qid[r - 1]) for r < rows, as u64 for
 *  LaunchScanU64 (flag 16-byte aligned): scanned, flag[r] is the group of a row
 *  that starts a run and the scan's total the number of groups G.  Rows of one
 *  query are taken to be adjacent; a qid that comes back later starts a new group.
 */
void LaunchQidFlags(const uint64_t* qid, size_t rows, uint64_t* flag, hipStream_t stream);
/*!
 * \brief Q2: group_ptr[scanned[r]] = r at every run start and group_ptr[*total]
 *  = rows; scanned / total: Q1's flags after LaunchScanU64.  group_ptr has
 *  capacity + 1 slots (capacity >= *total); a slot past them is not written.
 */
void LaunchQidGroupPtr(const uint64_t* qid, size_t rows, const uint64_t* scanned,
                       const uint64_t* total, uint64_t capacity, uint64_t* group_ptr,
                       hipStream_t stream);
/*!
 * \brief RK1 + RK2: the pairwise ranking loss of every group g = rows
 *  [group_ptr[g], group_ptr[g + 1]) of score / label [rows] and its gradient
 *  (the definitions: rank_kernels.hip).  ndcg_weights: LambdaRank's w_ij, else
 *  1 (RankNet).  Writes loss_g [groups], pairs_g [groups] (|P_g|) and grad[r]
 *  for the rows of every group that has no error; grad [rows] must be zeroed by
 *  the caller (rows outside every group and rows of a refused group keep 0).
 *  row_scratch: `rows` floats (only read and written with ndcg_weights; may be
 *  null without).  error: an int32 the caller zeroed, kRankErr* bits.  NaN
 *  scores violate a precondition (the outputs of their group are unspecified;
 *  no address depends on a score).  Both kernels run over all groups and each
 *  skips the other's; no atomics on the outputs, the same inputs give the same
 *  bytes.  groups == 0 returns before any HIP call.
 */
void LaunchRankLoss(const float* score, const float* label, const uint64_t* group_ptr, size_t groups,
                    uint64_t rows, bool ndcg_weights, float sigma, float* row_scratch, float* grad,
                    float* loss_g, int64_t* pairs_g, int* error, hipStream_t stream);
/*!
 * \brief RK1 + RK2 in metric mode: ndcg[g] = NDCG@k of group g (k >= 1; k >=
 *  the group's length is the whole group; a group whose ideal DCG is 0 gives
 *  1).  The same rank counting as LaunchRankLoss; a refused group gives 0.
 */
void LaunchRankNdcg(const float* score, const float* label, const uint64_t* group_ptr, size_t groups,
                    uint64_t rows, uint32_t k, float* ndcg, int* error, hipStream_t stream);
// ------------------------ HashedFM (fm_kernels.hip) ------------------------
/*! \brief factor rank of the HIP HashedFM kernels and the [w | V] column count */
constexpr int kFmRank = 16;
constexpr int kFmCols = kFmRank + 1;
/*! \brief dynamic LDS of LaunchFmForward for `dim` features */
size_t FmForwardSharedBytes(int dim);
/*!
 * \brief F1: y[r] = bias + sx x_r.w + 1/2 (|sx x_r V|^2 - sx^2 x_r^2.q) and
 *  xv[r] = sx x_r V for the fp8 e4m3 batch x [rows x dim]; wt_bf16 = [w | V]^T
 *  as bf16 [17 x dim], q[n] = sum_f V_nf^2.  dim: multiple of 128, 128 .. 2048
 *  (FmForwardSharedBytes: 38 dim + 272 bytes of dynamic LDS, above 64 KiB
 *  from dim 1792; the launch opts in to it and is checked).
 */
void LaunchFmForward(const uint8_t* x, int64_t rows, int dim, const void* wt_bf16, const float* q,
                     const float* bias, float sx, float* y, float* xv, int num_cus,
                     hipStream_t stream);
/*!
 * \brief F2: per-block partials part[nblocks][18][dim] of Z = G^T x (G_r =
 *  [g_r, g_r xv_r], rows 0..16) and t = (x^2)^T g (row 17); the caller sums
 *  over blocks.  dim: multiple of 128 (any number of 1024-feature slabs;
 *  waves past dim in the last slab only stage G); nblocks may exceed the
 *  32-row tiles (workgroups without rows write zeros).
 */
void LaunchFmBackward(const uint8_t* x, int64_t rows, int dim, const float* g, const float* xv,
                      int nblocks, float* part, hipStream_t stream);
/*! \brief [w | V]^T in bf16 ([kFmCols][dim]) and q = rowsum(V^2) for LaunchFmForward
 *  (w: [dim] f32, v: [dim][kFmRank] f32) */
void LaunchFmPrep(const float* w, const float* v, int dim, void* wt_bf16, float* q,
                  hipStream_t stream);
/*! \brief sum the LaunchFmBackward partials (z: [kFmCols + 1][dim] scratch)
 *  and write dw [dim] and dV [dim][kFmRank] (v: [dim][kFmRank] f32) */
void LaunchFmReduceGrads(const float* part, int nblocks, int dim, const float* v, float sx,
                         float* z, float* gw, float* gv, hipStream_t stream);
/*! \brief losses of the fused HashedFM step */
enum FmLoss : int { kFmLogistic = 0, kFmSquared = 1 };
/*! \brief largest dim of LaunchFmFused (one wave per 128 features, 8 waves) */
constexpr int kFmFusedMaxDim = 1024;
/*!
 * \brief F5: forward, loss and backward of one HashedFM step in one pass over
 *  the fp8 batch.  Per 32-row tile: F1's products (split over the
 *  workgroup's waves by feature block, summed through LDS), y, the loss and
 *  g = dloss/dy for the tile's labels (mean over `rows`: g is scaled by
 *  inv_n), then F2's G^T X products from the same registers.  Writes y
 *  (optional), part[nblocks][18][dim] as LaunchFmBackward, and
 *  lpart[nblocks][2] = (sum of weighted losses, sum of g) per block.
 *  dim: multiple of 128, <= kFmFusedMaxDim.  weight may be null.
 */
void LaunchFmFused(const uint8_t* x, int64_t rows, int dim, const void* wt_bf16, const float* q,
                   const float* bias, float sx, const float* label, const float* weight,
                   int loss, float inv_n, int nblocks, float* y, float* part, float* lpart,
                   hipStream_t stream);

/*! \brief K10: dst_offset[i] = src_offset[i] - src_base + dst_base for i<=nrows */
void LaunchOffsetRebase(const uint64_t* src_offset, size_t nrows, uint64_t src_base,
                        uint64_t dst_base, uint64_t* dst_offset, hipStream_t stream);
/*!
 * \brief page-cache row pointers: offset[r + 1] (r < nrows) holds the
 *  page-local end of row r; add its page's nnz base.  page_row_end[p] =
 *  rows of pages 0..p (cumulative), page_nnz_base[p] = entries before page p.
 */
void LaunchPageRebase(uint64_t* offset, size_t nrows, const uint64_t* page_row_end,
                      const uint64_t* page_nnz_base, int npages, hipStream_t stream);
/*!
 * \brief CSR -> CSC (transpose_kernels.hip): the rows of csr, whose entries
 *  are [base, base + nnz) of its index / value; writes col_ptr
 *  [num_features + 1] (u64, from 0), row_out [nnz] (u32 row ids, ascending
 *  within each column) and val_out [nnz] (when value != null).  With
 *  val_out == (float*)row_out + 1 (row_out 8-byte aligned) the output is
 *  interleaved (row, value) pairs, one 8-byte store per entry.  Feature ids
 *  >= num_features are clamped and set *error (device u32) to 1.
 *  num_features <= CSRTransposeMaxFeatures(); scratch of
 *  CSRTransposeScratchBytes(nnz, num_features) bytes (256-byte aligned).
 */
void LaunchCSRTranspose(const CsrView& csr, uint64_t base, uint64_t nnz, uint64_t num_features,
                        uint64_t* col_ptr, uint32_t* row_out, float* val_out, void* scratch,
                        uint32_t* error, hipStream_t stream);
size_t CSRTransposeScratchBytes(uint64_t nnz, uint64_t num_features);
uint64_t CSRTransposeMaxFeatures();
// ------------------- row gather (gather_kernels.hip) -------------------
/*! \brief bits of the row gather's device error word */
constexpr uint32_t kGatherErrRow = 1;       // a selected row id is >= nrows_src
constexpr uint32_t kGatherErrCapacity = 2;  // the batch has more entries than out_capacity
constexpr uint32_t kGatherErrSource = 4;    // a selected row's pointers do not fit the source arrays
/*! \brief output entries one wave of LaunchCSRGatherFill owns */
uint64_t CSRGatherRunEntries();
/*! \brief u64 words of scan scratch for a selection of n_sel rows (ScanPartials + 2) */
size_t CSRGatherScratchWords(size_t n_sel);
/*!
 * \brief G1: out_offset[i] = length of source row rows[i] (i < n_sel) and the
 *  per-row columns that are non-null (label / weight / qid -> out_*).  rows:
 *  n_sel int32 (rows64: int64) row ids of a CSR of nrows_src rows whose row
 *  pointer `offset` may be a slice of a larger one (offset[0] != 0); in any
 *  order, duplicates allowed.  An id >= nrows_src (a negative one is huge)
 *  counts 0 entries, reads nothing, writes zeros and sets kGatherErrRow in
 *  *error (device word, zeroed by the caller); a row whose pointers descend
 *  or end past src_entries (entries of index / value / field) counts 0 and
 *  sets kGatherErrSource.  Then scan out_offset in place with LaunchScanU64
 *  (scratch: CSRGatherScratchWords) and pass its total to G2.
 */
void LaunchCSRGatherCount(const uint64_t* offset, uint64_t nrows_src, uint64_t src_entries,
                          const void* rows, bool rows64, size_t n_sel, const float* label,
                          const float* weight, const uint64_t* qid, uint64_t* out_offset,
                          float* out_label, float* out_weight, uint64_t* out_qid, uint32_t* error,
                          hipStream_t stream);
/*!
 * \brief G2: the entries of every selected row of src (G1's offset, nrows_src
 *  = src.nrows) to their place in the batch:
 *  out_*[p] = *[offset[rows[i]] + p - out_offset[i]] for out_offset[i] <= p <
 *  out_offset[i + 1] (index, and value / field when non-null: a missing
 *  column stays missing; out_index / out_field have src's index type).
 *  out_offset: G1's lengths scanned (n_sel + 1 slots; the closing one is
 *  written here from *total, the scan's device total).  A
 *  wave owns CSRGatherRunEntries() consecutive output entries.  Positions at
 *  or past out_capacity (entries of out_*) are not written and set
 *  kGatherErrCapacity; the launch is sized by out_capacity, the total being
 *  known on the device only.  A source position at or past src_entries (the
 *  row pointer changed after G1 checked it) is not read and sets
 *  kGatherErrSource.  No atomics on the outputs.
 */
void LaunchCSRGatherFill(const CsrView& src, uint64_t src_entries, const void* rows, bool rows64,
                         size_t n_sel, uint64_t* out_offset, const uint64_t* total,
                         void* out_index, float* out_value, void* out_field,
                         uint64_t out_capacity, uint32_t* error, hipStream_t stream);
// ------------- compact feature ids of a batch (compact_kernels.hip) -------------
/*! \brief largest num_features of U1 - U4 (the bitmap's bits) */
constexpr uint64_t kCompactMaxFeatures = 1ull << 32;
/*! \brief bit U1 ORs into its error word: an id >= num_features */
constexpr uint32_t kCompactErrIndex = 1;
/*!
 * \brief bytes of the scratch U1 - U4 share (16-byte aligned): the bitmap of
 *  num_features bits, one u64 count per bitmap word (scanned in place) and the
 *  scan's partials -- about num_features / 4 bytes
 */
size_t CompactScratchBytes(uint64_t num_features);
/*!
 * \brief U1: clear the bitmap (in stream order, on every call), then set bit
 *  `id` for every entry [base, base + nnz) of csr's index (the rows' range of a
 *  row slice: entries outside it are not marked).  A set bit is seen by a load
 *  before any atomic.  An id >= num_features (with 64-bit indices: ids >= 2^32
 *  included) forms no address and ORs kCompactErrIndex into *error (a device
 *  word the caller zeroed).  num_features in 1 .. kCompactMaxFeatures, nnz <
 *  2^31.
 */
void LaunchCompactMark(const CsrView& csr, uint64_t base, uint64_t nnz, uint64_t num_features,
                       void* scratch, uint32_t* error, hipStream_t stream);
/*! \brief U2 + K3: the popcount of every bitmap word, scanned in place; *total
 *  (a device u64) receives U, the number of distinct ids */
void LaunchCompactCount(uint64_t num_features, void* scratch, uint64_t* total, hipStream_t stream);
/*! \brief U3: the set bits as ids[0 .. U), strictly ascending; a position at
 *  or past `capacity` (entries of ids) is not written */
void LaunchCompactEmit(uint64_t num_features, const void* scratch, uint64_t capacity, int64_t* ids,
                       hipStream_t stream);
/*! \brief U4: slot[j] = position in ids of the id of entry base + j, j < nnz;
 *  an id >= num_features (U1 flagged it) gets slot 0 */
void LaunchCompactRemap(const CsrView& csr, uint64_t base, uint64_t nnz, uint64_t num_features,
                        const void* scratch, int32_t* slot, hipStream_t stream);
// ----------------- lazy optimizer step (optim_kernels.hip) -----------------
/*! \brief update rules of L1 */
enum LazyRule : int { kLazyAdagrad = 0, kLazyFtrl = 1 };
/*! \brief hyper-parameters by position: adagrad (lr, eps, l2, -), ftrl (alpha, beta, l1, l2) */
struct LazyHyper {
  float a, b, c, d;
};
/*! \brief bit L1 ORs into its error word: a row id >= features or not strictly ascending */
constexpr uint32_t kLazyErrIds = 1;
/*!
 * \brief L1: one optimizer step on rows ids[0 .. nrows) of param [features x
 *  width] from grad [nrows x width] (ids == nullptr: rows 0 .. nrows - 1),
 *  updating state0 (adagrad: n; ftrl: z) and state1 (ftrl: n; else unused,
 *  may be null), all row-major contiguous f32 shaped as param.  The formulas:
 *  optim_kernels.hip.  A row whose id is >= features or not strictly between
 *  its neighbours' ids is skipped and ORs kLazyErrIds into *error (a device
 *  word the caller zeroed); rows not named are neither read nor written.  No
 *  atomics on the tensors.  nrows == 0 or width == 0 returns before any HIP
 *  call.
 */
void LaunchLazyUpdate(int rule, float* param, const int64_t* ids, const float* grad, float* state0,
                      float* state1, uint64_t features, uint64_t nrows, uint64_t width,
                      const LazyHyper& hyper, uint32_t* error, hipStream_t stream);
// ------------------- histogram GBDT (gbdt_kernels.hip) -------------------
/*! \brief entries of a column segment, the work unit of GB2 / GB3 (one workgroup) */
constexpr uint32_t kGbdtSegmentEntries = 4096;
uint64_t GbdtSegmentEntries();
/*! \brief most cuts (bins) of a feature */
constexpr uint32_t kGbdtMaxBins = 256;
/*! \brief most nodes of one GB3 / GB4 / GB5 call (a tree level: depth 15) */
constexpr uint32_t kGbdtMaxNodes = 1u << 15;
/*! \brief bit GB1 / GB2 OR into their error word: a value is NaN */
constexpr uint32_t kGbdtErrNaN = 1;
/*!
 * \brief the column-major binned matrix: offset [num_features + 1] (from 0),
 *  row / bin [nnz] (rows ascending within a column, bin < the column's cuts),
 *  cut_ptr [num_features + 1] ending at total_bins; `rows` bounds every row id
 */
struct GbdtBinned {
  const int64_t* offset;
  const int32_t* row;
  const uint8_t* bin;
  const int64_t* cut_ptr;
  uint64_t num_features, nnz, rows, total_bins;
};
/*!
 * \brief GB1, first run: counts[f] = distinct quantile candidates of column f,
 *  for keys [nnz] = (feature << 32 | order-preserving u32 of the value) sorted
 *  ascending and the column pointer of `columns` (a transpose of the same
 *  entries: offset [nrows + 1] from 0).  The candidates of a column of n
 *  values s are s[(i n + B - 1) / B - 1], i = 1 .. B = max_bins (2 .. 256).
 *  A column whose first or last value is a NaN ORs kGbdtErrNaN into *error.
 */
void LaunchGbdtCutCount(const int64_t* keys, const CsrView& columns, uint64_t nnz, uint32_t max_bins,
                        int64_t* counts, uint32_t* error, hipStream_t stream);
/*! \brief GB1, second run: the candidates kept, ascending, as cut[cut_ptr[f] ..);
 *  cut_ptr: the exclusive scan of the counts; a position at or past capacity is not written */
void LaunchGbdtCutEmit(const int64_t* keys, const CsrView& columns, uint64_t nnz, uint32_t max_bins,
                       const int64_t* cut_ptr, float* cut, uint64_t capacity, hipStream_t stream);
/*!
 * \brief GB2: for the nnz entries of `columns` (a transpose, pairs or separate
 *  arrays, value may be null: 1.0) row_out[j] = row id and bin_out[j] =
 *  min(#cuts of its column < x, ncuts - 1), 0 for a column without cuts.  No
 *  column may have more than kGbdtMaxBins cuts.  A NaN ORs kGbdtErrNaN.
 */
void LaunchGbdtBin(const CsrView& columns, uint64_t nnz, const int64_t* cut_ptr, const float* cut,
                   int32_t* row_out, uint8_t* bin_out, uint32_t* error, hipStream_t stream);
/*!
 * \brief GB3: hist[node, cut_ptr[f] + bin, :] += (llrint(g[r] scale), llrint(h[r]
 *  scale)) over the entries (r, bin) of every column f, node = pos[r] -
 *  first_node in [0, num_nodes) (other rows are skipped); hist: int64
 *  [num_nodes x total_bins x 2], zeroed by the caller.  Sums are formed in LDS
 *  per segment; integer sums: the same bytes on every run.
 */
void LaunchGbdtHistogram(const GbdtBinned& m, const float* grad, const float* hess,
                         const int32_t* pos, int32_t first_node, uint32_t num_nodes, double scale,
                         int64_t* hist, hipStream_t stream);
/*! \brief bytes of 16-byte aligned scratch of LaunchGbdtBestSplits */
size_t GbdtSplitScratchBytes(uint64_t num_nodes, uint64_t num_features);
/*!
 * \brief GB4: the best split of every node from hist (GB3) and node_sum [N x 2]
 *  (the quantised totals of the node's rows): over features with cuts, bins t
 *  and both sides for the rows without an entry, gain = 1/2 (GL^2 / (HL + l) +
 *  GR^2 / (HR + l) - G^2 / (H + l)) - gamma in f64 on sums / scale, valid with
 *  HL, HR >= min_child_weight, kept if > 0.  Equal gains: the lowest (feature,
 *  bin), then missing-right.  feature[n] = -1 (bin 0, gain 0) without a split.
 */
void LaunchGbdtBestSplits(const int64_t* hist, const int64_t* node_sum, const int64_t* cut_ptr,
                          uint64_t num_features, uint64_t total_bins, uint32_t num_nodes, double scale,
                          double reg_lambda, double gamma, double min_child_weight, void* scratch,
                          int64_t* feature, int32_t* bin, uint8_t* default_left, double* gain,
                          hipStream_t stream);
/*!
 * \brief GB5: pos_out[r] for every row: a row of node n = pos_in[r] -
 *  first_node in [0, num_nodes) goes to left[n] if feature[n] < 0, else by its
 *  entry in column feature[n] (bin <= split_bin[n]: left[n], else right[n]),
 *  and without one to the default side; other rows keep pos_in[r].  Reads pos
 *  once and only the split columns.  pos_out != pos_in.
 */
void LaunchGbdtAdvance(const GbdtBinned& m, const int32_t* pos_in, const int64_t* feature,
                       const int32_t* split_bin, const uint8_t* default_left, const int32_t* left,
                       const int32_t* right, int32_t first_node, uint32_t num_nodes, int32_t* pos_out,
                       hipStream_t stream);
/*! \brief fill n floats with v */
void LaunchFill(float* p, size_t n, float v, hipStream_t stream);
/*!
 * \brief packed H2D (unpack_kernels.hip): expand the packed chunk at `packed`
 *  (device copy of a text_pack.h chunk of n bytes with nexc exception blocks,
 *  256-byte aligned) into exactly n text bytes at dst (any alignment); bytes
 *  past dst + n are not written
 */
void LaunchUnpackText(const void* packed, size_t n, uint32_t nexc, const uint8_t alphabet[16],
                      char* dst, hipStream_t stream);
/*!
 * \brief the same for a dense chunk (text_pack_dense.h) of nranges ranges of
 *  range_blocks blocks: table and directory are read from the chunk's header
 *  on the device.  Exactly n bytes are written at dst (any alignment).
 */
void LaunchUnpackDense(const void* packed, size_t n, uint32_t nranges, uint32_t range_blocks,
                       char* dst, hipStream_t stream);

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_GPU_KERNELS_H_
