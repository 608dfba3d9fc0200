/*!
 * \file src/gpu/device_parser.cc
 * \brief The MI355X ingestion pipeline (see dmlc/gpu/device_parser.h): the
 *  parse strategies on the compute stream, the config keys and the public API.
 *  The text arrives through a ChunkFeed (chunk_feed.h: sources, device slots,
 *  copy / unpack streams and their events, the HBM epoch cache); each chunk is
 *  acquired from it, parsed here and released.
 *
 * LibSVM / LibFM chunks take the LDS-staged tile parser (tile_count_kernels.hip:
 * C1 count, C2 scan, C4 finish; tile_fill_kernels.hip: C3 fill; lane per token,
 * SWAR number decode).
 * A chunk it flags as irregular (qid tokens, digit-less tokens, label-less
 * lines, control bytes), and every CSV chunk the CSV tile kernels
 * (csv_kernels.hip) flag, is parsed by the exact wave-per-line kernels
 * (text_kernels.hip: K1 line index, K2 count, K3 scan, K4 fill).  Both write
 * bit-identical CSR for regular input.
 * The tile kernels write the chunk's sizes and flags into mapped pinned
 * memory (two stream synchronisations per chunk, no D2H copies).  After the
 * first of them the chunk's H2D is known to be complete: the feed recycles
 * its host slot and queues the next copies (FirstSyncDone), so PCIe transfers
 * overlap the kernels.
 * Over HBM-resident text (the feed replays its cache) the next chunk's count
 * + scan is prelaunched on a stream of its own beside the current fill
 * (PrelaunchCount, tile_pipeline.h), or the chunk is parsed in one pass with
 * decoupled look-back (cfg.one_pass / cfg.hash_one_pass).
 */
#include <dmlc/gpu/device_parser.h>
#include <dmlc/fault.h>
#include <dmlc/logging.h>
#include <dmlc/timer.h>

#include <cstdlib>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../io/uri_spec.h"
#include "./chunk_feed.h"
#include "./host_wait.h"
#include "./kernels.h"
#include "./tile_pipeline.h"

namespace dmlc {
namespace gpu {

void DeviceParserConfig::Update(const std::map<std::string, std::string>& args) {
  for (const auto& kv : args) {
    const std::string& k = kv.first;
    const std::string& v = kv.second;
    if (k == "chunk_mb") {
      chunk_bytes = static_cast<size_t>(std::atof(v.c_str()) * (1 << 20));
    } else if (k == "chunk_bytes") {
      chunk_bytes = std::strtoull(v.c_str(), nullptr, 10);
    } else if (k == "pinned_slots") {
      pinned_slots = std::atoi(v.c_str());
    } else if (k == "device_slots") {
      device_slots = std::atoi(v.c_str());
    } else if (k == "read_threads") {
      read_threads = std::atoi(v.c_str());
    } else if (k == "device") {
      device = std::atoi(v.c_str());
    } else if (k == "format") {
      format = v;
    } else if (k == "label_column") {
      label_column = std::atoi(v.c_str());
    } else if (k == "weight_column") {
      weight_column = std::atoi(v.c_str());
    } else if (k == "delimiter") {
      CHECK_EQ(v.size(), 1U) << "delimiter must be one character";
      delimiter = v[0];
    } else if (k == "fast_path") {
      fast_path = v != "0" && v != "false";
    } else if (k == "one_pass") {
      one_pass = v != "0" && v != "false";
    } else if (k == "hash_one_pass") {
      hash_one_pass = v != "0" && v != "false";
    } else if (k == "prelaunch") {
      prelaunch = v != "0" && v != "false";
    } else if (k == "replay_chunk_mb") {
      replay_chunk_bytes = static_cast<size_t>(std::atof(v.c_str()) * (1 << 20));
    } else if (k == "replay_first_mb") {
      replay_first_bytes = static_cast<size_t>(std::atof(v.c_str()) * (1 << 20));
    } else if (k == "zc_pin_budget_mb") {
      zc_pin_budget = static_cast<size_t>(std::atof(v.c_str()) * (1 << 20));
    } else if (k == "zc_window_mb") {
      zc_window_bytes = static_cast<size_t>(std::atof(v.c_str()) * (1 << 20));
    } else if (k == "hbm_cache") {
      hbm_cache = v != "0" && v != "false";
    } else if (k == "wait_spin_us") {
      wait_spin_us = std::atof(v.c_str());
    } else if (k == "shuffle_parts") {
      shuffle_parts = static_cast<unsigned>(std::atoi(v.c_str()));
    } else if (k == "shuffle_seed") {
      shuffle_seed = std::atoi(v.c_str());
    } else if (k == "zero_copy") {
      zero_copy = (v == "auto" || v == "-1") ? -1 : ((v == "0" || v == "false") ? 0 : 1);
    } else if (k == "pack_wait") {
      pack_wait = v != "0" && v != "false";
    } else if (k == "pack_head") {
      pack_head = v != "0" && v != "false";
    } else if (k == "copy_streams") {
      copy_streams = std::atoi(v.c_str());
    } else if (k == "pack_code") {
      CHECK(v == "auto" || v == "-1" || v == "nibble" || v == "dense")
          << "pack_code must be auto, nibble or dense";
      pack_code = v == "nibble" ? 0 : (v == "dense" ? 1 : -1);
    } else if (k == "packed_h2d") {
      packed_h2d = (v == "auto" || v == "-1") ? -1 : ((v == "0" || v == "false") ? 0 : 1);
    }
  }
  chunk_bytes = (chunk_bytes + 4095) & ~size_t(4095);
  CHECK_GE(chunk_bytes, 4096U) << "chunk_bytes too small";
  CHECK_LT(chunk_bytes, size_t(1) << 31) << "chunk_bytes must be < 2 GiB";
  // merged replay chunks go through the same kernels: 32-bit line offsets on
  // the exact path, 32-bit packed token counts on the tile path
  CHECK_LT(replay_chunk_bytes, size_t(1) << 31) << "replay_chunk_bytes must be < 2 GiB";
  CHECK_GE(pinned_slots, 1);
  CHECK_GE(device_slots, 1);
  CHECK(copy_streams == 1 || copy_streams == 2) << "copy_streams must be 1 or 2";
  CHECK_GE(shuffle_parts, 1U) << "shuffle_parts must be >= 1";
}

namespace {

/*! \brief per-chunk sizes the host needs to place the output */
struct ChunkPlan {
  size_t nlines{0}, ntok{0};
  uint64_t nrows{0}, nnz{0};
  unsigned flags{0};
};

template <typename IndexType>
class DeviceParserImpl : public DeviceParser<IndexType> {
 public:
  DeviceParserImpl(const std::string& uri, unsigned part, unsigned nparts,
                   const DeviceParserConfig& cfg)
      : cfg_(cfg) {
    if (cfg_.device >= 0) SetDevice(cfg_.device);
    DMLC_HIP_CHECK(hipGetDevice(&device_));
    if (cfg_.format == "libsvm") {
      tcfg_.format = TextFormat::kLibSVM;
    } else if (cfg_.format == "libfm") {
      tcfg_.format = TextFormat::kLibFM;
    } else if (cfg_.format == "csv") {
      tcfg_.format = TextFormat::kCSV;
    } else {
      LOG(FATAL) << "DeviceParser: unsupported format " << cfg_.format;
    }
    CHECK(tcfg_.format != TextFormat::kCSV || cfg_.label_column < 0 ||
          cfg_.label_column != cfg_.weight_column)
        << "label_column and weight_column must differ";
    tcfg_.label_column = cfg_.label_column;
    tcfg_.weight_column = cfg_.weight_column;
    tcfg_.delimiter = cfg_.delimiter;
    // the parse kernels' stream outranks the prelaunched counts' (a fill's or
    // hash's closing kernels are not queued behind the next chunk's count)
    int least_prio = 0, greatest_prio = 0;
    DMLC_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least_prio, &greatest_prio));
    compute_.reset(new Stream(greatest_prio));
    feed_.reset(new ChunkFeed(uri, part, nparts, cfg_, tcfg_.format == TextFormat::kCSV,
                              compute_->get(), &stats_));
    tiles_.Reserve(LineIndexTiles(cfg_.chunk_bytes) * sizeof(uint64_t));
    // with hbm_cache a second C1/C2 scratch set: the next resident chunk's
    // count + scan runs on its own stream, concurrently with the current fill
    // (PrelaunchCount)
    pre_.Init(2 * sizeof(ChunkMeta), /*with_next=*/cfg_.hbm_cache);
    pre_.cur.Reserve(TileCount(cfg_.chunk_bytes), /*with_masks=*/true);
    hmeta_.Reserve(2 * sizeof(ChunkMeta));
    slots_.Reserve(std::max<size_t>(kMaxPartialBlocks, TileScratchSlots(TileCount(cfg_.chunk_bytes))) *
                   sizeof(MetaPartial));
  }

  ~DeviceParserImpl() override {
    // no kernel still uses the scratch or the feed's text when they go away
    // (the feed drains its own streams); destructors never throw, so errors
    // are ignored here
    if (compute_) (void)hipStreamSynchronize(compute_->get());
    if (pre_.stream) (void)hipStreamSynchronize(pre_.stream->get());
  }

  // a rewind that does not restart a replay of the same order drops the
  // count prelaunched for the next epoch's first chunk (PrelaunchCount)
  void BeforeFirst() override {
    if (!feed_->BeforeFirst()) pre_.Drop();
  }
  void SetEpoch(unsigned e) override {
    if (!feed_->SetEpoch(e)) pre_.Drop();
  }
  void Seek(size_t cursor) override {
    if (!feed_->Seek(cursor)) pre_.Drop();
  }
  unsigned Epoch() const override { return feed_->Epoch(); }
  std::vector<unsigned> VisitOrder() const override { return feed_->VisitOrder(); }
  size_t Tell() const override { return feed_->Tell(); }

  bool Next() override {
    block_.Clear();
    block_.device_ = device_;
    ResetEpoch();
    if (!ProcessOne(&block_, /*append=*/false)) return false;
    FinishEpoch(&block_);
    view_ = block_.View();
    return true;
  }

  const DeviceRowBlock<IndexType>& Value() const override { return view_; }

  void ParseAll(DeviceCSR<IndexType>* out) override {
    ScopedRange range("DeviceParser::ParseAll");
    out->device_ = device_;
    ResetEpoch();
    // one pass per resident chunk: no count to hide behind a previous fill,
    // so no small first chunk
    const bool one_pass = cfg_.one_pass && feed_->Replaying() && cfg_.fast_path &&
                          tcfg_.format != TextFormat::kCSV && !one_pass_off_;
    ChunkFeed::ReplayMerge merge(feed_.get(), one_pass ? ResidentMergeLimit() : 0);
    // pipeline fill (start -> first chunk parsed) and drain (last chunk
    // handed to the pipeline -> pass done), host clock
    const double t0 = GetTime();
    double t_first = 0, t_last_in = 0;
    while (ProcessOne(out, /*append=*/true)) {
      const double t = GetTime();
      if (t_first == 0) t_first = t;
      if (feed_->InputDone() && t_last_in == 0) t_last_in = t;
    }
    FinishEpoch(out);
    const double t_end = GetTime();
    stats_.last_pass_sec = t_end - t0;
    stats_.last_fill_sec = t_first != 0 ? t_first - t0 : 0;
    stats_.last_drain_sec = t_last_in != 0 ? t_end - t_last_in : 0;
  }

  size_t PartitionBytes() const override { return feed_->PartitionBytes(); }
  const DeviceParserStats& Stats() const override { return stats_; }
  hipStream_t stream() const override { return compute_->get(); }

 private:
  void ResetEpoch() {
    acc_max_index_ = acc_max_field_ = 0;
    acc_flags_ = 0;
  }

  /*! \brief the ChunkMeta a kernel wrote into mapped pinned memory (synchronises) */
  ChunkMeta WaitMapped(ChunkMeta* hm) {
    const double t0 = GetTime();
    // polled rather than a blocking stream synchronise per chunk; bounded, so
    // a kernel that never publishes (a fault) still surfaces through the sync
    const ChunkMeta v = TakePublished(hm, cfg_.wait_spin_us, 0.05, &wait_stats_, [this] {
      compute_->Synchronize();
      if (pre_.stream) pre_.stream->Synchronize();
    });
    stats_.wait_gpu_sec += GetTime() - t0;
    stats_.waits_spun = wait_stats_.spun;
    stats_.waits_slept = wait_stats_.slept;
    stats_.waits_timed_out = wait_stats_.timed_out;
    return v;
  }

  /*! \brief device -> host copy of `bytes` at `src` (synchronises the compute stream) */
  template <typename T>
  T ReadBack(const void* src) {
    const double t0 = GetTime();
    DMLC_HIP_CHECK(hipMemcpyAsync(hmeta_.get(), src, sizeof(T), hipMemcpyDeviceToHost,
                                  compute_->get()));
    compute_->Synchronize();
    stats_.wait_gpu_sec += GetTime() - t0;
    T v;
    std::memcpy(&v, hmeta_.get(), sizeof(T));
    return v;
  }

  /*! \brief room for the whole partition, sized from the density of its first
   *  chunk: n items (rows, entries) in nbytes of text, with a margin factor */
  size_t ForPartition(uint64_t n, size_t nbytes, double margin) const {
    const double scale =
        static_cast<double>(PartitionBytes()) / std::max<size_t>(nbytes, 1) * margin;
    return static_cast<size_t>(n * scale) + 1;
  }

  /*! \brief merged chunk limit of a pass over resident text that merges from
   *  its first chunk on (the one-pass kernels, hashed batches): 2 x
   *  replay_chunk_bytes, below 2 GiB (the exact fallback's 32-bit offsets and
   *  the look-back's 31-bit counts) */
  size_t ResidentMergeLimit() const {
    return std::min(2 * cfg_.replay_chunk_bytes, (size_t(1) << 31) - (size_t(64) << 20));
  }

  /*! \brief per-chunk scratch for a chunk of nbytes (chunks may exceed chunk_bytes) */
  void EnsureScratch(size_t nbytes) {
    const size_t tiles = TileCount(nbytes);
    pre_.cur.Reserve(tiles, /*with_masks=*/true);
    slots_.Reserve(std::max<size_t>(kMaxPartialBlocks, TileScratchSlots(tiles)) * sizeof(MetaPartial));
    tiles_.Reserve(LineIndexTiles(nbytes) * sizeof(uint64_t));
  }

  void EnsureLineBuffers(size_t nlines) {
    lines_.Reserve((nlines + 1) * sizeof(uint32_t));
    info_.Reserve((nlines + 1) * sizeof(uint64_t));
    partials_.Reserve((ScanPartials(nlines) + 2) * sizeof(uint64_t));
  }

  /*! \brief the fill target over out's arrays: rows [row_base, row_limit) and
   *  entries [nnz_base, nnz_limit) may be written */
  FillTarget<IndexType> MakeFillTarget(DeviceCSR<IndexType>* out, size_t row_base, size_t nnz_base,
                                       size_t row_limit, size_t nnz_limit, bool with_qid) {
    FillTarget<IndexType> tgt;
    tgt.offset = out->offset();
    tgt.label = out->label();
    // an empty target has no weight column (only the one-pass fill meets one:
    // PrepareOutput has reserved >= 1 row -- its first-chunk Reserve asks for
    // nrows * scale + 1, later chunks follow written rows)
    tgt.weight = out->weight_capacity() >= out->row_capacity() && out->row_capacity() != 0
                     ? out->weight()
                     : nullptr;
    tgt.qid = with_qid ? out->qid() : nullptr;
    tgt.field = tcfg_.format == TextFormat::kLibFM ? out->field() : nullptr;
    tgt.index = out->index();
    tgt.value = out->value();
    tgt.row_base = row_base;
    tgt.nnz_base = nnz_base;
    tgt.row_limit = row_limit;
    tgt.nnz_limit = nnz_limit;
    return tgt;
  }

  /*! \brief grow the output for this chunk and build the fill target */
  FillTarget<IndexType> PrepareOutput(DeviceCSR<IndexType>* out, size_t row_base, size_t nnz_base,
                                      const ChunkPlan& plan, bool need_weight, size_t nbytes) {
    hipStream_t s = compute_->get();
    const bool libfm = tcfg_.format == TextFormat::kLibFM;
    if (row_base == 0) {
      // first chunk: reserve for the whole partition from this chunk's density
      out->Reserve(ForPartition(plan.nrows, nbytes, 1.05), ForPartition(plan.nnz, nbytes, 1.05),
                   libfm, s, 0, 0);
    }
    out->Reserve(row_base + plan.nrows, nnz_base + plan.nnz, libfm, s, row_base, nnz_base);
    if (need_weight) out->EnableWeight(s);
    if (plan.flags & kFlagQid) {
      out->EnableQid(s);
      out->has_qid_ = true;
    }
    return MakeFillTarget(out, row_base, nnz_base, row_base + plan.nrows, nnz_base + plan.nnz,
                          out->has_qid_);
  }

  /*! \brief the tile pipeline's count + scan (LibSVM / LibFM C1 + C2, or CSV S1 + scan) */
  void LaunchCountScan(const char* text, size_t nbytes, const TileScratchSet& set, hipStream_t s) {
    uint64_t* counts = set.counts.get<uint64_t>();
    uint32_t* flags = set.flags.get<uint32_t>();
    uint32_t* masks = set.masks.get<uint32_t>();
    if (tcfg_.format == TextFormat::kCSV) {
      LaunchCsvTileCount(text, nbytes, tcfg_.label_column, tcfg_.weight_column, tcfg_.delimiter,
                         counts, flags, masks, s);
      LaunchTileScanRaw(counts, flags, TileCount(nbytes), set.dmeta(), set.hmeta(), s);
    } else {
      LaunchTileCountScan(text, nbytes, counts, flags, masks, set.dmeta(), set.hmeta(), s);
    }
  }

  /*! \brief count + scan of this chunk into the current scratch set: adopt the
   *  prelaunched set when it holds this chunk (queued behind the previous
   *  fill), else launch them now */
  void CountScanCurrent(const char* text, size_t nbytes) {
    if (pre_.Adopt(text, nbytes, compute_->get())) return;
    pre_.Drop();
    LaunchCountScan(text, nbytes, pre_.cur, compute_->get());
  }

  /*!
   * \brief LDS-staged tile parse (tile_common.h); false when the chunk must
   *  take the exact path.  One blocking read-back (the chunk's sizes) before
   *  the fill, one for the maxima / flags after it.
   */
  bool FastParse(const char* text, size_t nbytes, DeviceCSR<IndexType>* out, size_t row_base,
                 size_t nnz_base, ChunkPlan* plan) {
    hipStream_t s = compute_->get();
    CountScanCurrent(text, nbytes);
    ChunkMeta* dmeta = pre_.cur.dmeta();
    ChunkMeta* hm = pre_.cur.hmeta();
    const ChunkMeta sizes = WaitMapped(hm);
    feed_->FirstSyncDone();
    if (sizes.flags & kFlagIrregular) return false;
    plan->nlines = sizes.nlines;
    plan->nrows = sizes.nrows;
    plan->nnz = sizes.nnz;
    // LibSVM `qid:` tokens: the column is needed (LibFM has none: a 'q'
    // token there is irregular and the chunk goes to the exact kernels)
    if (tcfg_.format == TextFormat::kLibSVM) plan->flags |= sizes.flags & kFlagQid;
    bool need_weight = false;
    for (;;) {
      FillTarget<IndexType> tgt = PrepareOutput(out, row_base, nnz_base, *plan, need_weight, nbytes);
      if (tgt.qid != nullptr && plan->nrows != 0) {
        // rows without a `qid:` token have qid 0; the fill writes the others
        DMLC_HIP_CHECK(hipMemsetAsync(tgt.qid + row_base, 0, plan->nrows * sizeof(uint64_t), s));
      }
      LaunchTileFill<IndexType>(text, nbytes, tcfg_.format, pre_.cur.counts.get<uint64_t>(),
                                pre_.cur.masks.get<uint32_t>(), tgt,
                                slots_.get<MetaPartial>(), dmeta, hm, s);
      PrelaunchCount();
      ChunkMeta m = WaitMapped(hm);
      if (m.flags & kFlagIrregular) return false;
      if ((m.flags & kFlagNeedWeight) && !need_weight) {
        // first weighted row of the epoch: allocate the column (earlier rows
        // get 1.0) and write this chunk again with it
        need_weight = true;
        m.flags &= ~kFlagNeedWeight;
        DMLC_HIP_CHECK(hipMemcpyAsync(dmeta, &sizes, sizeof(ChunkMeta), hipMemcpyHostToDevice, s));
        continue;
      }
      CHECK(!(m.flags & kFlagNeedWeight)) << "internal error: weight column not allocated";
      Accumulate(m);
      return true;
    }
  }

  /*!
   * \brief CSV on the tile pipeline (csv_kernels.hip): lane-per-row count ->
   *  raw scan -> fill -> finish, both size read-outs through mapped pinned
   *  memory; false when the chunk must take the exact path (rows longer than
   *  the tile extension, control bytes), found by the count (S1) or, with
   *  positional counts (S1p), by the fill.
   */
  bool CsvFastParse(const char* text, size_t nbytes, DeviceCSR<IndexType>* out, size_t row_base,
                    size_t nnz_base, ChunkPlan* plan) {
    hipStream_t s = compute_->get();
    const size_t ntiles = TileCount(nbytes);
    CountScanCurrent(text, nbytes);
    ChunkMeta* dmeta = pre_.cur.dmeta();
    ChunkMeta* hm = pre_.cur.hmeta();
    const ChunkMeta sizes = WaitMapped(hm);
    feed_->FirstSyncDone();
    if (sizes.flags & kFlagIrregular) return false;
    plan->nlines = sizes.nrows;
    plan->nrows = sizes.nrows;
    plan->nnz = sizes.nnz;
    const bool need_weight = tcfg_.weight_column >= 0;
    FillTarget<IndexType> tgt = PrepareOutput(out, row_base, nnz_base, *plan, need_weight, nbytes);
    LaunchCsvTileFill<IndexType>(text, nbytes, tcfg_.label_column, tcfg_.weight_column,
                                 tcfg_.delimiter, pre_.cur.counts.get<uint64_t>(),
                                 pre_.cur.masks.get<uint32_t>(), tgt,
                                 slots_.get<MetaPartial>(), s);
    LaunchTileFinish(slots_.get<MetaPartial>(), ntiles, dmeta, hm, tgt.offset, row_base, nnz_base,
                     s);
    PrelaunchCount();
    const ChunkMeta m = WaitMapped(hm);
    // with positional counts (S1p) the fill is where control bytes, crowded
    // steps and over-long rows are found: the exact kernels rewrite the chunk
    if (m.flags & kFlagIrregular) return false;
    Accumulate(m);
    return true;
  }

  /*!
   * \brief the exact kernels' index of a chunk: K1 line starts (lines_), K2
   *  per-line row validity / entry counts and K3 their scan (info_); returns
   *  the chunk's lines, rows, entries and K2's flags (two read-backs)
   */
  ChunkPlan ExactIndex(const char* text, size_t nbytes, bool first_sync_done) {
    hipStream_t s = compute_->get();
    ChunkMeta* dmeta = pre_.cur.dmeta();
    ChunkPlan plan;
    DMLC_HIP_CHECK(hipMemsetAsync(dmeta, 0, sizeof(ChunkMeta), s));
    LaunchLineCount(text, nbytes, tiles_.get<uint64_t>(), dmeta, s);
    plan.nlines = ReadBack<ChunkMeta>(dmeta).nlines;
    if (!first_sync_done) feed_->FirstSyncDone();
    EnsureLineBuffers(plan.nlines);
    LaunchLineEmit(text, nbytes, tiles_.get<uint64_t>(), lines_.get<uint32_t>(), s);
    LaunchTextCount(text, nbytes, lines_.get<uint32_t>(), plan.nlines, tcfg_,
                    info_.get<uint64_t>(), slots_.get<MetaPartial>(), dmeta, s);
    uint64_t* total = partials_.get<uint64_t>() + ScanPartials(plan.nlines) + 1;
    LaunchScanU64(info_.get<uint64_t>(), plan.nlines, partials_.get<uint64_t>(), total, s);
    LaunchMetaFromTotal(total, dmeta, s);
    const ChunkMeta hm = ReadBack<ChunkMeta>(dmeta);
    plan.nrows = hm.nrows;
    plan.nnz = hm.nnz;
    plan.flags = hm.flags;
    return plan;
  }

  /*! \brief exact wave-per-line parse (any input) */
  void ExactParse(const char* text, size_t nbytes, DeviceCSR<IndexType>* out, size_t row_base,
                  size_t nnz_base, ChunkPlan* plan, bool first_sync_done) {
    hipStream_t s = compute_->get();
    ChunkMeta* dmeta = pre_.cur.dmeta();
    *plan = ExactIndex(text, nbytes, first_sync_done);
    const bool csv = tcfg_.format == TextFormat::kCSV;
    const bool need_weight = (plan->flags & kFlagWeight) || (csv && tcfg_.weight_column >= 0);
    FillTarget<IndexType> tgt = PrepareOutput(out, row_base, nnz_base, *plan, need_weight, nbytes);
    DMLC_HIP_CHECK(hipMemsetAsync(dmeta, 0, sizeof(ChunkMeta), s));
    LaunchTextFill<IndexType>(text, nbytes, lines_.get<uint32_t>(), plan->nlines, tcfg_,
                              info_.get<uint64_t>(), tgt, plan->nrows, plan->nnz,
                              slots_.get<MetaPartial>(), dmeta, s);
    ChunkMeta m = ReadBack<ChunkMeta>(dmeta);
    m.flags |= plan->flags & (kFlagWeight | kFlagQid);
    if (csv && tcfg_.weight_column >= 0) m.flags |= kFlagWeight;
    Accumulate(m);
  }

  void CheckNoNegativeIndex(const ChunkMeta& m) const {
    CHECK(!(m.flags & kFlagNegIndex)) << "negative feature index in " << cfg_.format << " input";
  }

  void Accumulate(const ChunkMeta& m) {
    CheckNoNegativeIndex(m);
    CHECK(!(m.flags & kFlagOverflow))
        << "internal error: GPU fill pass disagreed with the count pass (writes were dropped)";
    acc_max_index_ = std::max<uint64_t>(acc_max_index_, m.max_index);
    acc_max_field_ = std::max<uint64_t>(acc_max_field_, m.max_field);
    acc_flags_ |= m.flags;
  }

  /*!
   * \brief ParseAll over HBM-resident text: queue the next chunk's count +
   *  scan (C1 + C2) into the second scratch set right behind the current
   *  fill, so the GPU does not idle while the host reads the fill's result
   *  and turns around (~20-50 us per chunk in the trace).  The next FastParse
   *  adopts the set when its chunk is the one prelaunched.
   */
  void PrelaunchCount() {
    if (!feed_->MergingReplay() || pre_.valid || !cfg_.prelaunch) return;
    const char* text = nullptr;
    size_t nbytes = 0;
    // the next chunk of this pass or, while the epoch's last chunk is being
    // parsed, the next epoch's first one (a ParseAll over the cache replays
    // the same merge); a next pass that starts otherwise drops the count
    // unused (CountScanCurrent matches text and size)
    if (feed_->PeekNextResident(&text, &nbytes) || feed_->NextEpochFirst(&text, &nbytes)) {
      PrelaunchFor(text, nbytes);
    }
  }

  void PrelaunchFor(const char* text, size_t nbytes) {
    // its own stream: count + scan (HBM- and VALU-light next to the fill)
    // overlap the current fill instead of queueing behind it
    pre_.Launch(text, nbytes, TileCount(nbytes), /*with_masks=*/true,
                [&](const TileScratchSet& set, hipStream_t s) {
                  LaunchCountScan(text, nbytes, set, s);
                });
  }

  /*!
   * \brief take the next device-resident chunk from the feed and run
   *  body(text, nbytes) on it (compute stream, after its H2D); false at the
   *  end.  The feed recycles the slots and keeps the resume cursor, also when
   *  body throws (ChunkFeed::Release).
   */
  template <typename Body>
  bool WithNextChunk(Body body) {
    DMLC_FAULT_POINT("parse");
    ChunkFeed::Chunk cur;
    if (!feed_->Acquire(&cur)) return false;
    try {
      EnsureScratch(cur.size);
      ScopedRange range("parse_chunk");
      body(cur.text, cur.size);
      DMLC_FAULT_POINT("parse_fill");
    } catch (...) {
      feed_->Release(/*delivered=*/false);
      throw;
    }
    feed_->Release(/*delivered=*/true);
    return true;
  }

  /*! \brief outcome of a one-pass chunk: written, needs the counted tile
   *  path (qid tokens), or needs the exact kernels (irregular text) */
  enum class OnePass { kDone, kCounted, kExact };

  /*!
   * \brief one-pass tile parse of a resident chunk (k_tile_fill<kOnePass>):
   *  look-back instead of C1 + C2, written straight into the target's
   *  capacity -- a single launch and one host wait per chunk.  Grows the
   *  target and runs again when the chunk did not fit (or met the first
   *  weighted row); chunks with letter-started tokens go to the counted path
   *  (`qid:` data: every later resident chunk too, see ProcessOne).
   */
  OnePass OnePassParse(const char* text, size_t nbytes, DeviceCSR<IndexType>* out, size_t row_base,
                       size_t nnz_base, ChunkPlan* plan) {
    hipStream_t s = compute_->get();
    pre_.Drop();
    ChunkMeta* dmeta = pre_.cur.dmeta();
    ChunkMeta* hm = pre_.cur.hmeta();
    const bool libfm = tcfg_.format == TextFormat::kLibFM;
    const size_t tiles = TileCount(nbytes);
    fstatus_.Reserve(tiles * sizeof(uint64_t));  // zeroed by the launcher, per launch
    tickets_.Ensure(s);
    bool first_wait = true;
    for (;;) {
      // every row / entry the capacity holds (the row pointer has one slot
      // more); no qid column: qid chunks take the counted path
      FillTarget<IndexType> tgt = MakeFillTarget(out, row_base, nnz_base, out->row_capacity(),
                                                 out->nnz_capacity(), /*with_qid=*/false);
      if (libfm && tgt.field == nullptr) tgt.nnz_limit = 0;
      const FillOnePass op{tickets_.For(fstatus_.get<uint64_t>())};
      tickets_.Advance(LaunchTileFill<IndexType>(text, nbytes, tcfg_.format, nullptr, nullptr, tgt,
                                                 slots_.get<MetaPartial>(), dmeta, hm, s, &op));
      ChunkMeta m = WaitMapped(hm);
      if (first_wait) {
        feed_->FirstSyncDone();
        first_wait = false;
      }
      // letter-started tokens: `qid:` (the counted path writes the zeroed
      // qid column; ProcessOne makes that sticky once it finds real ones)
      // or junk (the counted path sends the chunk on to the exact kernels)
      if (m.flags & kFlagQid) return OnePass::kCounted;
      if (m.flags & kFlagIrregular) return OnePass::kExact;
      if (m.flags & kFlagOverflow) {
        // grow to the chunk's sizes -- for the whole partition at its density
        // when this is the pass's first chunk (a new target) -- and run again
        size_t want_rows = row_base + m.nrows, want_nnz = nnz_base + m.nnz;
        if (row_base == 0) {
          want_rows = std::max(want_rows, ForPartition(m.nrows, nbytes, 1.05));
          want_nnz = std::max(want_nnz, ForPartition(m.nnz, nbytes, 1.05));
        }
        out->Reserve(want_rows, want_nnz, libfm, s, row_base, nnz_base);
        stats_.one_pass_reruns += 1;
        continue;
      }
      if ((m.flags & kFlagNeedWeight) && tgt.weight == nullptr) {
        out->EnableWeight(s);  // earlier rows get 1.0; write this chunk again with it
        stats_.one_pass_reruns += 1;
        continue;
      }
      m.flags &= ~kFlagNeedWeight;
      plan->nlines = m.nlines;
      plan->nrows = m.nrows;
      plan->nnz = m.nnz;
      Accumulate(m);
      stats_.one_pass_chunks += 1;
      return OnePass::kDone;
    }
  }

  /*! \brief parse one chunk into out (append or replace); false at end */
  bool ProcessOne(DeviceCSR<IndexType>* out, bool append) {
    const size_t row_base = append ? out->rows_ : 0;
    const size_t nnz_base = append ? out->nnz_ : 0;
    ChunkPlan plan;
    const bool csv = tcfg_.format == TextFormat::kCSV;
    const bool more = WithNextChunk([&](const char* text, size_t nbytes) {
      bool done = false;
      if (cfg_.fast_path) {
        // resident text (HBM replay) of a regular format: one pass, no count
        // kernel and no host turnaround between count and fill
        const bool one_pass = cfg_.one_pass && !csv && feed_->Replaying() && append &&
                              !one_pass_off_ && nbytes != 0;
        const OnePass r = one_pass ? OnePassParse(text, nbytes, out, row_base, nnz_base, &plan)
                                   : OnePass::kCounted;
        if (r == OnePass::kDone) {
          done = true;
        } else if (r == OnePass::kCounted) {
          done = csv ? CsvFastParse(text, nbytes, out, row_base, nnz_base, &plan)
                     : FastParse(text, nbytes, out, row_base, nnz_base, &plan);
          // qid data: every later resident chunk goes straight to this path
          if (done && feed_->Replaying() && (plan.flags & kFlagQid)) one_pass_off_ = true;
        }
        if (!done) stats_.exact_chunks += 1;
      }
      if (!done) ExactParse(text, nbytes, out, row_base, nnz_base, &plan, cfg_.fast_path);
    });
    if (!more) return false;
    out->rows_ = row_base + plan.nrows;
    out->nnz_ = nnz_base + plan.nnz;
    if (acc_flags_ & kFlagWeight) out->has_weight_ = true;
    if (tcfg_.format == TextFormat::kCSV) out->has_value_ = out->nnz_ != 0;
    if (tcfg_.format == TextFormat::kLibFM) out->has_field_ = true;
    stats_.rows += plan.nrows;
    stats_.nnz += plan.nnz;
    return true;
  }

  void ParseAllHashed(DeviceHashedBatch* out, int dim, float scale, uint32_t seed,
                      bool fp8) override {
    CHECK(tcfg_.format != TextFormat::kCSV) << "hashed batches are built from LibSVM / LibFM";
    CHECK(dim > 0 && dim % 4 == 0 && dim <= 4096) << "dim must be a multiple of 4 in (0, 4096]";
    ScopedRange range("DeviceParser::ParseAllHashed");
    if (out->row_cap != 0 && (out->dim != dim || out->fp8 != fp8 || out->device != device_)) {
      *out = DeviceHashedBatch();  // a reused batch of another shape: reallocate
    }
    out->device = device_;
    out->dim = dim;
    out->fp8 = fp8;
    out->rows = 0;
    // resident text and a batch that already has rows (a reused one): one pass
    // per chunk (k_tile_hash look-back, no C1 / C2) with hash_one_pass, else
    // the counted kernel; either way a merged chunk costs one host turnaround,
    // so merge up to 2 x replay_chunk_bytes from the start (measured: 1.97 ->
    // 1.91 ms per 1.49 GB pass with the whole pass in one chunk; below 2 GiB:
    // an irregular chunk falls back to the exact kernels' 32-bit offsets, as
    // DeviceParserConfig::Update checks for replay_chunk_bytes)
    const bool tile = cfg_.fast_path && dim % 16 == 0;  // else the exact kernels alone
    const bool reused = feed_->Replaying() && out->row_cap != 0 && tile;
    const bool one_pass = cfg_.hash_one_pass && reused;
    // resident text: parse adjacent cached chunks together
    ChunkFeed::ReplayMerge merge(feed_.get(), reused ? ResidentMergeLimit() : 0);
    while (WithNextChunk([&](const char* text, size_t nbytes) {
      bool done = false;
      if (one_pass && nbytes != 0 && out->row_cap != 0) {
        done = HashedOnePass(text, nbytes, out, scale, seed);
      } else if (tile) {
        done = HashedCounted(text, nbytes, out, scale, seed);
      }
      if (tile && !done) stats_.exact_chunks += 1;
      if (!done) HashedExact(text, nbytes, out, scale, seed, /*first_sync_done=*/tile);
    })) {
    }
    compute_->Synchronize();
  }

  /*! \brief room for chunk_rows more rows.  The first chunk sizes the batch for
   *  the whole partition from its density (no doubling copies of a multi-GB
   *  batch); a reused batch usually fits already */
  void ReserveHashed(DeviceHashedBatch* out, size_t chunk_rows, size_t nbytes) {
    if (out->rows == 0) {
      out->Reserve(ForPartition(chunk_rows, nbytes, 1.02), compute_->get());
    }
    out->Reserve(out->rows + chunk_rows, compute_->get());
  }

  /*! \brief one pass over a resident chunk into a batch that has capacity
   *  (k_tile_hash look-back, no C1 / C2); false: irregular, the exact kernels */
  bool HashedOnePass(const char* text, size_t nbytes, DeviceHashedBatch* out, float scale,
                     uint32_t seed) {
    hipStream_t s = compute_->get();
    pre_.Drop();
    ChunkMeta* dmeta = pre_.cur.dmeta();
    ChunkMeta* hm = pre_.cur.hmeta();
    const size_t tiles = TileCount(nbytes);
    if (hstatus_.bytes() < tiles * sizeof(uint64_t)) {
      hstatus_.Reserve(tiles * sizeof(uint64_t));
      DMLC_HIP_CHECK(hipMemsetAsync(hstatus_.get(), 0, hstatus_.bytes(), s));
    }
    tickets_.Ensure(s);
    for (;;) {
      if (++htag_ >= (1u << 30)) {  // tags wrapped: old words could match again
        htag_ = 1;
        DMLC_HIP_CHECK(hipMemsetAsync(hstatus_.get(), 0, hstatus_.bytes(), s));
      }
      const HashOnePass op{tickets_.For(hstatus_.get<uint64_t>()), htag_, out->row_cap};
      tickets_.Advance(LaunchTileHashed<IndexType>(
          text, nbytes, tcfg_.format, nullptr, nullptr, out->rows, 0, out->dim, scale, seed,
          out->fp8, out->x->get(), out->label->get<float>(), slots_.get<MetaPartial>(), dmeta, hm,
          s, &op));
      const ChunkMeta m = WaitMapped(hm);
      feed_->FirstSyncDone();
      CheckNoNegativeIndex(m);
      if (m.flags & kFlagIrregular) return false;
      if (m.flags & kFlagOverflow) {
        // more rows than the batch holds: grow it, write the chunk again
        ReserveHashed(out, m.nrows, nbytes);
        continue;
      }
      out->rows += m.nrows;
      stats_.rows += m.nrows;
      stats_.one_pass_chunks += 1;
      return true;
    }
  }

  /*! \brief tile parser: C1 + C2 sizes, then the fused tile kernel builds the
   *  rows of the lines each workgroup owns; false: irregular, the exact kernels */
  bool HashedCounted(const char* text, size_t nbytes, DeviceHashedBatch* out, float scale,
                     uint32_t seed) {
    hipStream_t s = compute_->get();
    CountScanCurrent(text, nbytes);  // may adopt a prelaunched count + scan
    ChunkMeta* hm = pre_.cur.hmeta();
    const ChunkMeta sizes = WaitMapped(hm);
    feed_->FirstSyncDone();
    if (sizes.flags & kFlagIrregular) return false;
    ReserveHashed(out, sizes.nrows, nbytes);
    LaunchTileHashed<IndexType>(text, nbytes, tcfg_.format, pre_.cur.counts.get<uint64_t>(),
                                pre_.cur.masks.get<uint32_t>(), out->rows, sizes.nlines, out->dim,
                                scale, seed, out->fp8, out->x->get(), out->label->get<float>(),
                                slots_.get<MetaPartial>(), pre_.cur.dmeta(), hm, s);
    PrelaunchCount();
    const ChunkMeta m = WaitMapped(hm);
    CheckNoNegativeIndex(m);
    if (m.flags & kFlagIrregular) return false;
    out->rows += sizes.nrows;
    stats_.rows += sizes.nrows;
    return true;
  }

  /*! \brief K1 line index, K2 row validity + K3 scan (as the exact CSR path),
   *  then the fused per-line hash kernel writes rows straight into the batch */
  void HashedExact(const char* text, size_t nbytes, DeviceHashedBatch* out, float scale,
                   uint32_t seed, bool first_sync_done) {
    hipStream_t s = compute_->get();
    ChunkMeta* dmeta = pre_.cur.dmeta();
    const ChunkPlan plan = ExactIndex(text, nbytes, first_sync_done);
    ReserveHashed(out, plan.nrows, nbytes);
    DMLC_HIP_CHECK(hipMemsetAsync(dmeta, 0, sizeof(ChunkMeta), s));
    LaunchTextHashed<IndexType>(text, nbytes, lines_.get<uint32_t>(), plan.nlines, tcfg_.format,
                                info_.get<uint64_t>(), out->rows, out->dim, scale, seed, out->fp8,
                                out->x->get(), out->label->get<float>(), slots_.get<MetaPartial>(),
                                dmeta, s);
    CheckNoNegativeIndex(ReadBack<ChunkMeta>(dmeta));
    out->rows += plan.nrows;
    stats_.rows += plan.nrows;
  }

  /*! \brief publish the accumulated max / flags of this epoch */
  void FinishEpoch(DeviceCSR<IndexType>* out) {
    out->max_index_ = std::max<uint64_t>(out->max_index_, acc_max_index_);
    out->max_field_ = std::max<uint64_t>(out->max_field_, acc_max_field_);
    if (acc_flags_ & kFlagValue) out->has_value_ = true;
    if (acc_flags_ & kFlagWeight) out->has_weight_ = true;
    if (out->rows_ == 0) {
      // keep a valid (zero) closing offset for empty partitions
      out->Reserve(1, 1, false, compute_->get());
      DMLC_HIP_CHECK(hipMemsetAsync(out->offset(), 0, sizeof(uint64_t), compute_->get()));
    }
    compute_->Synchronize();
  }

  DeviceParserConfig cfg_;
  TextParseConfig tcfg_;
  int device_{0};
  DeviceParserStats stats_;
  std::unique_ptr<Stream> compute_;
  /*! \brief chunk transport (after compute_ and stats_, which it uses) */
  std::unique_ptr<ChunkFeed> feed_;
  DeviceBuffer tiles_, lines_, info_, partials_;
  /*! \brief tile parser scratch (pre_.cur: counts, flags, masks, the device
   *  ChunkMeta and the mapped pinned one the tile kernels write directly) and,
   *  with hbm_cache, the prelaunched next chunk's C1 + C2 set and stream */
  CountPrelaunch pre_;
  /*! \brief per-workgroup reduction slots (MetaPartial) */
  DeviceBuffer slots_;
  PinnedBuffer hmeta_;
  // one-pass hashed batches: look-back words and their launch tag
  DeviceBuffer hstatus_;
  uint32_t htag_{0};
  // one-pass CSR fill: look-back words (zeroed per launch)
  DeviceBuffer fstatus_;
  /*! \brief workgroup tickets of both one-pass kernels */
  OnePassTickets tickets_;
  /*! \brief qid data met: resident chunks take the counted tile path */
  bool one_pass_off_{false};
  uint64_t acc_max_index_{0}, acc_max_field_{0};
  unsigned acc_flags_{0};
  DeviceCSR<IndexType> block_;
  DeviceRowBlock<IndexType> view_;
  HostWaitStats wait_stats_;
};

}  // namespace

template <typename IndexType>
DeviceParser<IndexType>* DeviceParser<IndexType>::Create(const std::string& uri,
                                                         unsigned part_index, unsigned num_parts,
                                                         const DeviceParserConfig& cfg) {
  io::URISpec spec(uri, part_index, num_parts);
  DeviceParserConfig c = cfg;
  c.Update(spec.args);
  return new DeviceParserImpl<IndexType>(spec.uri, part_index, num_parts, c);
}

template class DeviceParser<uint32_t>;
template class DeviceParser<uint64_t>;

}  // namespace gpu
}  // namespace dmlc
