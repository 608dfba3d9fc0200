/*!
 * \file src/gpu/chunk_feed.cc
 * \brief Chunk transport of the device parser (see chunk_feed.h).
 */
#include "./chunk_feed.h"

#include <dmlc/fault.h>
#include <dmlc/logging.h>
#include <dmlc/timer.h>

#include <algorithm>
#include <cstring>

#include "../io/filesys.h"
#include "../io/line_split.h"
#include "./kernels.h"
#include "./text_pack.h"
#include "./text_pack_codec.h"
#include "./text_pack_dense.h"

namespace dmlc {
namespace gpu {

ChunkFeed::ChunkFeed(const std::string& uri, unsigned part, unsigned nparts,
                     const DeviceParserConfig& cfg, bool csv_alphabet, hipStream_t compute,
                     DeviceParserStats* stats)
    : cfg_(cfg),
      compute_(compute),
      stats_(stats),
      walk_(&plan_, cfg.replay_first_bytes, cfg.replay_chunk_bytes) {
  io::URI path(uri.c_str());
  split_.reset(new io::LineSplitter(io::FileSystem::GetInstance(path), uri.c_str(), part, nparts));
  if (cfg_.shuffle_parts > 1) {
    // sub-shard i = partition part * K + i of nparts * K (record-aligned
    // byte ranges, as InputSplitShuffle's source splits); the pipeline reads
    // the epoch's concatenation of them
    const unsigned k = cfg_.shuffle_parts;
    std::vector<std::vector<EpochOrder::Segment>> subs;
    for (unsigned i = 0; i < k; ++i) {
      split_->ResetPartition(part * k + i, nparts * k);
      subs.push_back(split_->ShardSegments());
    }
    order_ = EpochOrder(part, nparts, k, cfg_.shuffle_seed, subs);  // epoch 0
    reader_.reset(new io::ShardReader(split_.get(), cfg_.read_threads, order_.Segments(),
                                      order_.Stops()));
  } else {
    order_ = EpochOrder(part, nparts, 1, cfg_.shuffle_seed, {split_->ShardSegments()});
    reader_.reset(new io::ShardReader(split_.get(), cfg_.read_threads));
  }
  // with hbm_cache only the first pass crosses the link, and the replay's
  // prelaunch stream is the process's fifth: a second copy stream beside it
  // measured 1,914 -> 1,537 M rows/s on the replay (profiles/link_idle)
  ncopy_ = (cfg_.copy_streams == 1 || cfg_.hbm_cache) ? 1 : 2;
  for (size_t s = 0; s < ncopy_; ++s) copy_[s].reset(new Stream());
  zeroed_.reset(new Event());
  for (int d = 0; d < cfg_.device_slots; ++d) {
    dtext_.emplace_back(new DeviceBuffer(cfg_.chunk_bytes + kTextPadBytes));
    // the pad is read (never used) by 16-byte loads past the chunk end.  The
    // memsets go on a copy stream: the streams are non-blocking, so a
    // null-stream hipMemset is not ordered before the H2D copy into the slot
    MemsetOrdered(dtext_.back()->get(), cfg_.chunk_bytes + kTextPadBytes);
    copied_.emplace_back(new Event());
    parsed_.emplace_back(new Event());
    parsed_.back()->Record(compute_);
  }
  iter_.set_max_capacity(static_cast<size_t>(cfg_.pinned_slots));
  if (cfg_.zero_copy != 0) {
    zc_.reset(new ZeroCopySource());
    const double t0 = GetTime();
    // windowed source: before a window is released, no queued piece may still
    // point into it, no pool thread may still read it and no DMA may
    zc_->SetDrain([this]() {
      RescueLookahead();
      SyncCopyStreams();
    });
    stats_->zc_pin_budget = ZeroCopySource::ShardPinBudget(cfg_.zc_pin_budget);
    if (!zc_->Init(split_.get(), cfg_.chunk_bytes, stats_->zc_pin_budget, cfg_.zc_window_bytes,
                   order_.shuffled() ? &order_.all_segments() : nullptr)) {
      CHECK(cfg_.zero_copy != 1) << "zero_copy=1 but the input cannot be mmap'ed + registered";
      zc_.reset();
    } else {
      stats_->register_sec = GetTime() - t0;
      stats_->zero_copy = true;
      if (order_.shuffled()) zc_->Reorder(order_.SegmentIndices());
    }
  }
  if (zc_ == nullptr) StartReader();
  if (zc_ != nullptr &&
      (cfg_.packed_h2d == 1 ||
       (cfg_.packed_h2d < 0 && cfg_.read_threads >= 2 && cfg_.chunk_bytes >= (size_t(1) << 20)))) {
    StartPacking(csv_alphabet);
  }
  if (cfg_.hbm_cache) StartCaching();
}

ChunkFeed::~ChunkFeed() {
  // make sure no transfer still reads a pinned slot we are about to free;
  // destructors never throw, so errors are ignored here
  for (auto& s : copy_) {
    if (s) (void)hipStreamSynchronize(s->get());
  }
  if (unpack_) (void)hipStreamSynchronize(unpack_->get());
  (void)hipStreamSynchronize(compute_);
  for (auto& f : inflight_) {
    if (f.slot != nullptr) iter_.Recycle(&f.slot);
  }
  inflight_.clear();
  iter_.Destroy();
  pool_.reset();  // before the mappings its threads read go away
  zc_.reset();
}

/*! \brief every copy queued so far is done */
void ChunkFeed::SyncCopyStreams() const {
  for (size_t s = 0; s < ncopy_; ++s) copy_[s]->Synchronize();
}

/*! \brief zero device memory before the first copy into it, whichever copy
 *  stream that copy runs on (rare: construction, a regrown slot, the arena) */
void ChunkFeed::MemsetOrdered(void* ptr, size_t bytes) {
  DMLC_HIP_CHECK(hipMemsetAsync(ptr, 0, bytes, copy_[0]->get()));
  if (ncopy_ < 2) return;
  zeroed_->Record(copy_[0]->get());
  DMLC_HIP_CHECK(hipStreamWaitEvent(copy_[1]->get(), zeroed_->get(), 0));
}

bool ChunkFeed::SetEpoch(unsigned e) {
  if (head_) DropLookahead();  // only a plain rewind adopts head jobs
  if (!order_.shuffled()) return Seek(0);
  DrainInflight();
  order_.Apply(e);
  if (zc_ != nullptr) {
    zc_->Reorder(order_.SegmentIndices());
  } else {
    reorder_reader_ = true;  // applied by the reader thread's rewind (Seek)
  }
  return Seek(0);
}

bool ChunkFeed::Seek(size_t cursor) {
  CHECK_LE(cursor, PartitionBytes()) << "DeviceParser::Seek: cursor beyond the partition";
  // a replay restarting at 0 keeps the next epoch's first count, prelaunched
  // beside the last fill (NextEpochFirst; dropped if the chunk differs)
  const bool keep_prelaunch = cursor == 0 && cache_complete_ && !order_.shuffled();
  // a rewind after a whole pass: this user runs pass after pass (QueueHeadJobs)
  if (cursor == 0 && reader_done_ && inflight_.empty() && busy_ == 0 && cursor_ != 0 &&
      cursor_ == PartitionBytes()) {
    head_armed_ = true;
  }
  // head jobs become this pass's lookahead: the source's cursor is after them
  const bool adopt = head_ && cursor == 0 && !(cfg_.hbm_cache && cache_complete_);
  DrainInflight(/*keep_head=*/adopt);
  replay_ = false;
  caching_ = false;
  if (cfg_.hbm_cache) {
    if (cache_complete_) {
      // replay from the cache when the cursor is a chunk boundary of this
      // epoch's order (sub-shards in visiting order, chunks in text order)
      plan_.Build(order_);
      const size_t i = plan_.FindCursor(cursor, PartitionBytes());
      if (i != ReplayPlan::kNotABoundary) {
        replay_ = true;
        walk_.Start(i);
        cursor_ = cursor;
        return keep_prelaunch;
      }
    } else if (cursor == 0) {
      StartCaching();
    } else {
      plan_.Clear();  // a partial pass cannot complete the cache
      arena_fill_ = 0;
    }
  }
  if (zc_ != nullptr) {
    if (!adopt) zc_->Seek(cursor);
  } else {
    seek_pos_ = cursor;
    iter_.BeforeFirst();
  }
  cursor_ = cursor;
  return keep_prelaunch;
}

void ChunkFeed::StartReader() {
  const size_t cap = cfg_.chunk_bytes;
  io::ShardReader* reader = reader_.get();
  iter_.Init(
      [reader, cap](HostSlot** dptr) {
        if (*dptr == nullptr) {
          *dptr = new HostSlot();
          (*dptr)->buf.Reserve(cap + kTextPadBytes);
          (*dptr)->cap = cap;
        }
        ScopedRange r("pinned_fill");
        HostSlot* slot = *dptr;
        size_t n = reader->Fill(slot->buf.get<char>(), slot->cap);
        while (n == io::ShardReader::kNeedMore) {
          // a record longer than the slot: grow it (the reader kept the bytes)
          slot->cap = reader->NeedCapacity();
          slot->buf.Free();
          slot->buf.Reserve(slot->cap + kTextPadBytes);
          n = reader->Fill(slot->buf.get<char>(), slot->cap);
        }
        (*dptr)->size = n;
        (*dptr)->end_pos = reader->Tell();
        return (*dptr)->size != 0;
      },
      // BeforeFirst / Seek: the consumer sets seek_pos_ before the
      // ThreadedIter handshake, which orders it before this call
      [this, reader]() {
        if (reorder_reader_) {  // shuffled mode: this epoch's sub-shard order
          reader->SetSegments(order_.Segments(), order_.Stops());
          reorder_reader_ = false;
        }
        reader->Seek(seek_pos_);
      });
}

/*! \brief the next piece of the pass from whichever source is active; false
 *  at the end of the partition */
bool ChunkFeed::NextPiece(Piece* out) {
  if (pool_ != nullptr) {
    out->job = NextPackJob();
    if (out->job == nullptr) return false;
    out->src = out->job->ptr;
    out->size = out->job->size;
    out->end_pos = out->job->end_pos;
  } else if (zc_ != nullptr) {
    ZeroCopySource::Piece piece;
    if (!zc_->Next(&piece)) return false;
    out->src = piece.ptr;
    out->size = piece.size;
    out->end_pos = zc_->Tell();
  } else {
    const double t0 = GetTime();
    if (!iter_.Next(&out->slot)) return false;
    stats_->wait_reader_sec += GetTime() - t0;
    out->src = out->slot->buf.get();
    out->size = out->slot->size;
    out->end_pos = out->slot->end_pos;
  }
  return true;
}

/*! \brief HBM epoch cache: chunks are already resident, no copy and no slot */
void ChunkFeed::FillFromCache() {
  while (static_cast<int>(inflight_.size()) < cfg_.device_slots && !walk_.AtEnd()) {
    // ParseAll over resident text: chunks adjacent in the arena and in this
    // epoch's order are parsed as one larger chunk (ReplayPlan::Merge, MergeCap)
    const ReplayPlan::Step s = walk_.Next(merge_);
    inflight_.push_back(
        Inflight{nullptr, -1, s.size, s.end_pos, arena_->get<char>() + s.off, -1, false});
  }
  reader_done_ = walk_.AtEnd();
}

/*! \brief first pass of an hbm_cache epoch: the chunk lands in its arena slot
 *  (returned as the arena offset) */
size_t ChunkFeed::CacheChunk(const Piece& p) {
  const size_t begin_pos = plan_.cached_end();
  CHECK_LE(arena_fill_ + p.size, arena_bytes_) << "HBM cache arena overflow";
  // (a packed piece's mapping may already be released: its last byte was kept)
  const char last = p.job != nullptr ? p.job->last
                    : p.size != 0    ? static_cast<const char*>(p.src)[p.size - 1]
                                     : '\n';
  CachedChunk c{arena_fill_, p.size, begin_pos, p.end_pos, 0, 0, 0, last == '\n' || last == '\r'};
  // the sub-shard the chunk belongs to (chunks never span two: the
  // zero-copy pieces stop at segment ends, the pinned fills at group ends)
  c.sub = order_.SubOf(begin_pos, &c.sub_begin);
  c.sub_end = c.sub_begin + (p.end_pos - begin_pos);
  CHECK_LE(c.sub_end, order_.sub_bytes(c.sub)) << "internal error: a chunk spans two sub-shards";
  plan_.Add(c);
  arena_fill_ += p.size;
  return c.off;
}

/*!
 * \brief queue H2D transfers until every device slot is in use.  The chunk
 *  being parsed (busy_) still owns its slot: its parsed_ event has not been
 *  recorded yet, so a copy queued into that slot would not wait for it.
 */
void ChunkFeed::FillPipeline() {
  if (replay_) {
    FillFromCache();
    return;
  }
  while (static_cast<int>(inflight_.size()) + busy_ < cfg_.device_slots && !reader_done_) {
    // the next piece's pack is not finished and the link has work: the parse
    // goes on with what is queued, and the piece is looked at again at the
    // next call (never with nothing queued: PreparePackJob)
    if (pool_ != nullptr && !PreparePackJob()) break;
    // fault points sit before a slot is taken, so a failure leaks nothing
    if (zc_ != nullptr) DMLC_FAULT_POINT("read");
    DMLC_FAULT_POINT("h2d");
    Piece p;
    if (!NextPiece(&p)) {
      reader_done_ = true;
      if (caching_) cache_complete_ = true;
      QueueHeadJobs();
      break;
    }
    const PackJob* job = p.job.get();
    const size_t size = p.size;
    const int d = next_dslot_;
    next_dslot_ = (next_dslot_ + 1) % cfg_.device_slots;
    if (size + kTextPadBytes > dtext_[d]->bytes()) {
      // a chunk longer than chunk_bytes (one long record): grow this device
      // slot once the parse that last used it has finished
      parsed_[d]->Synchronize();
      dtext_[d].reset(new DeviceBuffer(size + kTextPadBytes));
      MemsetOrdered(dtext_[d]->get(), size + kTextPadBytes);
    }
    char* dst = dtext_[d]->get<char>();
    if (caching_) dst = arena_->get<char>() + CacheChunk(p);
    // consecutive chunks alternate over the copy streams; the slot's events
    // carry every dependency of this copy
    const size_t cs = pass_chunks_++ % ncopy_;
    hipStream_t copy = copy_[cs]->get();
    DMLC_HIP_CHECK(hipStreamWaitEvent(copy, parsed_[d]->get(), 0));
    int pack_slot = -1;
    const bool packed = job != nullptr && job->state.load() == PackJob::kPacked;
    if (packed) {
      // the codes go to the slot's staging buffer
      if (dstage_[d] == nullptr || dstage_[d]->bytes() < job->packed_bytes) {
        parsed_[d]->Synchronize();
        if (dstage_[d] != nullptr) stats_->unpack_staging_bytes -= dstage_[d]->bytes();
        dstage_[d].reset(
            new DeviceBuffer(std::max(job->packed_bytes, PackSlotBytes(cfg_.chunk_bytes))));
        stats_->unpack_staging_bytes += dstage_[d]->bytes();
      }
      DMLC_HIP_CHECK(hipMemcpyAsync(dstage_[d]->get(), job->out, job->packed_bytes,
                                    hipMemcpyHostToDevice, copy));
      // expanded as soon as the codes have landed, on a stream of its own:
      // the copy stream goes straight on to the next DMA, the compute
      // stream is not held up behind a copy, and the text (the HBM-cache
      // arena's too) is whole even if the chunk is never parsed
      copied_[d]->Record(copy);
      DMLC_HIP_CHECK(hipStreamWaitEvent(unpack_->get(), copied_[d]->get(), 0));
      if (job->dense) {
        LaunchUnpackDense(dstage_[d]->get(), size,
                          static_cast<uint32_t>(DenseRanges(size, pool_->range_blocks())),
                          static_cast<uint32_t>(pool_->range_blocks()), dst, unpack_->get());
        stats_->dense_chunks += 1;
        stats_->escape_bytes += job->escape_bytes;
        stats_->raw_blocks += job->raw_blocks;
      } else {
        LaunchUnpackText(dstage_[d]->get(), size, job->nexc, alphabet_, dst, unpack_->get());
      }
      unpacked_[d]->Record(unpack_->get());
      pack_slot = job->slot;
      stats_->packed_chunks += 1;
      if (job->head && job->seq == 0) stats_->head_packed += 1;
      stats_->exception_blocks += job->nexc;
      stats_->link_bytes += job->packed_bytes;
    } else {
      DMLC_HIP_CHECK(hipMemcpyAsync(dst, p.src, size, hipMemcpyHostToDevice, copy));
      stats_->raw_chunks += 1;
      stats_->link_bytes += size;
      // a rescued piece is read from its pack slot until the copy is done
      if (job != nullptr) {
        if (job->rescued) {
          pack_slot = job->slot;
        } else {
          free_pack_slots_.push_back(job->slot);
        }
      }
      copied_[d]->Record(copy);
    }
    last_copy_d_[cs] = d;
    inflight_.push_back(Inflight{p.slot, d, size, p.end_pos, dst, pack_slot, packed});
  }
}

// --------------------------------------------------------------- packed H2D
void ChunkFeed::StartPacking(bool csv_alphabet) {
  PackAlphabet(csv_alphabet, cfg_.delimiter, alphabet_);
  // the pool packs every queued piece, the one nearest the cursor first
  // auto: the dense encoder packs about 9 GB/s of text per thread inside the
  // pool (EPYC 9575F) where the link takes 128 GB/s of it, and a pool that is
  // slower than the link loses more than the code saves: measured with 4 and
  // 8 threads, profiles/dense_pack/README.md
  const bool dense = cfg_.pack_code == 1 ||
                     (cfg_.pack_code < 0 && cfg_.chunk_bytes >= (size_t(1) << 20) &&
                      cfg_.read_threads >= kDenseMinThreads);
  pool_.reset(new PackPool(cfg_.read_threads,
                           MakePackCodec(dense ? PackCode::kDense : PackCode::kNibble,
                                         csv_alphabet, cfg_.delimiter),
                           /*distance=*/0));
  // a slot per lookahead entry and per packed chunk in flight
  pack_slots_ =
      std::vector<PinnedBuffer>(kPackLookahead + static_cast<size_t>(cfg_.device_slots) + 1);
  for (size_t i = 0; i < pack_slots_.size(); ++i) free_pack_slots_.push_back(static_cast<int>(i));
  dstage_.resize(static_cast<size_t>(cfg_.device_slots));
  unpack_.reset(new Stream());
  for (int d = 0; d < cfg_.device_slots; ++d) unpacked_.emplace_back(new Event());
}

/*! \brief pinned bytes a piece of n bytes needs: its packed form at the 3/4
 *  bound, or (windowed source) its raw bytes when it has to be rescued */
size_t ChunkFeed::PackSlotBytes(size_t n, bool may_hold_raw) const {
  const size_t packed = static_cast<size_t>(kPackMaxRatio * static_cast<double>(n)) + 64;
  return std::max<size_t>(may_hold_raw ? std::max(packed, n) : packed, 4096);
}

/*! \brief an H2D copy queued earlier in this pass, on either copy stream, is
 *  still outstanding */
bool ChunkFeed::LinkBusy() const {
  for (size_t s = 0; s < ncopy_; ++s) {
    if (last_copy_d_[s] >= 0 && !copied_[last_copy_d_[s]]->Query()) return true;
  }
  return false;
}

/*! \brief fetch pieces from the source until the lookahead holds `limit`,
 *  each with a pack slot of its own */
void ChunkFeed::FetchLookahead(size_t limit, bool head) {
  while (!la_end_ && la_.size() < limit) {
    ZeroCopySource::Piece piece;
    if (!zc_->Next(&piece)) {
      la_end_ = true;
      break;
    }
    std::unique_ptr<PackJob> job(new PackJob());
    job->ptr = piece.ptr;
    job->size = piece.size;
    job->end_pos = zc_->Tell();
    if (piece.size != 0) job->last = piece.ptr[piece.size - 1];
    job->seq = la_seq_++;
    job->head = head;
    CHECK(!free_pack_slots_.empty()) << "internal error: no free pack slot";
    job->slot = free_pack_slots_.back();
    free_pack_slots_.pop_back();
    PinnedBuffer& buf = pack_slots_[job->slot];
    if (buf.bytes() < PackSlotBytes(piece.size, zc_->windowed())) {
      buf.Reserve(PackSlotBytes(std::max(piece.size, cfg_.chunk_bytes), zc_->windowed()));
    }
    job->out = buf.get<uint8_t>();
    la_.push_back(std::move(job));
  }
}

/*!
 * \brief the source has handed in the last piece of this pass and the pool
 *  has nothing left to do: let it pack the first pieces of the next pass (same
 *  order), which Seek(0) adopts as that pass's lookahead.  The in-flight tail
 *  of this pass holds up to device_slots pack slots and the lookahead none, so
 *  kHeadJobs <= kPackLookahead slots are free.
 */
void ChunkFeed::QueueHeadJobs() {
  if (pool_ == nullptr || !cfg_.pack_head || !head_armed_ || cfg_.pack_wait ||
      cfg_.shuffle_parts > 1 || zc_->windowed() || (cfg_.hbm_cache && cache_complete_)) {
    return;
  }
  CHECK(la_.empty()) << "internal error: lookahead left at the end of a pass";
  // every job of this pass is settled: the pool's cursor restarts with the
  // source's, as in DropLookahead (retained windows stay mapped)
  la_seq_ = submitted_ = la_pushed_ = 0;
  la_end_ = front_unpushed_ = false;
  pool_->SetSubmitted(0);
  zc_->Seek(0);
  FetchLookahead(kHeadJobs, /*head=*/true);
  for (; la_pushed_ < la_.size(); ++la_pushed_) pool_->Push(la_[la_pushed_].get());
  head_ = true;
}

/*! \brief fetch pieces until the lookahead is full, hand them to the pool and
 *  decide what becomes of the piece at the submit cursor (DecideSubmit).
 *  false: it is left to the pool while the link has work (try again at the
 *  next call); true: NextPackJob carries the decision out */
bool ChunkFeed::PreparePackJob() {
  FetchLookahead(kPackLookahead, /*head=*/false);
  if (la_.empty()) return true;
  PackJob* job = la_.front().get();
  const int state = job->state.load();
  next_action_ = job->rescued ? SubmitAction::kSubmit
                              : DecideSubmit(state, cfg_.pack_wait != 0,
                                             inflight_.empty(), pool_behind_,
                                             [this]() { return LinkBusy(); });
  if (pool_behind_ && !job->rescued) {
    // the pool has caught up once kPackCaughtUp pieces in a row were found
    // packed at the cursor
    packed_in_a_row_ = state == PackJob::kPacked ? packed_in_a_row_ + 1 : 0;
    if (packed_in_a_row_ >= kPackCaughtUp) SetPoolBehind(false);
  }
  // the new pieces go to the pool in file order, only now: a piece fetched
  // straight to the cursor (the first of a pass) that goes raw is never
  // pushed, so the pool cannot have started it
  if (la_pushed_ == 0 && next_action_ == SubmitAction::kClaimRaw) {
    front_unpushed_ = true;
    la_pushed_ = 1;
  } else if (front_unpushed_ && next_action_ != SubmitAction::kClaimRaw) {
    front_unpushed_ = false;
    if (job->state.load() == PackJob::kQueued) pool_->Push(job);
  }
  for (; la_pushed_ < la_.size(); ++la_pushed_) {
    // (a piece rescued while it was fetched is settled already)
    if (la_[la_pushed_]->state.load() == PackJob::kQueued) pool_->Push(la_[la_pushed_].get());
  }
  return next_action_ != SubmitAction::kDefer;
}

/*! \brief the pool's rate is below what the link takes (it made the link wait),
 *  or it has caught up.  Behind, the pool leaves the pieces next to the cursor
 *  alone and they go raw, which adds the link's rate to half the pool's;
 *  otherwise it packs everything and only the first piece of a pass goes raw */
void ChunkFeed::SetPoolBehind(bool behind) {
  pool_behind_ = behind;
  packed_in_a_row_ = 0;
  pool_->SetDistance(behind ? kPackDistance : 0);
}

/*! \brief pop the piece PreparePackJob decided on (null at the end of the
 *  partition).  On return it is packed (state kPacked) or goes raw. */
std::unique_ptr<PackJob> ChunkFeed::NextPackJob() {
  if (la_.empty()) return nullptr;
  std::unique_ptr<PackJob> job = std::move(la_.front());
  la_.pop_front();
  --la_pushed_;
  front_unpushed_ = false;
  pool_->SetSubmitted(++submitted_);
  if (next_action_ == SubmitAction::kClaimRaw && !pool_->TryClaimRaw(job.get())) {
    next_action_ = SubmitAction::kWait;  // the pool got there first
  }
  if (next_action_ == SubmitAction::kWait) {
    const bool idle = !LinkBusy();
    const double t0 = GetTime();
    try {
      pool_->Wait(job.get());
    } catch (...) {
      free_pack_slots_.push_back(job->slot);
      throw;
    }
    stats_->wait_pack_sec += GetTime() - t0;
    if (idle) {
      stats_->wait_pack_idle_sec += GetTime() - t0;
      // the link stood still for the pool: the pool cannot feed it alone
      // (not so at a pass's start, for a piece queued ahead of the rewind)
      if (WaitMeansPoolBehind(idle, cfg_.pack_wait, job->head && job->seq == 0)) {
        SetPoolBehind(true);
      }
    }
  }
  stats_->pack_sec = pool_->pack_sec();
  return job;
}

/*! \brief the source is about to release a window: settle every queued
 *  piece of that window so that it no longer needs the mapping (packed, or
 *  its raw bytes copied into its slot).  Nothing is queued without the pool */
void ChunkFeed::RescueLookahead() {
  for (auto& job : la_) {
    if (job->rescued || !zc_->Releasing(job->ptr)) continue;
    if (!pool_->TryClaimRaw(job.get())) {
      try {
        pool_->Wait(job.get());
      } catch (...) {
        job->state.store(PackJob::kRejected);  // goes raw
      }
    }
    if (job->state.load() == PackJob::kPacked) continue;
    std::memcpy(job->out, job->ptr, job->size);
    job->ptr = reinterpret_cast<const char*>(job->out);
    job->rescued = true;
  }
}

/*! \brief forget the lookahead (Seek, a new epoch order): no pool thread
 *  reads a piece afterwards */
void ChunkFeed::DropLookahead() {
  if (pool_ == nullptr) return;
  pool_->Quiesce();
  for (auto& job : la_) free_pack_slots_.push_back(job->slot);
  la_.clear();
  la_end_ = false;
  front_unpushed_ = false;
  head_ = false;
  la_seq_ = submitted_ = la_pushed_ = 0;
  pool_->SetSubmitted(0);
}

void ChunkFeed::ReleasePackSlot(int* pack_slot) {
  if (*pack_slot < 0) return;
  free_pack_slots_.push_back(*pack_slot);
  *pack_slot = -1;
}

void ChunkFeed::StartCaching() {
  plan_.Clear();
  arena_fill_ = 0;
  cache_complete_ = false;
  if (arena_ == nullptr) {
    // + the '\n' the pinned reader inserts after a segment whose last line
    // has no EOL (one per segment at most)
    arena_bytes_ =
        PartitionBytes() + std::max(split_->files().size(), order_.all_segments().size()) + 16;
    arena_.reset(new DeviceBuffer(arena_bytes_ + kTextPadBytes));
    MemsetOrdered(arena_->get(), arena_bytes_ + kTextPadBytes);
  }
  caching_ = true;
}

void ChunkFeed::DrainInflight(bool keep_head) {
  SyncCopyStreams();
  if (unpack_) unpack_->Synchronize();
  DMLC_HIP_CHECK(hipStreamSynchronize(compute_));
  while (!inflight_.empty()) {
    if (inflight_.front().slot != nullptr) iter_.Recycle(&inflight_.front().slot);
    ReleasePackSlot(&inflight_.front().pack_slot);
    inflight_.pop_front();
  }
  ReleasePackSlot(&cur_.pack_slot);
  if (keep_head) {
    head_ = false;  // la_ is the new pass's lookahead from here on
  } else {
    DropLookahead();
  }
  last_copy_d_[0] = last_copy_d_[1] = -1;
  pass_chunks_ = 0;
  reader_done_ = false;
  busy_ = 0;
}

bool ChunkFeed::Acquire(Chunk* out) {
  FillPipeline();
  if (inflight_.empty()) return false;
  cur_ = inflight_.front();
  inflight_.pop_front();
  busy_ = 1;
  if (cur_.d >= 0) {
    // a packed chunk's text is there once its unpack (after its copy) is done
    Event* ready = cur_.packed ? unpacked_[cur_.d].get() : copied_[cur_.d].get();
    DMLC_HIP_CHECK(hipStreamWaitEvent(compute_, ready->get(), 0));
  }
  out->text = cur_.text;
  out->size = cur_.size;
  out->resident = cur_.d < 0;
  return true;
}

void ChunkFeed::FirstSyncDone() {
  if (cur_.slot != nullptr) iter_.Recycle(&cur_.slot);
  ReleasePackSlot(&cur_.pack_slot);
  FillPipeline();
}

void ChunkFeed::Release(bool delivered) {
  if (!delivered) {
    (void)hipStreamSynchronize(compute_);
    if (cur_.d >= 0) (void)hipEventRecord(parsed_[cur_.d]->get(), compute_);
    busy_ = 0;
    ReleasePackSlot(&cur_.pack_slot);
    if (head_) DropLookahead();  // a failed pass is not followed by its twin
    if (cur_.slot != nullptr) {
      try {
        iter_.Recycle(&cur_.slot);
      } catch (...) {
      }
    }
    return;
  }
  if (cur_.slot != nullptr) iter_.Recycle(&cur_.slot);
  ReleasePackSlot(&cur_.pack_slot);
  if (cur_.d >= 0) parsed_[cur_.d]->Record(compute_);
  busy_ = 0;
  cursor_ = cur_.end_pos;  // only once the chunk is delivered
  stats_->bytes += cur_.size;
  stats_->chunks += 1;
  if (zc_ != nullptr) stats_->zc_pinned_peak = zc_->PeakPinnedBytes();
}

bool ChunkFeed::PeekNextResident(const char** text, size_t* size) const {
  if (inflight_.empty() || inflight_.front().d >= 0) return false;
  *text = inflight_.front().text;
  *size = inflight_.front().size;
  return true;
}

bool ChunkFeed::NextEpochFirst(const char** text, size_t* size) const {
  if (!replay_ || !inflight_.empty() || !reader_done_ || order_.shuffled()) return false;
  ReplayPlan::Step s;
  if (!walk_.NextEpochFirst(merge_, &s) || s.size == 0) return false;
  *text = arena_->get<char>() + s.off;
  *size = s.size;
  return true;
}

}  // namespace gpu
}  // namespace dmlc
