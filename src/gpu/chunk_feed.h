/*!
 * \file src/gpu/chunk_feed.h
 * \brief Chunk transport of the device parser: brings the partition's text,
 *  chunk by chunk, into HBM and hands each chunk to the parse on the compute
 *  stream.  No parsing here and nothing that depends on the index type.
 *
 * Per chunk, in stream order (d: its device slot, n: its number in the pass):
 *   copy stream n&1 : wait(parsed[d]) -> H2D(text[d]) -> record(copied[d])
 *   compute stream  : wait(copied[d]) -> parse -> record(parsed[d])
 * The H2D of the next chunks is queued before the current chunk is parsed, so
 * PCIe transfers overlap the kernels.  Consecutive chunks alternate over two
 * copy streams (cfg.copy_streams), so chunk n + 1's copy is dispatched while
 * chunk n's runs and the link does not idle for the hand-over between two
 * dependent copies of one stream.  Nothing is ordered by the copy streams'
 * own order: a slot's copy, unpack and parse are chained by the slot's events
 * alone, and a memset of slot or arena memory (construction, a regrown slot,
 * StartCaching) is followed by an event both copy streams wait for
 * (MemsetOrdered).  Drains synchronise both.  With cfg.hbm_cache there is one
 * copy stream: only the first pass crosses the link, and a fifth stream in the
 * process slowed the replay passes (profiles/link_idle/README.md).
 *
 * Three host sources feed the ring of device slots through one function
 * (NextPiece): the pinned ring (a reader thread fills pinned slots ahead,
 * ThreadedIter over io::ShardReader), the zero-copy source (the page cache,
 * mmap'ed and registered: zero_copy_source.h) and, on top of that one, the
 * pack pool.
 *
 * Packed H2D (cfg.packed_h2d, zero-copy source only): a pool of read_threads
 * threads nibble-packs the pieces ahead of the submit cursor into pinned
 * slots (pack_pool.h).  A piece whose pack is finished crosses the link as
 * 4-bit codes into the device slot's staging buffer and is expanded into the
 * slot's text (or its HBM-cache arena range) on a stream of its own, right
 * after its copied event; its parse waits for that:
 *   copy stream n&1 : wait(parsed[d]) -> H2D(stage[d]) -> record(copied[d])
 *   unpack stream   : wait(copied[d]) -> unpack -> record(unpacked[d])
 *   compute stream  : wait(unpacked[d]) -> parse -> record(parsed[d])
 * stage[d] may be overwritten once parsed[d] is reached, on either copy
 * stream: the parse that recorded it waited for unpacked[d], the last reader
 * of stage[d].
 * A piece whose pack is not finished goes raw only when the link would
 * otherwise idle (pack_pool.h, DecideSubmit), as any other chunk of the pass:
 *   copy stream n&1 : wait(parsed[d]) -> H2D(text[d]) -> record(copied[d])
 * The first piece of a pass does, unless it was packed ahead (below).  While
 * copied[] of the last chunk submitted on either copy stream
 * is still outstanding, the piece is left to the pool and FillPipeline returns
 * with a device slot unfilled; Acquire, FirstSyncDone and the next Acquire try
 * again.  If the link ever has to wait for a pack, the pool is slower than the
 * link: until it has caught up, unstarted pieces next to the cursor go raw at
 * once.  The parse kernels see the same bytes either way.
 *
 * Head jobs (cfg.pack_head): the pool runs ahead of the link and idles before
 * a pass ends, and a pass that starts cold sends its first piece raw.  So once
 * the source has handed in the last piece of a pass, the first kHeadJobs
 * pieces of the same order are fetched again and queued to the pool, with
 * sequence numbers from 0.  Seek(0) / BeforeFirst adopts them as the new pass's
 * lookahead (their pack slots, the source cursor after them); any other Seek,
 * SetEpoch, a failed chunk or destruction quiesces the pool and drops them as
 * any lookahead.  Only when the mapping outlives the rewind (the source is not
 * windowed), the pass is unshuffled, the next pass is no HBM replay, pack_wait
 * is off and the parser has been rewound to 0 after a completed pass before (a
 * single pass pays nothing).  This is no cache: every pass packs, transfers and
 * parses every byte; the head is only read from the mapping at the end of the
 * previous pass instead of at the start of its own.
 *
 * HBM epoch cache (cfg.hbm_cache): the first full pass lands every chunk in
 * one device arena; later epochs replay it from there in the epoch's order
 * (epoch_order.h, replay_plan.h) with no copy, no slot and no event.
 *
 * Use, per chunk: Acquire -> (parse, calling FirstSyncDone after its first
 * host synchronisation) -> Release.
 */
#ifndef DMLC_SRC_GPU_CHUNK_FEED_H_
#define DMLC_SRC_GPU_CHUNK_FEED_H_

#include <dmlc/gpu/device_parser.h>
#include <dmlc/gpu/hip_utils.h>
#include <dmlc/threadediter.h>

#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "../io/input_split_base.h"
#include "../io/shard_reader.h"
#include "./epoch_order.h"
#include "./pack_pool.h"
#include "./replay_plan.h"
#include "./zero_copy_source.h"

namespace dmlc {
namespace gpu {

class ChunkFeed {
 public:
  /*! \brief a chunk whose text is (about to be) in HBM */
  struct Chunk {
    const char* text{nullptr};
    size_t size{0};
    /*! \brief replayed from the HBM cache (no copy to wait for) */
    bool resident{false};
  };

  /*!
   * \param csv_alphabet the pack alphabet holds cfg.delimiter instead of ':'
   * \param compute the parse's stream (not owned)
   * \param stats the owner's counters; the transport's fields are updated here
   */
  ChunkFeed(const std::string& uri, unsigned part, unsigned nparts, const DeviceParserConfig& cfg,
            bool csv_alphabet, hipStream_t compute, DeviceParserStats* stats);
  ~ChunkFeed();
  ChunkFeed(const ChunkFeed&) = delete;
  ChunkFeed& operator=(const ChunkFeed&) = delete;

  /*!
   * \brief continue from a Tell() cursor (drains in-flight work first).
   * \return whether a count prelaunched for the next epoch's first chunk
   *  (NextEpochFirst) may still be adopted: a replay restarting at 0
   */
  bool Seek(size_t cursor);
  /*! \brief shuffled mode: switch to epoch e's visiting order, rewound; else
   *  Seek(0).  Returns as Seek */
  bool SetEpoch(unsigned e);
  /*! \brief rewind; reshuffles in shuffled mode (reference
   *  InputSplitShuffle::BeforeFirst).  Returns as Seek */
  bool BeforeFirst() { return order_.shuffled() ? SetEpoch(order_.epoch() + 1) : Seek(0); }
  /*! \brief resume cursor (partition offset after the last delivered chunk) */
  size_t Tell() const { return cursor_; }
  unsigned Epoch() const { return order_.epoch(); }
  const std::vector<unsigned>& VisitOrder() const { return order_.order(); }
  size_t PartitionBytes() const {
    return zc_ != nullptr ? zc_->PartitionBytes() : reader_->PartitionBytes();
  }

  /*!
   * \brief queue transfers until every device slot is in use, pop the next
   *  chunk and make the compute stream wait for its text (its copy, or its
   *  unpack); false at the end of the partition
   */
  bool Acquire(Chunk* out);
  /*! \brief the H2D of the current chunk is complete (the parse synchronised
   *  with the compute stream): recycle its host slots and keep PCIe busy */
  void FirstSyncDone();
  /*!
   * \brief the current chunk's parse is queued (delivered) or failed.
   *  Delivered: its slots are recycled, parsed[d] is recorded and the cursor
   *  moves past it.  Failed: the cursor stays at its start (a resume from
   *  Tell() replays it), its slots go back to the pipeline; the event and
   *  the slot guard are settled first, and a producer error Recycle may
   *  rethrow is dropped: the parse error is the one the caller sees.
   */
  void Release(bool delivered);

  /*! \brief this pass replays the HBM cache */
  bool Replaying() const { return replay_; }
  /*! \brief and merges adjacent cached chunks (inside a ReplayMerge scope) */
  bool MergingReplay() const { return replay_ && merge_.merge; }
  /*! \brief the source has handed in its last chunk of the pass */
  bool InputDone() const { return reader_done_; }

  /*! \brief for the prelaunch policy: the chunk the next Acquire returns, if
   *  it is queued and resident (a copy would have to be waited for) */
  bool PeekNextResident(const char** text, size_t* size) const;
  /*! \brief for the prelaunch policy, while the epoch's last chunk is being
   *  parsed (unshuffled: the order is known): the first chunk of the next
   *  epoch, if a pass over the cache with this pass's merge settings follows */
  bool NextEpochFirst(const char** text, size_t* size) const;

  /*! \brief scope of a pass that parses adjacent cached chunks together, up to
   *  `limit` bytes (0: cfg.replay_chunk_bytes) */
  class ReplayMerge {
   public:
    ReplayMerge(ChunkFeed* feed, size_t limit) : feed_(feed) {
      feed_->merge_ = ReplayMergeSettings{true, limit};
    }
    ~ReplayMerge() { feed_->merge_ = ReplayMergeSettings(); }
    ReplayMerge(const ReplayMerge&) = delete;
    ReplayMerge& operator=(const ReplayMerge&) = delete;

   private:
    ChunkFeed* feed_;
  };

 private:
  /*! \brief a filled pinned host slot */
  struct HostSlot {
    PinnedBuffer buf;
    /*! \brief usable bytes of buf (grows for records longer than chunk_bytes) */
    size_t cap{0};
    size_t size{0};
    /*! \brief partition cursor after this chunk (ShardReader::Tell) */
    size_t end_pos{0};
  };
  struct Inflight {
    HostSlot* slot;  // nullptr in zero-copy / replay mode
    int d;           // device slot (events), -1 when replayed from the HBM cache
    size_t size;
    size_t end_pos;  // resume cursor once this chunk is delivered
    const char* text;  // device text of the chunk
    int pack_slot;     // >= 0: its H2D reads this pinned pack slot
    bool packed;       // sent as 4-bit codes: expanded from dstage_[d] before the parse
  };
  /*! \brief the next piece of host text a source hands in */
  struct Piece {
    HostSlot* slot{nullptr};  // pinned ring: the slot to recycle
    const void* src{nullptr};
    size_t size{0}, end_pos{0};
    std::unique_ptr<PackJob> job;  // packed H2D: the piece's lookahead entry
  };
  /*! \brief pieces fetched ahead of the submit cursor; while the pool is
   *  behind the link, how close to the cursor it may still start a pack (closer
   *  pieces go raw) and how many pieces found packed in a row end that state */
  static constexpr size_t kPackLookahead = 4;
  static constexpr size_t kPackDistance = 2;
  static constexpr size_t kPackCaughtUp = 8;
  /*! \brief pack_code=auto: pool threads from which the dense code
   *  (text_pack_dense.h) is used; its encoder is the slower one */
  static constexpr int kDenseMinThreads = 16;
  /*! \brief pieces of the next pass queued to the pool when a pass ends: the
   *  second is packed while the first crosses the link */
  static constexpr size_t kHeadJobs = 2;

  void SyncCopyStreams() const;
  void MemsetOrdered(void* ptr, size_t bytes);
  void FetchLookahead(size_t limit, bool head);
  void QueueHeadJobs();
  void StartReader();
  void StartPacking(bool csv_alphabet);
  void StartCaching();
  void FillPipeline();
  void FillFromCache();
  bool NextPiece(Piece* out);
  size_t CacheChunk(const Piece& p);
  size_t PackSlotBytes(size_t n, bool may_hold_raw = false) const;
  bool LinkBusy() const;
  bool PreparePackJob();
  void SetPoolBehind(bool behind);
  std::unique_ptr<PackJob> NextPackJob();
  void RescueLookahead();
  void DropLookahead();
  void ReleasePackSlot(int* pack_slot);
  void DrainInflight(bool keep_head = false);

  DeviceParserConfig cfg_;
  hipStream_t compute_;
  DeviceParserStats* stats_;
  std::unique_ptr<io::InputSplitBase> split_;
  std::unique_ptr<io::ShardReader> reader_;
  EpochOrder order_;
  /*! \brief chunk n of a pass is copied on stream n % ncopy_ */
  std::unique_ptr<Stream> copy_[2];
  size_t ncopy_{2};
  /*! \brief chunks submitted in this pass */
  size_t pass_chunks_{0};
  /*! \brief recorded after a memset of slot or arena memory; both copy
   *  streams wait for it */
  std::unique_ptr<Event> zeroed_;
  std::vector<std::unique_ptr<DeviceBuffer>> dtext_;
  std::vector<std::unique_ptr<Event>> copied_, parsed_;
  ThreadedIter<HostSlot> iter_;
  std::unique_ptr<ZeroCopySource> zc_;
  // packed H2D: the pool, the pieces fetched ahead of the submit cursor, the
  // pinned pack slots and the per-device-slot staging buffers of the codes
  std::unique_ptr<PackPool> pool_;
  std::deque<std::unique_ptr<PackJob>> la_;
  bool la_end_{false};
  size_t la_seq_{0}, submitted_{0};
  /*! \brief leading entries of la_ the pool has been handed; the front one may
   *  have been held back because it goes raw (front_unpushed_) */
  size_t la_pushed_{0};
  bool front_unpushed_{false};
  /*! \brief the submit thread had to wait for a pack with the link idle, and
   *  the pool has not caught up since (kept across passes) */
  bool pool_behind_{false};
  size_t packed_in_a_row_{0};
  /*! \brief PreparePackJob's decision for the front piece */
  SubmitAction next_action_{SubmitAction::kSubmit};
  /*! \brief la_ holds head jobs: pieces of the next pass, queued when this
   *  one's last piece was handed in */
  bool head_{false};
  /*! \brief this parser was rewound to 0 after a completed pass: its user runs
   *  pass after pass, and head jobs are worth queueing */
  bool head_armed_{false};
  /*! \brief per copy stream, the device slot of the last chunk submitted on it
   *  in this pass (-1: none) */
  int last_copy_d_[2]{-1, -1};
  std::vector<PinnedBuffer> pack_slots_;
  std::vector<int> free_pack_slots_;
  std::vector<std::unique_ptr<DeviceBuffer>> dstage_;
  std::unique_ptr<Stream> unpack_;
  std::vector<std::unique_ptr<Event>> unpacked_;
  uint8_t alphabet_[16];
  /*! \brief queued chunks, and the one being parsed (busy_) */
  std::deque<Inflight> inflight_;
  Inflight cur_{nullptr, -1, 0, 0, nullptr, -1, false};
  int busy_{0};
  int next_dslot_{0};
  bool reader_done_{false};
  /*! \brief resume cursor (partition offset after the last delivered chunk) */
  size_t cursor_{0};
  /*! \brief shuffled mode: the reader thread's rewind applies the epoch's order */
  bool reorder_reader_{false};
  /*! \brief where the reader restarts on the next BeforeFirst handshake */
  size_t seek_pos_{0};
  /*! \brief HBM epoch cache (cfg_.hbm_cache): the partition's chunks, resident */
  std::unique_ptr<DeviceBuffer> arena_;
  size_t arena_bytes_{0}, arena_fill_{0};
  bool caching_{false}, cache_complete_{false}, replay_{false};
  ReplayPlan plan_;
  ReplayWalk walk_;
  ReplayMergeSettings merge_;
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_CHUNK_FEED_H_
