/*!
 * \file src/gpu/replay_plan.h
 * \brief Bookkeeping of the HBM epoch cache (cfg.hbm_cache): the chunks the
 *  first pass left resident in the arena, the order an epoch replays them in,
 *  and how a ParseAll over them merges neighbours into larger chunks.  The
 *  merge rule and its cap schedule are written here once; the pipeline's
 *  replay walk and the next epoch's prelaunched first chunk both come from
 *  ReplayWalk, so they cannot disagree (CountPrelaunch::Adopt matches a
 *  prelaunched count by text pointer and size, and silently drops a miss).
 *
 * Plain C++ (no HIP): unit-tested on the CPU, tests/cpp/unittest_replay_plan.cc.
 */
#ifndef DMLC_SRC_GPU_REPLAY_PLAN_H_
#define DMLC_SRC_GPU_REPLAY_PLAN_H_

#include <algorithm>
#include <cstddef>
#include <vector>

#include "./epoch_order.h"

namespace dmlc {
namespace gpu {

/*! \brief a chunk held in the HBM epoch cache */
struct CachedChunk {
  size_t off, size, begin_pos, end_pos;
  unsigned sub;               // its sub-shard (0 when unshuffled)
  size_t sub_begin, sub_end;  // and its cursor range inside it
  bool eol_end;               // its text ends with an EOL byte (mergeable with the next)
};

/*! \brief what a ParseAll / ParseAllHashed sets for its pass: whether adjacent
 *  cached chunks are parsed together, and up to how many bytes (0: the
 *  configured replay_chunk_bytes) */
struct ReplayMergeSettings {
  bool merge{false};
  size_t limit{0};
};

/*!
 * \brief the merged chunk size cap, advanced once per replayed chunk.  It
 *  doubles per chunk from replay_first_bytes (else replay_chunk_bytes): the
 *  first chunk's count + scan is the only one not hidden behind a previous
 *  chunk's fill (the next count runs on its own stream meanwhile, and next to
 *  a fill it takes about half the fill's time per byte: 2x keeps it hidden).
 *  A pass with a merge limit (one pass per resident chunk: no count to hide,
 *  so no small first chunk) starts at the limit.
 */
class MergeCap {
 public:
  MergeCap(size_t replay_first_bytes, size_t replay_chunk_bytes)
      : first_(replay_first_bytes != 0 ? replay_first_bytes : replay_chunk_bytes),
        chunk_(replay_chunk_bytes) {}
  /*! \brief the cap of the next chunk of the walk */
  size_t Next(size_t limit) {
    if (cap_ == 0 && limit == 0) {
      cap_ = first_;
    } else {
      const size_t from = cap_ == 0 ? limit : cap_;
      cap_ = from > kHalf ? ~size_t(0) : 2 * from;  // saturates instead of wrapping to 0
    }
    return std::min(cap_, limit != 0 ? limit : chunk_);
  }

 private:
  static constexpr size_t kHalf = ~size_t(0) / 2;
  size_t first_, chunk_;
  size_t cap_{0};  // 0: the next chunk is the walk's first
};

/*! \brief the cached chunks and this epoch's replay order over them */
class ReplayPlan {
 public:
  static constexpr size_t kNotABoundary = ~size_t(0);
  /*! \brief one (merged) chunk of a replay walk: its arena range, the epoch
   *  cursor after it, and the replay index the walk continues from */
  struct Step {
    size_t off, size, end_pos, next;
  };

  /*! \brief a new first pass: forget the cached chunks */
  void Clear() {
    cached_.clear();
    list_.clear();
    begin_.clear();
    end_.clear();
  }
  void Add(const CachedChunk& c) { cached_.push_back(c); }
  const std::vector<CachedChunk>& cached() const { return cached_; }
  /*! \brief partition cursor after the last cached chunk */
  size_t cached_end() const { return cached_.empty() ? 0 : cached_.back().end_pos; }

  /*! \brief cached chunks in this epoch's order (sub-shards in visiting order,
   *  chunks in text order), with their epoch cursors */
  void Build(const EpochOrder& order) {
    list_.clear();
    begin_.clear();
    end_.clear();
    for (unsigned j : order.order()) {
      for (size_t i = 0; i < cached_.size(); ++i) {
        if (cached_[i].sub != j) continue;
        list_.push_back(i);
        begin_.push_back(order.sub_pos(j) + cached_[i].sub_begin);
        end_.push_back(order.sub_pos(j) + cached_[i].sub_end);
      }
    }
  }
  /*! \brief chunks in the replay order */
  size_t size() const { return list_.size(); }
  size_t begin_pos(size_t i) const { return begin_[i]; }
  size_t end_pos(size_t i) const { return end_[i]; }
  const CachedChunk& chunk(size_t i) const { return cached_[list_[i]]; }

  /*! \brief replay index whose chunk starts at `cursor` (size() for the end of
   *  the partition), or kNotABoundary */
  size_t FindCursor(size_t cursor, size_t partition_bytes) const {
    for (size_t i = 0; i <= list_.size(); ++i) {
      if ((i < list_.size() ? begin_[i] : partition_bytes) == cursor) return i;
    }
    return kNotABoundary;
  }

  /*!
   * \brief the chunk at replay index i, with `merge` grown by its successors
   *  while they are adjacent in the arena and in this epoch's order and the
   *  sum stays within `cap` (fewer launches and host round trips per byte).
   *  A chunk whose text ends without EOL -- a file's unterminated last line on
   *  the zero-copy path -- is never continued.
   */
  Step Merge(size_t i, size_t cap, bool merge) const {
    const CachedChunk& c = chunk(i);
    Step s{c.off, c.size, end_[i], i + 1};
    while (merge && s.next < list_.size() && chunk(s.next - 1).eol_end &&
           chunk(s.next).off == c.off + s.size && s.size + chunk(s.next).size <= cap) {
      s.size += chunk(s.next).size;
      s.end_pos = end_[s.next];
      ++s.next;
    }
    return s;
  }

 private:
  std::vector<CachedChunk> cached_;
  std::vector<size_t> list_, begin_, end_;
};

/*! \brief a pass over the plan from some replay index: position and cap */
class ReplayWalk {
 public:
  ReplayWalk(const ReplayPlan* plan, size_t replay_first_bytes, size_t replay_chunk_bytes)
      : plan_(plan), fresh_cap_(replay_first_bytes, replay_chunk_bytes), cap_(fresh_cap_) {}
  /*! \brief restart at replay index i, as the first chunk of a pass */
  void Start(size_t i) {
    idx_ = i;
    cap_ = fresh_cap_;
  }
  bool AtEnd() const { return idx_ >= plan_->size(); }
  /*! \brief the next (merged) chunk; the cap advances whether or not the pass merges */
  ReplayPlan::Step Next(const ReplayMergeSettings& s) {
    const ReplayPlan::Step step = plan_->Merge(idx_, cap_.Next(s.limit), s.merge);
    idx_ = step.next;
    return step;
  }
  /*! \brief the first chunk a pass from replay index 0 takes with settings
   *  `s`: what the next epoch will ask for first if it runs as this one does;
   *  false without cached chunks */
  bool NextEpochFirst(const ReplayMergeSettings& s, ReplayPlan::Step* out) const {
    ReplayWalk w = *this;
    w.Start(0);
    if (w.AtEnd()) return false;
    *out = w.Next(s);
    return true;
  }

 private:
  const ReplayPlan* plan_;
  MergeCap fresh_cap_, cap_;
  size_t idx_{0};
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_REPLAY_PLAN_H_
