/*!
 * \file src/gpu/pack_pool.h
 * \brief Thread pool that packs upcoming text pieces into pinned slots ahead
 *  of the H2D submit cursor, and the rule by which the submit loop sends a
 *  piece packed or raw (DecideSubmit).  The pool is the scheduler only: the
 *  code it packs with is a PackCodec (pack_codec.h; the text codes are in
 *  text_pack_codec.h).
 *
 * The pool packs the queue front.  A job is cut into ranges of `range_blocks`
 * 256-byte blocks which the threads claim with an atomic cursor; a thread that
 * finds no range left in an open job moves straight on to the next queued one
 * (two jobs are open at most).  The thread that reports the last range done
 * ends the phase (PackJobState::Finish): the job is then settled, or the codec
 * names the ranges of a further phase, which are claimed the same way, the
 * first of them by that thread.  No thread waits for another.  A job that does
 * not fit, or whose codec throws, does no further work: it is settled rejected
 * or failed, and Wait rethrows what was thrown.
 *
 * The consumer queues jobs in file order (Push), and at submit time either
 * finds a job settled, claims a job the pool has not started (TryClaimRaw: the
 * piece goes over the link raw, the pool never touches it), or waits for the
 * pack in progress (Wait).
 *
 * With a non-zero distance (SetDistance) the pool
 * leaves jobs closer than that many pieces to the submit cursor unstarted, for
 * a consumer that claims them raw because the pool cannot keep up with the
 * link; with distance 0 it packs every job.
 */
#ifndef DMLC_SRC_GPU_PACK_POOL_H_
#define DMLC_SRC_GPU_PACK_POOL_H_

#include <dmlc/fault.h>
#include <dmlc/logging.h>
#include <dmlc/timer.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "./pack_codec.h"
#include "./text_pack.h"        // kPackMaxRatio
#include "./text_pack_dense.h"  // PackJob::table

namespace dmlc {
namespace gpu {

/*! \brief one text piece queued ahead of the submit cursor */
struct PackJob {
  enum State : int { kQueued = 0, kPacking, kPacked, kRejected, kClaimedRaw, kFailed };
  const char* ptr{nullptr};
  size_t size{0};
  /*! \brief partition cursor after this piece */
  size_t end_pos{0};
  /*! \brief the piece's last byte (ptr may be gone once the piece is packed) */
  char last{'\n'};
  /*! \brief position in the pass (0: its first piece) */
  size_t seq{0};
  /*! \brief pinned slot (index and memory) the packed bytes go to */
  int slot{-1};
  uint8_t* out{nullptr};
  double ratio{kPackMaxRatio};
  std::atomic<int> state{kQueued};
  // results, valid once state is kPacked
  size_t packed_bytes{0};
  uint32_t nexc{0};
  /*! \brief dense code: the job's table (set by Push), and once packed whether
   *  packed_bytes is a dense chunk, its escaped bytes and its raw blocks */
  DenseTable table;
  bool dense{false};
  size_t escape_bytes{0}, raw_blocks{0};
  /*! \brief the piece's bytes were copied into the slot (its window goes away) */
  bool rescued{false};
  /*! \brief queued at the end of the previous pass for the start of this one
   *  (a head job: chunk_feed.h) */
  bool head{false};
};

/*! \brief what the submit loop does with the piece at its cursor */
enum class SubmitAction : int {
  /*! \brief the job is settled: packed it crosses the link as codes, rejected raw */
  kSubmit = 0,
  /*! \brief TryClaimRaw and send it raw (if the pool got there first: kWait) */
  kClaimRaw,
  /*! \brief block until the pool has settled it */
  kWait,
  /*! \brief leave it to the pool and come back at the next call */
  kDefer
};

/*!
 * \brief the link-aware rule: a piece whose pack has not finished goes raw only
 *  when the link would otherwise idle.  While a copy queued earlier is still
 *  outstanding the piece is left to the pool (kDefer); with the link idle an
 *  unstarted job is claimed raw and a pack in progress is waited for.
 * \param state the job's PackJob::State
 * \param pack_wait wait for every pack (only the 3/4 rule sends a piece raw)
 * \param nothing_inflight no chunk is queued for the parse: the caller has to
 *  produce one, so the piece is never deferred
 * \param pool_behind the pool has made the link wait and not caught up since:
 *  nothing is deferred, an unstarted piece goes raw at once, so that link and
 *  pool work side by side (deferring a pack in progress here was measured: the
 *  link then idles until the pack is done and the pool never catches up)
 * \param link_busy callable: an H2D copy queued earlier is still outstanding
 *  (asked only when the answer decides)
 */
template <typename LinkBusy>
inline SubmitAction DecideSubmit(int state, bool pack_wait, bool nothing_inflight,
                                 bool pool_behind, LinkBusy&& link_busy) {
  if (state == PackJob::kFailed) return SubmitAction::kWait;  // Wait rethrows the pool's error
  if (state != PackJob::kQueued && state != PackJob::kPacking) return SubmitAction::kSubmit;
  if (pack_wait) return SubmitAction::kWait;
  if (!nothing_inflight && !pool_behind && link_busy()) return SubmitAction::kDefer;
  return state == PackJob::kQueued ? SubmitAction::kClaimRaw : SubmitAction::kWait;
}

/*!
 * \brief whether a wait for a pack (SubmitAction::kWait) shows that the pool is
 *  slower than the link.  It does when the wait began with no copy outstanding,
 *  unless every pack is waited for anyway (pack_wait), and unless the piece is
 *  the first of a pass that was queued ahead of the rewind (a head job): the
 *  link is idle there because the pass has only begun, not because the pool
 *  fell behind it.
 */
inline bool WaitMeansPoolBehind(bool link_idle, bool pack_wait, bool head_of_pass) {
  return link_idle && !pack_wait && !head_of_pass;
}

class PackPool {
 public:
  /*! \brief blocks per range: 256 KiB of text */
  static constexpr size_t kRangeBlocks = 1024;

  /*! \param codec the code the pool packs with */
  PackPool(int threads, std::unique_ptr<PackCodec> codec, size_t distance,
           size_t range_blocks = kRangeBlocks)
      : nthreads_(std::max(threads, 1)),
        distance_(distance),
        range_blocks_(std::max<size_t>(range_blocks, 1)),
        codec_(std::move(codec)) {
    for (Open& o : open_) o.state = codec_->NewState();
    for (int t = 0; t < nthreads_; ++t) workers_.emplace_back([this]() { Work(); });
  }
  ~PackPool() {
    {
      // the open jobs are finished first
      std::unique_lock<std::mutex> lk(mu_);
      queue_.clear();
      cv_done_.wait(lk, [&] { return nopen_ == 0; });
      stop_ = true;
    }
    cv_work_.notify_all();
    for (auto& w : workers_) w.join();
  }
  PackPool(const PackPool&) = delete;
  PackPool& operator=(const PackPool&) = delete;

  /*! \brief queue a job (file order); it must stay alive until it is settled
   *  (packed, rejected, claimed) or dropped by Quiesce */
  void Push(PackJob* job) {
    codec_->Prepare(job);
    {
      std::lock_guard<std::mutex> lk(mu_);
      queue_.push_back(job);
    }
    cv_work_.notify_all();
  }
  /*! \brief from the next job opened on, skip jobs closer than this to the cursor */
  void SetDistance(size_t distance) { distance_.store(distance, std::memory_order_relaxed); }
  /*! \brief the submit cursor: pieces submitted so far in this pass */
  void SetSubmitted(size_t n) { submitted_.store(n, std::memory_order_relaxed); }
  /*! \brief true: the pool had not started the job and will not */
  bool TryClaimRaw(PackJob* job) {
    std::lock_guard<std::mutex> lk(mu_);
    int expect = PackJob::kQueued;
    if (!job->state.compare_exchange_strong(expect, PackJob::kClaimedRaw)) return false;
    // the pool keeps no pointer to a claimed job (its owner may free it)
    queue_.erase(std::remove(queue_.begin(), queue_.end(), job), queue_.end());
    return true;
  }
  /*! \brief wait until a pushed job is settled (packed or rejected), whether
   *  its pack is in progress or still queued; rethrows what a pool thread threw */
  void Wait(PackJob* job) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] {
      const int st = job->state.load();
      return st != PackJob::kPacking && st != PackJob::kQueued;
    });
    if (job->state.load() == PackJob::kFailed) {
      std::exception_ptr e = error_;
      error_ = nullptr;
      lk.unlock();
      if (e) std::rethrow_exception(e);
      LOG(FATAL) << "text pack failed";
    }
  }
  /*! \brief drop every queued job and wait until no thread reads or writes one
   *  (the open jobs are finished) */
  void Quiesce() {
    std::unique_lock<std::mutex> lk(mu_);
    queue_.clear();
    cv_done_.wait(lk, [&] { return nopen_ == 0; });
    error_ = nullptr;
  }
  /*! \brief cumulative wall seconds during which at least one job was open */
  double pack_sec() const { return pack_sec_.load(std::memory_order_relaxed); }
  size_t range_blocks() const { return range_blocks_; }

 private:
  /*! \brief a job being packed.  A thread may touch an Open (and its job) only
   *  under mu_ or while it holds a claimed range it has not reported done: the
   *  job is settled, and the Open reused, only after every range is reported */
  struct Open {
    PackJob* job{nullptr};
    /*! \brief the codec's side of the job (made once, reused job after job) */
    std::unique_ptr<PackJobState> state;
    /*! \brief the phase the ranges belong to and their count: changed under
     *  mu_ by the thread that ends a phase */
    int phase{0};
    size_t nranges{0};
    /*! \brief order of opening: the older job's ranges are claimed first */
    size_t order{0};
    std::atomic<size_t> next{0}, done{0};
    std::atomic<bool> fits{true};
    int result{PackJob::kRejected};
    std::exception_ptr err;  // under mu_
  };
  static constexpr int kOpenJobs = 2;

  /*! \brief under mu_: a range of an open job, the older job first */
  Open* ClaimLocked(size_t* range) {
    Open* order[kOpenJobs] = {&open_[0], &open_[1]};
    if (order[1]->job != nullptr && (order[0]->job == nullptr || order[1]->order < order[0]->order)) {
      std::swap(order[0], order[1]);
    }
    for (Open* o : order) {
      if (o->job == nullptr || o->next.load(std::memory_order_relaxed) >= o->nranges) continue;
      const size_t r = o->next.fetch_add(1);
      if (r < o->nranges) {
        *range = r;
        return o;
      }
    }
    return nullptr;
  }
  /*! \brief under mu_: open the queue front in a free slot; false: nothing to open */
  bool OpenLocked() {
    Open* o = open_[0].job == nullptr ? &open_[0] : open_[1].job == nullptr ? &open_[1] : nullptr;
    while (o != nullptr && !queue_.empty()) {
      PackJob* job = queue_.front();
      queue_.pop_front();
      // too close to the submit cursor: left unstarted for the consumer to claim
      const size_t distance = distance_.load(std::memory_order_relaxed);
      if (distance != 0 && job->seq < submitted_.load(std::memory_order_relaxed) + distance) {
        continue;
      }
      int expect = PackJob::kQueued;
      if (!job->state.compare_exchange_strong(expect, PackJob::kPacking)) continue;
      o->job = job;
      o->phase = 0;
      o->nranges = 1;  // (should Begin throw: one range, which does nothing)
      o->order = ++opened_;
      o->next.store(0);
      o->done.store(0);
      o->err = nullptr;
      o->result = PackJob::kRejected;
      try {
        bool fits = true;
        o->nranges = o->state->Begin(job, range_blocks_, &fits);
        o->fits.store(fits);
        DMLC_FAULT_POINT("pack");  // under mu_: the k-th pass is the k-th job
      } catch (...) {
        o->err = std::current_exception();
        o->fits.store(false);
      }
      if (nopen_++ == 0) open_since_ = GetTime();
      return true;
    }
    return false;
  }
  /*! \brief every range of the phase is reported and this thread alone holds
   *  the job: end the phase.  true: a further phase is opened and the caller
   *  holds its range 0; false: the job is ready to be settled (o->result) */
  bool FinishPhase(Open* o) {
    if (!o->fits.load()) return false;
    try {
      bool packed = false;
      const size_t nranges = o->state->Finish(o->phase, &packed);
      if (nranges == 0) {
        if (packed) o->result = PackJob::kPacked;
        return false;
      }
      {
        std::lock_guard<std::mutex> lk(mu_);
        ++o->phase;
        o->nranges = nranges;
        o->done.store(0);
        o->next.store(1);  // range 0 is the caller's
      }
      cv_work_.notify_all();
      return true;
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu_);
      if (!o->err) o->err = std::current_exception();
      return false;
    }
  }
  void Settle(Open* o) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      int result = o->result;
      if (o->err) {
        error_ = o->err;
        result = PackJob::kFailed;
      }
      o->job->state.store(result);
      o->job = nullptr;  // from here on the pool holds no pointer to the job
      if (--nopen_ == 0) {
        pack_sec_.store(pack_sec_.load(std::memory_order_relaxed) + (GetTime() - open_since_),
                        std::memory_order_relaxed);
      }
    }
    cv_done_.notify_all();
    cv_work_.notify_all();  // a slot is free for the next queued job
  }
  void Work() {
    // the codec's scratch buffer of this thread, 64-byte aligned
    const size_t scratch_bytes = codec_->ScratchBytes(range_blocks_);
    std::vector<uint8_t> buffer(scratch_bytes != 0 ? scratch_bytes + 64 : 0);
    uint8_t* scratch =
        buffer.data() + ((64 - (reinterpret_cast<uintptr_t>(buffer.data()) & 63)) & 63);
    for (;;) {
      Open* o = nullptr;
      size_t r = 0;
      {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
          if (stop_) return;
          if ((o = ClaimLocked(&r)) != nullptr) break;
          if (OpenLocked()) {
            cv_work_.notify_all();
            continue;
          }
          cv_work_.wait(lk);
        }
      }
      // range after range of this job; the next one is claimed before this
      // one is reported, so the job stays open in between
      while (o != nullptr) {
        // (the phase and its ranges: read while a range is held)
        const int phase = o->phase;
        const size_t nranges = o->nranges;
        try {
          // "does not fit" is sticky: the job's remaining ranges do no work
          if (o->fits.load(std::memory_order_relaxed) && !o->state->Run(phase, r, scratch)) {
            o->fits.store(false, std::memory_order_relaxed);
          }
        } catch (...) {
          o->fits.store(false);
          std::lock_guard<std::mutex> lk(mu_);
          if (!o->err) o->err = std::current_exception();
        }
        const size_t next = o->next.fetch_add(1);
        if (o->done.fetch_add(1) + 1 == nranges) {
          if (FinishPhase(o)) {
            r = 0;
          } else {
            Settle(o);
            o = nullptr;
          }
        } else if (next < nranges) {
          r = next;
        } else {
          o = nullptr;
        }
      }
    }
  }

  const int nthreads_;
  std::atomic<size_t> distance_;
  const size_t range_blocks_;
  const std::unique_ptr<PackCodec> codec_;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_done_;
  std::deque<PackJob*> queue_;
  Open open_[kOpenJobs];
  int nopen_{0};
  size_t opened_{0};
  double open_since_{0};
  std::atomic<size_t> submitted_{0};
  std::atomic<double> pack_sec_{0};
  std::exception_ptr error_;
  bool stop_{false};
  std::vector<std::thread> workers_;
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_PACK_POOL_H_
