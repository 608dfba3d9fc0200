/*!
 * \file src/gpu/pack_pool.h
 * \brief Thread pool that nibble-packs upcoming text pieces (text_pack.h) into
 *  pinned slots ahead of the H2D submit cursor.  The pool works cooperatively
 *  on one piece at a time: every thread packs a contiguous block range into
 *  the nibble area's fixed positions, the per-thread exception lists are
 *  concatenated afterwards.
 *
 * The consumer queues jobs in file order (Push), and at submit time either
 * finds a job packed, claims a job the pool has not started (TryClaimRaw: the
 * piece goes over the link raw, the pool skips it), or waits for the pack in
 * progress (Wait).  The pool skips jobs closer than `distance` pieces to the
 * submit cursor (they stay unstarted and go raw), so the link is not made to
 * wait for work started too late.  With distance 0 it packs every job and the
 * consumer waits for each (never claiming one raw).
 */
#ifndef DMLC_SRC_GPU_PACK_POOL_H_
#define DMLC_SRC_GPU_PACK_POOL_H_

#include <dmlc/fault.h>
#include <dmlc/logging.h>
#include <dmlc/timer.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "./text_pack.h"

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
  /*! \brief the piece's bytes were copied into the slot (its window goes away) */
  bool rescued{false};
};

class PackPool {
 public:
  PackPool(int threads, const uint8_t alphabet[16], size_t distance)
      : nthreads_(std::max(threads, 1)), distance_(distance), exc_(nthreads_) {
    std::memcpy(alphabet_, alphabet, 16);
    for (int t = 0; t < nthreads_; ++t) {
      workers_.emplace_back([this, t]() { t == 0 ? Lead() : Help(t); });
    }
  }
  ~PackPool() {
    {
      // the helpers finish the current job first: the leader waits for them
      std::unique_lock<std::mutex> lk(mu_);
      queue_.clear();
      cv_done_.wait(lk, [&] { return current_ == nullptr; });
      stop_ = true;
    }
    cv_work_.notify_all();
    cv_part_.notify_all();
    for (auto& w : workers_) w.join();
  }
  PackPool(const PackPool&) = delete;
  PackPool& operator=(const PackPool&) = delete;

  /*! \brief queue a job (file order); it must stay alive until it is settled
   *  (packed, rejected, claimed) or dropped by Quiesce */
  void Push(PackJob* job) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      queue_.push_back(job);
    }
    cv_work_.notify_all();
  }
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
  /*! \brief drop every queued job and wait until no thread reads or writes one */
  void Quiesce() {
    std::unique_lock<std::mutex> lk(mu_);
    queue_.clear();
    cv_done_.wait(lk, [&] { return current_ == nullptr; });
    error_ = nullptr;
  }
  /*! \brief cumulative seconds the pool spent packing */
  double pack_sec() const { return pack_sec_.load(std::memory_order_relaxed); }

 private:
  /*! \brief blocks [begin, end) of part p of `parts` */
  static void PartRange(size_t blocks, int parts, int p, size_t* begin, size_t* end) {
    *begin = blocks * static_cast<size_t>(p) / parts;
    *end = blocks * static_cast<size_t>(p + 1) / parts;
  }
  void PackPart(PackJob* job, int p) {
    size_t b0, b1;
    PartRange(PackBlocks(job->size), parts_, p, &b0, &b1);
    exc_[p].clear();
    if (!fits_.load(std::memory_order_relaxed)) return;
    if (!PackRange(reinterpret_cast<const uint8_t*>(job->ptr), job->size, b0, b1, alphabet_,
                   job->out + sizeof(PackedHeader), &exc_[p], &exc_total_, exc_limit_)) {
      fits_.store(false, std::memory_order_relaxed);
    }
  }
  /*! \brief thread 0: takes the jobs, shares each with the helpers, finishes it */
  void Lead() {
    for (;;) {
      PackJob* job = nullptr;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_work_.wait(lk, [&] { return stop_ || !queue_.empty(); });
        if (stop_) return;
        job = queue_.front();
        queue_.pop_front();
        // too close to the submit cursor: left unstarted, it goes raw.  With
        // distance 0 the consumer waits for every job (it never claims one),
        // so none may be skipped, however far the cursor has come
        if (distance_ != 0 && job->seq < submitted_.load(std::memory_order_relaxed) + distance_) {
          continue;
        }
        int expect = PackJob::kQueued;
        if (!job->state.compare_exchange_strong(expect, PackJob::kPacking)) continue;
        current_ = job;
        exc_limit_ = PackMaxExceptions(job->size, job->ratio);
        exc_total_.store(0);
        fits_.store(exc_limit_ >= 0);
        // at least 64 KiB of text per thread
        parts_ = static_cast<int>(
            std::min<size_t>(nthreads_, std::max<size_t>(1, PackBlocks(job->size) / 256)));
        pending_ = parts_ - 1;
        ++generation_;
      }
      const double t0 = GetTime();
      if (parts_ > 1) cv_part_.notify_all();
      int result = PackJob::kRejected;
      std::exception_ptr err;
      try {
        DMLC_FAULT_POINT("pack");
        if (fits_.load()) PackPart(job, 0);
      } catch (...) {
        err = std::current_exception();
      }
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_lead_.wait(lk, [&] { return pending_ == 0; });
        if (!err && part_error_) err = part_error_;
        part_error_ = nullptr;
      }
      if (!err && fits_.load()) {
        try {
          std::vector<uint32_t>& all = exc_[0];
          for (int p = 1; p < parts_; ++p) all.insert(all.end(), exc_[p].begin(), exc_[p].end());
          if (static_cast<long>(all.size()) <= exc_limit_) {
            job->packed_bytes = PackFinish(reinterpret_cast<const uint8_t*>(job->ptr), job->size,
                                           alphabet_, all, job->out);
            job->nexc = static_cast<uint32_t>(all.size());
            result = PackJob::kPacked;
          }
        } catch (...) {
          err = std::current_exception();
        }
      }
      pack_sec_.store(pack_sec_.load(std::memory_order_relaxed) + (GetTime() - t0),
                      std::memory_order_relaxed);
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (err) {
          error_ = err;
          result = PackJob::kFailed;
        }
        job->state.store(result);
        current_ = nullptr;
      }
      cv_done_.notify_all();
    }
  }
  /*! \brief threads 1..: pack their part of the leader's current job */
  void Help(int t) {
    size_t seen = 0;
    for (;;) {
      PackJob* job = nullptr;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_part_.wait(lk, [&] { return stop_ || generation_ != seen; });
        if (stop_) return;
        seen = generation_;
        if (t >= parts_) continue;
        job = current_;
      }
      std::exception_ptr err;
      try {
        PackPart(job, t);
      } catch (...) {
        err = std::current_exception();
      }
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (err && !part_error_) part_error_ = err;
        --pending_;
      }
      cv_lead_.notify_one();
    }
  }

  const int nthreads_;
  const size_t distance_;
  uint8_t alphabet_[16];
  std::mutex mu_;
  std::condition_variable cv_work_, cv_part_, cv_lead_, cv_done_;
  std::deque<PackJob*> queue_;
  PackJob* current_{nullptr};
  size_t generation_{0};
  int parts_{1}, pending_{0};
  long exc_limit_{0};
  std::atomic<long> exc_total_{0};
  std::atomic<bool> fits_{true};
  std::atomic<size_t> submitted_{0};
  std::atomic<double> pack_sec_{0};
  std::vector<std::vector<uint32_t>> exc_;
  std::exception_ptr error_, part_error_;
  bool stop_{false};
  std::vector<std::thread> workers_;
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_PACK_POOL_H_
