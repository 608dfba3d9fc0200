/*!
 * \file tests/cpp/unittest_pack_codec.cc
 * \brief The pack pool's scheduler (src/gpu/pack_pool.h) on its own, driven
 *  through the codec seam (src/gpu/pack_codec.h) by a toy codec that packs
 *  nothing and records what the pool calls: phases in order, each range once,
 *  a job that stops fitting, a codec that throws, and teardown with jobs open.
 *  Jobs are a few ranges long, so every case takes milliseconds.  Part of the
 *  sanitizer runs of the suite.
 */
#include <atomic>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../src/gpu/pack_pool.h"
#include "./testing.h"

namespace {

using dmlc::gpu::PackJob;
using dmlc::gpu::PackPool;

constexpr int kMaxPhases = 3;
constexpr size_t kMaxRanges = 8;

/*! \brief a job, what the toy codec is to do with it, and what it did */
struct Toy {
  /*! \brief ranges of each phase */
  std::vector<size_t> phases;
  /*! \brief Run reports "does not fit" from this range */
  int unfit_phase{-1};
  size_t unfit_range{0};
  /*! \brief where `message` is thrown: Begin, this Run, Finish of this phase */
  bool throw_begin{false};
  int throw_phase{-1};
  size_t throw_range{0};
  int throw_finish{-1};
  std::string message;
  /*! \brief Run waits for this flag */
  const std::atomic<bool>* gate{nullptr};

  std::atomic<int> begins{0};
  /*! \brief runs that have returned */
  std::atomic<int> completed{0};
  std::atomic<int> runs[kMaxPhases][kMaxRanges];
  std::atomic<size_t> thread[kMaxPhases][kMaxRanges];
  /*! \brief calls of Finish(p), and `completed` as the last of them saw it */
  std::atomic<int> finishes[kMaxPhases];
  std::atomic<int> finish_saw[kMaxPhases];
  PackJob job;

  explicit Toy(std::vector<size_t> phase_sizes) : phases(std::move(phase_sizes)) {
    for (int p = 0; p < kMaxPhases; ++p) {
      finishes[p].store(0);
      finish_saw[p].store(-1);
      for (size_t r = 0; r < kMaxRanges; ++r) {
        runs[p][r].store(0);
        thread[p][r].store(0);
      }
    }
    // the job's "text" is this record; range_blocks is 1: a block per range
    job.ptr = reinterpret_cast<const char*>(this);
    job.size = phases[0] * 256;
  }
  int state() const { return job.state.load(); }
};

class ToyCodec : public dmlc::gpu::PackCodec {
 public:
  std::unique_ptr<dmlc::gpu::PackJobState> NewState() const override {
    return std::unique_ptr<dmlc::gpu::PackJobState>(new State());
  }

 private:
  class State : public dmlc::gpu::PackJobState {
   public:
    size_t Begin(PackJob* job, size_t, bool* fits) override {
      toy_ = reinterpret_cast<Toy*>(const_cast<char*>(job->ptr));
      toy_->begins.fetch_add(1);
      if (toy_->throw_begin) throw std::runtime_error(toy_->message);
      *fits = true;
      return toy_->phases[0];
    }
    bool Run(int phase, size_t r, uint8_t*) override {
      Toy* t = toy_;
      if (t->gate != nullptr) {
        while (!t->gate->load()) std::this_thread::yield();
      }
      t->runs[phase][r].fetch_add(1);
      t->thread[phase][r].store(std::hash<std::thread::id>()(std::this_thread::get_id()));
      if (phase == t->throw_phase && r == t->throw_range) throw std::runtime_error(t->message);
      t->completed.fetch_add(1);
      return !(phase == t->unfit_phase && r == t->unfit_range);
    }
    size_t Finish(int phase, bool* packed) override {
      Toy* t = toy_;
      t->finishes[phase].fetch_add(1);
      t->finish_saw[phase].store(t->completed.load());
      if (phase == t->throw_finish) throw std::runtime_error(t->message);
      if (static_cast<size_t>(phase) + 1 < t->phases.size()) return t->phases[phase + 1];
      t->job.packed_bytes = static_cast<size_t>(t->completed.load());
      *packed = true;
      return 0;
    }

   private:
    Toy* toy_{nullptr};
  };
};

std::unique_ptr<PackPool> ToyPool(int threads) {
  return std::make_unique<PackPool>(threads, std::make_unique<ToyCodec>(), /*distance=*/0,
                                    /*range_blocks=*/1);
}

const std::vector<std::vector<size_t>>& PhaseLists() {
  static const std::vector<std::vector<size_t>> lists = {{5, 3, 1}, {1}, {1, 4}};
  return lists;
}

/*! \brief phases [0, nphases) ran in full, each range once, and each Finish
 *  ran once and saw every run of its phase and none of the next */
void ExpectPhases(const Toy& t, size_t nphases, int threads) {
  EXPECT_EQ(t.begins.load(), 1);
  int sum = 0;
  const size_t first_thread = t.thread[0][0].load();
  for (size_t p = 0; p < nphases; ++p) {
    const size_t n = t.phases[p];
    for (size_t r = 0; r < kMaxRanges; ++r) {
      EXPECT_EQ(t.runs[p][r].load(), r < n ? 1 : 0);
      if (threads == 1 && r < n) EXPECT_EQ(t.thread[p][r].load(), first_thread);
    }
    sum += static_cast<int>(n);
    EXPECT_EQ(t.finishes[p].load(), 1);
    EXPECT_EQ(t.finish_saw[p].load(), sum);
  }
}

void ExpectPacked(const Toy& t, int threads) {
  EXPECT_EQ(t.state(), static_cast<int>(PackJob::kPacked));
  ExpectPhases(t, t.phases.size(), threads);
  size_t total = 0;
  for (size_t n : t.phases) total += n;
  EXPECT_EQ(t.job.packed_bytes, total);
}

/*! \brief the job stopped in `phase`: the phases before it are complete, no
 *  range of it ran twice, its Finish and every later phase never ran */
void ExpectStoppedIn(const Toy& t, int phase, int threads) {
  ExpectPhases(t, static_cast<size_t>(phase), threads);
  for (int p = phase; p < kMaxPhases; ++p) {
    EXPECT_EQ(t.finishes[p].load(), 0);
    for (size_t r = 0; r < kMaxRanges; ++r) {
      EXPECT_LE(t.runs[p][r].load(), p == phase && r < t.phases[p] ? 1 : 0);
    }
  }
}

/*! \brief Wait throws std::runtime_error with this message */
void ExpectWaitThrows(PackPool* pool, Toy* t) {
  std::string what;
  try {
    pool->Wait(&t->job);
  } catch (const std::runtime_error& e) {
    what = e.what();
  }
  EXPECT_EQ(what, t->message);
  EXPECT_EQ(t->state(), static_cast<int>(PackJob::kFailed));
}

}  // namespace

TEST(PackCodec, PhasesInOrder) {
  for (int threads : {1, 4}) {
    for (const auto& phases : PhaseLists()) {
      std::unique_ptr<PackPool> pool = ToyPool(threads);
      Toy t(phases);
      pool->Push(&t.job);
      pool->Wait(&t.job);
      ExpectPacked(t, threads);
    }
  }
}

TEST(PackCodec, InterleavedJobs) {
  for (int threads : {1, 4}) {
    std::unique_ptr<PackPool> pool = ToyPool(threads);
    std::vector<std::unique_ptr<Toy>> toys;
    for (size_t i = 0; i < 8; ++i) {
      toys.emplace_back(new Toy(PhaseLists()[i % PhaseLists().size()]));
      toys.back()->job.seq = i;
    }
    for (auto& t : toys) pool->Push(&t->job);
    for (auto& t : toys) {
      pool->Wait(&t->job);
      ExpectPacked(*t, threads);
    }
    EXPECT_GT(pool->pack_sec(), 0.0);
  }
}

TEST(PackCodec, DoesNotFitIsSticky) {
  const std::vector<size_t> phases = {5, 3, 1};
  for (int threads : {1, 4}) {
    for (int phase : {0, 1}) {
      for (size_t k : {size_t(0), phases[phase] - 1}) {
        std::unique_ptr<PackPool> pool = ToyPool(threads);
        Toy bad(phases), good(phases);
        bad.unfit_phase = phase;
        bad.unfit_range = k;
        pool->Push(&bad.job);
        pool->Push(&good.job);
        pool->Wait(&bad.job);
        EXPECT_EQ(bad.state(), static_cast<int>(PackJob::kRejected));
        ExpectStoppedIn(bad, phase, threads);
        EXPECT_EQ(bad.runs[phase][k].load(), 1);
        pool->Wait(&good.job);
        ExpectPacked(good, threads);
      }
    }
  }
}

TEST(PackCodec, ThrowSurfacesInWait) {
  const std::vector<size_t> phases = {5, 3, 1};
  for (int threads : {1, 4}) {
    std::unique_ptr<PackPool> pool = ToyPool(threads);
    {
      Toy bad(phases), good(phases);
      bad.throw_begin = true;
      bad.message = "thrown from Begin";
      pool->Push(&bad.job);
      pool->Push(&good.job);
      ExpectWaitThrows(pool.get(), &bad);
      EXPECT_EQ(bad.begins.load(), 1);
      EXPECT_EQ(bad.completed.load(), 0);
      EXPECT_EQ(bad.finishes[0].load(), 0);
      pool->Wait(&good.job);
      ExpectPacked(good, threads);
    }
    {
      Toy bad(phases), good(phases);
      bad.throw_phase = 1;
      bad.throw_range = phases[1] - 1;
      bad.message = "thrown from Run";
      pool->Push(&bad.job);
      pool->Push(&good.job);
      ExpectWaitThrows(pool.get(), &bad);
      ExpectStoppedIn(bad, 1, threads);
      EXPECT_EQ(bad.runs[1][phases[1] - 1].load(), 1);
      pool->Wait(&good.job);
      ExpectPacked(good, threads);
    }
    {
      Toy bad(phases), good(phases);
      bad.throw_finish = 1;
      bad.message = "thrown from Finish";
      pool->Push(&bad.job);
      pool->Push(&good.job);
      ExpectWaitThrows(pool.get(), &bad);
      ExpectPhases(bad, 2, threads);  // (Finish(1) itself ran, once)
      EXPECT_EQ(bad.finishes[2].load(), 0);
      EXPECT_EQ(bad.runs[2][0].load(), 0);
      pool->Wait(&good.job);
      ExpectPacked(good, threads);
    }
    pool->Quiesce();
    Toy after(phases);
    pool->Push(&after.job);
    pool->Wait(&after.job);
    ExpectPacked(after, threads);
  }
}

TEST(PackCodec, TeardownWhileJobsAreOpen) {
  for (int threads : {1, 4}) {
    for (bool destroy : {false, true}) {
      std::atomic<bool> gate{false};
      std::vector<std::unique_ptr<Toy>> toys;
      for (size_t i = 0; i < 5; ++i) {
        toys.emplace_back(new Toy({2}));
        toys.back()->gate = &gate;
      }
      std::unique_ptr<PackPool> pool = ToyPool(threads);
      for (auto& t : toys) pool->Push(&t->job);
      // four threads: the first two hold the ranges of job 0, the third opens
      // job 1; one thread: it holds a range of job 0 and job 1 stays queued
      const size_t nopen = threads == 1 ? 1 : 2;
      for (size_t i = 0; i < nopen; ++i) {
        while (toys[i]->begins.load() == 0) std::this_thread::yield();
      }
      std::atomic<bool> started{false};
      std::thread release([&] {
        while (!started.load()) std::this_thread::yield();
        // (most likely the teardown now waits for the open jobs; it has to
        // return whichever comes first)
        for (int i = 0; i < 1000; ++i) std::this_thread::yield();
        gate.store(true);
      });
      started.store(true);
      if (destroy) {
        pool.reset();
      } else {
        pool->Quiesce();
      }
      release.join();
      // the open jobs were finished; a queued job was dropped as it was, or
      // opened and finished after the release: nothing is left in progress
      size_t queued = 0;
      for (size_t i = 0; i < toys.size(); ++i) {
        const int st = toys[i]->state();
        if (i < nopen) {
          ExpectPacked(*toys[i], threads);
        } else if (st == PackJob::kPacked) {
          ExpectPacked(*toys[i], threads);
        } else {
          EXPECT_EQ(st, static_cast<int>(PackJob::kQueued));
          EXPECT_EQ(toys[i]->begins.load(), 0);
          ++queued;
        }
      }
      EXPECT_LE(queued, toys.size() - nopen);
      if (!destroy) {
        Toy after({1, 4});
        pool->Push(&after.job);
        pool->Wait(&after.job);
        ExpectPacked(after, threads);
      }
    }
  }
}
