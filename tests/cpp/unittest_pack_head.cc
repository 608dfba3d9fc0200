/*!
 * \file tests/cpp/unittest_pack_head.cc
 * \brief Head jobs of the packed H2D transfer (src/gpu/chunk_feed.h): when a
 *  pass ends, the chunk feed queues the first pieces of the next pass to the
 *  pack pool (src/gpu/pack_pool.h) and a rewind adopts them.  Driven here as
 *  the feed drives the pool: a pass is settled, two more jobs are pushed with
 *  sequence numbers from 0, and they are then dropped (Quiesce) or adopted;
 *  the rule for the first piece of a pass in each job state (DecideSubmit,
 *  WaitMeansPoolBehind).  Part of the ThreadSanitizer run of the suite.
 */
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../src/gpu/pack_pool.h"
#include "../../src/gpu/text_pack_codec.h"
#include "./testing.h"

namespace {

using dmlc::gpu::DecideSubmit;
using dmlc::gpu::PackJob;
using dmlc::gpu::PackPool;
using dmlc::gpu::SubmitAction;
using dmlc::gpu::WaitMeansPoolBehind;

std::string Text(size_t n, unsigned seed) {
  static const char kSym[] = "0123456789:. \n-e";
  std::string s(n, '0');
  unsigned x = seed * 2654435761u + 7u;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    s[i] = kSym[(x >> 24) % 16];
  }
  return s;
}

struct Piece {
  std::string text;
  std::vector<uint8_t> out;
  std::unique_ptr<PackJob> job;
};

Piece MakePiece(size_t n, unsigned seed, size_t seq, bool head) {
  Piece p;
  p.text = Text(n, seed);
  p.out.assign(p.text.size() + 4096, 0xEE);
  p.job.reset(new PackJob());
  p.job->ptr = p.text.data();
  p.job->size = p.text.size();
  p.job->seq = seq;
  p.job->head = head;
  p.job->out = p.out.data();
  return p;
}

/*! \brief a pass of `count` pieces, every job waited for as the cursor passes it */
void RunPass(PackPool* pool, size_t count, size_t n) {
  std::vector<Piece> pass;
  for (size_t i = 0; i < count; ++i) pass.push_back(MakePiece(n + 31 * i, 100 + i, i, false));
  for (auto& p : pass) pool->Push(p.job.get());
  for (size_t i = 0; i < count; ++i) {
    pool->SetSubmitted(i + 1);
    pool->Wait(pass[i].job.get());
    ASSERT_EQ(pass[i].job->state.load(), static_cast<int>(PackJob::kPacked));
  }
}

bool Busy() { return true; }
bool Idle() { return false; }

}  // namespace

TEST(PackHead, AdoptedHeadJobsEqualPackText) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  // distance 2, as while the pool is behind the link: head jobs carry the
  // sequence numbers 0 and 1, so the cursor has to restart with them
  for (size_t distance : {size_t(0), size_t(2)}) {
    PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), distance);
    pool.SetDistance(0);
    RunPass(&pool, 6, 300000);
    pool.SetDistance(distance);
    // the pass is settled: the cursor restarts and the next pass's first two
    // pieces are queued
    pool.SetSubmitted(0);
    std::vector<Piece> head;
    head.push_back(MakePiece(300000, 1, 0, true));
    head.push_back(MakePiece(300017, 2, 1, true));
    for (auto& p : head) pool.Push(p.job.get());
    if (distance != 0) {
      // left unstarted for the consumer, which claims them raw as any piece
      // next to the cursor in that state
      pool.Quiesce();
      for (auto& p : head) {
        EXPECT_EQ(p.job->state.load(), static_cast<int>(PackJob::kQueued));
        EXPECT_TRUE(pool.TryClaimRaw(p.job.get()));
      }
      continue;
    }
    // the rewind adopts them: found packed or waited for, never packed twice
    for (size_t i = 0; i < head.size(); ++i) {
      pool.SetSubmitted(i + 1);
      pool.Wait(head[i].job.get());
      const Piece& p = head[i];
      ASSERT_EQ(p.job->state.load(), static_cast<int>(PackJob::kPacked));
      std::vector<uint8_t> want;
      ASSERT_TRUE(dmlc::gpu::PackText(reinterpret_cast<const uint8_t*>(p.text.data()),
                                      p.text.size(), alphabet, dmlc::gpu::kPackMaxRatio, &want));
      ASSERT_EQ(p.job->packed_bytes, want.size());
      EXPECT_EQ(std::memcmp(p.out.data(), want.data(), want.size()), 0);
    }
  }
}

TEST(PackHead, QuiesceLeavesNoHeadJobReferenced) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  for (int round = 0; round < 8; ++round) {
    PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
    RunPass(&pool, 3, 100000);
    pool.SetSubmitted(0);
    std::vector<Piece> head;
    head.push_back(MakePiece(1 << 20, 3, 0, true));
    head.push_back(MakePiece(1 << 20, 4, 1, true));
    for (auto& p : head) pool.Push(p.job.get());
    // any other Seek, a failed pass: dropped at whatever point the pool is
    pool.Quiesce();
    for (auto& p : head) {
      const int st = p.job->state.load();
      EXPECT_TRUE(st == PackJob::kPacked || st == PackJob::kQueued);
    }
    // freed at once: a pool thread that still touched one would be a
    // use-after-free (the sanitizer builds of this binary see it)
    head.clear();
    // the pool goes on with the pass that follows
    RunPass(&pool, 2, 100000);
  }
}

TEST(PackHead, DestroyedWithHeadJobsOpen) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  std::vector<Piece> head;
  head.push_back(MakePiece(1 << 20, 5, 0, true));
  head.push_back(MakePiece(1 << 20, 6, 1, true));
  {
    PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
    RunPass(&pool, 2, 100000);
    pool.SetSubmitted(0);
    for (auto& p : head) pool.Push(p.job.get());
  }  // the destructor finishes the open jobs and forgets the queued ones
  for (auto& p : head) {
    const int st = p.job->state.load();
    EXPECT_TRUE(st == PackJob::kPacked || st == PackJob::kQueued);
  }
}

TEST(PackHead, FirstPieceOfAPassInEachState) {
  // nothing is in flight when a pass begins, and no copy is outstanding
  const bool kNothingInflight = true;
  for (bool behind : {false, true}) {
    // packed ahead of the rewind: submitted packed
    EXPECT_TRUE(DecideSubmit(PackJob::kPacked, false, kNothingInflight, behind, Idle) ==
                SubmitAction::kSubmit);
    // its pack is in progress: waited for
    EXPECT_TRUE(DecideSubmit(PackJob::kPacking, false, kNothingInflight, behind, Idle) ==
                SubmitAction::kWait);
    // not started: claimed raw, as a pass that starts cold
    EXPECT_TRUE(DecideSubmit(PackJob::kQueued, false, kNothingInflight, behind, Idle) ==
                SubmitAction::kClaimRaw);
    // rejected by the 3/4 rule: submitted (raw); failed: Wait rethrows
    EXPECT_TRUE(DecideSubmit(PackJob::kRejected, false, kNothingInflight, behind, Idle) ==
                SubmitAction::kSubmit);
    EXPECT_TRUE(DecideSubmit(PackJob::kFailed, false, kNothingInflight, behind, Idle) ==
                SubmitAction::kWait);
  }
  // the second head job, while the first crosses the link: left to the pool
  EXPECT_TRUE(DecideSubmit(PackJob::kPacking, false, false, false, Busy) == SubmitAction::kDefer);
  EXPECT_TRUE(DecideSubmit(PackJob::kQueued, false, false, false, Busy) == SubmitAction::kDefer);
}

TEST(PackHead, WaitAtPassStartDoesNotMarkThePoolBehind) {
  // a wait with the link idle means the pool is slower than the link ...
  EXPECT_TRUE(WaitMeansPoolBehind(/*link_idle=*/true, /*pack_wait=*/false, /*head_of_pass=*/false));
  // ... unless the piece is the first of a pass and was queued ahead of the
  // rewind: the link idles because the pass has only begun
  EXPECT_FALSE(WaitMeansPoolBehind(true, false, true));
  // never under pack_wait, never while a copy was outstanding
  EXPECT_FALSE(WaitMeansPoolBehind(true, true, false));
  EXPECT_FALSE(WaitMeansPoolBehind(true, true, true));
  EXPECT_FALSE(WaitMeansPoolBehind(false, false, false));
  EXPECT_FALSE(WaitMeansPoolBehind(false, false, true));
}
