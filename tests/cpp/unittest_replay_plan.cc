/*!
 * \file tests/cpp/unittest_replay_plan.cc
 * \brief Replay planning over the HBM epoch cache (src/gpu/replay_plan.h):
 *  replay order and cursors, the merge rule, the cap schedule, and that the
 *  next epoch's prelaunched first chunk is the first step of a fresh walk.
 */
#include <algorithm>
#include <vector>

#include "../../src/gpu/replay_plan.h"
#include "./testing.h"

namespace {

using dmlc::gpu::CachedChunk;
using dmlc::gpu::EpochOrder;
using dmlc::gpu::MergeCap;
using dmlc::gpu::ReplayMergeSettings;
using dmlc::gpu::ReplayPlan;
using dmlc::gpu::ReplayWalk;
using Segment = EpochOrder::Segment;

/*! \brief an unshuffled partition cached as chunks of `sizes`, back to back
 *  in the arena, every chunk ending with an EOL */
std::vector<CachedChunk> Chunks(const std::vector<size_t>& sizes) {
  std::vector<CachedChunk> v;
  size_t pos = 0;
  for (size_t n : sizes) {
    v.push_back(CachedChunk{pos, n, pos, pos + n, 0, pos, pos + n, true});
    pos += n;
  }
  return v;
}

size_t Sum(const std::vector<size_t>& sizes) {
  size_t n = 0;
  for (size_t s : sizes) n += s;
  return n;
}

ReplayPlan Plan(const std::vector<CachedChunk>& chunks, size_t total) {
  ReplayPlan plan;
  for (const CachedChunk& c : chunks) plan.Add(c);
  plan.Build(EpochOrder(0, 1, 1, 0, {{Segment{0, 0, total}}}));
  return plan;
}

void ExpectContiguous(const ReplayPlan& plan, size_t total) {
  ASSERT_GT(plan.size(), 0U);
  EXPECT_EQ(plan.begin_pos(0), 0U);
  for (size_t i = 0; i < plan.size(); ++i) {
    EXPECT_EQ(plan.end_pos(i) - plan.begin_pos(i), plan.chunk(i).size);
    if (i != 0) EXPECT_EQ(plan.begin_pos(i), plan.end_pos(i - 1));
  }
  EXPECT_EQ(plan.end_pos(plan.size() - 1), total);
}

void ExpectCursors(const ReplayPlan& plan, size_t total) {
  for (size_t i = 0; i < plan.size(); ++i) {
    EXPECT_EQ(plan.FindCursor(plan.begin_pos(i), total), i);
    EXPECT_EQ(plan.FindCursor(plan.begin_pos(i) + 1, total), ReplayPlan::kNotABoundary);
  }
  EXPECT_EQ(plan.FindCursor(total, total), plan.size());
}

}  // namespace

TEST(ReplayPlan, BuildUnshuffled) {
  const std::vector<size_t> sizes = {10, 20, 30, 40, 50};
  const ReplayPlan plan = Plan(Chunks(sizes), Sum(sizes));
  ASSERT_EQ(plan.size(), sizes.size());
  EXPECT_EQ(plan.cached_end(), 150U);
  ExpectContiguous(plan, 150);
  ExpectCursors(plan, 150);
  for (size_t i = 0; i < plan.size(); ++i) EXPECT_EQ(plan.chunk(i).size, sizes[i]);
}

TEST(ReplayPlan, BuildShuffled) {
  // sub-shards of 60, 0 and 90 bytes; the first pass cached 0's chunks
  // (30, 30) and then 2's (40, 50), tagged with their sub-shard ranges
  EpochOrder eo(0, 1, 3, 11,
                {{Segment{0, 0, 60}}, {Segment{0, 60, 60}}, {Segment{0, 60, 150}}});
  ReplayPlan plan;
  plan.Add(CachedChunk{0, 30, 0, 30, 0, 0, 30, true});
  plan.Add(CachedChunk{30, 30, 30, 60, 0, 30, 60, true});
  plan.Add(CachedChunk{60, 40, 60, 100, 2, 0, 40, true});
  plan.Add(CachedChunk{100, 50, 100, 150, 2, 40, 90, true});
  bool swapped = false;
  for (unsigned epoch = 0; epoch < 8; ++epoch) {
    eo.Apply(epoch);
    plan.Build(eo);
    ASSERT_EQ(plan.size(), 4U);
    ExpectContiguous(plan, 150);
    ExpectCursors(plan, 150);
    // sub-shards in visiting order, chunks in text order inside each
    const bool two_first = eo.sub_pos(2) < eo.sub_pos(0);
    swapped |= two_first;
    EXPECT_EQ(plan.chunk(0).off, two_first ? 60U : 0U);
    EXPECT_EQ(plan.chunk(1).off, two_first ? 100U : 30U);
    EXPECT_EQ(plan.chunk(2).off, two_first ? 0U : 60U);
    EXPECT_EQ(plan.chunk(3).off, two_first ? 30U : 100U);
    if (two_first) {
      // 2's last chunk and 0's first are neighbours in the order, not in the arena
      const ReplayPlan::Step s = plan.Merge(0, 1000, true);
      EXPECT_EQ(s.off, 60U);
      EXPECT_EQ(s.size, 90U);
      EXPECT_EQ(s.end_pos, 90U);
      EXPECT_EQ(s.next, 2U);
    }
  }
  EXPECT_TRUE(swapped);
}

TEST(ReplayPlan, EmptyPlan) {
  ReplayPlan plan;
  plan.Build(EpochOrder());
  EXPECT_EQ(plan.size(), 0U);
  EXPECT_EQ(plan.FindCursor(0, 0), 0U);  // the end of an empty partition
  EXPECT_EQ(plan.FindCursor(1, 0), ReplayPlan::kNotABoundary);
  ReplayWalk walk(&plan, 0, 100);
  ReplayPlan::Step s;
  EXPECT_TRUE(walk.AtEnd());
  EXPECT_FALSE(walk.NextEpochFirst(ReplayMergeSettings{true, 0}, &s));
}

TEST(ReplayPlan, MergeStopsAtAChunkWithoutEol) {
  std::vector<CachedChunk> chunks = Chunks({10, 10, 10});
  chunks[1].eol_end = false;
  const ReplayPlan plan = Plan(chunks, 30);
  ReplayPlan::Step s = plan.Merge(0, 1000, true);
  EXPECT_EQ(s.size, 20U);  // chunk 1 joins chunk 0, nothing joins chunk 1
  EXPECT_EQ(s.end_pos, 20U);
  EXPECT_EQ(s.next, 2U);
  s = plan.Merge(1, 1000, true);
  EXPECT_EQ(s.off, 10U);
  EXPECT_EQ(s.size, 10U);
  EXPECT_EQ(s.next, 2U);
}

TEST(ReplayPlan, MergeStopsAtAnArenaGap) {
  std::vector<CachedChunk> chunks = Chunks({10, 10, 10});
  chunks[2].off += 5;
  const ReplayPlan plan = Plan(chunks, 30);
  const ReplayPlan::Step s = plan.Merge(0, 1000, true);
  EXPECT_EQ(s.size, 20U);
  EXPECT_EQ(s.next, 2U);
}

TEST(ReplayPlan, MergeStopsAtTheCap) {
  const ReplayPlan plan = Plan(Chunks({10, 10, 10}), 30);
  ReplayPlan::Step s = plan.Merge(0, 20, true);  // size + next == cap: merged
  EXPECT_EQ(s.off, 0U);
  EXPECT_EQ(s.size, 20U);
  EXPECT_EQ(s.end_pos, 20U);
  EXPECT_EQ(s.next, 2U);
  s = plan.Merge(0, 19, true);  // size + next == cap + 1: not merged
  EXPECT_EQ(s.size, 10U);
  EXPECT_EQ(s.end_pos, 10U);
  EXPECT_EQ(s.next, 1U);
  s = plan.Merge(0, 5, true);  // a chunk above the cap is still taken whole
  EXPECT_EQ(s.size, 10U);
  EXPECT_EQ(s.next, 1U);
  s = plan.Merge(1, 1000, true);  // to the end of the list
  EXPECT_EQ(s.off, 10U);
  EXPECT_EQ(s.size, 20U);
  EXPECT_EQ(s.end_pos, 30U);
  EXPECT_EQ(s.next, 3U);
}

TEST(ReplayPlan, WithoutMergingEveryStepIsOneChunk) {
  const std::vector<size_t> sizes = {10, 20, 30, 40};
  const ReplayPlan plan = Plan(Chunks(sizes), Sum(sizes));
  ReplayWalk walk(&plan, 0, 1000);
  walk.Start(0);
  size_t pos = 0;
  for (size_t i = 0; i < sizes.size(); ++i) {
    ASSERT_FALSE(walk.AtEnd());
    const ReplayPlan::Step s = walk.Next(ReplayMergeSettings{false, 0});
    EXPECT_EQ(s.off, pos);
    EXPECT_EQ(s.size, sizes[i]);
    pos += sizes[i];
    EXPECT_EQ(s.end_pos, pos);
    EXPECT_EQ(s.next, i + 1);
  }
  EXPECT_TRUE(walk.AtEnd());
}

TEST(ReplayPlan, CapSchedule) {
  {
    MergeCap cap(/*replay_first_bytes=*/16, /*replay_chunk_bytes=*/100);
    const size_t want[] = {16, 32, 64, 100, 100, 100};
    for (size_t w : want) EXPECT_EQ(cap.Next(0), w);
    for (int i = 0; i < 200; ++i) EXPECT_EQ(cap.Next(0), 100U);  // no wrap-around
  }
  {
    MergeCap cap(0, 100);  // no ramp: every chunk takes replay_chunk_bytes
    for (int i = 0; i < 4; ++i) EXPECT_EQ(cap.Next(0), 100U);
  }
  {
    MergeCap cap(16, 100);  // a merge limit: the walk starts at the limit
    for (int i = 0; i < 4; ++i) EXPECT_EQ(cap.Next(150), 150U);
  }
  {
    MergeCap cap(200, 100);  // a first cap above the chunk cap is clipped
    EXPECT_EQ(cap.Next(0), 100U);
  }
}

TEST(ReplayPlan, WalkMergesUnderTheSchedule) {
  const std::vector<size_t> sizes(12, 8);  // 96 bytes in chunks of 8
  const ReplayPlan plan = Plan(Chunks(sizes), 96);
  ReplayWalk walk(&plan, /*first=*/16, /*chunk=*/40);
  walk.Start(0);
  const size_t want[] = {16, 32, 40, 8};  // caps 16, 32, 40 (clipped), then the rest
  size_t pos = 0;
  for (size_t w : want) {
    ASSERT_FALSE(walk.AtEnd());
    const ReplayPlan::Step s = walk.Next(ReplayMergeSettings{true, 0});
    EXPECT_EQ(s.off, pos);
    EXPECT_EQ(s.size, w);
    pos += w;
    EXPECT_EQ(s.end_pos, pos);
  }
  EXPECT_TRUE(walk.AtEnd());
  // a restart in the middle begins the schedule again
  walk.Start(3);
  const ReplayPlan::Step s = walk.Next(ReplayMergeSettings{true, 0});
  EXPECT_EQ(s.off, 24U);
  EXPECT_EQ(s.size, 16U);
}

TEST(ReplayPlan, NextEpochFirstIsTheFirstStepOfAFreshWalk) {
  struct Setting {
    size_t first, chunk, limit, chunk_size;
    bool merge;
  };
  const Setting table[] = {
      {0, 64, 0, 8, true},     // no ramp, chunk size divides the cap
      {0, 64, 0, 12, true},    // does not divide it
      {16, 64, 0, 8, true},    // ramp from 16
      {20, 64, 0, 8, true},    // a first cap the chunk size does not divide
      {16, 64, 120, 8, true},  // a merge limit: starts at the limit
      {0, 64, 100, 12, true},  // limit the chunk size does not divide
      {100, 64, 0, 8, true},   // first cap above the chunk cap
      {4, 64, 0, 8, true},     // first cap below one chunk: that chunk alone
      {16, 64, 0, 8, false},   // merging off
  };
  for (const Setting& t : table) {
    const std::vector<size_t> sizes(20, t.chunk_size);
    const ReplayPlan plan = Plan(Chunks(sizes), Sum(sizes));
    const ReplayMergeSettings settings{t.merge, t.limit};
    // from the rule as documented: the first cap is the limit if there is
    // one, else replay_first_bytes, else replay_chunk_bytes, and never above
    // the limit / replay_chunk_bytes; whole chunks are added while they fit
    const size_t bound = t.limit != 0 ? t.limit : t.chunk;
    const size_t cap = std::min(t.limit != 0 ? t.limit : (t.first != 0 ? t.first : t.chunk), bound);
    size_t want = t.chunk_size;
    while (t.merge && want + t.chunk_size <= cap) want += t.chunk_size;

    ReplayWalk fresh(&plan, t.first, t.chunk);
    fresh.Start(0);
    const ReplayPlan::Step first = fresh.Next(settings);
    EXPECT_EQ(first.off, 0U);
    EXPECT_EQ(first.size, want);

    // asked at the start, in the middle and at the end of a pass
    ReplayWalk walk(&plan, t.first, t.chunk);
    walk.Start(0);
    for (;;) {
      ReplayPlan::Step pre{99, 99, 99, 99};
      ASSERT_TRUE(walk.NextEpochFirst(settings, &pre));
      EXPECT_EQ(pre.off, first.off);
      EXPECT_EQ(pre.size, first.size);
      EXPECT_EQ(pre.end_pos, first.end_pos);
      EXPECT_EQ(pre.next, first.next);
      if (walk.AtEnd()) break;
      walk.Next(settings);
    }
  }
}
