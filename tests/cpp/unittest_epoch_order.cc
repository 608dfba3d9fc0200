/*!
 * \file tests/cpp/unittest_epoch_order.cc
 * \brief The device parser's shuffled epoch order (src/gpu/epoch_order.h):
 *  segment lists, stops and cursor lookup over hand-made sub-shards.
 */
#include <algorithm>
#include <vector>

#include "../../src/gpu/epoch_order.h"
#include "./testing.h"

namespace {

using dmlc::gpu::EpochOrder;
using Segment = EpochOrder::Segment;

// sub-shard 0: two segments (150 bytes), 1: zero bytes, 2: one segment (70)
std::vector<std::vector<Segment>> Subs() {
  return {{Segment{0, 0, 100}, Segment{1, 0, 50}}, {Segment{1, 50, 50}}, {Segment{1, 50, 120}}};
}
// all_segments() indices of each sub-shard (the empty segment is dropped)
const std::vector<std::vector<size_t>> kSubSegs = {{0, 1}, {}, {2}};
const size_t kBytes[3] = {150, 0, 70};
const size_t kTotal = 220;

EpochOrder Make() { return EpochOrder(0, 1, 3, /*shuffle_seed=*/7, Subs()); }

}  // namespace

TEST(EpochOrder, SegmentsFollowTheVisitingOrder) {
  EpochOrder eo = Make();
  ASSERT_EQ(eo.all_segments().size(), 3U);
  EXPECT_EQ(eo.total_bytes(), kTotal);
  for (unsigned epoch = 0; epoch < 4; ++epoch) {
    eo.Apply(epoch);
    EXPECT_EQ(eo.epoch(), epoch);
    const std::vector<unsigned> order = eo.order();
    EXPECT_TRUE(order == dmlc::InputSplitShuffle::VisitOrder(0, 1, 3, 7, epoch));
    std::vector<unsigned> sorted = order;
    std::sort(sorted.begin(), sorted.end());
    EXPECT_TRUE(sorted == (std::vector<unsigned>{0, 1, 2}));

    std::vector<size_t> want_idx;
    std::vector<bool> want_stop;
    size_t pos = 0;
    for (unsigned j : order) {
      for (size_t g : kSubSegs[j]) {
        want_idx.push_back(g);
        want_stop.push_back(g == kSubSegs[j].back());
      }
      EXPECT_EQ(eo.sub_pos(j), pos);  // running sum in visiting order
      EXPECT_EQ(eo.sub_bytes(j), kBytes[j]);
      pos += kBytes[j];
    }
    EXPECT_EQ(pos, kTotal);
    const std::vector<size_t> idx = eo.SegmentIndices();
    EXPECT_TRUE(idx == want_idx);
    std::vector<size_t> perm = idx;
    std::sort(perm.begin(), perm.end());
    EXPECT_TRUE(perm == (std::vector<size_t>{0, 1, 2}));
    EXPECT_TRUE(eo.Stops() == want_stop);
    const std::vector<Segment> segs = eo.Segments();
    ASSERT_EQ(segs.size(), idx.size());
    for (size_t i = 0; i < segs.size(); ++i) {
      const Segment& a = eo.all_segments()[idx[i]];
      EXPECT_EQ(segs[i].file_index, a.file_index);
      EXPECT_EQ(segs[i].begin, a.begin);
      EXPECT_EQ(segs[i].end, a.end);
    }
  }
}

TEST(EpochOrder, SubOfAtSubShardEnds) {
  EpochOrder eo = Make();
  for (unsigned epoch = 0; epoch < 4; ++epoch) {
    eo.Apply(epoch);
    for (unsigned j : {0U, 2U}) {
      size_t local = 99;
      EXPECT_EQ(eo.SubOf(eo.sub_pos(j), &local), j);
      EXPECT_EQ(local, 0U);
      EXPECT_EQ(eo.SubOf(eo.sub_pos(j) + kBytes[j] - 1, &local), j);
      EXPECT_EQ(local, kBytes[j] - 1);
    }
    // the empty sub-shard holds no cursor: the one visited after it does
    size_t local = 99;
    // (visited last it starts at the end of the partition, see below)
    if (eo.sub_pos(1) < kTotal) {
      const unsigned at_empty = eo.SubOf(eo.sub_pos(1), &local);
      EXPECT_NE(at_empty, 1U);
      EXPECT_EQ(eo.sub_pos(at_empty), eo.sub_pos(1));
      EXPECT_EQ(local, 0U);
    }
    // the end of the partition: the last sub-shard in order, offset 0
    local = 99;
    EXPECT_EQ(eo.SubOf(kTotal, &local), eo.order().back());
    EXPECT_EQ(local, 0U);
  }
}

TEST(EpochOrder, EmptySubShardIsSkippedWhereverItIsVisited) {
  // over enough epochs the empty sub-shard is visited first, in the middle and last
  EpochOrder eo = Make();
  bool first = false, middle = false, last = false;
  for (unsigned epoch = 0; epoch < 64; ++epoch) {
    eo.Apply(epoch);
    const std::vector<unsigned>& o = eo.order();
    first |= o[0] == 1;
    middle |= o[1] == 1;
    last |= o[2] == 1;
    for (size_t pos = 0; pos < kTotal; pos += 10) {
      size_t local = 0;
      const unsigned j = eo.SubOf(pos, &local);
      EXPECT_NE(j, 1U);
      EXPECT_EQ(eo.sub_pos(j) + local, pos);
      EXPECT_LT(local, kBytes[j]);
    }
  }
  EXPECT_TRUE(first && middle && last);
}

TEST(EpochOrder, UnshuffledIsTheIdentity) {
  EpochOrder eo(2, 5, 1, 3, {{Segment{0, 10, 60}, Segment{1, 0, 0}, Segment{2, 0, 30}}});
  EXPECT_FALSE(eo.shuffled());
  EXPECT_EQ(eo.total_bytes(), 80U);
  for (unsigned epoch = 0; epoch < 3; ++epoch) {
    eo.Apply(epoch);
    EXPECT_TRUE(eo.order() == (std::vector<unsigned>{0}));
    EXPECT_EQ(eo.sub_pos(0), 0U);
    EXPECT_EQ(eo.sub_bytes(0), 80U);
    EXPECT_TRUE(eo.SegmentIndices() == (std::vector<size_t>{0, 1}));
    for (size_t pos : {size_t(0), size_t(5), size_t(79), size_t(80), size_t(83)}) {
      size_t local = 99;
      EXPECT_EQ(eo.SubOf(pos, &local), 0U);
      EXPECT_EQ(local, pos);
    }
  }
  // shuffle_parts 0 is treated as 1
  EpochOrder zero(0, 1, 0, 0, {{Segment{0, 0, 8}}});
  size_t local = 0;
  EXPECT_EQ(zero.SubOf(3, &local), 0U);
  EXPECT_EQ(local, 3U);
  EXPECT_FALSE(EpochOrder().shuffled());
  EXPECT_EQ(EpochOrder().total_bytes(), 0U);
}
