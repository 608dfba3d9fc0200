/*!
 * \file src/gpu/epoch_order.h
 * \brief The shuffled mode's epoch order (cfg.shuffle_parts > 1): the
 *  partition's K sub-shards, each a list of file segments, visited in
 *  InputSplitShuffle::VisitOrder's per-epoch order.  Epoch cursors run over
 *  the concatenation of the sub-shards in that order.  With shuffle_parts <= 1
 *  it is the identity: one sub-shard holding the whole partition.
 *
 * Plain C++ (no HIP): unit-tested on the CPU, tests/cpp/unittest_epoch_order.cc.
 */
#ifndef DMLC_SRC_GPU_EPOCH_ORDER_H_
#define DMLC_SRC_GPU_EPOCH_ORDER_H_

#include <dmlc/input_split_shuffle.h>
#include <dmlc/logging.h>

#include <vector>

#include "../io/input_split_base.h"

namespace dmlc {
namespace gpu {

class EpochOrder {
 public:
  using Segment = io::InputSplitBase::Segment;

  /*! \brief the identity over an empty partition */
  EpochOrder() : EpochOrder(0, 1, 1, 0, std::vector<std::vector<Segment>>(1)) {}
  /*!
   * \param subs the segments of sub-shard 0, 1, ... (one list when
   *  shuffle_parts <= 1); empty segments are dropped
   */
  EpochOrder(unsigned part, unsigned nparts, unsigned shuffle_parts, int shuffle_seed,
             const std::vector<std::vector<Segment>>& subs)
      : part_(part),
        nparts_(nparts),
        shuffle_parts_(shuffle_parts > 1 ? shuffle_parts : 1),
        shuffle_seed_(shuffle_seed) {
    CHECK_EQ(subs.size(), static_cast<size_t>(shuffle_parts_)) << "one segment list per sub-shard";
    for (const auto& sub : subs) {
      sub_first_.push_back(all_segs_.size());
      size_t bytes = 0;
      for (const Segment& sg : sub) {
        if (sg.end <= sg.begin) continue;
        all_segs_.push_back(sg);
        bytes += sg.end - sg.begin;
      }
      sub_bytes_.push_back(bytes);
      total_bytes_ += bytes;
    }
    sub_first_.push_back(all_segs_.size());
    Apply(0);
  }

  /*! \brief switch to epoch `epoch`'s visiting order and sub-shard offsets */
  void Apply(unsigned epoch) {
    epoch_ = epoch;
    order_ = InputSplitShuffle::VisitOrder(part_, nparts_, shuffle_parts_, shuffle_seed_, epoch);
    sub_pos_.assign(shuffle_parts_, 0);
    size_t pos = 0;
    for (unsigned j : order_) {
      sub_pos_[j] = pos;
      pos += sub_bytes_[j];
    }
  }

  bool shuffled() const { return shuffle_parts_ > 1; }
  unsigned epoch() const { return epoch_; }
  const std::vector<unsigned>& order() const { return order_; }
  /*! \brief sub-shard 0's segments, 1's, ... (what SegmentIndices indexes) */
  const std::vector<Segment>& all_segments() const { return all_segs_; }
  size_t total_bytes() const { return total_bytes_; }
  /*! \brief epoch cursor at which sub-shard j starts, and its bytes */
  size_t sub_pos(unsigned j) const { return sub_pos_[j]; }
  size_t sub_bytes(unsigned j) const { return sub_bytes_[j]; }

  /*! \brief this epoch's segments, as indices into all_segments() */
  std::vector<size_t> SegmentIndices() const {
    std::vector<size_t> idx;
    for (unsigned j : order_) {
      for (size_t g = sub_first_[j]; g < sub_first_[j + 1]; ++g) idx.push_back(g);
    }
    return idx;
  }
  std::vector<Segment> Segments() const {
    std::vector<Segment> segs;
    for (size_t g : SegmentIndices()) segs.push_back(all_segs_[g]);
    return segs;
  }
  /*! \brief a pinned fill ends with each sub-shard (chunks never mix two) */
  std::vector<bool> Stops() const {
    std::vector<bool> stop;
    for (unsigned j : order_) {
      for (size_t g = sub_first_[j]; g < sub_first_[j + 1]; ++g) {
        stop.push_back(g + 1 == sub_first_[j + 1]);
      }
    }
    return stop;
  }
  /*! \brief sub-shard holding epoch cursor `pos` (the first one starting at or
   *  before it with bytes left), and the offset inside it */
  unsigned SubOf(size_t pos, size_t* local) const {
    for (unsigned j : order_) {
      if (pos >= sub_pos_[j] && pos < sub_pos_[j] + sub_bytes_[j]) {
        *local = pos - sub_pos_[j];
        return j;
      }
    }
    // the end of the partition.  The identity keeps the cursor (chunks of an
    // unshuffled partition are addressed by partition offset)
    *local = shuffled() ? 0 : pos;
    return order_.back();
  }

 private:
  unsigned part_, nparts_, shuffle_parts_;
  int shuffle_seed_;
  unsigned epoch_{0};
  std::vector<unsigned> order_;
  std::vector<Segment> all_segs_;
  std::vector<size_t> sub_first_, sub_bytes_, sub_pos_;
  size_t total_bytes_{0};
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_EPOCH_ORDER_H_
