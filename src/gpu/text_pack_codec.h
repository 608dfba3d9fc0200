/*!
 * \file src/gpu/text_pack_codec.h
 * \brief The two text codes as codecs of the pack pool (pack_codec.h,
 *  pack_pool.h), and the factory that picks one.
 *
 * NibbleCodec (text_pack.h).  Phase 0 packs: a range writes its nibbles into
 * the job's slot and lists its exception blocks.  The lists are kept per range
 * and concatenated in range order when the phase ends, so a job's packed bytes
 * equal PackText of the same input whatever the thread count or the timing.
 * The end of phase 0 also writes the header and the exception indices; up to
 * kCopyBlocks exception blocks are copied there and then, a longer list is
 * copied in phase 1, in ranges of kCopyBlocks blocks.
 *
 * DenseCodec (text_pack_dense.h).  A range's packed size is not known
 * beforehand: a thread packs its range into its scratch buffer, which stays in
 * its cache, reserves that many bytes of the job's slot through an atomic
 * cursor (ranges start at multiples of 16 bytes), copies the range there with
 * streaming stores and fills the range's directory entry.  Ranges land in the
 * order the threads finish them, so the packed bytes of a job depend on
 * timing; the decoded text, the packed size and the set of per-range payloads
 * do not.  The end of the one phase writes the header (n, the table, the
 * escape code, the directory).  There are no exception blocks.  The table of a
 * job is chosen from a sample of its text when it is queued (Prepare).
 */
#ifndef DMLC_SRC_GPU_TEXT_PACK_CODEC_H_
#define DMLC_SRC_GPU_TEXT_PACK_CODEC_H_

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include "./pack_codec.h"
#include "./pack_pool.h"
#include "./text_pack.h"
#include "./text_pack_dense.h"

namespace dmlc {
namespace gpu {

class NibbleCodec : public PackCodec {
 public:
  /*! \brief exception blocks per range of the copy that follows the pack */
  static constexpr size_t kCopyBlocks = 1024;

  explicit NibbleCodec(const uint8_t alphabet[16]) : encoder_(alphabet) {
    std::memcpy(alphabet_, alphabet, 16);
  }
  std::unique_ptr<PackJobState> NewState() const override {
    return std::unique_ptr<PackJobState>(new State(this));
  }

 private:
  class State : public PackJobState {
   public:
    explicit State(const NibbleCodec* codec) : codec_(codec) {}
    size_t Begin(PackJob* job, size_t range_blocks, bool* fits) override {
      job_ = job;
      range_blocks_ = range_blocks;
      nranges_ = std::max<size_t>(1, (PackBlocks(job->size) + range_blocks - 1) / range_blocks);
      exc_limit_ = PackMaxExceptions(job->size, job->ratio);
      exc_total_.store(0);
      if (exc_.size() < nranges_) exc_.resize(nranges_);
      *fits = exc_limit_ >= 0;
      return nranges_;
    }
    bool Run(int phase, size_t r, uint8_t*) override {
      const PackJob* job = job_;
      const uint8_t* text = reinterpret_cast<const uint8_t*>(job->ptr);
      if (phase == 1) {
        PackCopyExceptions(text, job->size, all_, r * kCopyBlocks,
                           std::min(all_.size(), (r + 1) * kCopyBlocks), job->out);
        return true;
      }
      std::vector<uint32_t>& exc = exc_[r];
      exc.clear();
      const size_t b0 = r * range_blocks_;
      const size_t b1 = std::min(PackBlocks(job->size), b0 + range_blocks_);
      return PackRange(text, job->size, b0, b1, codec_->encoder_, job->out + sizeof(PackedHeader),
                       &exc, &exc_total_, exc_limit_);
    }
    size_t Finish(int phase, bool* packed) override {
      PackJob* job = job_;
      *packed = true;
      if (phase == 1) return 0;
      all_.clear();
      for (size_t r = 0; r < nranges_; ++r) {
        all_.insert(all_.end(), exc_[r].begin(), exc_[r].end());
      }
      if (static_cast<long>(all_.size()) > exc_limit_) {
        *packed = false;
        return 0;
      }
      job->packed_bytes = PackFinishHeader(job->size, codec_->alphabet_, all_, job->out);
      job->nexc = static_cast<uint32_t>(all_.size());
      const size_t ncopy = (all_.size() + kCopyBlocks - 1) / kCopyBlocks;
      if (ncopy <= 1) {
        PackCopyExceptions(reinterpret_cast<const uint8_t*>(job->ptr), job->size, all_, 0,
                           all_.size(), job->out);
        return 0;
      }
      return ncopy;
    }

   private:
    const NibbleCodec* codec_;
    PackJob* job_{nullptr};
    size_t range_blocks_{0}, nranges_{0};
    long exc_limit_{0};
    std::atomic<long> exc_total_{0};
    /*! \brief exception blocks per range (entries keep their capacity) */
    std::vector<std::vector<uint32_t>> exc_;
    std::vector<uint32_t> all_;
  };

  const PackEncoder encoder_;
  uint8_t alphabet_[16];
};

class DenseCodec : public PackCodec {
 public:
  /*! \param csv, delimiter the format, for the jobs' tables */
  DenseCodec(bool csv, char delimiter) : csv_(csv), delimiter_(delimiter) {}
  void Prepare(PackJob* job) const override {
    job->table = DenseSelectTable(reinterpret_cast<const uint8_t*>(job->ptr), job->size, csv_,
                                  delimiter_);
  }
  /*! \brief a range's buffer */
  size_t ScratchBytes(size_t range_blocks) const override {
    return DenseRangeCapacity(range_blocks);
  }
  std::unique_ptr<PackJobState> NewState() const override {
    return std::unique_ptr<PackJobState>(new State());
  }

 private:
  class State : public PackJobState {
   public:
    size_t Begin(PackJob* job, size_t range_blocks, bool* fits) override {
      job_ = job;
      range_blocks_ = range_blocks;
      const size_t nranges = DenseRanges(job->size, range_blocks);
      dense_.reset(new DenseEncoder(job->table));
      dir_.assign(nranges, DenseDirEntry{0, 0});
      cursor_.store(DenseHeaderBytes(nranges, DenseEntryBytes(job->table)));
      escape_bytes_.store(0);
      raw_blocks_.store(0);
      limit_ = job->ratio < 0 ? DenseMaxBytes(job->size, range_blocks)
                              : static_cast<size_t>(job->ratio * static_cast<double>(job->size));
      *fits = true;
      return std::max<size_t>(1, nranges);
    }
    bool Run(int, size_t r, uint8_t* scratch) override {
      const PackJob* job = job_;
      const size_t b0 = r * range_blocks_;
      const size_t b1 = std::min(PackBlocks(job->size), b0 + range_blocks_);
      if (b0 >= b1) return true;  // (an empty job has one range and no block)
      size_t escapes = 0, raw = 0;
      const size_t len = PackRangeDense(reinterpret_cast<const uint8_t*>(job->ptr), job->size, b0,
                                        b1, *dense_, scratch, &escapes, &raw);
      const size_t at = cursor_.fetch_add(len);
      if (at + len > limit_) return false;
      DenseCopyOut(scratch, len, job->out + at);
      dir_[r] = DenseDirEntry{static_cast<uint32_t>(at), static_cast<uint32_t>(len)};
      escape_bytes_.fetch_add(escapes, std::memory_order_relaxed);
      raw_blocks_.fetch_add(raw, std::memory_order_relaxed);
      return true;
    }
    size_t Finish(int, bool* packed) override {
      PackJob* job = job_;
      DenseWriteHeader(job->size, range_blocks_, job->table, dir_, job->out);
      job->packed_bytes = cursor_.load();
      job->nexc = 0;
      job->dense = true;
      job->escape_bytes = escape_bytes_.load();
      job->raw_blocks = raw_blocks_.load();
      *packed = true;
      return 0;
    }

   private:
    PackJob* job_{nullptr};
    size_t range_blocks_{0};
    // the slot's cursor and its bound, the directory, the job's encoder and
    // its counters
    std::atomic<size_t> cursor_{0}, escape_bytes_{0}, raw_blocks_{0};
    size_t limit_{0};
    std::vector<DenseDirEntry> dir_;
    std::unique_ptr<DenseEncoder> dense_;
  };

  const bool csv_;
  const char delimiter_;
};

/*! \brief the code a pool packs with */
enum class PackCode : int { kNibble = 0, kDense = 1 };

/*! \param csv, delimiter the format: the nibble code's alphabet, the dense
 *  code's tables */
inline std::unique_ptr<PackCodec> MakePackCodec(PackCode code, bool csv, char delimiter) {
  if (code == PackCode::kDense) return std::unique_ptr<PackCodec>(new DenseCodec(csv, delimiter));
  uint8_t alphabet[16];
  PackAlphabet(csv, delimiter, alphabet);
  return std::unique_ptr<PackCodec>(new NibbleCodec(alphabet));
}

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_TEXT_PACK_CODEC_H_
