/*!
 * \file src/gpu/pack_codec.h
 * \brief The seam between the pack pool's scheduler (pack_pool.h) and the code
 *  it packs with.  The pool cuts a job into phases of ranges and hands the
 *  ranges to its threads; what a range, a phase and a job's header are is the
 *  codec's business.  The text codes are in text_pack_codec.h.
 *
 * A PackCodec is shared by the pool's threads and is not changed after the
 * pool is built.  It makes the pool's PackJobState objects, one per job the
 * pool may have open at a time; each is reused job after job (Begin), so what
 * it allocates keeps its capacity.
 *
 * Of a PackJobState the pool calls, for each job it opens:
 *  - Begin, once, by one thread;
 *  - Run(phase, r, scratch) for every range r of the phase, by any thread,
 *    several at a time, each range once;
 *  - Finish(phase), once, by the thread that reported the phase's last range,
 *    after every Run of the phase has returned and before any Run of the next.
 * Once Begin or a Run has said that the job does not fit, or any call has
 * thrown, the pool calls no further Run that does work and no Finish: the job
 * is settled rejected, or failed with the first exception.
 */
#ifndef DMLC_SRC_GPU_PACK_CODEC_H_
#define DMLC_SRC_GPU_PACK_CODEC_H_

#include <cstddef>
#include <cstdint>
#include <memory>

namespace dmlc {
namespace gpu {

struct PackJob;  // pack_pool.h

/*! \brief one open job of a codec */
class PackJobState {
 public:
  virtual ~PackJobState() = default;
  /*!
   * \brief take up a job whose ranges are range_blocks 256-byte blocks long
   * \param fits set to false when the job cannot fit from the start
   * \return ranges of phase 0, at least 1 (an empty job has one range)
   */
  virtual size_t Begin(PackJob* job, size_t range_blocks, bool* fits) = 0;
  /*!
   * \brief do range r of a phase
   * \param scratch this thread's PackCodec::ScratchBytes bytes, 64-byte aligned
   * \return false: the job does not fit
   */
  virtual bool Run(int phase, size_t r, uint8_t* scratch) = 0;
  /*!
   * \brief end a phase
   * \param packed set when 0 is returned: the job's result fields are written
   *  and it is packed (false: rejected)
   * \return ranges of the next phase; 0: the job is done
   */
  virtual size_t Finish(int phase, bool* packed) = 0;
};

class PackCodec {
 public:
  virtual ~PackCodec() = default;
  /*! \brief prepare a job as it is queued: on the consumer's thread, outside
   *  the pool's lock */
  virtual void Prepare(PackJob*) const {}
  /*! \brief bytes of scratch a pool thread needs for its ranges */
  virtual size_t ScratchBytes(size_t /*range_blocks*/) const { return 0; }
  virtual std::unique_ptr<PackJobState> NewState() const = 0;
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_PACK_CODEC_H_
