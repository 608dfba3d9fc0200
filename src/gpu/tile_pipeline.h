/*!
 * \file src/gpu/tile_pipeline.h
 * \brief Host driver state shared by the tile pipelines (device_parser.cc,
 *  device_recordio.cc): the count + scan scratch set, the second set a next
 *  chunk's count + scan is prelaunched into, the one-pass ticket counter.
 */
#ifndef DMLC_SRC_GPU_TILE_PIPELINE_H_
#define DMLC_SRC_GPU_TILE_PIPELINE_H_

#include <dmlc/gpu/hip_utils.h>

#include <cstring>
#include <memory>

#include "./kernels.h"

namespace dmlc {
namespace gpu {

/*! \brief what a chunk's count + scan writes: per-tile counts (scanned in
 *  place), flags and start masks (text only), the chunk's ChunkMeta on the
 *  device and in mapped pinned memory (polled by TakePublished, host_wait.h) */
struct TileScratchSet {
  DeviceBuffer counts, flags, masks, meta;
  PinnedBuffer hmap;

  void Init(size_t meta_bytes) {
    meta.Reserve(meta_bytes);
    hmap.Reserve(sizeof(ChunkMeta), /*mapped=*/true);
    std::memset(hmap.get(), 0, sizeof(ChunkMeta));  // its pad word is the flag
  }
  void Reserve(size_t ntiles, bool with_masks) {
    counts.Reserve(TileScratchWords(ntiles) * sizeof(uint64_t));
    flags.Reserve(TileScratchWords(ntiles) * sizeof(uint32_t));
    if (with_masks) masks.Reserve(TileMaskWords(ntiles) * sizeof(uint32_t));
  }
  void swap(TileScratchSet& o) noexcept {
    counts.swap(o.counts);
    flags.swap(o.flags);
    masks.swap(o.masks);
    meta.swap(o.meta);
    hmap.swap(o.hmap);
  }
  ChunkMeta* dmeta() const { return meta.get<ChunkMeta>(); }
  ChunkMeta* hmeta() const { return hmap.get<ChunkMeta>(); }
};

/*!
 * \brief the current scratch set and, with_next, a second one with its own
 *  stream (default priority): the next resident chunk's count + scan runs in
 *  it beside the current fill and is adopted when that chunk's turn comes.
 *  When to prelaunch, and what, is the owner's policy.
 */
struct CountPrelaunch {
  TileScratchSet cur, next;
  std::unique_ptr<Stream> stream;  // null without a second set
  std::unique_ptr<Event> done;
  bool valid{false};  // next holds the count + scan of (ptr, bytes)
  const void* ptr{nullptr};
  size_t bytes{0};

  void Init(size_t meta_bytes, bool with_next) {
    cur.Init(meta_bytes);
    if (!with_next) return;
    stream.reset(new Stream());
    done.reset(new Event());
    next.Init(meta_bytes);
  }
  /*! \brief if (p, n) is the prelaunched chunk: its set becomes the current
   *  one (its sizes are published, or about to be, in cur.hmap) and `compute`
   *  waits for the scan that wrote the tile prefix */
  bool Adopt(const void* p, size_t n, hipStream_t compute) {
    if (!(valid && ptr == p && bytes == n)) return false;
    cur.swap(next);
    valid = false;
    DMLC_HIP_CHECK(hipStreamWaitEvent(compute, done->get(), 0));
    return true;
  }
  /*! \brief fn(set, stream) launches the count + scan of (p, n) into the
   *  second set, last used by the chunk before the current one (done) */
  template <typename Fn>
  void Launch(const void* p, size_t n, size_t ntiles, bool with_masks, Fn&& fn) {
    next.Reserve(ntiles, with_masks);
    fn(next, stream->get());
    done->Record(stream->get());
    valid = true;
    ptr = p;
    bytes = n;
  }
  /*! \brief retire a prelaunched count nobody will adopt (its flag re-armed) */
  void Drop() {
    if (!valid) return;
    stream->Synchronize();
    next.hmeta()->pad = 0;
    valid = false;
  }
};

/*! \brief the one-pass kernels' workgroup ticket counter (zeroed at first
 *  use) and its value before the next launch */
struct OnePassTickets {
  DeviceBuffer counter;
  unsigned long long ticket0{0};

  void Ensure(hipStream_t s) {
    if (counter.bytes() != 0) return;
    counter.Reserve(sizeof(unsigned long long));
    DMLC_HIP_CHECK(hipMemsetAsync(counter.get(), 0, counter.bytes(), s));
    ticket0 = 0;
  }
  /*! \brief the next launch's look-back state over `status` */
  LookBack For(uint64_t* status) const {
    return LookBack{status, counter.get<unsigned long long>(), ticket0};
  }
  /*! \brief a launch took `groups` tickets (the launcher's return value) */
  void Advance(size_t groups) { ticket0 += groups; }
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_TILE_PIPELINE_H_
