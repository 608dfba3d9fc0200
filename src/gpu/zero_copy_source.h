/*!
 * \file src/gpu/zero_copy_source.h
 * \brief Zero-copy chunk source for the GPU pipelines: the partition's file
 *  ranges are mmap'ed and registered with hipHostRegister(ReadOnly), so every
 *  H2D DMA reads the page cache directly -- no CPU memcpy into pinned slots
 *  (measured: 87.0M rows/s vs 55.3M with the pread ring, profiles/r01_zero_copy).
 *
 * The partition is mapped and registered in windows of `window_bytes`; the
 * next window is prepared (mmap + MAP_POPULATE + hipHostRegister) on a
 * background thread while the current one is consumed, and the first window
 * of a pass is small (4 chunks), so the first chunk's DMA starts after one
 * small registration instead of after the whole shard was read and pinned.
 * Two modes:
 *  - retained: a partition of at most `pin_budget` bytes keeps every window
 *    pinned once registered (registration is paid once per parser, not per
 *    epoch; later epochs find every window mapped);
 *  - windowed: larger partitions (a 288 GB shard per GPU) keep at most two
 *    windows pinned (plus the one being prefetched).  A window is released
 *    only after the owner's drain callback (the copy stream's
 *    synchronisation) has run, so no DMA still reads it.
 * `pin_budget` is per process; ShardPinBudget() divides the configured budget
 * among the ranks of a host and bounds it by the host's available memory.
 *
 * Chunks never cross a file boundary and end on a record boundary (a record
 * longer than chunk_bytes makes its chunk longer):
 *  - text: after the last EOL of the window (reference LineSplitter,
 *    `src/io/line_split.cc:27-34`);
 *  - RecordIO: at the last aligned record head (magic word followed by an lrec
 *    with cflag 0 or 1) of the window (reference RecordIOSplitter,
 *    `src/io/recordio_split.cc:26-42`), so a multi-part record is never split.
 */
#ifndef DMLC_SRC_GPU_ZERO_COPY_SOURCE_H_
#define DMLC_SRC_GPU_ZERO_COPY_SOURCE_H_

#include <dmlc/gpu/hip_utils.h>
#include <dmlc/logging.h>
#include <dmlc/recordio.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <vector>

#include "../io/filesys.h"
#include "../io/input_split_base.h"

namespace dmlc {
namespace gpu {

class ZeroCopySource {
 public:
  enum class Cut { kLine, kRecordIO };
  struct Piece {
    const char* ptr;
    size_t size;
  };
  explicit ZeroCopySource(Cut cut = Cut::kLine) : cut_(cut) {}
  ~ZeroCopySource() {
    JoinPending();
    for (auto& w : windows_) Unmap(&w);
    windows_.clear();
    for (int fd : fds_) {
      if (fd >= 0) ::close(fd);
    }
  }
  ZeroCopySource(const ZeroCopySource&) = delete;
  ZeroCopySource& operator=(const ZeroCopySource&) = delete;

  /*!
   * \brief prepare the partition; false (nothing left mapped) when it cannot be
   *  mmap'ed + registered
   * \param pin_budget partitions up to this size keep every window pinned (retained)
   * \param window_bytes window size of the windowed mode
   */
  bool Init(io::InputSplitBase* split, size_t chunk_bytes, size_t pin_budget = 64UL << 30,
            size_t window_bytes = 1UL << 30,
            const std::vector<io::InputSplitBase::Segment>* segments = nullptr) {
    chunk_bytes_ = chunk_bytes;
    page_ = static_cast<size_t>(sysconf(_SC_PAGESIZE));
    window_bytes_ = std::max(window_bytes, 2 * chunk_bytes);
    // explicit segments: the shuffled mode's sub-shards (Reorder permutes them)
    const std::vector<io::InputSplitBase::Segment> own =
        segments != nullptr ? *segments : split->ShardSegments();
    for (size_t i = 0; i < own.size(); ++i) {
      const auto& seg = own[i];
      if (seg.end <= seg.begin) continue;
      const int fd = split->filesystem()->OpenRawFd(split->files()[seg.file_index].path);
      if (fd < 0) return Fail();
      fds_.push_back(fd);
      segs_.push_back(Seg{fds_.size() - 1, seg.begin, seg.end - seg.begin, i});
    }
    windowed_ = PartitionBytes() > pin_budget;
    // probe once: a file that cannot be mapped + registered fails here
    if (!segs_.empty()) {
      Mapping probe;
      if (!MapRange(segs_[0], 0, std::min(segs_[0].size, page_), &probe)) return Fail();
      Unmap(&probe);
    }
    all_ = segs_;
    return true;
  }
  /*!
   * \brief visit the Init segments in a new order: `order[i]` = index (in the
   *  Init list) of the i-th segment to visit.  Eager mappings are kept;
   *  windows are released (after the drain callback).  Rewinds to the start.
   */
  void Reorder(const std::vector<size_t>& order) {
    if (all_.empty() && !segs_.empty()) all_ = segs_;
    Rewind();
    std::vector<Seg> next;
    for (size_t want : order) {
      for (const Seg& s : all_) {
        if (s.init_index == want) next.push_back(s);
      }
    }
    segs_ = next;
    seg_ = 0;
    off_ = 0;
  }
  /*!
   * \brief called before a window is released: must wait until no transfer
   *  reads pieces handed out earlier (the owner's copy-stream sync)
   */
  void SetDrain(std::function<void()> drain) { drain_ = std::move(drain); }
  /*!
   * \brief inside the drain callback: whether the piece at p lies in a mapping
   *  about to be released (an owner that holds pieces back, not yet submitted,
   *  must stop using exactly those)
   */
  bool Releasing(const char* p) const {
    return release_all_ || (p >= release_begin_ && p < release_end_);
  }
  bool windowed() const { return windowed_; }
  void Reset() { Seek(0); }
  /*! \brief next chunk of whole records; false at the end */
  bool Next(Piece* out) {
    while (seg_ < segs_.size() && off_ >= segs_[seg_].size) {
      ++seg_;
      off_ = 0;
    }
    if (seg_ >= segs_.size()) return false;
    const Seg& s = segs_[seg_];
    const size_t remain = s.size - off_;
    size_t want = std::min(chunk_bytes_, remain);
    for (;;) {
      const Mapping* w = Window(s.init_index, off_, want);
      const char* b = w->data + (off_ - w->seg_off);
      const size_t avail = w->seg_off + w->len - off_;  // bytes of the segment visible from b
      size_t len = want;
      if (off_ + len < s.size) {
        len = cut_ == Cut::kLine ? CutLine(b, len, avail) : CutRecord(b, len, avail);
        if (len == avail && off_ + avail < s.size) {
          // one record runs past the mapped window: map a larger one
          want = std::min(remain, 2 * avail);
          continue;
        }
      }
      out->ptr = b;
      out->size = len;
      off_ += len;
      return true;
    }
  }
  /*!
   * \brief partition byte offset of the next piece (same cursor space as
   *  io::ShardReader::Tell: file bytes only, always a record boundary)
   */
  size_t Tell() const {
    size_t n = 0;
    for (size_t i = 0; i < seg_ && i < segs_.size(); ++i) n += segs_[i].size;
    return n + off_;
  }
  /*! \brief continue from a Tell() cursor */
  void Seek(size_t pos) {
    Rewind();
    seg_ = 0;
    off_ = pos;
    while (seg_ < segs_.size() && off_ >= segs_[seg_].size) {
      off_ -= segs_[seg_].size;
      ++seg_;
    }
    CHECK(seg_ < segs_.size() || off_ == 0) << "cursor beyond the partition";
  }
  size_t PartitionBytes() const {
    size_t n = 0;
    for (const auto& s : segs_) n += s.size;
    return n;
  }
  /*! \brief bytes currently registered with HIP (for stats and tests) */
  size_t PinnedBytes() const {
    std::lock_guard<std::mutex> lk(pinned_mu_);
    return pinned_;
  }
  /*! \brief the most bytes registered at once so far */
  size_t PeakPinnedBytes() const {
    std::lock_guard<std::mutex> lk(pinned_mu_);
    return peak_pinned_;
  }
  /*!
   * \brief the zero-copy pin budget of one process: the configured per-host
   *  budget divided among the ranks on this host (DMLC_LOCAL_WORLD_SIZE from
   *  the dmlc launchers, LOCAL_WORLD_SIZE from torchrun) and bounded by half
   *  of the host's MemAvailable shared the same way -- 8 ranks must not lock
   *  8 x the budget, nor more memory than the host has free.
   */
  static size_t ShardPinBudget(size_t configured) {
    size_t local = 1;
    for (const char* k : {"DMLC_LOCAL_WORLD_SIZE", "LOCAL_WORLD_SIZE"}) {
      const char* v = std::getenv(k);
      if (v != nullptr && std::atoi(v) > 0) {
        local = static_cast<size_t>(std::atoi(v));
        break;
      }
    }
    size_t budget = configured / local;
    const size_t avail = MemAvailableBytes();
    if (avail != 0) budget = std::min(budget, avail / 2 / local);
    return budget;
  }
  /*! \brief MemAvailable of /proc/meminfo (0 when unknown) */
  static size_t MemAvailableBytes() {
    std::FILE* f = std::fopen("/proc/meminfo", "r");
    if (f == nullptr) return 0;
    char line[256];
    size_t kb = 0;
    while (std::fgets(line, sizeof(line), f) != nullptr) {
      if (std::sscanf(line, "MemAvailable: %zu kB", &kb) == 1) break;
    }
    std::fclose(f);
    return kb * 1024;
  }

 private:
  struct Seg {
    size_t fd_index;
    size_t file_begin;  // first byte of the segment in its file
    size_t size;
    size_t init_index;  // position in the Init segment list (window key)
  };
  struct Mapping {
    void* map{nullptr};
    size_t map_len{0};
    const char* data{nullptr};  // segment byte seg_off
    size_t seg_index{0}, seg_off{0}, len{0};
    bool registered{false};
  };

  bool MapRange(const Seg& s, size_t seg_off, size_t len, Mapping* m) {
    const size_t file_off = s.file_begin + seg_off;
    const size_t map_off = file_off & ~(page_ - 1);
    m->map_len = file_off + len - map_off;
    m->map = mmap(nullptr, m->map_len, PROT_READ, MAP_SHARED | MAP_POPULATE, fds_[s.fd_index],
                  static_cast<off_t>(map_off));
    if (m->map == MAP_FAILED) {
      m->map = nullptr;
      return false;
    }
    if (hipHostRegister(m->map, m->map_len, hipHostRegisterReadOnly) != hipSuccess) {
      (void)hipGetLastError();
      munmap(m->map, m->map_len);
      m->map = nullptr;
      return false;
    }
    m->registered = true;
    {
      std::lock_guard<std::mutex> lk(pinned_mu_);
      pinned_ += m->map_len;
      peak_pinned_ = std::max(peak_pinned_, pinned_);
    }
    m->data = static_cast<const char*>(m->map) + (file_off - map_off);
    m->seg_off = seg_off;
    m->len = len;
    return true;
  }
  void Unmap(Mapping* m) {
    if (m->map == nullptr) return;
    if (m->registered) {
      (void)hipHostUnregister(m->map);
      std::lock_guard<std::mutex> lk(pinned_mu_);
      pinned_ -= m->map_len;
    }
    munmap(m->map, m->map_len);
    m->map = nullptr;
  }
  /*! \brief finish the background registration; retained mode keeps its window */
  void JoinPending() {
    if (!pending_.valid()) return;
    Mapping m = pending_.get();
    if (!windowed_ && m.map != nullptr) {
      windows_.push_back(m);
    } else {
      Unmap(&m);
    }
  }
  /*! \brief a new pass (Seek / Reorder): windowed mode releases its windows
   *  (after the drain), retained mode keeps them */
  void Rewind() {
    JoinPending();
    if (!windowed_) return;
    if (!windows_.empty() && drain_) {
      release_all_ = true;
      drain_();
      release_all_ = false;
    }
    for (auto& w : windows_) Unmap(&w);
    windows_.clear();
  }
  /*! \brief the Init-list segment with key si */
  const Seg& SegByKey(size_t si) const {
    for (const Seg& s : all_) {
      if (s.init_index == si) return s;
    }
    LOG(FATAL) << "zero-copy: no segment " << si;
    return all_[0];
  }
  /*! \brief the window of segment si (Init index) holding [off, off + want),
   *  mapped on demand */
  const Mapping* Window(size_t si, size_t off, size_t want) {
    for (const auto& w : windows_) {
      if (w.seg_index == si && off >= w.seg_off && off + want <= w.seg_off + w.len) return &w;
    }
    const Seg& s = SegByKey(si);
    Mapping m;
    bool have = false;
    if (pending_.valid()) {
      Mapping p = pending_.get();  // prefetched by the background thread
      if (p.map != nullptr && p.seg_index == si && off >= p.seg_off &&
          off + want <= p.seg_off + p.len) {
        m = p;
        have = true;
      } else if (!windowed_ && p.map != nullptr) {
        windows_.push_back(p);  // retained: another part of the shard, kept
        for (const auto& w : windows_) {
          if (w.seg_index == si && off >= w.seg_off && off + want <= w.seg_off + w.len) return &w;
        }
      } else {
        Unmap(&p);
      }
    }
    if (!have) {
      // mapped synchronously (the pass's first window, or a record longer
      // than the window): small, so the pipeline starts after little I/O
      const size_t first = std::max(4 * chunk_bytes_, want);
      const size_t len = std::min(s.size - off, std::min(std::max(window_bytes_, want), first));
      CHECK(MapRange(s, off, len, &m)) << "zero-copy: cannot map + register a window";
      m.seg_index = si;
    }
    // windowed: at most two windows pinned, the oldest released once its DMAs are done
    if (windowed_ && windows_.size() >= 2) {
      if (drain_) {
        release_begin_ = static_cast<const char*>(windows_.front().map);
        release_end_ = release_begin_ + windows_.front().map_len;
        drain_();
        release_begin_ = release_end_ = nullptr;
      }
      Unmap(&windows_.front());
      windows_.pop_front();
    }
    windows_.push_back(m);
    // the next window overlaps this one by two chunks, so the piece that no
    // longer fits here starts inside the prefetched window
    const size_t overlap = std::min(m.len, 2 * chunk_bytes_);
    if (m.seg_off + m.len < s.size) Prefetch(si, m.seg_off + m.len - overlap);
    return &windows_.back();
  }
  /*! \brief map + register the window after this one on a background thread
   *  (nothing to do when a retained window already covers it) */
  void Prefetch(size_t si, size_t off) {
    const Seg& seg = SegByKey(si);
    if (off >= seg.size) return;
    const size_t len = std::min(seg.size - off, window_bytes_);
    for (const auto& w : windows_) {
      if (w.seg_index == si && off >= w.seg_off && off + 2 * chunk_bytes_ <= w.seg_off + w.len) {
        return;
      }
    }
    const Seg s = seg;
    pending_ = std::async(std::launch::async, [this, s, si, off, len]() {
      Mapping m;
      if (!MapRange(s, off, len, &m)) m.map = nullptr;
      m.seg_index = si;
      return m;
    });
  }
  size_t CutLine(const char* b, size_t len, size_t avail) const {
    size_t cut = len;
    while (cut > 0 && b[cut - 1] != '\n' && b[cut - 1] != '\r') --cut;
    if (cut != 0) return cut;
    // one line fills the window: extend to its end (up to what is mapped),
    // as the reference's InputSplitBase grows its buffer for long records
    // (src/io/input_split_base.cc:241-258)
    cut = len;
    while (cut < avail && b[cut] != '\n' && b[cut] != '\r') ++cut;
    while (cut < avail && (b[cut] == '\n' || b[cut] == '\r')) ++cut;
    return cut;
  }
  static bool IsHead(const uint32_t* w, size_t p) {
    return w[p] == RecordIOWriter::kMagic && RecordIOWriter::DecodeFlag(w[p + 1]) <= 1U;
  }
  /*! \brief last record head in the window; past it when one record fills it */
  size_t CutRecord(const char* b, size_t len, size_t avail) const {
    // segments start 4-byte aligned (RecordIO partitions align to 4 bytes)
    const uint32_t* w = reinterpret_cast<const uint32_t*>(b);
    const size_t nw = len / 4;
    for (size_t p = nw >= 2 ? nw - 2 : 0; p > 0; --p) {
      if (IsHead(w, p)) return p * 4;
    }
    const size_t aw = avail / 4;
    for (size_t p = nw > 1 ? nw - 1 : 1; p + 1 < aw; ++p) {
      if (IsHead(w, p)) return p * 4;
    }
    return avail;
  }
  bool Fail() {
    for (int fd : fds_) {
      if (fd >= 0) ::close(fd);
    }
    fds_.clear();
    segs_.clear();
    return false;
  }

  Cut cut_;
  size_t chunk_bytes_{0}, page_{4096}, window_bytes_{1UL << 30};
  bool windowed_{false};
  std::vector<int> fds_;
  std::vector<Seg> segs_;
  std::vector<Seg> all_;  // the Init list (Reorder's source)
  std::deque<Mapping> windows_;
  mutable std::mutex pinned_mu_;  // MapRange runs on the prefetch thread too
  size_t pinned_{0}, peak_pinned_{0};
  std::future<Mapping> pending_;
  std::function<void()> drain_;
  // the mapping the running drain callback precedes the release of
  const char* release_begin_{nullptr};
  const char* release_end_{nullptr};
  bool release_all_{false};
  size_t seg_{0}, off_{0};
};

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_ZERO_COPY_SOURCE_H_
