/*!
 * \file src/gpu/pinned_file.h
 * \brief A byte range of a local file in page-locked host memory, so that an
 *  H2D DMA can read it in place.  Two ways to get there:
 *  - registered: the range is mmap'ed and the mapping registered with
 *    hipHostRegister(ReadOnly) -- the DMA reads the page cache, no host copy;
 *  - staged: where the runtime cannot register memory the process already
 *    has (hipHostRegister fails on some virtualised hosts), the range is read
 *    once into a hipHostMalloc allocation of the same layout.
 *  Either way the bytes of file offset `off` start at `map`, `off` is a
 *  multiple of the page size and so is the address, so a pointer into the
 *  range has the alignment its file offset has.
 */
#ifndef DMLC_SRC_GPU_PINNED_FILE_H_
#define DMLC_SRC_GPU_PINNED_FILE_H_

#include <dmlc/gpu/hip_utils.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstring>
#include <future>
#include <vector>

namespace dmlc {
namespace gpu {

struct PinnedFileRange {
  void* map{nullptr};
  size_t map_len{0};
  /*! \brief true: mmap + hipHostRegister; false: hipHostMalloc + read */
  bool registered{false};
};

/*! \brief pread until `len` bytes are there; false on an error or a short file */
inline bool PreadAll(int fd, char* dst, size_t len, size_t off) {
  while (len != 0) {
    const ssize_t n = pread(fd, dst, len, static_cast<off_t>(off));
    if (n < 0 && errno == EINTR) continue;
    if (n <= 0) return false;
    dst += n;
    off += static_cast<size_t>(n);
    len -= static_cast<size_t>(n);
  }
  return true;
}

/*! \brief PreadAll with the range split among threads: one thread copies out
 *  of the page cache, into pinned pages it touches for the first time, at a
 *  fraction of what the link takes.  Measured on the flagship shard (6.4 GB,
 *  1 GiB windows, first pass of a parser): 590 ms with 8 threads, 455 ms with
 *  16; every later pass finds the windows filled. */
inline bool PreadAllParallel(int fd, char* dst, size_t len, size_t off) {
  constexpr size_t kMinPart = size_t(8) << 20;
  constexpr size_t kMaxThreads = 16;
  const size_t parts = std::min(kMaxThreads, len / kMinPart);
  if (parts <= 1) return PreadAll(fd, dst, len, off);
  const size_t step = (len / parts + 4095) & ~size_t(4095);
  std::vector<std::future<bool>> jobs;
  for (size_t b = step; b < len; b += step) {
    const size_t n = std::min(step, len - b);
    jobs.push_back(std::async(std::launch::async,
                              [fd, dst, off, b, n]() { return PreadAll(fd, dst + b, n, off + b); }));
  }
  bool ok = PreadAll(fd, dst, std::min(step, len), off);
  for (auto& j : jobs) ok = j.get() && ok;
  return ok;
}

/*!
 * \brief page-lock bytes [off, off + len) of fd; `off` is page-aligned.
 *  Registration is tried first unless try_register is false (a caller that saw
 *  it fail once does not ask again for every window).  false: nothing is held.
 */
inline bool PinFileRange(int fd, size_t off, size_t len, bool try_register, PinnedFileRange* out) {
  *out = PinnedFileRange();
  if (try_register) {
    void* m = mmap(nullptr, len, PROT_READ, MAP_SHARED | MAP_POPULATE, fd, static_cast<off_t>(off));
    if (m == MAP_FAILED) return false;
    if (hipHostRegister(m, len, hipHostRegisterReadOnly) == hipSuccess) {
      out->map = m;
      out->map_len = len;
      out->registered = true;
      return true;
    }
    (void)hipGetLastError();  // the runtime keeps the failure for the next check
    munmap(m, len);
  }
  // whole pages, the rest of the last one zero as in a file mapping
  const size_t page = static_cast<size_t>(sysconf(_SC_PAGESIZE));
  const size_t alloc = (len + page - 1) & ~(page - 1);
  void* p = nullptr;
  if (hipHostMalloc(&p, alloc, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (!PreadAllParallel(fd, static_cast<char*>(p), len, off)) {
    (void)hipHostFree(p);
    return false;
  }
  std::memset(static_cast<char*>(p) + len, 0, alloc - len);
  out->map = p;
  out->map_len = len;
  return true;
}

/*! \brief release the range; no DMA may still read it */
inline void UnpinFileRange(PinnedFileRange* r) {
  if (r->map == nullptr) return;
  if (r->registered) {
    (void)hipHostUnregister(r->map);
    munmap(r->map, r->map_len);
  } else {
    (void)hipHostFree(r->map);
  }
  *r = PinnedFileRange();
}

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_SRC_GPU_PINNED_FILE_H_
