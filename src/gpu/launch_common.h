/*!
 * \file src/gpu/launch_common.h
 * \brief Host-side helpers the kernel launchers share: grid sizing, alignment,
 *  and the checks and index-width dispatch of a CsrView operand.
 */
#ifndef DMLC_GPU_LAUNCH_COMMON_H_
#define DMLC_GPU_LAUNCH_COMMON_H_

#include <dmlc/logging.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "./kernels.h"

namespace dmlc {
namespace gpu {

/*! \brief workgroups of a grid-stride launch over `work` items, per_block each: 1 .. 16384 */
inline int GridFor(size_t work, size_t per_block) {
  size_t blocks = (work + per_block - 1) / per_block;
  if (blocks == 0) blocks = 1;
  return static_cast<int>(blocks < 16384 ? blocks : 16384);
}

inline bool Aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int NextPow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

/*!
 * \brief what every op launcher checks of its operand, before any early
 *  return: a paired view is refused by an op without a pairs kernel
 *  (takes_pairs false) and must be what a pairs kernel reads, 8-byte aligned
 *  (u32 index, f32 value) pairs
 */
inline void CheckView(const char* op, const CsrView& csr, bool takes_pairs) {
  if (!csr.paired) return;
  CHECK(takes_pairs) << op << ": takes no interleaved (index, value) pairs";
  CHECK(!csr.index64) << op << ": pairs have 32-bit indices";
  CHECK(csr.value != nullptr &&
        csr.value == static_cast<const float*>(csr.index) + 1)
      << op << ": a pair's value is the float after its index";
  CHECK_EQ(reinterpret_cast<uintptr_t>(csr.index) & 7u, 0u) << op << ": pairs not 8-byte aligned";
}

template <typename IndexType>
inline const IndexType* IndexOf(const CsrView& csr) {
  return static_cast<const IndexType*>(csr.index);
}
template <typename IndexType>
inline const IndexType* FieldOf(const CsrView& csr) {
  return static_cast<const IndexType*>(csr.field);
}

/*! \brief f(IndexType{}) for the view's index width; read the arrays with IndexOf / FieldOf */
template <typename F>
inline void DispatchIndex(const CsrView& csr, F&& f) {
  if (csr.index64) {
    f(uint64_t{});
  } else {
    f(uint32_t{});
  }
}

/*! \brief f(IndexType{}, std::true_type / std::false_type{}): the index width and
 *  whether the view has values, for kernels with a compile-time no-value variant */
template <typename F>
inline void DispatchIndexValue(const CsrView& csr, F&& f) {
  DispatchIndex(csr, [&](auto tag) {
    if (csr.value != nullptr) {
      f(tag, std::true_type{});
    } else {
      f(tag, std::false_type{});
    }
  });
}

}  // namespace gpu
}  // namespace dmlc
#endif  // DMLC_GPU_LAUNCH_COMMON_H_
