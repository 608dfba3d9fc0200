/*!
 * \file src/gpu/forest_kernels.hip
 * \brief GB6 / GB6m: fused inference of a packed forest on the row-major CSR --
 *  every tree, every level, the margin sum or the leaf ids in one launch,
 *  without a transpose and without bins.
 *
 *  GB6 k_forest_predict  one wave per row, one lane per tree, 64 trees per
 *                        pass, all 64 walking level-synchronously over the
 *                        row's (id, value) pairs staged in the wave's LDS slice.
 *  GB6m the same, <.., kVector>: leaves of K values, margins [rows, K]; after a
 *                        pass the lanes regroup as (tree, output) to sum.
 *
 *  The forest (ops.pack_forest) is int32 [T, size, 2] in heap layout, 8 bytes a
 *  node: word 0 = feature | default_left << 31 (-1: a leaf), word 1 = the bits
 *  of the float threshold (+inf for a feature's last bin) or of the leaf value.
 *  x <= threshold is GB2's bin <= split bin, so the walk ends where GB5's does.
 *
 *  Work split.  A 256-thread workgroup is four waves that stride over the rows
 *  independently (there is no workgroup barrier).  A wave stages its row once,
 *  by coalesced loads, as (u32 key, f32 bits) pairs: 8 bytes an entry,
 *  kForestRowEntries of them, 8 KiB per wave and 32 KiB per workgroup.  The key
 *  is the id, or for a 64-bit id >= 2^31 a word no feature (< 2^28) equals; an
 *  id forms no address, so one that is no split feature just matches nothing.
 *
 *  Level step.  Every lane loads its node with one 8-byte load, then the wave
 *  loops over the staged entries: all lanes read the same LDS address (a
 *  broadcast, no bank conflicts), compare the key with their own split feature
 *  and keep the value on a match.  Found: 2i + 1 when x <= thr, else 2i + 2 (a
 *  NaN compares false and goes right); not found: the default side; a lane on a
 *  leaf stays, and a level no lane can move on ends the pass.  ceil(T / 64) *
 *  depth * len broadcast reads per row, the row's global memory read once.
 *
 *  Long rows.  A row of more than kForestRowEntries entries is staged chunk by
 *  chunk at every level, the match carried across chunks: any length is
 *  correct, and only such rows pay the re-reads (and one more read of their
 *  values for the NaN check, which must not depend on what the trees walk).
 *
 *  Build.  This file is compiled with the target feature packed-fp32-ops
 *  turned off (Makefile, CMakeLists.txt): the margins must be the bytes of the
 *  level-by-level path, a chain of single f32 adds, and the compiler is kept
 *  from ever selecting v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 here.  With
 *  ROCm's present compiler neither build contains a packed op; the flag also
 *  changes how the staging loop is unrolled.  The recorded figures
 *  (profiles/gbdt/README.md) are of the build with the flag.
 *
 *  Margins.  The wave adds lane 0's, lane 1's, ... leaf value to one
 *  wave-uniform f32 accumulator that lives across passes: ((0 + leaf_0) +
 *  leaf_1) + ..., the order of the level-by-level path.  No atomics, one owner
 *  per row: the same inputs give the same bytes.  Leaf ids are written by the
 *  lanes at leaf[r, pass * 64 + lane].
 *
 *  GB6m: vector leaves (ForestView::outputs = K in 1 .. kGbdtMaxOutputs).  The
 *  same kernel with kVector set: the walk above is shared line for line, word 1
 *  of a leaf is unused, and the leaves' K values lie in a f32 table leaf_value
 *  [T, size, K].  margin[r, k] = ((0 + leaf_value[0, i_0, k]) + leaf_value[1,
 *  i_1, k]) + ... for every k, the level-by-level path's order again.  After a
 *  pass lane l holds the end node i_l of tree t0 + l, and the wave turns from
 *  one lane per tree to one lane per (tree, output): with Kp = the power of two
 *  >= K and G = 64 / Kp, lane = g * Kp + k.  A step takes G consecutive trees:
 *  lane (g, k) fetches the end node of tree u = step * G + g from lane u (one
 *  ds_bpermute) and loads leaf_value[((t0 + u) * size + i_u) * K + k] -- a
 *  tree's K floats are one segment, one wave instruction reads G segments --
 *  and then the G values of output k are added in tree order, acc += the value
 *  of lane g' * Kp + k for g' = 0 .. G - 1 (a bpermute each), so every lane of
 *  one k carries the same accumulator across steps and passes.  Trees past the
 *  pass's last and lanes with k >= K form no address and add nothing.  The
 *  loads of kVecSteps successive steps are issued before the first ordered add
 *  of the block: the adds are a dependent chain, the loads are not.  Per pass:
 *  ceil(here / G) loads and bpermutes and `here` bpermute + add pairs, where
 *  the scalar kernel has `here` readlane + add pairs.  Lanes 0 .. K - 1 store
 *  the row's K margins as one segment.  Kp is a runtime shift (no template per
 *  Kp: the sum is a small part of a row's time, and the flag already doubles
 *  the file's instantiations from four to eight); no LDS beyond the row slice.
 */
#include <dmlc/gpu/hip_utils.h>
#include <dmlc/logging.h>
#include <hip/hip_runtime.h>

#include "./device_common.h"
#include "./kernels.h"
#include "./launch_common.h"

namespace dmlc {
namespace gpu {

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / dev::kWave;
constexpr uint32_t kCap = kForestRowEntries;
/*! \brief staged key of an id that cannot be a split feature */
constexpr uint32_t kNoFeature = 0xFFFFFFFFu;
/*! \brief the staged entries are padded with kNoFeature keys to a multiple of this many, the
 *  step of the scan: its LDS reads issue together and it has no tail */
constexpr uint32_t kStep = 16;
static_assert(kCap % kStep == 0, "a full slice needs no padding");
/*! \brief GB6m: steps of the vector sum whose leaf loads are in flight before the ordered adds */
constexpr uint32_t kVecSteps = 4;
static_assert(kForestTreesPerPass == dev::kWave, "one lane per tree of a pass");

/*! \brief one thread ORs the wave's error into the status word (not an output) */
__device__ __forceinline__ void report(bool bad, uint32_t bit, uint32_t* error) {
  const uint64_t m = __ballot(bad);
  if (m != 0 && dev::lane_id() == __builtin_ctzll(m)) atomicOr(error, bit);
}

/*! \brief the row's entry arrays */
template <typename IndexType, bool kHasValue>
struct RowEntries {
  const IndexType* __restrict__ index;
  const float* __restrict__ value;
  /*! \brief entry j as a staged pair; a 64-bit id that does not fit 31 bits is no feature */
  __device__ __forceinline__ uint2 Load(uint64_t j) const {
    const IndexType id = index[j];
    uint32_t key = static_cast<uint32_t>(id);
    if (sizeof(IndexType) == 8 && static_cast<uint64_t>(id) > 0x7FFFFFFFull) key = kNoFeature;
    return make_uint2(key, __float_as_uint(kHasValue ? value[j] : 1.0f));
  }
};

/*!
 * \brief entries [first, first + count) of the row into the wave's slice, count
 *  <= kCap, padded to a multiple of kStep; fenced on both sides, so it may
 *  overwrite what the wave just read.  Returns whether this lane staged a NaN.
 */
template <typename Entries>
__device__ __forceinline__ bool stage(const Entries& src, uint64_t first, uint32_t count,
                                      uint2* s_row) {
  bool bad = false;
  dev::wave_sync();
  for (uint32_t j = dev::lane_id(); j < count; j += dev::kWave) {
    const uint2 p = src.Load(first + j);
    const float x = __uint_as_float(p.y);
    bad |= x != x;
    s_row[j] = p;
  }
  const uint32_t pad = count + dev::lane_id();  // kStep <= the wave: one store covers the padding
  if (pad < ((count + kStep - 1) & ~(kStep - 1))) s_row[pad] = make_uint2(kNoFeature, 0u);
  dev::wave_sync();
  return bad;
}

/*! \brief the lane's feature among the count staged entries (and their padding): its value
 *  replaces *x */
__device__ __forceinline__ void scan(const uint2* s_row, uint32_t count, uint32_t feature,
                                     bool* found, uint32_t* x) {
  bool f = *found;
  uint32_t v = *x;
  for (uint32_t k = 0; k < count; k += kStep) {
#pragma unroll
    for (uint32_t u = 0; u < kStep; ++u) {
      const uint2 p = s_row[k + u];  // one address for the wave: an LDS broadcast
      const bool hit = p.x == feature;
      f |= hit;  // selects, not branches: the reads of a step issue together
      v = hit ? p.y : v;
    }
  }
  *found = f;
  *x = v;
}

/*! \brief GB6m: the leaf table and how the wave's lanes regroup to sum it: lane = g * Kp + k,
 *  Kp = 1 << kp_log >= outputs; unused by GB6 */
struct LeafTable {
  const float* __restrict__ value;  // [trees x size x outputs]
  uint32_t outputs, kp_log;
};

/*!
 * \brief GB6m's sum of one pass: acc += leaf_value[t0 + u, i_u, k] for u = 0 .. here - 1 in
 *  that order, i_u = lane u's `i`; acc is the same in every lane of one k (k = lane % Kp < K).
 *  Called by the whole wave; i < size and t0 + u < trees, so every address is in the table.
 */
__device__ __forceinline__ float add_leaf_vectors(const LeafTable& table, uint32_t t0,
                                                  uint32_t here, uint32_t size, uint32_t i,
                                                  float acc) {
  const uint32_t lane = dev::lane_id();
  const uint32_t k = lane & ((1u << table.kp_log) - 1u), g = lane >> table.kp_log;
  const uint32_t group = static_cast<uint32_t>(dev::kWave) >> table.kp_log;  // G trees a step
  const bool mine = k < table.outputs;
  for (uint32_t u0 = 0; u0 < here; u0 += kVecSteps * group) {
    float v[kVecSteps];
#pragma unroll
    for (uint32_t j = 0; j < kVecSteps; ++j) {  // independent loads, all issued before the adds
      const uint32_t u = u0 + j * group + g;    // a lane index once it is < here <= 64
      v[j] = 0.0f;
      if (u0 + j * group >= here) continue;  // wave-uniform: no tree left for this step
      const uint32_t id = static_cast<uint32_t>(
          __shfl(static_cast<int>(i), static_cast<int>(u & (dev::kWave - 1)), dev::kWave));
      if (mine && u < here) {
        v[j] = table.value[(static_cast<size_t>(t0 + u) * size + id) * table.outputs + k];
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < kVecSteps; ++j) {
      const uint32_t first = u0 + j * group;  // wave-uniform, as is the trip count below
      const uint32_t count = first < here ? (here - first < group ? here - first : group) : 0;
      for (uint32_t gg = 0; gg < count; ++gg) {
        const float x = __shfl(v[j], static_cast<int>((gg << table.kp_log) + k), dev::kWave);
        if (mine) acc += x;
      }
    }
  }
  return acc;
}

template <typename IndexType, bool kHasValue, bool kVector>
__global__ __launch_bounds__(kThreads) void k_forest_predict(
    const uint64_t* __restrict__ offset, const RowEntries<IndexType, kHasValue> src, size_t nrows,
    const int2* __restrict__ node, uint32_t trees, uint32_t size, uint32_t depth,
    const LeafTable table, float* __restrict__ margin, int32_t* __restrict__ leaf,
    uint32_t* error) {
  __shared__ __attribute__((aligned(16))) uint2 s_lds[kWaves][kCap];
  const uint32_t lane = dev::lane_id();
  const uint32_t wave = threadIdx.x / dev::kWave;
  uint2* const s_row = s_lds[wave];
  bool bad = false;
  const size_t stride = static_cast<size_t>(gridDim.x) * kWaves;
  for (size_t r = static_cast<size_t>(blockIdx.x) * kWaves + wave; r < nrows; r += stride) {
    const uint64_t b = dev::uniform(offset[r]), e = dev::uniform(offset[r + 1]);
    const uint64_t n = e > b ? e - b : 0;
    const bool staged = n <= kCap;
    if (staged) {
      bad |= stage(src, b, static_cast<uint32_t>(n), s_row);
    } else if (kHasValue) {
      // a long row is staged only at the levels some tree walks (a forest of bare leaves: at
      // none), so its values are checked here, as a short row's are whatever the trees hold
      for (uint64_t j = lane; j < n; j += dev::kWave) {
        const float x = src.value[b + j];
        bad |= x != x;
      }
    }
    float acc = 0.0f;
    for (uint32_t t0 = 0; t0 < trees; t0 += dev::kWave) {
      const uint32_t t = t0 + lane;
      const bool live = t < trees;
      const int2* const tree = node + static_cast<size_t>(live ? t : 0) * size;
      uint32_t i = 0;  // at level l: i < 2^(l + 1) - 1 <= size, whatever the nodes hold
      int2 nd;
      for (uint32_t level = 0;; ++level) {
        nd = tree[i];
        const bool inner = live && nd.x != -1;
        if (level == depth || __ballot(inner) == 0) break;
        const uint32_t feature = static_cast<uint32_t>(nd.x) & 0x7FFFFFFFu;
        bool found = false;
        uint32_t xbits = 0;
        if (staged) {
          scan(s_row, static_cast<uint32_t>(n), feature, &found, &xbits);
        } else {
          for (uint64_t c = 0; c < n; c += kCap) {
            const uint32_t count = static_cast<uint32_t>(n - c < kCap ? n - c : kCap);
            bad |= stage(src, b + c, count, s_row);
            scan(s_row, count, feature, &found, &xbits);
          }
        }
        const bool go_left = found ? __uint_as_float(xbits) <= __int_as_float(nd.y) : nd.x < 0;
        if (inner) i = 2 * i + (go_left ? 1 : 2);
      }
      if (leaf != nullptr && live) leaf[r * trees + t] = static_cast<int32_t>(i);
      if (margin != nullptr) {
        const uint32_t here = trees - t0 < dev::kWave ? trees - t0 : dev::kWave;
        if (kVector) {
          acc = add_leaf_vectors(table, t0, here, size, i, acc);
        } else {
          for (uint32_t l = 0; l < here; ++l) {
            acc += __int_as_float(__builtin_amdgcn_readlane(nd.y, static_cast<int>(l)));
          }
        }
      }
    }
    if (kVector) {  // lanes 0 .. K - 1 are (g = 0, k = lane): one segment a row
      if (margin != nullptr && lane < table.outputs) margin[r * table.outputs + lane] = acc;
    } else if (margin != nullptr && lane == 0) {
      margin[r] = acc;
    }
  }
  report(bad, kGbdtErrNaN, error);
}
}  // namespace

void LaunchForestPredict(const CsrView& csr, const ForestView& forest, float* margin, int32_t* leaf,
                         uint32_t* error, hipStream_t stream) {
  CheckView("forest predict", csr, false);
  CHECK(forest.depth >= 1 && forest.depth <= 14 && forest.size == (2u << forest.depth) - 1u)
      << "forest predict: size must be 2^(depth + 1) - 1 with depth in [1, 14]";
  CHECK(margin != nullptr || leaf != nullptr) << "forest predict: no output";
  CHECK(error != nullptr) << "forest predict: no error word";
  const bool vector = forest.outputs != kGbdtScalar;
  if (vector) {
    CHECK(forest.outputs <= kGbdtMaxOutputs)
        << "forest predict: " << forest.outputs << " outputs, at most " << kGbdtMaxOutputs;
    CHECK(margin == nullptr || forest.leaf_value != nullptr || forest.trees == 0)
        << "forest predict: margins of vector leaves need leaf_value";
    CHECK_EQ((reinterpret_cast<uintptr_t>(forest.leaf_value) |
              reinterpret_cast<uintptr_t>(margin)) & 3u, 0u)
        << "forest predict: leaf_value / margin not 4-byte aligned";
  }
  if (csr.nrows == 0 || forest.trees == 0) return;
  CHECK(forest.node != nullptr) << "forest predict: no nodes";
  CHECK_EQ(reinterpret_cast<uintptr_t>(forest.node) & 7u, 0u)
      << "forest predict: nodes not 8-byte aligned";
  LeafTable table{forest.leaf_value, forest.outputs, 0};
  while (vector && (1u << table.kp_log) < forest.outputs) ++table.kp_log;
  const dim3 grid(GridFor(csr.nrows, kWaves));
  DispatchIndexValue(csr, [&](auto tag, auto has_value) {
    using IndexType = decltype(tag);
    constexpr bool kHasValue = decltype(has_value)::value;
    const RowEntries<IndexType, kHasValue> src{IndexOf<IndexType>(csr), csr.value};
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, csr.offset, src, csr.nrows,
                         reinterpret_cast<const int2*>(forest.node), forest.trees, forest.size,
                         forest.depth, table, margin, leaf, error);
    };
    if (vector) {
      launch(k_forest_predict<IndexType, kHasValue, true>);
    } else {
      launch(k_forest_predict<IndexType, kHasValue, false>);
    }
  });
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
