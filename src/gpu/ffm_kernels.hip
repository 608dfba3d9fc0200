/*!
 * \file src/gpu/ffm_kernels.hip
 * \brief FF1 / FF2: the pairwise term of a field-aware factorisation machine
 *  over a CSR with per-entry fields, and its gradient (f32).
 *
 * FF1  p[r] = sum_{a < b} x_a x_b sum_c V[i_a, f_b, c] V[i_b, f_a, c]   k_ffm_forward
 * FF2  dV[i_a, f_b, :] += g_r x_a x_b V[i_b, f_a, :], a != b (atomics)  k_ffm_backward
 *
 * V is [features x num_fields x k] row-major, k a multiple of 4 up to
 * kFFMMaxRank, so every V[i, f, :] slice starts on a 16-byte boundary of a
 * 16-byte aligned table.  An entry whose id is >= features or whose field is
 * >= num_fields is skipped: it is marked when it is read, takes part in no
 * pair, and no address is ever formed from it.  FF1 also reports it (error
 * word, kFFMErr*).  All address arithmetic is size_t.
 *
 * FF1.  A row belongs to a group of 32 lanes (8 rows per 256-thread
 * workgroup).  Its (id, field, value) triples are staged once in LDS when
 * there are at most kFFMStagedRowEntries of them; the group is split into
 * pair slots times column lanes (cpr = next_pow2(k / 4) lanes share one pair,
 * each reading one float4 of both slices), and the slots sweep the n (n - 1) / 2
 * pairs as {a, (a + d) mod n}, d = 1 .. n / 2, d fastest: a flat index space,
 * so a row of 39 entries keeps 96 % of its slots busy where a triangle swept
 * row by row keeps half.  Longer rows sweep the triangle and re-read
 * their entries from global memory.  Every lane sums its own pairs in sweep
 * order and the lanes are folded by __shfl_xor from the widest distance down:
 * no atomics, an order fixed by the row's length and k, the same bytes for the
 * same inputs.
 *
 * FF2.  One wave per row, a fixed per wave-instruction, the lanes over (b, c)
 * with c fastest: 64 / k entries b at a time.  With a row's entries in field
 * order (as LibFM writers emit them) the targets dV[i_a, f_b, c] of one
 * instruction are one contiguous stretch of the V[i_a, :, :] block -- 256
 * bytes for k = 4 .. 32 with one entry per field -- which is the shape the
 * memory-side f32 atomics run at full rate in (MI355X_MICROARCH.md, Global
 * float atomics); one pair per lane with a loop over c would put 64 lanes in
 * 64 rows.  Rows whose g is +-0 add nothing and are skipped.
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
constexpr int kGroup = 32;                           // FF1: lanes per row
constexpr int kGroupsPerBlock = kThreads / kGroup;   // FF1: rows per workgroup
constexpr int kWavesPerBlock = kThreads / dev::kWave;  // FF2: rows per workgroup
constexpr uint32_t kSkip = 0xFFFFFFFFu;              // field of an entry that is out of range
constexpr uint32_t kCap = kFFMStagedRowEntries;

/*! \brief the entry arrays and the table's extent; Load marks what is out of range */
template <typename IndexType, bool kHasValue>
struct FieldEntries {
  const IndexType* __restrict__ index;
  const IndexType* __restrict__ field;
  const float* __restrict__ value;
  uint64_t features;
  uint64_t num_fields;
  /*! \brief entry j; *f = kSkip if its id or field is out of range.  Returns kFFMErr* bits */
  __device__ __forceinline__ uint32_t Load(uint64_t j, IndexType* id, uint32_t* f, float* x) const {
    const IndexType i = index[j];
    const IndexType fl = field[j];
    const uint32_t err = (static_cast<uint64_t>(i) >= features ? kFFMErrIndex : 0u) |
                         (static_cast<uint64_t>(fl) >= num_fields ? kFFMErrField : 0u);
    *id = i;
    *f = err != 0u ? kSkip : static_cast<uint32_t>(fl);
    *x = kHasValue ? value[j] : 1.0f;
    return err;
  }
};

/*! \brief one row's staged entries */
template <typename IndexType>
struct StagedRow {
  IndexType id[kCap];
  uint32_t field[kCap];
  float x[kCap];
};

__device__ __forceinline__ float Dot(const float4& a, const float4& b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

/*!
 * \brief FF1.  units = k / 4; cpr = next_pow2(units) <= 8 lanes per pair.
 *  The row loop is uniform over the workgroup (a group past the last row runs
 *  an empty row), so every lane takes part in every fold.  A group's LDS image
 *  is written and read by lanes of one wave: dev::wave_sync orders them.
 */
template <typename IndexType, bool kHasValue>
__global__ __launch_bounds__(kThreads) void k_ffm_forward(
    const uint64_t* __restrict__ offset, const FieldEntries<IndexType, kHasValue> src, size_t nrows,
    const float* __restrict__ v, int units, int cpr, float* __restrict__ y, int* __restrict__ error) {
  __shared__ StagedRow<IndexType> lds[kGroupsPerBlock];
  const int in_group = threadIdx.x & (kGroup - 1);
  const int grp = threadIdx.x / kGroup;
  const uint32_t col = in_group & (cpr - 1);
  const uint32_t slot = in_group / cpr;
  const uint32_t slots = kGroup / cpr;
  const bool live_col = col < static_cast<uint32_t>(units);
  const float4* __restrict__ vu = reinterpret_cast<const float4*>(v);
  const size_t nf = static_cast<size_t>(src.num_fields);
  const size_t un = static_cast<size_t>(units);
  StagedRow<IndexType>& s = lds[grp];
  uint32_t err = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kGroupsPerBlock;
  for (size_t r0 = static_cast<size_t>(blockIdx.x) * kGroupsPerBlock; r0 < nrows; r0 += stride) {
    const size_t r = r0 + grp;
    uint64_t b = 0, e = 0;
    if (r < nrows) {
      b = offset[r];
      e = offset[r + 1];
    }
    const uint64_t n = e > b ? e - b : 0;
    const bool staged = n <= kCap;
    // every entry is read (and checked) once here, staged or not
    for (uint64_t j = in_group; j < n; j += kGroup) {
      IndexType id;
      uint32_t f;
      float x;
      err |= src.Load(b + j, &id, &f, &x);
      if (staged) {
        s.id[j] = id;
        s.field[j] = f;
        s.x[j] = x;
      }
    }
    dev::wave_sync();
    float acc = 0.0f;
    if (staged) {
      const uint32_t n32 = static_cast<uint32_t>(n);
      auto add_pair = [&](uint32_t a, uint32_t bb) {
        const uint32_t fa = s.field[a], fb = s.field[bb];
        if (fa != kSkip && fb != kSkip && live_col) {
          const float4 va = vu[(static_cast<size_t>(s.id[a]) * nf + fb) * un + col];
          const float4 vb = vu[(static_cast<size_t>(s.id[bb]) * nf + fa) * un + col];
          acc = fmaf(s.x[a] * s.x[bb], Dot(va, vb), acc);
        }
      };
      // full distances d = 1 .. nd: flat pair p = a nd + (d - 1) stands for
      // {a, (a + d) mod n}, d fastest -- the slots of one step read neighbouring
      // slices of V[i_a, :, :], and V[i_b, f_a, :] stays in one cache line of
      // every block i_b while a moves through neighbouring fields
      const uint32_t nd = n32 >= 2 ? (n32 - 1) / 2 : 0;
      if (nd != 0) {
        const uint32_t npairs = n32 * nd;
        const uint32_t aq = slots / nd, dr = slots % nd;
        uint32_t a = slot / nd, dd = slot % nd;
        for (uint32_t p = slot; p < npairs; p += slots) {
          uint32_t bb = a + dd + 1;
          if (bb >= n32) bb -= n32;
          add_pair(a, bb);
          dd += dr;
          a += aq;
          if (dd >= nd) {
            dd -= nd;
            ++a;
          }
        }
      }
      // an even n has the half distance n / 2 once per pair
      if (n32 >= 2 && (n32 & 1u) == 0) {
        const uint32_t half = n32 / 2;
        for (uint32_t a = slot; a < half; a += slots) add_pair(a, a + half);
      }
    } else {
      for (uint64_t a = 0; a + 1 < n; ++a) {
        IndexType ia, ib;
        uint32_t fa, fb;
        float xa, xb;
        src.Load(b + a, &ia, &fa, &xa);
        if (fa == kSkip) continue;
        for (uint64_t bb = a + 1 + slot; bb < n; bb += slots) {
          src.Load(b + bb, &ib, &fb, &xb);
          if (fb != kSkip && live_col) {
            const float4 va = vu[(static_cast<size_t>(ia) * nf + fb) * un + col];
            const float4 vb = vu[(static_cast<size_t>(ib) * nf + fa) * un + col];
            acc = fmaf(xa * xb, Dot(va, vb), acc);
          }
        }
      }
    }
#pragma unroll
    for (int dist = kGroup >> 1; dist >= 1; dist >>= 1) acc += __shfl_xor(acc, dist, dev::kWave);
    if (in_group == 0 && r < nrows) y[r] = acc;
    dev::wave_sync();  // the next row's staging overwrites this one's
  }
  if (err != 0u) atomicOr(error, static_cast<int>(err));
}

/*!
 * \brief FF2.  bpi = 64 / k entries b per wave-instruction; lane = bl * k + c
 *  (lanes with bl >= bpi idle when k does not divide 64).  The wave index is
 *  made scalar, so the row and a are uniform to the compiler.
 */
template <typename IndexType, bool kHasValue>
__global__ __launch_bounds__(kThreads) void k_ffm_backward(
    const uint64_t* __restrict__ offset, const FieldEntries<IndexType, kHasValue> src, size_t nrows,
    const float* __restrict__ g, const float* __restrict__ v, int k, float* __restrict__ dv) {
  __shared__ StagedRow<IndexType> lds[kWavesPerBlock];
  const uint32_t lane = threadIdx.x & (dev::kWave - 1);
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  const uint32_t uk = static_cast<uint32_t>(k);
  const uint32_t bpi = dev::kWave / uk;
  const uint32_t bl = lane / uk;
  const size_t c = lane - bl * uk;
  const size_t nf = static_cast<size_t>(src.num_fields);
  const size_t sk = static_cast<size_t>(k);
  StagedRow<IndexType>& s = lds[wave];
  const size_t stride = static_cast<size_t>(gridDim.x) * kWavesPerBlock;
  for (size_t r = static_cast<size_t>(blockIdx.x) * kWavesPerBlock + wave; r < nrows; r += stride) {
    const float gr = g[r];
    const uint64_t b = offset[r], e = offset[r + 1];
    const uint64_t n = e > b ? e - b : 0;
    if (gr == 0.0f || n < 2) continue;
    const bool staged = n <= kCap;
    if (staged) {
      for (uint64_t j = lane; j < n; j += dev::kWave) {
        src.Load(b + j, &s.id[j], &s.field[j], &s.x[j]);
      }
    }
    dev::wave_sync();
    for (uint64_t a = 0; a < n; ++a) {
      IndexType ia, ib;
      uint32_t fa, fb;
      float xa, xb;
      if (staged) {
        ia = s.id[a];
        fa = s.field[a];
        xa = s.x[a];
      } else {
        src.Load(b + a, &ia, &fa, &xa);
      }
      if (fa == kSkip) continue;
      const float ga = gr * xa;
      const size_t block_a = static_cast<size_t>(ia) * nf;
      if (bl < bpi) {
        for (uint64_t bb = bl; bb < n; bb += bpi) {
          if (staged) {
            ib = s.id[bb];
            fb = s.field[bb];
            xb = s.x[bb];
          } else {
            src.Load(b + bb, &ib, &fb, &xb);
          }
          if (bb != a && fb != kSkip) {
            const float w = v[(static_cast<size_t>(ib) * nf + fa) * sk + c];
            atomicAdd(&dv[(block_a + fb) * sk + c], ga * xb * w);
          }
        }
      }
    }
    dev::wave_sync();  // the next row's staging overwrites this one's
  }
}

void CheckShape(const char* what, int num_fields, int k) {
  CHECK(k >= 4 && k <= kFFMMaxRank && k % 4 == 0)
      << what << ": k must be a multiple of 4 in [4, " << kFFMMaxRank << "], got " << k;
  CHECK_GE(num_fields, 1) << what << ": num_fields must be >= 1";
}
}  // namespace

void LaunchFFMForward(const CsrView& csr, const float* v, uint64_t features, int num_fields, int k,
                      float* y, int* error, hipStream_t stream) {
  CheckView("ffm_forward", csr, false);
  CheckShape("ffm_forward", num_fields, k);
  CHECK(Aligned16(v)) << "ffm_forward: v must be 16-byte aligned";
  const size_t nrows = csr.nrows;
  if (nrows == 0) return;
  const int units = k / 4;
  const int cpr = NextPow2(units);
  const dim3 grid(GridFor(nrows, kGroupsPerBlock));
  DispatchIndexValue(csr, [&](auto tag, auto has_value) {
    using IndexType = decltype(tag);
    constexpr bool kHasValue = decltype(has_value)::value;
    using Entries = FieldEntries<IndexType, kHasValue>;
    hipLaunchKernelGGL((k_ffm_forward<IndexType, kHasValue>), grid, dim3(kThreads), 0, stream,
                       csr.offset,
                       Entries{IndexOf<IndexType>(csr), FieldOf<IndexType>(csr), csr.value, features,
                               static_cast<uint64_t>(num_fields)},
                       nrows, v, units, cpr, y, error);
  });
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchFFMBackward(const CsrView& csr, const float* g, const float* v, uint64_t features,
                       int num_fields, int k, float* dv, hipStream_t stream) {
  CheckView("ffm_backward", csr, false);
  CheckShape("ffm_backward", num_fields, k);
  const size_t nrows = csr.nrows;
  if (nrows == 0) return;
  const dim3 grid(GridFor(nrows, kWavesPerBlock));
  DispatchIndexValue(csr, [&](auto tag, auto has_value) {
    using IndexType = decltype(tag);
    constexpr bool kHasValue = decltype(has_value)::value;
    using Entries = FieldEntries<IndexType, kHasValue>;
    hipLaunchKernelGGL((k_ffm_backward<IndexType, kHasValue>), grid, dim3(kThreads), 0, stream,
                       csr.offset,
                       Entries{IndexOf<IndexType>(csr), FieldOf<IndexType>(csr), csr.value, features,
                               static_cast<uint64_t>(num_fields)},
                       nrows, g, v, k, dv);
  });
  DMLC_HIP_CHECK_LAUNCH();
}

}  // namespace gpu
}  // namespace dmlc
