/*!
 * \file src/gpu/rank_kernels.hip
 * \brief Q1 / Q2: runs of equal qid to a group pointer; RK1 / RK2: the pairwise
 *  ranking loss (RankNet / LambdaRank) of every query group with its gradient,
 *  and NDCG@k, over a score vector (f32).
 *
 * Q1   flag[r] = r == 0 || qid[r] != qid[r - 1]                     k_qid_flags
 * K3   LaunchScanU64: flag[r] becomes the number of run starts before r
 * Q2   ptr[scanned[r]] = r at every run start, ptr[G] = rows        k_qid_group_ptr
 * RK1  one wave per group of at most kRankWaveGroupRows rows        k_rank_wave
 * RK2  one 256-thread workgroup per longer group (< 2^31 rows)      k_rank_block
 *
 * A group g is rows [ptr[g], ptr[g + 1]).  Row i has score s_i, an integer
 * label l_i in [0, kRankMaxLabel] (held in f32) and gain G_i = 2^l_i - 1;
 * r_i / q_i are its positions in stable descending sorts by score / by label,
 * D(r) = 1 / log2(2 + r), IDCG = sum_i G_i D(q_i).  Over the pairs
 * P = {(i, j) : l_i > l_j}, with x_ij = sigma (s_i - s_j) and w_ij = 1 or
 * |G_i - G_j| |D(r_i) - D(r_j)| / IDCG,
 *   loss_g  = 1/|P| sum_P w_ij softplus(-x_ij)
 *   grad[i] = sigma/|P| (- sum_{j: l_i > l_j} w_ij rho(x_ij) + sum_{j: l_j > l_i} w_ji rho(x_ji))
 * (rho(z) = 1 / (1 + e^z); w is a constant of the gradient), and
 *   NDCG@k  = sum_{r_i < k} G_i D(r_i) / sum_{q_i < k} G_i D(q_i), 1 if the latter is 0.
 *
 * No sort.  r_i and q_i are counts -- #{j : s_j > s_i or (s_j == s_i and j < i)}
 * -- taken by comparing row i with every staged row j (CountRanks, the one
 * rank-counting routine of both kernels and of both the loss and the metric:
 * the kernels are templates over RankMode).  A count over the other rows of the
 * group is below n whatever a NaN score makes the comparisons return.
 *
 * Gather form, no atomics.  Row i has an owner that sums its pair terms over all
 * j (PairTerm): every pair is evaluated twice, once from each side, which buys
 * a grad[i] that is written once, by one lane, in an order fixed by the group's
 * length alone -- the same inputs give the same bytes.  One exp serves a pair's
 * softplus and rho.  The loss and |P| are taken from the l_i > l_j side only.
 * IDCG and the two NDCG sums are accumulated in f64 (their error would otherwise
 * enter every pair weight); everything else is f32.
 *
 * RK1 mapping.  The wave stages the group's (score, label, gain) in LDS once
 * (kRankWaveGroupRows rows x 20 bytes per wave with D(r_i) and the unscaled
 * gradient next to them).  Its 64 lanes are split into rows x slices: a group
 * of n rows gets lpr = 64 / next_pow2(n) lanes per row (1 from 33 rows up), lane
 * = row slot * lpr + slice, slice t sweeping j = t, t + lpr, ...; the slices of
 * a row are folded by __shfl_xor over distances lpr / 2 .. 1.  A 24-row group
 * (typical of the Yahoo set) thus keeps 48 lanes busy with 12 steps each where
 * one lane per row would keep 24 busy for 24 steps.  Lanes that read LDS in the
 * same instruction read lpr consecutive words (all row slots of one slice read
 * the same j: a broadcast), so the sweep is free of bank conflicts.  Groups
 * above 64 rows take 64 rows per round.  |P| is known after the last round, so
 * the unscaled sums wait in LDS and one coalesced sweep writes grad.
 *
 * RK2 mapping.  Thread t owns rows t, t + 256, ...; the group's rows j pass
 * through LDS in tiles of kRankTileRows, every thread reading the same j of the
 * tile at a time (a broadcast).  A first pass checks the labels and counts them
 * per value with ballots (lane c keeps the count of label c), which gives |P| =
 * sum_c count_c * #{labels below c} before any pair is formed; a counting pass
 * leaves D(r_i) in a per-row scratch (row_scratch[ptr[g] + i]) and sums IDCG
 * over the workgroup in a fixed order (lanes, then waves); the pair pass reads
 * D(r_j) back with the tile and writes grad[i] scaled, once.
 *
 * Both kernels are launched over all groups and each skips the other's: no
 * group length is read back to size a launch.  A group whose pointers descend,
 * end past `rows` or span 2^31 rows or more forms no address, and a group with a
 * label that is negative, fractional, NaN or above kRankMaxLabel forms no pair:
 * both leave their rows of grad as the caller zeroed them, write loss 0 /
 * pairs 0 (NDCG 0) and OR kRankErrGroup / kRankErrLabel into the error word.
 * All address arithmetic is size_t.
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
constexpr int kWaves = kThreads / dev::kWave;  // RK1: groups per workgroup
constexpr uint32_t kCap = kRankWaveGroupRows;
constexpr uint32_t kTile = kRankTileRows;
constexpr uint32_t kLabels = kRankMaxLabel + 1;
constexpr uint64_t kMaxGroupRows = 1ull << 31;
static_assert(kTile == kThreads, "RK2 stages one tile row per thread");
static_assert(kLabels <= dev::kWave, "RK2 keeps one label count per lane");

enum class RankMode : int { kLoss = 0, kNdcg = 1 };

// --------------------------------- Q1 / Q2 ---------------------------------
__global__ __launch_bounds__(kThreads) void k_qid_flags(const uint64_t* __restrict__ qid, size_t rows,
                                                        uint64_t* __restrict__ flag) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (r < rows) flag[r] = (r == 0 || qid[r] != qid[r - 1]) ? 1ull : 0ull;
}

__global__ __launch_bounds__(kThreads) void k_qid_group_ptr(
    const uint64_t* __restrict__ qid, size_t rows, const uint64_t* __restrict__ scanned,
    const uint64_t* __restrict__ total, uint64_t capacity, uint64_t* __restrict__ ptr) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (r == 0) {
    const uint64_t g = *total;
    if (g <= capacity) ptr[g] = rows;  // the closing pointer
  }
  if (r < rows && (r == 0 || qid[r] != qid[r - 1])) {
    const uint64_t g = scanned[r];
    if (g < capacity) ptr[g] = r;
  }
}

// ------------------------- shared by RK1 and RK2 ---------------------------
/*! \brief the label as an integer, or -1 if it is not one in [0, kRankMaxLabel] (a NaN is not) */
__device__ __forceinline__ int LabelOf(float l) {
  const bool ok = l >= 0.0f && l <= static_cast<float>(kRankMaxLabel) && l == truncf(l);
  return ok ? static_cast<int>(l) : -1;
}

/*! \brief 2^l - 1 for l in [0, 31] (one rounding from l = 25) */
__device__ __forceinline__ float GainOf(int l) {
  return static_cast<float>((1u << static_cast<uint32_t>(l)) - 1u);
}

/*! \brief D(r) = 1 / log2(2 + r), r < 2^31 */
__device__ __forceinline__ float Discount(uint32_t r) {
  return 1.0f / log2f(static_cast<float>(r + 2u));
}

/*!
 * \brief the rank counts of row i (score si, label li) against staged rows
 *  jbeg, jbeg + jstep, ... < jend, whose positions in the group are jbase + j:
 *  *r += rows that sort before i by score, *q += by label (stable, descending)
 */
__device__ __forceinline__ void CountRanks(const float* ts, const int* tl, uint32_t jbeg,
                                           uint32_t jend, uint32_t jstep, uint32_t jbase, float si,
                                           int li, uint32_t i, uint32_t* r, uint32_t* q) {
  for (uint32_t j = jbeg; j < jend; j += jstep) {
    const float sj = ts[j];
    const int lj = tl[j];
    const bool before = jbase + j < i;
    *r += (sj > si || (sj == si && before)) ? 1u : 0u;
    *q += (lj > li || (lj == li && before)) ? 1u : 0u;
  }
}

/*! \brief row i's terms of NDCG@k: G_i D(r_i) if r_i < k, G_i D(q_i) if q_i < k (f64 sums) */
__device__ __forceinline__ void NdcgTerms(float gain, uint32_t r, uint32_t q, uint32_t k, double* dcg,
                                          double* idcg) {
  if (r < k) *dcg += static_cast<double>(gain) * static_cast<double>(Discount(r));
  if (q < k) *idcg += static_cast<double>(gain) * static_cast<double>(Discount(q));
}

/*! \brief what is the same for every pair of a launch */
struct PairParams {
  float sigma;
  bool ndcg;       // w_ij = |G_i - G_j| |D_i - D_j| / IDCG, else 1
  float inv_idcg;  // 1 / IDCG (0 if IDCG is 0: such a group has no pair)
};

/*!
 * \brief the pair {i, j} seen from row i: nothing if l_i == l_j; with l_i > l_j
 *  loss += w softplus(-x_ij), acc -= w rho(x_ij), one pair counted; with
 *  l_j > l_i acc += w rho(x_ji).  e = exp(-|x|) serves softplus(-x) = max(-x, 0)
 *  + log1p(e) and rho(x) = e / (1 + e) (x > 0), 1 / (1 + e) (x <= 0): no
 *  overflow, and a saturated pair gives exactly 0 or 1.  Written without
 *  branches (an equal-label pair has weight 0 and adds +-0): the lanes of a
 *  wave rarely agree on the side, so a branch would run both anyway.
 */
__device__ __forceinline__ void PairTerm(const PairParams& p, float si, int li, float gi, float di,
                                         float sj, int lj, float gj, float dj, float* loss, float* acc,
                                         uint32_t* pairs) {
  const bool upper = li > lj;
  const float x = p.sigma * (upper ? si - sj : sj - si);
  float w = li != lj ? 1.0f : 0.0f;
  if (p.ndcg) w *= fabsf(gi - gj) * fabsf(di - dj) * p.inv_idcg;
  const float e = expf(-fabsf(x));
  const float wrho = w * ((x > 0.0f ? e : 1.0f) / (1.0f + e));
  *loss += upper ? w * (fmaxf(-x, 0.0f) + log1pf(e)) : 0.0f;
  *acc += upper ? -wrho : wrho;
  *pairs += upper ? 1u : 0u;
}

/*! \brief the extent of group g, checked: *n = its rows; false (and *n = 0) if the pointers are bad */
__device__ __forceinline__ bool GroupExtent(const uint64_t* __restrict__ ptr, size_t g, uint64_t rows,
                                            size_t* b, uint64_t* n) {
  const uint64_t lo = ptr[g], hi = ptr[g + 1];
  const bool ok = lo <= hi && hi <= rows && hi - lo < kMaxGroupRows;
  *b = static_cast<size_t>(lo);
  *n = ok ? hi - lo : 0;
  return ok;
}

/*! \brief what a kernel writes for a group: (loss, |P|) or NDCG */
struct GroupOut {
  float* loss;     // kLoss: [groups]; kNdcg: the NDCG values
  int64_t* pairs;  // kLoss only
};
template <RankMode kMode>
__device__ __forceinline__ void WriteGroup(const GroupOut& out, size_t g, float v, uint64_t pairs) {
  out.loss[g] = v;
  if (kMode == RankMode::kLoss) out.pairs[g] = static_cast<int64_t>(pairs);
}

// ----------------------------------- RK1 -----------------------------------
/*! \brief one wave's staged group */
struct StagedGroup {
  float s[kCap];
  int l[kCap];
  float gain[kCap];
  float d[kCap];    // D(r_i)
  float acc[kCap];  // row i's unscaled gradient sum
};

/*!
 * \brief RK1.  The group loop is uniform over the wave and a wave's LDS image
 *  is written and read by its own lanes only: dev::wave_sync orders them.
 *  k: the NDCG cutoff (kNdcg).
 */
template <RankMode kMode>
__global__ __launch_bounds__(kThreads) void k_rank_wave(
    const float* __restrict__ score, const float* __restrict__ label,
    const uint64_t* __restrict__ ptr, size_t groups, uint64_t rows, PairParams prm, uint32_t k,
    float* __restrict__ grad, GroupOut out, int* __restrict__ error) {
  __shared__ StagedGroup lds[kWaves];
  const uint32_t lane = threadIdx.x & (dev::kWave - 1);
  const uint32_t wave = dev::uniform(static_cast<uint32_t>(threadIdx.x / dev::kWave));
  StagedGroup& s = lds[wave];
  uint32_t err = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kWaves;
  for (size_t g = static_cast<size_t>(blockIdx.x) * kWaves + wave; g < groups; g += stride) {
    size_t b;
    uint64_t n64;
    if (!GroupExtent(ptr, g, rows, &b, &n64)) {
      err |= kRankErrGroup;
      if (lane == 0) WriteGroup<kMode>(out, g, 0.0f, 0);
      continue;
    }
    if (n64 > kCap) continue;  // RK2's
    const uint32_t n = static_cast<uint32_t>(n64);
    bool bad = false;
    for (uint32_t j = lane; j < n; j += dev::kWave) {
      const int l = LabelOf(label[b + j]);
      bad |= l < 0;
      s.s[j] = score[b + j];
      s.l[j] = l;
      s.gain[j] = GainOf(l < 0 ? 0 : l);
    }
    dev::wave_sync();
    if (__any(bad)) {
      err |= kRankErrLabel;
      if (lane == 0) WriteGroup<kMode>(out, g, 0.0f, 0);
      dev::wave_sync();
      continue;
    }
    // lanes = row slots x slices
    uint32_t lpr = 1;
    while (lpr * 2u * n <= static_cast<uint32_t>(dev::kWave) && lpr < 32u) lpr <<= 1;
    const uint32_t slice = lane & (lpr - 1u);
    const uint32_t slot = lane / lpr;
    const uint32_t slots = static_cast<uint32_t>(dev::kWave) / lpr;
    const bool counted = kMode == RankMode::kNdcg || prm.ndcg;
    double dcg = 0.0, idcg = 0.0;
    if (counted) {
      for (uint32_t i0 = 0; i0 < n; i0 += slots) {  // uniform: every lane folds
        const uint32_t i = i0 + slot;
        const bool live = i < n;
        uint32_t r = 0, q = 0;
        if (live) CountRanks(s.s, s.l, slice, n, lpr, 0u, s.s[i], s.l[i], i, &r, &q);
        for (uint32_t dist = lpr >> 1; dist >= 1u; dist >>= 1) {
          r += __shfl_xor(r, dist, dev::kWave);
          q += __shfl_xor(q, dist, dev::kWave);
        }
        if (live && slice == 0u) {
          if (kMode == RankMode::kNdcg) {
            NdcgTerms(s.gain[i], r, q, k, &dcg, &idcg);
          } else {
            s.d[i] = Discount(r);
            NdcgTerms(s.gain[i], r, q, n, &dcg, &idcg);
          }
        }
      }
#pragma unroll
      for (int dist = dev::kWave >> 1; dist >= 1; dist >>= 1) {
        dcg += __shfl_xor(dcg, dist, dev::kWave);
        idcg += __shfl_xor(idcg, dist, dev::kWave);
      }
      dev::wave_sync();  // d[] is read by other lanes below
    }
    if (kMode == RankMode::kNdcg) {
      if (lane == 0) WriteGroup<kMode>(out, g, idcg > 0.0 ? static_cast<float>(dcg / idcg) : 1.0f, 0);
    } else {
      PairParams p = prm;
      const float idcg32 = static_cast<float>(idcg);
      p.inv_idcg = idcg32 > 0.0f ? 1.0f / idcg32 : 0.0f;
      float loss = 0.0f;
      uint32_t pairs = 0;
      for (uint32_t i0 = 0; i0 < n; i0 += slots) {
        const uint32_t i = i0 + slot;
        const bool live = i < n;
        float acc = 0.0f;
        if (live) {
          const float si = s.s[i], gi = s.gain[i], di = prm.ndcg ? s.d[i] : 0.0f;
          const int li = s.l[i];
          for (uint32_t j = slice; j < n; j += lpr) {
            PairTerm(p, si, li, gi, di, s.s[j], s.l[j], s.gain[j], prm.ndcg ? s.d[j] : 0.0f, &loss,
                     &acc, &pairs);
          }
        }
        for (uint32_t dist = lpr >> 1; dist >= 1u; dist >>= 1) {
          acc += __shfl_xor(acc, dist, dev::kWave);
        }
        if (live && slice == 0u) s.acc[i] = acc;
      }
#pragma unroll
      for (int dist = dev::kWave >> 1; dist >= 1; dist >>= 1) {
        loss += __shfl_xor(loss, dist, dev::kWave);
      }
      const uint32_t np = dev::wave_sum(pairs);
      const float fp = static_cast<float>(np);
      const float scale = np != 0u ? prm.sigma / fp : 0.0f;
      dev::wave_sync();  // acc[] is read by other lanes below
      for (uint32_t i = lane; i < n; i += dev::kWave) grad[b + i] = scale * s.acc[i];
      if (lane == 0) WriteGroup<kMode>(out, g, np != 0u ? loss / fp : 0.0f, np);
    }
    dev::wave_sync();  // the next group's staging overwrites this one's
  }
  if (err != 0u) atomicOr(error, static_cast<int>(err));  // the status word, not an output
}

// ----------------------------------- RK2 -----------------------------------
/*! \brief v summed over the workgroup in a fixed order (lanes by __shfl_xor, then
 *  the waves in turn); every thread gets the sum.  Contains two __syncthreads. */
template <typename T>
__device__ __forceinline__ T BlockSum(T v, T* smem) {
#pragma unroll
  for (int dist = dev::kWave >> 1; dist >= 1; dist >>= 1) v += __shfl_xor(v, dist, dev::kWave);
  __syncthreads();  // smem's last readers are done
  if ((threadIdx.x & (dev::kWave - 1)) == 0) smem[threadIdx.x / dev::kWave] = v;
  __syncthreads();
  T sum = smem[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) sum += smem[w];
  return sum;
}

/*!
 * \brief RK2.  Everything that decides a branch around a __syncthreads (the
 *  group's extent, its label check, the mode) is uniform over the workgroup.
 */
template <RankMode kMode>
__global__ __launch_bounds__(kThreads) void k_rank_block(
    const float* __restrict__ score, const float* __restrict__ label,
    const uint64_t* __restrict__ ptr, size_t groups, uint64_t rows, PairParams prm, uint32_t k,
    float* row_scratch, float* __restrict__ grad, GroupOut out, int* __restrict__ error) {
  __shared__ float ts[kTile];
  __shared__ int tl[kTile];
  __shared__ float tg[kTile];
  __shared__ float td[kTile];
  __shared__ uint32_t hist[kWaves][kLabels];
  __shared__ double sum64[kWaves];
  __shared__ float sum32[kWaves];
  const uint32_t t = threadIdx.x;
  const uint32_t lane = t & (dev::kWave - 1);
  const uint32_t wave = t / dev::kWave;
  uint32_t err = 0;
  for (size_t g = blockIdx.x; g < groups; g += gridDim.x) {
    size_t b;
    uint64_t n64;
    if (!GroupExtent(ptr, g, rows, &b, &n64)) continue;  // RK1 reports it
    if (n64 <= kCap) continue;                           // RK1's
    const uint32_t n = static_cast<uint32_t>(n64);
    // the labels, checked, and (lane c of every wave) the rows with label c
    bool bad = false;
    uint32_t mine = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += kThreads) {
      const uint32_t i = i0 + t;
      const int l = i < n ? LabelOf(label[b + i]) : static_cast<int>(kLabels);  // past the end: none
      bad |= l < 0;
      for (uint32_t c = 0; c < kLabels; ++c) {
        const uint32_t cnt = static_cast<uint32_t>(__popcll(__ballot(l == static_cast<int>(c))));
        mine += lane == c ? cnt : 0u;
      }
    }
    if (__syncthreads_or(bad ? 1 : 0)) {
      err |= kRankErrLabel;
      if (t == 0) WriteGroup<kMode>(out, g, 0.0f, 0);
      continue;
    }
    const bool counted = kMode == RankMode::kNdcg || prm.ndcg;
    double dcg = 0.0, idcg = 0.0;
    if (counted) {
      for (uint32_t i0 = 0; i0 < n; i0 += kThreads) {
        const uint32_t i = i0 + t;
        const bool live = i < n;
        const float si = live ? score[b + i] : 0.0f;
        const int li = live ? LabelOf(label[b + i]) : 0;
        uint32_t r = 0, q = 0;
        for (uint32_t j0 = 0; j0 < n; j0 += kTile) {
          __syncthreads();  // the tile's last readers are done
          if (j0 + t < n) {
            ts[t] = score[b + j0 + t];
            tl[t] = LabelOf(label[b + j0 + t]);
          }
          __syncthreads();
          const uint32_t tn = n - j0 < kTile ? n - j0 : kTile;
          if (live) CountRanks(ts, tl, 0u, tn, 1u, j0, si, li, i, &r, &q);
        }
        if (live) {
          const float gi = GainOf(li);
          if (kMode == RankMode::kNdcg) {
            NdcgTerms(gi, r, q, k, &dcg, &idcg);
          } else {
            row_scratch[b + i] = Discount(r);  // read back by the pair pass, after a barrier
            NdcgTerms(gi, r, q, n, &dcg, &idcg);
          }
        }
      }
      idcg = BlockSum(idcg, sum64);
      if (kMode == RankMode::kNdcg) dcg = BlockSum(dcg, sum64);
    }
    if (kMode == RankMode::kNdcg) {
      if (t == 0) WriteGroup<kMode>(out, g, idcg > 0.0 ? static_cast<float>(dcg / idcg) : 1.0f, 0);
      continue;
    }
    // |P| = sum_c count_c * #{labels below c}, before any pair is formed
    __syncthreads();
    if (lane < kLabels) hist[wave][lane] = mine;
    __syncthreads();
    uint64_t np = 0, below = 0;
    for (uint32_t c = 0; c < kLabels; ++c) {
      uint64_t cnt = 0;
      for (int w = 0; w < kWaves; ++w) cnt += hist[w][c];
      np += cnt * below;
      below += cnt;
    }
    PairParams p = prm;
    const float idcg32 = static_cast<float>(idcg);
    p.inv_idcg = idcg32 > 0.0f ? 1.0f / idcg32 : 0.0f;
    const float fp = static_cast<float>(np);
    const float scale = np != 0 ? prm.sigma / fp : 0.0f;
    float loss = 0.0f;
    // the D(r_i) other threads left in row_scratch are read below after a barrier
    // (IDCG's BlockSum and the one that opens every tile)
    for (uint32_t i0 = 0; i0 < n; i0 += kThreads) {
      const uint32_t i = i0 + t;
      const bool live = i < n;
      const float si = live ? score[b + i] : 0.0f;
      const int li = live ? LabelOf(label[b + i]) : 0;
      const float gi = GainOf(li);
      const float di = (live && prm.ndcg) ? row_scratch[b + i] : 0.0f;
      float acc = 0.0f;
      uint32_t seen = 0;  // |P| comes from the label counts
      for (uint32_t j0 = 0; j0 < n; j0 += kTile) {
        __syncthreads();  // the tile's last readers are done
        if (j0 + t < n) {
          const int l = LabelOf(label[b + j0 + t]);
          ts[t] = score[b + j0 + t];
          tl[t] = l;
          tg[t] = GainOf(l);
          td[t] = prm.ndcg ? row_scratch[b + j0 + t] : 0.0f;
        }
        __syncthreads();
        const uint32_t tn = n - j0 < kTile ? n - j0 : kTile;
        if (live) {
          for (uint32_t j = 0; j < tn; ++j) {
            PairTerm(p, si, li, gi, di, ts[j], tl[j], tg[j], td[j], &loss, &acc, &seen);
          }
        }
      }
      if (live) grad[b + i] = scale * acc;
    }
    loss = BlockSum(loss, sum32);
    if (t == 0) WriteGroup<kMode>(out, g, np != 0 ? loss / fp : 0.0f, np);
  }
  if (err != 0u && t == 0) atomicOr(error, static_cast<int>(err));  // the status word, not an output
}

template <RankMode kMode>
void LaunchRank(const float* score, const float* label, const uint64_t* group_ptr, size_t groups,
                uint64_t rows, const PairParams& prm, uint32_t k, float* row_scratch, float* grad,
                const GroupOut& out, int* error, hipStream_t stream) {
  hipLaunchKernelGGL(k_rank_wave<kMode>, dim3(GridFor(groups, kWaves)), dim3(kThreads), 0, stream,
                     score, label, group_ptr, groups, rows, prm, k, grad, out, error);
  hipLaunchKernelGGL(k_rank_block<kMode>, dim3(GridFor(groups, 1)), dim3(kThreads), 0, stream, score,
                     label, group_ptr, groups, rows, prm, k, row_scratch, grad, out, error);
  DMLC_HIP_CHECK_LAUNCH();
}
}  // namespace

void LaunchQidFlags(const uint64_t* qid, size_t rows, uint64_t* flag, hipStream_t stream) {
  if (rows == 0) return;
  const size_t blocks = (rows + kThreads - 1) / kThreads;
  CHECK_LT(blocks, (1ull << 32) / kThreads) << "qid_groups: too many rows for one launch";
  hipLaunchKernelGGL(k_qid_flags, dim3(blocks), dim3(kThreads), 0, stream, qid, rows, flag);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchQidGroupPtr(const uint64_t* qid, size_t rows, const uint64_t* scanned,
                       const uint64_t* total, uint64_t capacity, uint64_t* group_ptr,
                       hipStream_t stream) {
  if (rows == 0) return;
  const size_t blocks = (rows + kThreads - 1) / kThreads;
  CHECK_LT(blocks, (1ull << 32) / kThreads) << "qid_groups: too many rows for one launch";
  hipLaunchKernelGGL(k_qid_group_ptr, dim3(blocks), dim3(kThreads), 0, stream, qid, rows, scanned,
                     total, capacity, group_ptr);
  DMLC_HIP_CHECK_LAUNCH();
}

void LaunchRankLoss(const float* score, const float* label, const uint64_t* group_ptr, size_t groups,
                    uint64_t rows, bool ndcg_weights, float sigma, float* row_scratch, float* grad,
                    float* loss_g, int64_t* pairs_g, int* error, hipStream_t stream) {
  if (groups == 0) return;
  CHECK(sigma > 0.0f) << "rank_loss: sigma must be > 0";
  CHECK(!ndcg_weights || row_scratch != nullptr) << "rank_loss: ndcg weights need the row scratch";
  LaunchRank<RankMode::kLoss>(score, label, group_ptr, groups, rows,
                              PairParams{sigma, ndcg_weights, 0.0f}, 0u, row_scratch, grad,
                              GroupOut{loss_g, pairs_g}, error, stream);
}

void LaunchRankNdcg(const float* score, const float* label, const uint64_t* group_ptr, size_t groups,
                    uint64_t rows, uint32_t k, float* ndcg, int* error, hipStream_t stream) {
  if (groups == 0) return;
  CHECK_GE(k, 1u) << "ndcg: k must be >= 1";
  LaunchRank<RankMode::kNdcg>(score, label, group_ptr, groups, rows, PairParams{1.0f, false, 0.0f}, k,
                              nullptr, nullptr, GroupOut{ndcg, nullptr}, error, stream);
}

}  // namespace gpu
}  // namespace dmlc
