/*!
 * \file tests/cpp/unittest_pack_ranges.cc
 * \brief The range-stealing pack pool (src/gpu/pack_pool.h): a job is cut into
 *  ranges that the threads claim one by one, two jobs are open at once and the
 *  thread that reports the last range settles the job.  Whatever the thread
 *  count and the timing, the packed bytes equal PackText of the same input.
 *  Also the link-aware submit rule (DecideSubmit), driven with a fake link.
 *  Part of the ThreadSanitizer and AddressSanitizer runs of the suite.
 */
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../src/gpu/pack_pool.h"
#include "../../src/gpu/text_pack_codec.h"
#include "./testing.h"

namespace {

using dmlc::gpu::DecideSubmit;
using dmlc::gpu::PackJob;
using dmlc::gpu::PackPool;
using dmlc::gpu::SubmitAction;

constexpr size_t kBlock = dmlc::gpu::kPackBlockBytes;
constexpr size_t kRange = PackPool::kRangeBlocks * kBlock;  // text bytes of one range
constexpr uint8_t kGuard = 0xEE;
constexpr size_t kGuardBytes = 256;

std::string Text(size_t n, unsigned seed) {
  static const char kSym[] = "0123456789:. \n-e";
  std::string s(n, '0');
  unsigned x = seed * 2654435761u + 99u;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    s[i] = kSym[(x >> 24) % 16];
  }
  return s;
}

/*! \brief a byte outside the alphabet in block b (if the text has one) */
void Spoil(std::string* s, size_t b) {
  if (b * kBlock < s->size()) (*s)[std::min(s->size() - 1, b * kBlock + b % kBlock)] = '\r';
}

struct Piece {
  std::string text;
  std::vector<uint8_t> out;
  size_t bound{0};  // bytes of `out` before the guard
  std::unique_ptr<PackJob> job;
};

void MakeJob(Piece* p, size_t seq, double ratio) {
  const size_t n = p->text.size();
  // what the feed reserves for a slot (ratio < 0, the tests' "pack anything":
  // every block may be an exception)
  p->bound = ratio < 0 ? dmlc::gpu::PackedBytes(n, dmlc::gpu::PackBlocks(n))
                       : static_cast<size_t>(ratio * static_cast<double>(n)) + 64;
  p->out.assign(p->bound + kGuardBytes, kGuard);
  p->job.reset(new PackJob());
  p->job->ptr = p->text.data();
  p->job->size = n;
  p->job->seq = seq;
  p->job->ratio = ratio;
  p->job->out = p->out.data();
}

bool GuardIntact(const Piece& p) {
  for (size_t i = p.bound; i < p.out.size(); ++i) {
    if (p.out[i] != kGuard) return false;
  }
  return true;
}

/*! \brief the job is packed, and to exactly the bytes PackText gives */
void ExpectEqualsPackText(const Piece& p, const uint8_t alphabet[16]) {
  ASSERT_EQ(p.job->state.load(), static_cast<int>(PackJob::kPacked));
  std::vector<uint8_t> want;
  ASSERT_TRUE(dmlc::gpu::PackText(reinterpret_cast<const uint8_t*>(p.text.data()), p.text.size(),
                                  alphabet, p.job->ratio, &want));
  ASSERT_EQ(p.job->packed_bytes, want.size());
  EXPECT_TRUE(std::memcmp(p.out.data(), want.data(), want.size()) == 0);
  EXPECT_TRUE(GuardIntact(p));
  std::string back(p.text.size(), '#');
  dmlc::gpu::UnpackReference(p.out.data(), reinterpret_cast<uint8_t*>(&back[0]));
  EXPECT_TRUE(back == p.text);
}

}  // namespace

TEST(PackRanges, OutputEqualsPackText) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  // around one block; one range minus one block, exactly one, one plus one
  // byte; several ranges with an odd tail
  const size_t sizes[] = {1,      255,        256,          257, kRange - kBlock,
                          kRange, kRange + 1, 3 * kRange + 777};
  for (int threads : {1, 3, 16}) {  // 16: more threads than any of these has ranges
    PackPool pool(threads, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
    std::vector<Piece> pieces;
    for (size_t n : sizes) {
      // 0: none; 1: a few; 2: every block, whose copy is shared in ranges too
      for (int exceptions = 0; exceptions < 3; ++exceptions) {
        pieces.emplace_back();
        Piece& p = pieces.back();
        p.text = Text(n, static_cast<unsigned>(n + exceptions));
        if (exceptions == 2) {
          for (size_t b = 0; b * kBlock < n; ++b) Spoil(&p.text, b);
        } else if (exceptions == 1) {
          // every 37th block, and the first and the last block of every range
          for (size_t b = 0; b * kBlock < n; b += 37) Spoil(&p.text, b);
          for (size_t r = 0; r * kRange < n; ++r) {
            Spoil(&p.text, r * PackPool::kRangeBlocks);
            Spoil(&p.text, (r + 1) * PackPool::kRangeBlocks - 1);
          }
          Spoil(&p.text, dmlc::gpu::PackBlocks(n) - 1);
        }
      }
    }
    for (size_t i = 0; i < pieces.size(); ++i) MakeJob(&pieces[i], i, -1.0);
    for (auto& p : pieces) pool.Push(p.job.get());
    for (size_t i = 0; i < pieces.size(); ++i) {
      pool.Wait(pieces[i].job.get());
      ExpectEqualsPackText(pieces[i], alphabet);
      EXPECT_EQ(pieces[i].job->nexc != 0, i % 3 != 0);
      if (i % 3 == 2) {
        EXPECT_EQ(size_t(pieces[i].job->nexc), dmlc::gpu::PackBlocks(pieces[i].text.size()));
      }
    }
  }
}

TEST(PackRanges, SmallJobsBetweenLargeOnes) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  // jobs of one range (the next one opens while the large one before it is
  // still being packed) between jobs of three
  std::vector<Piece> pieces(30);
  for (size_t i = 0; i < pieces.size(); ++i) {
    pieces[i].text = Text(i % 3 == 2 ? 2 * kRange + 4097 + i : 3000 + 131 * i,
                          static_cast<unsigned>(i));
    if (i % 5 == 0) Spoil(&pieces[i].text, 3);
    MakeJob(&pieces[i], i, -1.0);
  }
  PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
  for (auto& p : pieces) pool.Push(p.job.get());
  for (auto& p : pieces) {
    pool.Wait(p.job.get());
    ExpectEqualsPackText(p, alphabet);
  }
  EXPECT_GT(pool.pack_sec(), 0.0);
}

TEST(PackRanges, RejectedInALateRange) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  std::vector<Piece> pieces(3);
  for (size_t i = 0; i < pieces.size(); ++i) pieces[i].text = Text(4 * kRange + 300, 7 + i);
  // the second job: every block of its last two ranges is an exception, twice
  // what the 3/4 rule allows; the first two ranges are clean
  const size_t blocks = dmlc::gpu::PackBlocks(pieces[1].text.size());
  for (size_t b = 2 * PackPool::kRangeBlocks; b < blocks; ++b) Spoil(&pieces[1].text, b);
  ASSERT_GT(static_cast<long>(blocks - 2 * PackPool::kRangeBlocks),
            dmlc::gpu::PackMaxExceptions(pieces[1].text.size()));
  for (size_t i = 0; i < pieces.size(); ++i) MakeJob(&pieces[i], i, dmlc::gpu::kPackMaxRatio);
  PackPool pool(3, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
  for (auto& p : pieces) pool.Push(p.job.get());
  for (auto& p : pieces) pool.Wait(p.job.get());
  ExpectEqualsPackText(pieces[0], alphabet);
  EXPECT_EQ(pieces[1].job->state.load(), static_cast<int>(PackJob::kRejected));
  EXPECT_TRUE(GuardIntact(pieces[1]));
  std::vector<uint8_t> unused;
  EXPECT_FALSE(dmlc::gpu::PackText(reinterpret_cast<const uint8_t*>(pieces[1].text.data()),
                                   pieces[1].text.size(), alphabet, dmlc::gpu::kPackMaxRatio,
                                   &unused));
  ExpectEqualsPackText(pieces[2], alphabet);
}

TEST(PackRanges, QuiesceWhileTwoJobsAreOpen) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
  for (int round = 0; round < 8; ++round) {
    // three ranges each and four threads: when the first job is settled, the
    // next two are open
    std::vector<Piece> pieces(6);
    for (size_t i = 0; i < pieces.size(); ++i) {
      pieces[i].text = Text(2 * kRange + 999 + i, static_cast<unsigned>(round * 8 + i));
      MakeJob(&pieces[i], i, -1.0);
    }
    for (auto& p : pieces) pool.Push(p.job.get());
    pool.Wait(pieces[0].job.get());
    pool.Quiesce();
    for (auto& p : pieces) {
      const int st = p.job->state.load();
      EXPECT_TRUE(st == PackJob::kPacked || st == PackJob::kQueued);
      if (st == PackJob::kPacked) ExpectEqualsPackText(p, alphabet);
    }
    pieces.clear();  // nothing is read or written after Quiesce
  }
}

TEST(PackRanges, ClaimRawRacesThePool) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  std::vector<Piece> pieces(40);
  for (size_t i = 0; i < pieces.size(); ++i) {
    pieces[i].text = Text(70000 + 13 * i, static_cast<unsigned>(i));
    MakeJob(&pieces[i], i, -1.0);
    pieces[i].bound = 0;  // the whole buffer is guard: a claimed job's slot is never written
  }
  size_t claimed = 0, packed = 0;
  {
    PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
    for (auto& p : pieces) pool.Push(p.job.get());
    // from the back, where the pool arrives last
    for (size_t i = pieces.size(); i-- > 0;) {
      if (pool.TryClaimRaw(pieces[i].job.get())) {
        ++claimed;
      } else {
        pool.Wait(pieces[i].job.get());
      }
    }
  }
  for (auto& p : pieces) {
    if (p.job->state.load() == PackJob::kClaimedRaw) {
      EXPECT_TRUE(GuardIntact(p));
    } else {
      p.bound = p.out.size() - kGuardBytes;
      ExpectEqualsPackText(p, alphabet);
      ++packed;
    }
  }
  EXPECT_EQ(claimed + packed, pieces.size());
}

TEST(PackRanges, DecideSubmitTable) {
  const auto busy = []() { return true; };
  const auto idle = []() { return false; };
  // link idle: an unstarted job goes raw, a pack in progress is waited for
  EXPECT_TRUE(DecideSubmit(PackJob::kQueued, false, false, false, idle) == SubmitAction::kClaimRaw);
  EXPECT_TRUE(DecideSubmit(PackJob::kPacking, false, false, false, idle) == SubmitAction::kWait);
  // copies outstanding: the piece is left to the pool
  EXPECT_TRUE(DecideSubmit(PackJob::kQueued, false, false, false, busy) == SubmitAction::kDefer);
  EXPECT_TRUE(DecideSubmit(PackJob::kPacking, false, false, false, busy) == SubmitAction::kDefer);
  // nothing in flight: never deferred, whatever the link says
  for (int st : {PackJob::kQueued, PackJob::kPacking, PackJob::kPacked, PackJob::kRejected,
                 PackJob::kClaimedRaw, PackJob::kFailed}) {
    EXPECT_TRUE(DecideSubmit(st, false, true, false, busy) != SubmitAction::kDefer);
    EXPECT_TRUE(DecideSubmit(st, false, true, false, idle) != SubmitAction::kDefer);
    EXPECT_TRUE(DecideSubmit(st, true, true, false, busy) != SubmitAction::kDefer);
  }
  // a settled job is submitted as it is; a failed one is waited for (Wait rethrows)
  for (bool wait : {false, true}) {
    EXPECT_TRUE(DecideSubmit(PackJob::kPacked, wait, false, false, busy) == SubmitAction::kSubmit);
    EXPECT_TRUE(DecideSubmit(PackJob::kRejected, wait, false, false, busy) == SubmitAction::kSubmit);
    EXPECT_TRUE(DecideSubmit(PackJob::kClaimedRaw, wait, false, false, idle) == SubmitAction::kSubmit);
    EXPECT_TRUE(DecideSubmit(PackJob::kFailed, wait, false, false, busy) == SubmitAction::kWait);
  }
  // a pool that has fallen behind the link: nothing is deferred, an unstarted
  // piece goes raw at once
  EXPECT_TRUE(DecideSubmit(PackJob::kQueued, false, false, true, busy) == SubmitAction::kClaimRaw);
  EXPECT_TRUE(DecideSubmit(PackJob::kPacking, false, false, true, busy) == SubmitAction::kWait);
  EXPECT_TRUE(DecideSubmit(PackJob::kPacking, false, false, true, idle) == SubmitAction::kWait);
  EXPECT_TRUE(DecideSubmit(PackJob::kPacking, false, true, true, busy) == SubmitAction::kWait);
  EXPECT_TRUE(DecideSubmit(PackJob::kPacked, false, false, true, busy) == SubmitAction::kSubmit);
  EXPECT_TRUE(DecideSubmit(PackJob::kQueued, true, false, true, busy) == SubmitAction::kWait);
  // pack_wait: every pack is waited for and the link is not asked
  bool asked = false;
  const auto ask = [&asked]() {
    asked = true;
    return true;
  };
  EXPECT_TRUE(DecideSubmit(PackJob::kQueued, true, false, false, ask) == SubmitAction::kWait);
  EXPECT_TRUE(DecideSubmit(PackJob::kPacking, true, false, false, ask) == SubmitAction::kWait);
  EXPECT_FALSE(asked);
}

TEST(PackRanges, SubmitLoopWithABusyLink) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  // the feed's submit loop with a link that always has a copy outstanding
  // once the first piece is on it: the first piece goes raw (never pushed, as
  // in the feed), every later one is deferred until the pool has packed it
  const size_t kLookahead = 4;
  std::vector<Piece> pieces(24);
  for (size_t i = 0; i < pieces.size(); ++i) {
    pieces[i].text = Text(kRange + 5000 + 13 * i, static_cast<unsigned>(i));
    MakeJob(&pieces[i], i, -1.0);
  }
  PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
  size_t pushed = 0, raw = 0, packed = 0, inflight = 0;
  const auto link_busy = [&inflight]() { return inflight != 0; };
  for (size_t submitted = 0; submitted < pieces.size();) {
    PackJob* job = pieces[submitted].job.get();
    SubmitAction action = DecideSubmit(job->state.load(), false, inflight == 0, false, link_busy);
    const size_t first = pushed == submitted && action == SubmitAction::kClaimRaw ? 1 : 0;
    for (pushed = std::max(pushed, submitted + first);
         pushed < pieces.size() && pushed < submitted + kLookahead; ++pushed) {
      pool.Push(pieces[pushed].job.get());
    }
    if (action == SubmitAction::kDefer) {
      ASSERT_GT(inflight, size_t(0));  // deferring with nothing in flight is impossible
      std::this_thread::yield();
      continue;
    }
    EXPECT_TRUE(action == (submitted == 0 ? SubmitAction::kClaimRaw : SubmitAction::kSubmit));
    if (action == SubmitAction::kClaimRaw) {
      ASSERT_TRUE(pool.TryClaimRaw(job));
      ++raw;
    } else {
      ExpectEqualsPackText(pieces[submitted], alphabet);
      ++packed;
    }
    pool.SetSubmitted(++submitted);
    inflight = 1;
  }
  EXPECT_EQ(raw, size_t(1));
  EXPECT_EQ(packed, pieces.size() - 1);
}
