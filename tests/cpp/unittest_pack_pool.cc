/*!
 * \file tests/cpp/unittest_pack_pool.cc
 * \brief The cooperative pack pool of the packed H2D transfer
 *  (src/gpu/pack_pool.h), driven as the device parser's submit loop drives it:
 *  jobs pushed in order, then each found packed, claimed raw or waited for.
 *  Part of the ThreadSanitizer run of the suite.
 */
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../src/gpu/pack_pool.h"
#include "../../src/gpu/text_pack_codec.h"
#include "./testing.h"

namespace {

using dmlc::gpu::PackJob;
using dmlc::gpu::PackPool;

std::string Text(size_t n, unsigned seed, size_t exception_every = 0) {
  static const char kSym[] = "0123456789:. \n-e";
  std::string s(n, '0');
  unsigned x = seed * 2654435761u + 99u;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    s[i] = kSym[(x >> 24) % 16];
  }
  if (exception_every != 0) {
    for (size_t b = 0; b * 256 < n; b += exception_every) s[b * 256 + 1] = '\r';
  }
  return s;
}

struct Piece {
  std::string text;
  std::vector<uint8_t> out;
  std::unique_ptr<PackJob> job;
};

std::vector<Piece> MakePieces(size_t count, size_t n, size_t exception_every_of_odd = 0) {
  std::vector<Piece> pieces(count);
  for (size_t i = 0; i < count; ++i) {
    Piece& p = pieces[i];
    p.text = Text(n + 13 * i, static_cast<unsigned>(i), (i & 1) ? exception_every_of_odd : 0);
    p.out.assign(p.text.size() + 4096, 0xEE);
    p.job.reset(new PackJob());
    p.job->ptr = p.text.data();
    p.job->size = p.text.size();
    p.job->seq = i;
    p.job->out = p.out.data();
  }
  return pieces;
}

void ExpectRoundTrip(const Piece& p) {
  ASSERT_EQ(p.job->state.load(), static_cast<int>(PackJob::kPacked));
  const dmlc::gpu::PackedView v = dmlc::gpu::ViewPacked(p.out.data());
  ASSERT_EQ(v.header.n, p.text.size());
  EXPECT_EQ(v.bytes, p.job->packed_bytes);
  EXPECT_EQ(v.header.nexc, p.job->nexc);
  std::string back(p.text.size(), '#');
  dmlc::gpu::UnpackReference(p.out.data(), reinterpret_cast<uint8_t*>(&back[0]));
  EXPECT_TRUE(back == p.text);
}

}  // namespace

TEST(PackPool, EveryJobWaitedFor) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  // 1 MiB pieces: all four threads take a part; every 40th block of the odd
  // pieces is an exception (inside the 3/4 rule)
  std::vector<Piece> pieces = MakePieces(6, 1 << 20, 40);
  PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), /*distance=*/0);
  for (auto& p : pieces) pool.Push(p.job.get());
  for (size_t i = 0; i < pieces.size(); ++i) {
    // the submit cursor passes a job before its pack has started: with
    // distance 0 the pool must still pack it (the consumer waits, never claims)
    pool.SetSubmitted(i + 1);
    pool.Wait(pieces[i].job.get());
    ExpectRoundTrip(pieces[i]);
    EXPECT_EQ(pieces[i].job->nexc != 0, (i & 1) != 0);
  }
  EXPECT_GT(pool.pack_sec(), 0.0);
}

TEST(PackPool, RejectedWhenMostlyExceptions) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  std::vector<Piece> pieces = MakePieces(4, 300000, 1);  // odd pieces: every block
  PackPool pool(3, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
  for (auto& p : pieces) pool.Push(p.job.get());
  for (size_t i = 0; i < pieces.size(); ++i) {
    pool.Wait(pieces[i].job.get());
    if (i & 1) {
      EXPECT_EQ(pieces[i].job->state.load(), static_cast<int>(PackJob::kRejected));
    } else {
      ExpectRoundTrip(pieces[i]);
    }
  }
}

TEST(PackPool, HybridSubmitLoop) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  const size_t kLookahead = 4, kDistance = 2;
  std::vector<Piece> pieces = MakePieces(40, 70000);
  PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), kDistance);
  size_t pushed = 0, packed = 0, raw = 0;
  for (size_t submitted = 0; submitted < pieces.size();) {
    // as DeviceParserImpl::NextPackJob: fill the lookahead, pop the front
    while (pushed < pieces.size() && pushed < submitted + kLookahead) {
      if (pushed >= submitted + kDistance) pool.Push(pieces[pushed].job.get());
      ++pushed;
    }
    Piece& p = pieces[submitted];
    pool.SetSubmitted(++submitted);
    if (p.job->state.load() != PackJob::kPacked && !pool.TryClaimRaw(p.job.get())) {
      pool.Wait(p.job.get());
    }
    if (p.job->state.load() == PackJob::kPacked) {
      ExpectRoundTrip(p);
      ++packed;
    } else {
      EXPECT_EQ(p.job->state.load(), static_cast<int>(PackJob::kClaimedRaw));
      ++raw;
    }
    p.job.reset();  // the owner frees a settled job: the pool must hold no pointer to it
  }
  EXPECT_EQ(packed + raw, pieces.size());
  EXPECT_GE(raw, kDistance);  // the first pieces of a pass go raw
}

TEST(PackPool, PoolThreadErrorSurfacesInWait) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  std::vector<Piece> pieces = MakePieces(5, 65536);
  PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
  dmlc::fault::Configure("pack:2");
  for (auto& p : pieces) pool.Push(p.job.get());
  pool.SetSubmitted(pieces.size());
  pool.Wait(pieces[0].job.get());
  ExpectRoundTrip(pieces[0]);
  EXPECT_THROW(pool.Wait(pieces[1].job.get()), dmlc::Error);
  dmlc::fault::Configure("");
  pool.Quiesce();
  pieces.clear();
  std::vector<Piece> more = MakePieces(3, 65536);
  for (auto& p : more) pool.Push(p.job.get());
  for (auto& p : more) {
    pool.Wait(p.job.get());
    ExpectRoundTrip(p);
  }
}

TEST(PackPool, QuiesceDropsQueuedJobs) {
  uint8_t alphabet[16];
  dmlc::gpu::PackAlphabet(false, ',', alphabet);
  for (int round = 0; round < 5; ++round) {
    std::vector<Piece> pieces = MakePieces(8, 200000);
    PackPool pool(4, std::make_unique<dmlc::gpu::NibbleCodec>(alphabet), 0);
    for (auto& p : pieces) pool.Push(p.job.get());
    pool.Wait(pieces[0].job.get());
    pool.Quiesce();
    // nothing is read or written after Quiesce: the pieces may go away
    size_t settled = 0;
    for (auto& p : pieces) {
      const int st = p.job->state.load();
      EXPECT_TRUE(st == PackJob::kPacked || st == PackJob::kQueued);
      settled += st == PackJob::kPacked;
    }
    EXPECT_GE(settled, size_t(1));
    pieces.clear();
    // and the pool still works
    std::vector<Piece> more = MakePieces(2, 100000);
    for (auto& p : more) pool.Push(p.job.get());
    for (auto& p : more) {
      pool.Wait(p.job.get());
      ExpectRoundTrip(p);
    }
  }
}
