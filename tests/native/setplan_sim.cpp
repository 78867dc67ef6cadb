// setplan_sim.cpp -- the set planner of the receive-side host units (pybitmessage_amd/csrc/bmpow_set_plan.h) as
// a stand-alone program: tests/test_native.py builds it with g++ under AddressSanitizer + UBSan.  The limits are
// tiny (4 objects, 8 blocks of 64 bytes) so that every boundary the library only meets at 2^18 rows or 256 MB
// is met here: the fixed cases below, then 1,000 seeded random lists of at most 40 bounds in 0 .. 12, each cut
// into sets from front to back and checked for partition, limits and maximality, and compared with a naive
// restatement that shares no code with the planner (it tries every candidate end and sums it from scratch).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "bmpow_set_plan.h"

namespace {

constexpr size_t kObjects = 4;
constexpr uint64_t kPoolBlocks = 8, kPoolBytes = 64 * kPoolBlocks;

int g_fail = 0;

#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                     \
      std::fprintf(stderr, "\n");                            \
      ++g_fail;                                              \
    }                                                        \
  } while (0)

struct Row {  // as the host units' items: the planner reads the bound through the accessor only
  uint32_t orig;
  uint32_t bound;
};

std::vector<Row> rows_of(const std::vector<uint32_t>& bounds) {
  std::vector<Row> rows;
  for (size_t i = 0; i < bounds.size(); ++i) rows.push_back({(uint32_t)i, bounds[i]});
  return rows;
}

bmhost::SetCut cut_at(const std::vector<Row>& rows, size_t i0) {
  return bmhost::plan_set(rows, i0, [](const Row& r) { return r.bound; }, kObjects, kPoolBytes);
}

// The rule restated: the longest [i0, end) of at most kObjects rows whose blocks, summed anew for every
// candidate, fit the pool -- and one row where not even that fits.
size_t naive_end(const std::vector<uint32_t>& bounds, size_t i0, uint64_t& blocks) {
  size_t best = i0;
  blocks = 0;
  for (size_t end = i0 + 1; end <= bounds.size() && end - i0 <= kObjects; ++end) {
    uint64_t sum = 0;
    for (size_t i = i0; i < end; ++i) sum += bounds[i];
    if (sum > kPoolBlocks) break;  // bounds are not negative: no longer candidate fits either
    best = end;
    blocks = sum;
  }
  if (best == i0 && i0 < bounds.size()) {
    best = i0 + 1;
    blocks = bounds[i0];
  }
  return best;
}

struct Set {
  size_t i0, i1;
  uint64_t blocks;
};

std::vector<Set> all_sets(const std::vector<Row>& rows) {
  std::vector<Set> sets;
  size_t i0 = 0;
  while (i0 < rows.size()) {
    const bmhost::SetCut c = cut_at(rows, i0);
    sets.push_back({i0, c.i1, c.blocks});
    if (c.i1 <= i0) break;  // no progress: the checks below report it
    i0 = c.i1;
  }
  return sets;
}

void expect_sets(const char* name, const std::vector<uint32_t>& bounds, const std::vector<Set>& want) {
  const std::vector<Set> got = all_sets(rows_of(bounds));
  CHECK(got.size() == want.size(), "%s: %zu sets, want %zu", name, got.size(), want.size());
  for (size_t k = 0; k < got.size() && k < want.size(); ++k)
    CHECK(got[k].i0 == want[k].i0 && got[k].i1 == want[k].i1 && got[k].blocks == want[k].blocks,
          "%s: set %zu is [%zu, %zu) of %llu blocks, want [%zu, %zu) of %llu", name, k, got[k].i0, got[k].i1,
          (unsigned long long)got[k].blocks, want[k].i0, want[k].i1, (unsigned long long)want[k].blocks);
}

void fixed_cases() {
  {  // an empty range: the cut is empty, wherever it starts
    const std::vector<Row> none;
    const bmhost::SetCut c = cut_at(none, 0);
    CHECK(c.i1 == 0 && c.blocks == 0, "empty range: [0, %zu) of %llu blocks", c.i1, (unsigned long long)c.blocks);
    const std::vector<Row> two = rows_of({1, 1});
    const bmhost::SetCut e = cut_at(two, 2);
    CHECK(e.i1 == 2 && e.blocks == 0, "cut at the end: [2, %zu) of %llu blocks", e.i1, (unsigned long long)e.blocks);
  }
  // a first row above the pool on its own: a set of one, its blocks reported as they are
  expect_sets("over-limit first row", {9, 1, 1}, {{0, 1, 9}, {1, 3, 2}});
  expect_sets("over-limit row alone", {12}, {{0, 1, 12}});
  expect_sets("over-limit rows in a row", {12, 9, 8}, {{0, 1, 12}, {1, 2, 9}, {2, 3, 8}});
  // an exact fill: 8 blocks are taken whole, the ninth block starts the next set
  expect_sets("exact fill", {4, 3, 1, 1}, {{0, 3, 8}, {3, 4, 1}});
  expect_sets("exact fill by one row", {8, 1}, {{0, 1, 8}, {1, 2, 1}});
  expect_sets("one block over", {4, 3, 2}, {{0, 2, 7}, {2, 3, 2}});
  // the object limit first: four rows although the pool has room
  expect_sets("object limit first", {1, 1, 1, 1, 1}, {{0, 4, 4}, {4, 5, 1}});
  expect_sets("both limits at once", {2, 2, 2, 2, 2}, {{0, 4, 8}, {4, 5, 2}});
  // rows of bound 0 take no pool but count as objects
  expect_sets("zero bounds", {0, 0, 0, 0, 0, 0}, {{0, 4, 0}, {4, 6, 0}});
  expect_sets("zeros behind a full pool", {8, 0, 0, 0, 0}, {{0, 4, 8}, {4, 5, 0}});
  expect_sets("zeros behind an over-limit row", {9, 0, 0}, {{0, 1, 9}, {1, 3, 0}});
}

void random_lists() {
  std::mt19937_64 rng(0x5e7c0de5ull);
  for (int round = 0; round < 1000; ++round) {
    std::vector<uint32_t> bounds(rng() % 41);
    for (uint32_t& b : bounds) b = (uint32_t)(rng() % 13);
    const std::vector<Row> rows = rows_of(bounds);
    const std::vector<Set> sets = all_sets(rows);
    size_t at = 0;
    for (const Set& s : sets) {
      // the sets partition the range, in order
      CHECK(s.i0 == at && s.i1 > s.i0 && s.i1 <= bounds.size(), "round %d: set [%zu, %zu) behind %zu", round, s.i0, s.i1, at);
      if (s.i1 <= s.i0 || s.i1 > bounds.size()) break;
      at = s.i1;
      uint64_t sum = 0;
      for (size_t i = s.i0; i < s.i1; ++i) sum += bounds[i];
      CHECK(sum == s.blocks, "round %d: set [%zu, %zu) reports %llu blocks, has %llu", round, s.i0, s.i1,
            (unsigned long long)s.blocks, (unsigned long long)sum);
      // within both limits, but for a singleton that its first row forced
      const size_t count = s.i1 - s.i0;
      const bool forced = bounds[s.i0] > kPoolBlocks;
      CHECK(count <= kObjects, "round %d: set [%zu, %zu) above the object limit", round, s.i0, s.i1);
      if (forced) CHECK(count == 1, "round %d: set [%zu, %zu) goes on behind an over-limit row", round, s.i0, s.i1);
      else CHECK(sum <= kPoolBlocks, "round %d: set [%zu, %zu) of %llu blocks", round, s.i0, s.i1, (unsigned long long)sum);
      // maximal: the next row would not have fitted
      if (s.i1 < bounds.size())
        CHECK(count == kObjects || sum + bounds[s.i1] > kPoolBlocks, "round %d: set [%zu, %zu) stops early", round, s.i0, s.i1);
      // and what the naive restatement says
      uint64_t nblocks = 0;
      const size_t nend = naive_end(bounds, s.i0, nblocks);
      CHECK(nend == s.i1 && nblocks == s.blocks, "round %d: from %zu the planner ends at %zu (%llu), the naive cut at %zu (%llu)",
            round, s.i0, s.i1, (unsigned long long)s.blocks, nend, (unsigned long long)nblocks);
    }
    CHECK(at == bounds.size(), "round %d: the sets end at %zu of %zu", round, at, bounds.size());
  }
}

}  // namespace

int main() {
  fixed_cases();
  random_lists();
  if (g_fail) {
    std::fprintf(stderr, "%d set planner checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all set planner checks passed\n");
  return 0;
}
