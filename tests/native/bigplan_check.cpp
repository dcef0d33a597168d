// Checks the long-row path's host-side decisions (fdoct_amd/csrc/fdoct_big_plan.h) and prints a table of them.  Host-only: no GPU
// and no library needed.
//
// Invariants, asserted for every length 2^a 3^b 5^c from 2 to 2^24 (any failure is printed to stderr and the exit status is 1):
// a grouped plan exists; the groups' Q multiply to n and P Q F = n in each, P the product of the earlier Q; Q <= TILE / 4,
// Q << log2ts <= TILE, 1 << log2ts <= P F; 1 .. MAX_PASSES radices that multiply to Q; the LDS of a launch is at most 64 KB; the
// group count is 1 up to 256 points, 2 up to 65 536, 3 beyond (4 where the factors cannot be dealt to 3 groups within TILE / 4).  For the chunks of a batch, over a grid of geometries, batch sizes
// and budgets: 1 <= cg <= G, the chunks cover G exactly, the workspaces hold cg A H rows, and cg is the largest count that fits the
// budget (or 1).
//
// Table (tests/test_abi.py compares it with bigplan_check.expected; tests/test_gpu_long_rows.py reads the claims about its cases
// from it): for every transform length the GPU tests of the long-row path run -- kLengths below --, grouped or chirp (Bluestein)
// and around which power of two, the launches of one transform, and per launch P Q F log2ts, the radices and whether the last
// tile of a row is short; for the chunk grid of those tests, the bytes of a group, cg, the rows and the chunk sequence.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "fdoct_big_plan.h"

using namespace fdoct;

static int g_failures = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      if (g_failures++ < 20) {                                 \
        std::fprintf(stderr, "FAILED %s: ", #cond);            \
        std::fprintf(stderr, __VA_ARGS__);                     \
        std::fprintf(stderr, "\n");                            \
      }                                                        \
    }                                                          \
  } while (0)

// every transform length of tests/test_gpu_long_rows.py (its CPU test asserts that none is missing)
static const int kLengths[] = {
    // three-launch transforms and the lengths next to them in their cases
    131072, 78125, 65610, 98304, 16384, 8192, 96000, 3000, 57344, 34816, 4480, 35840, 4096,
    // the hand-over matrix
    56, 64, 224, 243, 250, 256, 448, 1000, 1001, 1024,
    // chunked batches
    512, 32768,
    // the per-pass form
    640, 2560,
};

// can the prime factors of n be dealt to G groups of at most TILE / 4 points each?  (every divisor tried as the first group)
static bool can_deal(long long n, int G) {
  if (G == 1) return n <= BIG_GROUP_TILE_VALUES / 4;
  for (long long q = 1; q <= BIG_GROUP_TILE_VALUES / 4; q++)
    if (n % q == 0 && can_deal(n / q, G - 1)) return true;
  return false;
}

static void check_groups(int n) {
  std::vector<BigGroupPlan> gs;
  const bool ok = big_plan_groups(n, gs);
  CHECK(ok && !gs.empty(), "n=%d has no grouped plan", n);
  if (!ok) return;
  long long prodq = 1;
  for (const BigGroupPlan& g : gs) {
    CHECK(g.P == prodq, "n=%d P=%d", n, g.P);
    CHECK((long long)g.P * g.Q * g.F == n, "n=%d P Q F = %d %d %d", n, g.P, g.Q, g.F);
    CHECK(g.Q <= BIG_GROUP_TILE_VALUES / 4, "n=%d Q=%d", n, g.Q);
    CHECK(((long long)g.Q << g.log2ts) <= BIG_GROUP_TILE_VALUES, "n=%d Q=%d log2ts=%d", n, g.Q, g.log2ts);
    CHECK(g.log2ts >= 0 && (1LL << g.log2ts) <= (long long)g.P * g.F, "n=%d log2ts=%d S=%lld", n, g.log2ts, (long long)g.P * g.F);
    CHECK(!g.rad.empty() && (int)g.rad.size() <= BIG_GROUP_MAX_PASSES, "n=%d passes=%zu", n, g.rad.size());
    long long q = 1;
    for (int r : g.rad) {
      CHECK(r == 2 || r == 3 || r == 4 || r == 5 || r == 8, "n=%d radix %d", n, r);
      q *= r;
    }
    CHECK(q == g.Q, "n=%d radices multiply to %lld, Q=%d", n, q, g.Q);
    CHECK(big_group_lds_bytes(g.Q, g.log2ts) <= 64 * 1024, "n=%d LDS %zu", n, big_group_lds_bytes(g.Q, g.log2ts));
    prodq *= g.Q;
  }
  CHECK(prodq == n, "n=%d product of Q = %lld", n, prodq);
  // one group up to 256 points, two up to 65 536, three beyond -- or one more where no dealing of the factors into that many groups
  // keeps every Q within TILE / 4 (5^10 = 9 765 625: three groups hold 5^9 at most)
  const size_t want = n <= 256 ? 1 : n <= 65536 ? 2 : 3;
  CHECK(gs.size() == want || (gs.size() == want + 1 && !can_deal(n, (int)want)), "n=%d has %zu groups, the smallest count is %zu", n, gs.size(), want);
  // the one-launch-per-pass form of the same length
  std::vector<int> rad;
  CHECK(big_radices(n, rad), "n=%d: no radices", n);
  long long q = 1;
  for (int r : rad) q *= r;
  CHECK(q == n, "n=%d: radices multiply to %lld", n, q);
}

static std::string chunk_sequence(const BigChunks& c, int G) {
  std::string s;
  for (long long g0 = 0; g0 < G; g0 += c.cg) s += (s.empty() ? "" : ",") + std::to_string(std::min<long long>(c.cg, G - g0));
  return s;
}

static void check_chunks(int W, int H, int A, int G, size_t lmax, size_t budget) {
  const BigChunks c = make_big_chunks(W, H, A, G, lmax, budget);
  const size_t per_group = (size_t)A * H * ((size_t)W * 4 + 2 * lmax * 8);
  CHECK(c.per_group == per_group, "per_group %zu", c.per_group);
  CHECK(c.cg >= 1 && c.cg <= G, "cg=%lld G=%d", c.cg, G);
  CHECK(c.rows == (size_t)c.cg * A * H, "rows=%zu", c.rows);
  // the largest count within the budget, or the clamps
  CHECK(c.cg == 1 || (size_t)c.cg * per_group <= budget, "cg=%lld exceeds the budget %zu", c.cg, budget);
  CHECK(c.cg == G || (size_t)(c.cg + 1) * per_group > budget, "cg=%lld wastes the budget %zu", c.cg, budget);
  long long covered = 0, chunks = 0;
  for (long long g0 = 0; g0 < G; g0 += c.cg) {
    const long long ng = std::min<long long>(c.cg, G - g0);
    CHECK(ng >= 1 && ng <= c.cg && g0 == covered, "chunk at %lld of %lld", g0, ng);
    covered += ng, chunks++;
  }
  CHECK(covered == G && chunks == (G + c.cg - 1) / c.cg, "chunks cover %lld of %d", covered, G);
}

static std::string list(const std::vector<int>& v) {
  std::string s;
  for (int x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
  return s;
}

static void print_length(int n) {
  const BigTransform t = make_big_transform(n, false);
  if (t.mb)
    std::printf("n=%d chirp mb=%d launches=%zu", n, t.mb, t.groups.size());
  else
    std::printf("n=%d grouped launches=%zu", n, t.groups.size());
  for (const BigGroupPlan& g : t.groups) {
    const long long S = (long long)g.P * g.F;
    std::printf(" | P=%d Q=%d F=%d log2ts=%d rad=%s tail=%s", g.P, g.Q, g.F, g.log2ts, list(g.rad).c_str(), S % (1LL << g.log2ts) ? "short" : "full");
  }
  std::printf(" | per-pass=%s\n", list(t.rad).c_str());
  // a chirp transform runs around a length that has a grouped plan, long enough for the convolution
  if (t.mb) CHECK(t.mb >= 2 * n - 1 && t.mb / 2 < 2 * n - 1 && (t.mb & (t.mb - 1)) == 0 && !t.groups.empty(), "n=%d mb=%d", n, t.mb);
  CHECK(make_big_transform(n, true).groups.empty() && make_big_transform(n, true).rad == t.rad, "n=%d: the per-pass form", n);
}

// the values per row of a geometry's buffers, as run_big takes them from its transforms' plans
static size_t row_values(int W, int M, int N) {
  const int MW = W + 2 * ((W * M - W) / 2);
  size_t lmax = (size_t)std::max(N, M > 1 ? MW : 0);
  for (int n : {N, M > 1 ? W : 0, M > 1 ? MW : 0})
    if (n) lmax = std::max(lmax, (size_t)make_big_transform(n, false).tn);
  return lmax;
}

static void print_chunks(int W, int M, int N, int H, int A, int G, long long mb) {
  const size_t lmax = row_values(W, M, N);
  const BigChunks c = make_big_chunks(W, H, A, G, lmax, big_chunk_budget(mb));
  std::printf("chunks W=%d M=%d N=%d H=%d A=%d G=%d mb=%lld: lmax=%zu per_group=%zu cg=%lld rows=%zu seq=%s\n", W, M, N, H, A, G, mb, lmax, c.per_group,
              c.cg, c.rows, chunk_sequence(c, G).c_str());
  check_chunks(W, H, A, G, lmax, big_chunk_budget(mb));
}

int main() {
  // ---- invariants of the grouped plans
  long long lengths = 0;
  for (long long p5 = 1; p5 <= (1 << 24); p5 *= 5)
    for (long long p3 = p5; p3 <= (1 << 24); p3 *= 3)
      for (long long n = p3; n <= (1 << 24); n *= 2)
        if (n >= 2) check_groups((int)n), lengths++;
  {  // lengths with another prime factor have none; they run around a power of two
    std::vector<BigGroupPlan> gs;
    for (int n : {1, 7, 14, 77, 8191, 2 * 8191, 57344}) CHECK(!big_plan_groups(n, gs) && gs.empty(), "n=%d has a grouped plan", n);
    for (int n = 2; n <= 5000; n++) {
      const BigTransform t = make_big_transform(n, false);
      CHECK(!t.groups.empty() && t.tn == (t.mb ? t.mb : n) && (!t.mb || t.mb >= 2 * n - 1), "n=%d: tn=%d mb=%d", n, t.tn, t.mb);
    }
  }
  // ---- invariants of the chunks
  CHECK(big_chunk_budget(0) == ((size_t)2 << 30) && big_chunk_budget(-5) == ((size_t)2 << 30) && big_chunk_budget(3) == ((size_t)3 << 20), "budget");
  for (int W : {64, 2048, 16384})
    for (int H : {1, 3, 500})
      for (int A : {1, 2, 3})
        for (int G : {1, 2, 5, 64, 1001})
          for (size_t lmax : {(size_t)256, (size_t)65536, (size_t)1 << 24}) {
            const size_t pg = (size_t)A * H * ((size_t)W * 4 + 2 * lmax * 8);
            for (size_t budget : {(size_t)1, (size_t)1 << 20, pg - 1, pg, pg + 1, 2 * pg - 1, 2 * pg, 3 * pg, 5 * pg, (size_t)2 << 30, (size_t)1 << 40})
              check_chunks(W, H, A, G, lmax, budget);
          }
  // ---- the table
  std::printf("lengths 2^a 3^b 5^c from 2 to 2^24 checked: %lld\n", lengths);
  std::set<int> seen;
  for (int n : kLengths)
    if (seen.insert(n).second) print_length(n);
  // tests/test_gpu_long_rows.py's chunked batches: five groups, the default budget, one that holds two groups, one below a group
  for (long long mb : {0LL, 4LL, 1LL}) {
    print_chunks(512, 8, 16384, 3, 2, 5, mb);
    print_chunks(512, 8, 32768, 3, 1, 5, mb);
  }
  // a group of 6 MB, and the default budget at work on 500-row frames of 4096 samples upsampled x16 to 65536 points
  for (long long mb : {0LL, 13LL, 1LL}) print_chunks(2048, 8, 65536, 3, 2, 5, mb);
  for (int G : {1, 2, 3, 7}) print_chunks(4096, 16, 8192, 500, 2, G, 0);
  if (g_failures) {
    std::fprintf(stderr, "%d checks failed\n", g_failures);
    return 1;
  }
  return 0;
}
