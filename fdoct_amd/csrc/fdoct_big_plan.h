// fdoct_big_plan.h -- what the long-row path (fdoct_big.hip, run_big in fdoct_big_host.cpp) decides on the host, as values made before
// anything is enqueued: how the passes of an n-point transform are dealt to grouped launches, the radices of the one-launch-per-pass
// form, the length of the power-of-two transforms a chirp (Bluestein) transform runs around, and how a batch is cut into chunks of
// whole averaging groups that fit the workspace budget.  Plain C++ without HIP: tests/native/bigplan_check.cpp asserts the
// invariants over every length the path takes and pins the plans of the tested lengths against bigplan_check.expected.
#pragma once
#include <cstddef>
#include <vector>

namespace fdoct {

constexpr int BIG_GROUP_MAX_PASSES = 6;
constexpr int BIG_GROUP_TILE_VALUES = 2048;  // values of one workgroup's tile (sub-problems x local length): 8 per thread in registers during a pass

struct BigGroupPlan {          // one launch: a group of the transform's passes with the data in LDS (fdoct_big.h)
  int P = 1, Q = 1, F = 1, log2ts = 0;
  std::vector<int> rad;
};

// LDS of one grouped launch: Q rows of 2^log2ts sub-problems, padded by one value
inline size_t big_group_lds_bytes(int Q, int log2ts) { return (size_t)Q * ((1u << log2ts) + 1) * 8; }

// The passes of an n-point transform (n = 2^a 3^b 5^c) as a few groups, each one launch with its data in LDS: the prime
// factors are dealt to G groups so that the groups' lengths come out as equal as they can (16384 = 128 x 128, 4096 = 64 x 64),
// G the smallest count that keeps every length within what a workgroup's tile holds.
inline bool big_plan_groups(int n, std::vector<BigGroupPlan>& groups) {
  groups.clear();
  std::vector<int> primes;
  int m = n;
  for (int p : {5, 3, 2})
    while (m % p == 0) { primes.push_back(p); m /= p; }
  if (m != 1 || n < 2) return false;
  constexpr int kQmax = BIG_GROUP_TILE_VALUES / 8;   // 8 sub-problems of this many points fill the tile (64 contiguous bytes per element index)
  int G = 1;
  for (double cap = kQmax; cap < (double)n; cap *= kQmax) G++;
  for (; G <= 4; G++) {
    std::vector<long long> prod(G, 1);
    std::vector<std::vector<int>> fac(G);
    for (int p : primes) {  // largest factors first, each to the group that is shortest so far
      int best = 0;
      for (int g = 1; g < G; g++)
        if (prod[g] < prod[best]) best = g;
      prod[best] *= p;
      fac[best].push_back(p);
    }
    bool ok = true;
    for (int g = 0; g < G; g++) ok = ok && prod[g] <= BIG_GROUP_TILE_VALUES / 4;
    if (!ok) continue;
    long long P = 1;
    for (int g = 0; g < G; g++) {
      BigGroupPlan gp;
      gp.P = (int)P;
      gp.Q = (int)prod[g];
      gp.F = (int)(n / (P * prod[g]));
      int twos = 0;
      for (int p : fac[g]) {
        if (p == 2) twos++;
        else gp.rad.push_back(p);
      }
      for (; twos >= 3; twos -= 3) gp.rad.push_back(8);
      if (twos == 2) gp.rad.push_back(4);
      if (twos == 1) gp.rad.push_back(2);
      if ((int)gp.rad.size() > BIG_GROUP_MAX_PASSES || gp.rad.empty()) { ok = false; break; }
      const long long S = (long long)gp.P * gp.F;
      int l2 = 4;
      while (l2 > 0 && (((long long)gp.Q << l2) > BIG_GROUP_TILE_VALUES || (1LL << l2) > S)) l2--;
      gp.log2ts = l2;
      groups.push_back(gp);
      P *= prod[g];
    }
    if (ok) return true;
    groups.clear();
  }
  return false;
}

// Stockham radices of the one-launch-per-pass form: 5s and 3s first, then 8s, then what is left of the power of two.
// False: the length has a prime factor above 5.
inline bool big_radices(int len, std::vector<int>& rad) {
  rad.clear();
  while (len % 5 == 0) { rad.push_back(5); len /= 5; }
  while (len % 3 == 0) { rad.push_back(3); len /= 3; }
  while (len % 8 == 0) { rad.push_back(8); len /= 8; }
  if (len % 4 == 0) { rad.push_back(4); len /= 4; }
  if (len % 2 == 0) { rad.push_back(2); len /= 2; }
  return len == 1;
}

// The power of two >= 2n - 1 whose transforms a chirp (Bluestein) transform of n points runs around.
inline int big_chirp_length(int n) {
  int mb = 1;
  while (mb < 2 * n - 1) mb <<= 1;
  return mb;
}

// DFT plan of one length: Stockham radices when it factors into 2, 3, 5, else Bluestein around a power of two >= 2n - 1.
struct BigTransform {
  int tn = 0;                        // the length whose passes run: n, or mb
  int mb = 0;                        // > 0: the length has a prime factor above 5 and runs as Bluestein around two mb-point DFTs
  std::vector<int> rad;              // the one-launch-per-pass form of tn
  std::vector<BigGroupPlan> groups;  // tn as a few launches of several passes each (empty: not available, or per_pass)
};
inline BigTransform make_big_transform(int n, bool per_pass) {
  BigTransform t;
  t.tn = n;
  if (!big_radices(n, t.rad)) {
    t.mb = big_chirp_length(n);
    big_radices(t.mb, t.rad);
    t.tn = t.mb;
  }
  if (!per_pass) big_plan_groups(t.tn, t.groups);
  return t;
}

// The chunks of run_big: whole averaging groups (A frames of H rows) whose float rows of W samples and two buffers of lmax complex
// values per row fit the budget; at least one group, at most the batch's G.
constexpr size_t kBigChunkBudget = (size_t)2 << 30;
// FDOCT_BIG_CHUNK_MB as read (0 or less: the default)
inline size_t big_chunk_budget(long long mb) { return mb > 0 ? (size_t)mb << 20 : kBigChunkBudget; }
struct BigChunks {
  size_t per_group = 0;  // workspace bytes of one averaging group
  long long cg = 1;      // groups per chunk
  size_t rows = 0;       // rows of the three workspaces: cg A H
};
inline BigChunks make_big_chunks(int W, int H, int A, int G, size_t lmax, size_t budget) {
  BigChunks c;
  c.per_group = (size_t)A * H * ((size_t)W * 4 + 2 * lmax * 8);
  c.cg = (long long)(budget / c.per_group);
  if (c.cg < 1) c.cg = 1;
  if (c.cg > G) c.cg = G;
  c.rows = (size_t)c.cg * A * H;
  return c;
}

}  // namespace fdoct
