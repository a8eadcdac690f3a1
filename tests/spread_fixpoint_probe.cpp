// spread_fixpoint_probe.cpp -- the fix point of the spread's sweeps does not depend on the order in which the blocks of sources
// rescan (csrc/cg_attacker.hpp, attacker_spread_ct: the serial verification sweeps and the merged one).  A stand-alone host model,
// built with the address and undefined-behaviour sanitizers (tests/test_spread_fixpoint_probe_cpu.py).
//
// The model: sources 0 .. n-1 in id order, source i in block i / 64; a row of 1 .. 8 slots, each a target; the lowest source id
// wins a target, a loser rescans its row from behind its pick and may take what a LATER source holds.  T[v] = the lowest source
// that took v.  Sweep 0 scans two blocks at a time on the table as it stood before the group, then takes.  A verification sweep
// runs while some take hit a target that was already held: every pick is checked against the table at the START of the sweep;
//   serial: the losers of block 0 rescan and take, then those of block 1 (they see block 0's takes), then block 2;
//   merged: the losers of blocks 0 and 1 rescan on the table as it stood at the start of the sweep and take together, then block 2.
// Both must end with the picks of the definition: the sources in id order, each takes its first slot no earlier source took.
// Prints: <instances> <largest number of extra sweeps of the merged order> ok
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

constexpr int WAVE = 64, FREE = 1 << 30;

struct Inst {
  int n_targets = 0;
  std::vector<std::vector<int>> rows;   // per source: its slots (targets), in row order
};

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

// first slot >= from of source i whose target no EARLIER source holds in `table`, or the row's length
int scan(const Inst& in, int i, int from, const std::vector<int>& table) {
  const auto& row = in.rows[i];
  for (int k = from; k < (int)row.size(); ++k)
    if (table[row[k]] >= i) return k;
  return (int)row.size();
}

std::vector<int> by_definition(const Inst& in) {
  std::vector<int> T(in.n_targets, FREE), pick(in.rows.size());
  for (int i = 0; i < (int)in.rows.size(); ++i) {
    pick[i] = scan(in, i, 0, T);
    if (pick[i] < (int)in.rows[i].size()) T[in.rows[i][pick[i]]] = i;
  }
  return pick;
}

// returns the picks; sweeps = number of sweeps (sweep 0 included)
std::vector<int> run(const Inst& in, bool merged, int& sweeps) {
  const int n = (int)in.rows.size();
  std::vector<int> T(in.n_targets, FREE), pick(n);
  bool lost_any = false;
  auto take = [&](int i) {
    if (pick[i] >= (int)in.rows[i].size()) return;
    int& t = T[in.rows[i][pick[i]]];
    if (t != FREE) lost_any = true;
    t = std::min(t, i);
  };
  for (int g0 = 0; g0 < n; g0 += 2 * WAVE) {
    const std::vector<int> snap = T;
    const int g1 = std::min(n, g0 + 2 * WAVE);
    for (int i = g0; i < g1; ++i) pick[i] = scan(in, i, 0, snap);
    for (int i = g0; i < g1; ++i) take(i);
  }
  sweeps = 1;
  while (lost_any) {
    if (++sweeps > 4 * n + 8) { std::fprintf(stderr, "no fix point after %d sweeps\n", sweeps); std::exit(1); }
    lost_any = false;
    const std::vector<int> tv = T;
    std::vector<char> lost(n);
    for (int i = 0; i < n; ++i) lost[i] = pick[i] < (int)in.rows[i].size() && tv[in.rows[i][pick[i]]] < i;
    for (int b0 = 0; b0 < n;) {
      const int b1 = std::min(n, b0 + ((merged && b0 == 0) ? 2 * WAVE : WAVE));
      const std::vector<int> snap = T;
      for (int i = b0; i < b1; ++i) if (lost[i]) pick[i] = scan(in, i, pick[i] + 1, snap);
      for (int i = b0; i < b1; ++i) if (lost[i]) take(i);
      b0 = b1;
    }
  }
  return pick;
}

long g_instances = 0;
int g_extra = 0, g_fewer = 0;

void check(const Inst& in, const char* what) {
  for (const auto& r : in.rows)
    if (r.empty() || r.size() > 8) { std::fprintf(stderr, "%s: a row of %zu slots\n", what, r.size()); std::exit(1); }
  const std::vector<int> want = by_definition(in);
  int ss = 0, sm = 0;
  const std::vector<int> a = run(in, false, ss), b = run(in, true, sm);
  if (a != want || b != want) {
    std::fprintf(stderr, "%s: n = %zu: %s order differs from the definition\n", what, in.rows.size(), a != want ? "serial" : "merged");
    std::exit(1);
  }
  g_extra = std::max(g_extra, sm - ss);
  g_fewer = std::max(g_fewer, ss - sm);
  ++g_instances;
}

// `n` sources; the rows listed in `at` sit at the given indices, every other source holds a target of its own
Inst place(int n, const std::vector<std::pair<int, std::vector<int>>>& at, int n_shared) {
  Inst in;
  in.rows.assign(n, {});
  in.n_targets = n_shared + n;
  for (const auto& p : at) in.rows[p.first] = p.second;
  for (int i = 0; i < n; ++i)
    if (in.rows[i].empty()) in.rows[i] = {n_shared + i};
  return in;
}

}  // namespace

int main() {
  Rng rng{0x5eed5eedull};
  // ---- random instances: 2 .. 130 sources, rows of 1 .. 8 slots, few targets (shared) or many ----
  for (int it = 0; it < 6000; ++it) {
    Inst in;
    const int n = 2 + rng.below(129);
    in.n_targets = 1 + rng.below(it % 3 == 0 ? 6 : (it % 3 == 1 ? n : 3 * n));
    in.rows.resize(n);
    for (auto& r : in.rows) {
      const int len = 1 + rng.below(it % 5 == 0 ? 8 : 3);
      for (int k = 0; k < len; ++k) r.push_back(rng.below(in.n_targets));   // (a target may recur in a row: the second visit finds it held)
    }
    check(in, "random");
  }
  // ---- steal chains of depth 1 .. 6: s0: [c0]; s1: [c0, c1]; s2: [c1, c2]; ...: s1 loses c0 and takes c1 from s2, which takes c2 from s3 ...
  // with the members at every kind of place: all in block 0, all in block 1, one block each from some link on, the last in block 2
  for (int depth = 1; depth <= 6; ++depth)
    for (int n : {depth + 2, 64, 65, 100, 128, 129, 130})
      for (int rep = 0; rep < 40; ++rep) {
        const int m = depth + 2;   // chain members
        if (n < m) continue;
        std::vector<int> idx;   // ascending places
        if (rep == 0) for (int j = 0; j < m; ++j) idx.push_back(j);
        else if (rep == 1) for (int j = 0; j < m; ++j) idx.push_back(n - m + j);
        else if (rep < 2 + m && n > WAVE + m) { const int cut = rep - 2; for (int j = 0; j < m; ++j) idx.push_back(j < cut ? WAVE - cut + j : WAVE + (j - cut)); }
        else {
          std::vector<int> all(n);
          for (int i = 0; i < n; ++i) all[i] = i;
          for (int j = 0; j < m; ++j) { const int k = j + rng.below(n - j); std::swap(all[j], all[k]); idx.push_back(all[j]); }
          std::sort(idx.begin(), idx.end());
        }
        std::vector<std::pair<int, std::vector<int>>> at;
        at.push_back({idx[0], {0}});
        for (int j = 1; j < m; ++j) at.push_back({idx[j], {j - 1, j}});
        check(place(n, at, m), "chain");
        // the same with a third slot that two neighbours of the chain share: losers of both blocks rescan to the SAME target
        for (int j = 1; j + 1 < m; j += 2) { at[j].second = {j - 1, m, j}; at[j + 1].second = {j - 1, m, j + 1}; }
        check(place(n, at, m + 1), "chain+shared");
      }
  // ---- every source after the same few targets, rows of eight ----
  for (int n : {2, 63, 64, 65, 127, 128, 129, 130})
    for (int nt = 1; nt <= 9; ++nt) {
      Inst in;
      in.n_targets = nt;
      in.rows.resize(n);
      for (int i = 0; i < n; ++i)
        for (int k = 0; k < std::min(8, nt); ++k) in.rows[i].push_back((k + (i % 3 == 2 ? 1 : 0)) % nt);
      check(in, "crowd");
    }
  std::printf("%ld %d ok\n", g_instances, g_extra);
  std::fprintf(stderr, "(the merged order needed up to %d sweeps more and up to %d fewer than the serial one)\n", g_extra, g_fewer);
  return 0;
}
