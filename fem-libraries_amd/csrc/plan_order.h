// LDS add order of one 16-lane quarter of a table gather (fa_plan_order, k_order_slots), as plain
// host / device code so that a stand-alone host program can test it (tests/test_plan_order_host.py).
//
// Model: every lane of a quarter adds its NBG blocks one per step; the 64-bit LDS op
// serves the quarter's lanes whose block slots agree mod 16 (the residue) one after the other, so a
// step costs as many passes as its fullest residue holds lanes (same-slot lanes count as distinct).
// The order assigns each lane's blocks to the NBG steps; passes = sum over steps of the largest
// residue count. Bound per quarter: max(NBG, largest residue total).
//
// That assignment is an edge colouring of the bipartite multigraph lanes x residues (one edge per
// block) with NBG colours in which every lane sees each colour once. De Werra's theorem: an equitable
// colouring exists, every residue of total d seeing each colour floor(d / NBG) or ceil(d / NBG) times.
// order_equitable builds one by balancing colour pairs (each pair's subgraph is oriented along Euler
// trails); where no residue total exceeds NBG it has exactly NBG passes, the optimum. Elsewhere the
// theorem does not say on which steps a residue gets its ceil: order_align moves the ceil-steps of
// over-full residues onto common steps by alternating-path (Kempe) swaps of two colours. It lowers
// the passes of any order; order_quarter runs it on the earlier pairwise descent's order (measured:
// fewer passes than from the equitable colouring, and never more than the descent alone) and, when
// asked for two starts, on the equitable colouring as well, keeping the better.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PO_HD __host__ __device__
#else
#define PO_HD
#endif

namespace plan_order {

constexpr int kLanes = 16, kRes = 16;
// the earlier search's chain length (lanes per alternating path)
constexpr int kChainLen = 6;
// order_align: sweeps over the colour pairs
constexpr int kAlignSweeps = 2;  // (4 sweeps: 0.02 % fewer passes on the 16^3 P2 cube)

// One quarter's state. st[q][t]: what lane q adds at step t, residue | block << 4 (NBG <= 16). The
// caller sets st[q][k] = residue of block k | k << 4 for lanes 0 .. nl-1 (the identity order) and
// reads the order back as st[q][t] >> 4. A kernel keeps one per thread in LDS.
template <int NBG>
struct Quarter {
  uint8_t st[kLanes][NBG];
  uint8_t keep[kLanes][NBG];  // the first order while the second is computed
  uint8_t cnt[NBG][kRes];     // lanes per (step, residue)
  uint8_t mx[NBG], nmx[NBG];  // a step's largest count, and how many residues reach it
  uint8_t aux[kRes];          // trail degrees / path parents
};

template <int NBG>
PO_HD inline int res_at(const Quarter<NBG>& S, int q, int t) { return S.st[q][t] & 15; }
template <int NBG>
PO_HD inline int block_at(const Quarter<NBG>& S, int q, int t) { return S.st[q][t] >> 4; }

template <int NBG>
PO_HD inline void recount(Quarter<NBG>& S, int t) {
  int m = 0, n = 0;
  for (int r = 0; r < kRes; ++r) {
    const int v = S.cnt[t][r];
    if (v > m) { m = v; n = 1; } else if (v == m) ++n;
  }
  S.mx[t] = (uint8_t)m;
  S.nmx[t] = (uint8_t)n;
}

// counts of step t from the picks
template <int NBG>
PO_HD inline void tally(Quarter<NBG>& S, int nl, int t) {
  for (int r = 0; r < kRes; ++r) S.cnt[t][r] = 0;
  for (int q = 0; q < nl; ++q) ++S.cnt[t][res_at(S, q, t)];
  recount(S, t);
}

// identity order: block t at step t (every lane's entries sorted by block), and the counts
template <int NBG>
PO_HD inline void reset(Quarter<NBG>& S, int nl) {
  for (int q = 0; q < nl; ++q)
    for (int t = 0; t < NBG; ++t)
      while (block_at(S, q, t) != t) {
        const int k = block_at(S, q, t);
        if (k >= NBG || block_at(S, q, k) == k) break;  // (not a permutation of the blocks: the caller's error)
        const uint8_t x = S.st[q][t];
        S.st[q][t] = S.st[q][k];
        S.st[q][k] = x;
      }
  for (int t = 0; t < NBG; ++t) tally(S, nl, t);
}

template <int NBG>
PO_HD inline int passes(const Quarter<NBG>& S) {
  int p = 0;
  for (int t = 0; t < NBG; ++t) p += S.mx[t];
  return p;
}

// max(NBG, largest residue total) (0 for an empty quarter)
template <int NBG>
PO_HD inline int bound(const Quarter<NBG>& S, int nl) {
  if (nl <= 0) return 0;
  int m = NBG;
  for (int r = 0; r < kRes; ++r) {
    int d = 0;
    for (int t = 0; t < NBG; ++t) d += S.cnt[t][r];
    if (d > m) m = d;
  }
  return m;
}

// lane q swaps its blocks of steps t1 and t2
template <int NBG>
PO_HD inline void swap_pick(Quarter<NBG>& S, int q, int t1, int t2) {
  const int ra = res_at(S, q, t1), rb = res_at(S, q, t2);
  --S.cnt[t1][ra]; ++S.cnt[t1][rb]; --S.cnt[t2][rb]; ++S.cnt[t2][ra];
  const uint8_t x = S.st[q][t1];
  S.st[q][t1] = S.st[q][t2];
  S.st[q][t2] = x;
}
template <int NBG>
PO_HD inline void swap_recount(Quarter<NBG>& S, int q, int t1, int t2) {
  swap_pick(S, q, t1, t2);
  recount(S, t1);
  recount(S, t2);
}

// new maximum of step t after one add moves from a residue of count co to one of count cn
template <int NBG>
PO_HD inline int moved_max(const Quarter<NBG>& S, int t, int co, int cn) {
  const int m = S.mx[t];
  if (cn + 1 > m) return cn + 1;
  if (co == m && S.nmx[t] == 1 && cn + 1 < m) return m - 1;
  return m;
}

// ---- the earlier heuristic: pairwise descent, and the opt-in chain search ----------------------

// pairwise step swaps per lane until none lowers the passes (tie-break: sum of squared counts)
template <int NBG>
PO_HD inline void descend(Quarter<NBG>& S, int nl) {
  for (int pass = 0; pass < 32; ++pass) {
    bool improved = false;
    for (int q = 0; q < nl; ++q)
      for (int t1 = 0; t1 < NBG; ++t1)
        for (int t2 = t1 + 1; t2 < NBG; ++t2) {
          const int ra = res_at(S, q, t1), rb = res_at(S, q, t2);
          if (ra == rb) continue;
          const int a1 = S.cnt[t1][ra], b1 = S.cnt[t1][rb], a2 = S.cnt[t2][ra], b2 = S.cnt[t2][rb];
          // step t1: ra -> rb; step t2: rb -> ra
          const int d = moved_max(S, t1, a1, b1) + moved_max(S, t2, b2, a2) - S.mx[t1] - S.mx[t2];
          const int sq = 2 * (b1 - a1) + 2 + 2 * (a2 - b2) + 2;
          if (d < 0 || (d == 0 && sq < 0)) {
            swap_recount(S, q, t1, t2);
            improved = true;
          }
        }
    if (!improved) break;
  }
}

// identity start, descent, then `rounds` rounds of alternating-path chains between two steps: a lane
// on a residue that two lanes hit at step t1 swaps its blocks of steps t1 and t2; the residue it
// brings to t1 may collide there with another lane, which swaps too, and so on (at most kChainLen
// lanes). A chain is kept when the two steps' passes drop, otherwise undone; then the descent again.
template <int NBG>
PO_HD inline void search_chains(Quarter<NBG>& S, int nl, int rounds) {
  if (NBG < 2) return;
  for (int round = 0; round < rounds; ++round) {
    bool improved = false;
    for (int t1 = 0; t1 < NBG; ++t1) {
      for (int r = 0; r < kRes; ++r) {
        if (S.cnt[t1][r] < 2) continue;
        int q0 = -1;
        for (int q = 0; q < nl; ++q)
          if (res_at(S, q, t1) == r) { q0 = q; break; }
        bool done = false;
        for (int t2 = 0; t2 < NBG && !done; ++t2) {
          if (t2 == t1) continue;
          const int before = S.mx[t1] + S.mx[t2];
          uint32_t used = 0;
          uint64_t path = 0;  // 4 bits per lane of the chain
          int len = 0;
          int q = q0;
          while (true) {
            swap_recount(S, q, t1, t2);
            path |= (uint64_t)q << (4 * len);
            ++len;
            used |= 1u << q;
            const int rn = res_at(S, q, t1);  // brought from t2
            if (S.cnt[t1][rn] < 2 || len == kChainLen) break;
            int qn = -1;
            for (int qq = 0; qq < nl && qn < 0; ++qq)
              if (!((used >> qq) & 1) && res_at(S, qq, t1) == rn) qn = qq;
            if (qn < 0) break;
            q = qn;
          }
          if (S.mx[t1] + S.mx[t2] < before) {
            done = improved = true;
          } else {
            for (int l = len - 1; l >= 0; --l) swap_recount(S, (int)((path >> (4 * l)) & 15), t1, t2);
          }
        }
        if (done) break;  // counts changed: rescan from the next step
      }
    }
    if (!improved) break;
    descend(S, nl);
  }
}
template <int NBG>
PO_HD inline void order_descent(Quarter<NBG>& S, int nl, int rounds) {
  reset(S, nl);
  descend(S, nl);
  search_chains(S, nl, rounds);
}

// ---- the exact order ----------------------------------------------------------------------------

// Steps a and b: every lane is an edge between the residues of its two blocks; orient the edges along
// Euler trails (odd-degree residues first, so each ends at most one trail) and give the tail the
// a-block. Every residue then has as many a- as b-blocks, to within one.
template <int NBG>
PO_HD inline void balance_pair(Quarter<NBG>& S, int nl, int a, int b) {
  uint32_t unused = 0;
  for (int r = 0; r < kRes; ++r) S.aux[r] = 0;
  for (int q = 0; q < nl; ++q) {
    const int u = res_at(S, q, a), v = res_at(S, q, b);
    if (u == v) continue;  // a loop: one of each whichever way
    unused |= 1u << q;
    ++S.aux[u];
    ++S.aux[v];
  }
  while (unused) {
    int cur = -1;
    for (int r = 0; r < kRes; ++r)
      if (S.aux[r] & 1) { cur = r; break; }
    if (cur < 0) cur = res_at(S, __builtin_ctz(unused), a);
    while (S.aux[cur] > 0) {
      int q = -1;
      bool tail = true;
      for (uint32_t m = unused; m; m &= m - 1) {
        const int qq = __builtin_ctz(m);
        const bool ta = res_at(S, qq, a) == cur;
        if (ta || res_at(S, qq, b) == cur) { q = qq; tail = ta; break; }
      }
      if (q < 0) break;  // (not reached: aux counts the unused edges at cur)
      if (!tail) {
        const uint8_t x = S.st[q][a];
        S.st[q][a] = S.st[q][b];
        S.st[q][b] = x;
      }
      unused &= ~(1u << q);
      --S.aux[cur];
      cur = res_at(S, q, b);
      --S.aux[cur];
    }
  }
  tally(S, nl, a);
  tally(S, nl, b);
}

// Equitable colouring from the current order: balance every pair of steps in which some residue's
// counts differ by two or more, until none does. Each balancing lowers the sum of squared counts, so
// the loop ends; the cap is a guard only.
template <int NBG>
PO_HD inline void equitable(Quarter<NBG>& S, int nl) {
  for (int sweep = 0; sweep < 64; ++sweep) {
    bool changed = false;
    for (int a = 0; a < NBG; ++a)
      for (int b = a + 1; b < NBG; ++b) {
        bool off = false;
        for (int r = 0; r < kRes && !off; ++r) {
          const int d = (int)S.cnt[a][r] - (int)S.cnt[b][r];
          off = d > 1 || d < -1;
        }
        if (off) {
          balance_pair(S, nl, a, b);
          changed = true;
        }
      }
    if (!changed) break;
  }
}
template <int NBG>
PO_HD inline void order_equitable(Quarter<NBG>& S, int nl) {
  reset(S, nl);
  equitable(S, nl);
}

// step t after one add moves from residue ro to rn: its new maximum m and the residues n that
// reach it; false when the maximum drops (a recount tells n)
template <int NBG>
PO_HD inline bool moved(const Quarter<NBG>& S, int t, int ro, int rn, int& m, int& n) {
  const int co = S.cnt[t][ro], cn = S.cnt[t][rn];
  m = S.mx[t];
  n = S.nmx[t];
  if (cn + 1 > m) { m = cn + 1; n = 1; return true; }
  n += (cn + 1 == m ? 1 : 0) - (co == m ? 1 : 0);
  return n > 0;
}

// what the alignment minimises over two steps: passes first, then (steps that conflict at all) the
// more residues share a step's maximum the better, so that ceil-steps of different residues meet
template <int NBG>
PO_HD inline int align_cost(const Quarter<NBG>& S, int a, int b) {
  const int wa = S.mx[a] >= 2 ? S.nmx[a] * S.nmx[a] : 0, wb = S.mx[b] >= 2 ? S.nmx[b] * S.nmx[b] : 0;
  return 1024 * (S.mx[a] + S.mx[b]) - wa - wb;
}

// Kempe swaps on an order. In steps (a, b) a lane is an arc from its a-block's residue to its
// b-block's; swapping the lanes of a directed path u -> v moves one a-block from u to v and one
// b-block from v to u and leaves the residues between as they were. u is a residue at step a's
// maximum with a ceil there (more a- than b-blocks), v one with a ceil at b: an equitable order stays
// equitable. A swap is kept when it lowers align_cost, so the passes never rise. kAlignSweeps sweeps
// over the ordered pairs (a, b) and the residues u, fewer when a sweep changes nothing or the passes
// reach `target`.
// The sweep is one flat scan for the next (a, b, u) that passes the cheap tests, and the costly part
// (candidates, path search, swap) after that scan: threads of a wave that each order their own
// quarter meet there, instead of each waiting through the others' triples.
template <int NBG>
PO_HD inline void order_align(Quarter<NBG>& S, int nl, int target) {
  if (NBG < 2) return;
  constexpr int kEnd = NBG * NBG * kRes;
  for (int sweep = 0; sweep < kAlignSweeps; ++sweep) {
    bool improved = false;
    int idx = 0;
    while (true) {
      int a = 0, b = 0, u = 0;
      for (; idx < kEnd; ++idx) {
        a = idx / (NBG * kRes);
        b = (idx / kRes) % NBG;
        u = idx % kRes;
        if (b == a || S.mx[a] < 2) {
          idx |= kRes - 1;  // no u of this pair
          continue;
        }
        if (S.cnt[a][u] == S.mx[a] && S.cnt[a][u] > S.cnt[b][u]) break;
      }
      if (idx >= kEnd) break;
      ++idx;
      // the residues v whose swap with u would lower the cost (predicted from the counts; a step
      // whose maximum would drop needs a recount and counts as a candidate)
      const int before = align_cost(S, a, b);
      uint32_t cand = 0;
      for (int v = 0; v < kRes; ++v) {
        if (v == u || S.cnt[b][v] <= S.cnt[a][v]) continue;
        int ma, na, mb, nb;
        const bool ka = moved(S, a, u, v, ma, na), kb = moved(S, b, v, u, mb, nb);
        if (!ka || !kb || 1024 * (ma + mb) - (ma >= 2 ? na * na : 0) - (mb >= 2 ? nb * nb : 0) < before)
          cand |= 1u << v;
      }
      if (!cand) continue;
      // breadth-first over the arcs from u until a candidate is reached: aux[v] = the lane that
      // reached v
      uint32_t vis = 1u << u, front = 1u << u;
      while (front && !(vis & cand)) {
        uint32_t next = 0;
        for (int q = 0; q < nl; ++q) {
          if (!((front >> res_at(S, q, a)) & 1)) continue;
          const int w = res_at(S, q, b);
          if ((vis >> w) & 1) continue;
          vis |= 1u << w;
          next |= 1u << w;
          S.aux[w] = (uint8_t)q;
        }
        front = next;
      }
      for (uint32_t m = vis & cand; m; m &= m - 1) {
        const int v = __builtin_ctz(m);
        // swap the path's lanes from v back to u (aux is not touched by the swaps)
        for (int w = v; w != u;) {
          const int q = S.aux[w];
          w = res_at(S, q, a);
          swap_pick(S, q, a, b);
        }
        recount(S, a);
        recount(S, b);
        if (align_cost(S, a, b) < before) {
          improved = true;
          break;  // counts changed: the tree is stale
        }
        // undo: the same lanes, now pointing the other way
        for (int w = v; w != u;) {
          const int q = S.aux[w];
          w = res_at(S, q, b);
          swap_pick(S, q, a, b);
        }
        recount(S, a);
        recount(S, b);
      }
      if (passes(S) <= target) return;
    }
    if (!improved) break;
  }
}

// The plan's order of one quarter; returns its passes.
// No residue total above NBG: the equitable colouring, NBG passes (optimal). Otherwise the earlier
// order (identity, pairwise descent; rounds > 0: and its chain search) and then the alignment, which
// can only lower the passes: the result never has more than the earlier order had. two_starts: where
// that misses the bound, also the alignment of the equitable colouring, and the better of the two.
template <int NBG>
PO_HD inline int order_quarter(Quarter<NBG>& S, int nl, int rounds, bool two_starts) {
  reset(S, nl);
  const int lb = bound(S, nl);
  const bool easy = lb <= NBG;
  int p1 = 1 << 20;
  if (!easy) {
    descend(S, nl);
    search_chains(S, nl, rounds);
    if (passes(S) > lb) order_align(S, nl, lb);
    p1 = passes(S);
    if (p1 <= lb || !two_starts) return p1;
    for (int q = 0; q < nl; ++q)
      for (int t = 0; t < NBG; ++t) S.keep[q][t] = S.st[q][t];
  }
  // (one call for both cases: a kernel's threads that each order their own quarter run it together)
  order_equitable(S, nl);
  if (easy) return passes(S);
  order_align(S, nl, lb);
  const int p2 = passes(S);
  if (p2 < p1) return p2;
  for (int q = 0; q < nl; ++q)
    for (int t = 0; t < NBG; ++t) S.st[q][t] = S.keep[q][t];
  for (int t = 0; t < NBG; ++t) tally(S, nl, t);
  return p1;
}

}  // namespace plan_order
