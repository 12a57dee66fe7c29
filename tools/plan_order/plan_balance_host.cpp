// Stand-alone experiment (no GPU, no Python): the greedy fill of k_plan_perm and an exchange descent
// after it, to count what balancing a chunk's 16-lane quarters would save (plan_balance_counts.py;
// DESIGN.md 3.2b "Quarter balance": measured on config E and left out of the plan).
// usage: plan_balance_host NN NSPLIT MQ [placed|fill] < chunks > placements
//        placed: the entries come in position order (a recorded placement) and are not filled again
//        fill:   the greedy fill alone, no exchanges: what k_plan_perm writes (the test compares it with
//                chunks recorded from device plans)
// input, per chunk:  na (uint16), then na x NN residues (1 byte each, entry-major), the entries in the
//                    order in which the fill visits them
// output, per chunk: 3 x uint16 (summed bound after the fill, after the descent, exchanges made), then
//                    na x uint16: the input index of the entry at each position
// (all uint16 little-endian)
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PO_HD

namespace plan_order {

// ---- which entries share a quarter (k_plan_perm) ------------------------------------------------
//
// A chunk's adjacency entries (NN blocks each, split into NSPLIT lanes that stay together) are placed
// into 16-lane quarters of EQ = 16 / NSPLIT entries; only the last quarter may be short. A quarter's
// order cannot have fewer passes than max(NBG, largest residue total), so the placement decides the
// sum of that bound over the chunk's quarters. place_entry is the greedy fill (least histogram overlap,
// never revisited); balance_chunk then exchanges entries between quarters while the summed bound falls.

// sweeps of balance_chunk over the chunk's over-full quarters (the plan's time is linear in it)
constexpr int kBalanceSweeps = 2;

// One chunk's placement. hw[q]: the residue histogram of quarter q, one byte per residue (a quarter holds
// at most 16 x 16 blocks, and the exchange test adds one entry's <= 16 to it before it subtracts); nib:
// the residues of the entry at each position (q * EQ + place in the quarter), two per byte; ent: which
// entry that is (the caller's index). A kernel keeps one per thread in LDS.
template <int NN, int NSPLIT, int MQ>
struct Chunk {
  static constexpr int EQ = NSPLIT <= 16 ? 16 / NSPLIT : 1;
  static constexpr int NE = MQ * EQ;
  static constexpr int NB = (NN + 1) / 2;
  uint64_t hw[MQ][2];
  uint16_t ent[NE];
  uint8_t nib[NE][NB];
  uint8_t fill[MQ];
  uint8_t mx[MQ];  // largest residue total of a quarter (balance_chunk)
};

template <class C>
PO_HD inline int hist(const C& S, int q, int r) { return (int)((S.hw[q][r >> 3] >> (8 * (r & 7))) & 255u); }
template <class C>
PO_HD inline int res_of(const C& S, int pos, int b) { return (S.nib[pos][b >> 1] >> (4 * (b & 1))) & 15; }
// the largest byte of a histogram
PO_HD inline int max_byte(uint64_t lo, uint64_t hi) {
  int m = 0;
  for (int r = 0; r < 8; ++r) {
    const int a = (int)((lo >> (8 * r)) & 255u), b = (int)((hi >> (8 * r)) & 255u);
    m = a > m ? a : m;
    m = b > m ? b : m;
  }
  return m;
}
// an entry's residues as a histogram
template <class C>
PO_HD inline void entry_hist(const C& S, int pos, int nn, uint64_t& lo, uint64_t& hi) {
  lo = hi = 0;
  for (int b = 0; b < nn; ++b) {
    const int r = res_of(S, pos, b);
    const uint64_t one = 1ull << (8 * (r & 7));
    lo += r < 8 ? one : 0ull;
    hi += r < 8 ? 0ull : one;
  }
}
// entries quarter q of nq can hold when the chunk has na
template <class C>
PO_HD inline int capacity(int q, int nq, int na) { return q + 1 < nq ? C::EQ : na - C::EQ * (nq - 1); }

template <int NN, int NSPLIT, int MQ>
PO_HD inline void clear_chunk(Chunk<NN, NSPLIT, MQ>& S, int nq) {
  for (int q = 0; q < nq; ++q) {
    S.fill[q] = 0;
    S.hw[q][0] = S.hw[q][1] = 0;
  }
}

// the greedy fill's step: entry `id` with residues res goes to the quarter with room whose histogram
// overlaps them least (the first of equals); returns its position
template <int NN, int NSPLIT, int MQ>
PO_HD inline int place_entry(Chunk<NN, NSPLIT, MQ>& S, int nq, int na, const uint8_t (&res)[NN], int id) {
  using C = Chunk<NN, NSPLIT, MQ>;
  int best = -1, bc = 1 << 30;
  for (int q = 0; q < nq; ++q) {
    if (S.fill[q] >= capacity<C>(q, nq, na)) continue;
    int cost = 0;
    for (int b = 0; b < NN; ++b) cost += hist(S, q, res[b]);
    if (cost < bc) { bc = cost; best = q; }
  }
  const int pos = best * C::EQ + S.fill[best];
  ++S.fill[best];
  for (int b = 0; b < C::NB; ++b) S.nib[pos][b] = 0;
  for (int b = 0; b < NN; ++b) {
    S.hw[best][res[b] >> 3] += 1ull << (8 * (res[b] & 7));
    S.nib[pos][b >> 1] |= (uint8_t)(res[b] << (4 * (b & 1)));
  }
  S.ent[pos] = (uint16_t)id;
  return pos;
}

// sum over the quarters of max(NBG, largest residue total)
template <int NN, int NSPLIT, int MQ>
PO_HD inline int chunk_bound(const Chunk<NN, NSPLIT, MQ>& S, int nq) {
  constexpr int NBG = NN / NSPLIT;
  int s = 0;
  for (int q = 0; q < nq; ++q) {
    const int m = max_byte(S.hw[q][0], S.hw[q][1]);
    s += S.fill[q] == 0 ? 0 : (m > NBG ? m : NBG);
  }
  return s;
}

// Pairwise exchange descent on a filled chunk. Quarters are visited in index order (the greedy fill loads
// the first ones most); in a quarter whose largest residue total exceeds NBG, every entry that holds the
// first residue at that total is tried against every entry of the other quarters that holds it less
// often, in position order, and the first exchange that lowers the summed bound, or keeps it and lowers
// the sum of squared totals, is made. An exchange keeps both quarters' fill, so capacities hold, and the
// summed bound never rises. kBalanceSweeps sweeps, fewer when one changes nothing. Returns the exchanges.
template <int NN, int NSPLIT, int MQ>
PO_HD inline int balance_chunk(Chunk<NN, NSPLIT, MQ>& S, int nq) {
  using C = Chunk<NN, NSPLIT, MQ>;
  constexpr int NBG = NN / NSPLIT, EQ = C::EQ;
  if (nq < 2) return 0;
  for (int q = 0; q < nq; ++q) S.mx[q] = (uint8_t)max_byte(S.hw[q][0], S.hw[q][1]);
  int moves = 0;
  for (int sweep = 0; sweep < kBalanceSweeps; ++sweep) {
    bool improved = false;
    for (int q1 = 0; q1 < nq; ++q1) {
      for (int i = 0; i < S.fill[q1]; ++i) {
        const int m1 = S.mx[q1];
        if (m1 <= NBG) break;
        int hot = 0;
        while (hist(S, q1, hot) != m1) ++hot;
        const int pa = q1 * EQ + i;
        int ca = 0;
        for (int b = 0; b < NN; ++b) ca += res_of(S, pa, b) == hot ? 1 : 0;
        if (ca == 0) continue;
        uint64_t alo, ahi;
        entry_hist(S, pa, NN, alo, ahi);
        const uint64_t h1lo = S.hw[q1][0], h1hi = S.hw[q1][1];
        bool done = false;
        for (int q2 = 0; q2 < nq && !done; ++q2) {
          if (q2 == q1) continue;
          const int m2 = S.mx[q2];
          // q2 takes at least one more of the hot residue: skipped if that lifts it to q1's total
          if (hist(S, q2, hot) + 1 >= m1) continue;
          const uint64_t h2lo = S.hw[q2][0], h2hi = S.hw[q2][1];
          for (int j = 0; j < S.fill[q2]; ++j) {
            const int pb = q2 * EQ + j;
            int cb = 0;
            for (int b = 0; b < NN; ++b) cb += res_of(S, pb, b) == hot ? 1 : 0;
            if (cb >= ca) continue;
            uint64_t blo, bhi;
            entry_hist(S, pb, NN, blo, bhi);
            const uint64_t n1lo = h1lo + blo - alo, n1hi = h1hi + bhi - ahi;
            const uint64_t n2lo = h2lo + alo - blo, n2hi = h2hi + ahi - bhi;
            const int k1 = max_byte(n1lo, n1hi), k2 = max_byte(n2lo, n2hi);
            const int d = (k1 > NBG ? k1 : NBG) + (k2 > NBG ? k2 : NBG) - m1 - (m2 > NBG ? m2 : NBG);
            if (d > 0) continue;
            if (d == 0) {  // the tie: sum of squared totals
              int sq = 0;
              for (int r = 0; r < 16; ++r) {
                const uint64_t w1 = r < 8 ? h1lo : h1hi, w2 = r < 8 ? h2lo : h2hi;
                const uint64_t v1 = r < 8 ? n1lo : n1hi, v2 = r < 8 ? n2lo : n2hi;
                const int s = 8 * (r & 7);
                const int o1 = (int)((w1 >> s) & 255u), o2 = (int)((w2 >> s) & 255u);
                const int e1 = (int)((v1 >> s) & 255u), e2 = (int)((v2 >> s) & 255u);
                sq += e1 * e1 + e2 * e2 - o1 * o1 - o2 * o2;
              }
              if (sq >= 0) continue;
            }
            for (int b = 0; b < C::NB; ++b) {
              const uint8_t x = S.nib[pa][b];
              S.nib[pa][b] = S.nib[pb][b];
              S.nib[pb][b] = x;
            }
            const uint16_t x = S.ent[pa];
            S.ent[pa] = S.ent[pb];
            S.ent[pb] = x;
            S.hw[q1][0] = n1lo; S.hw[q1][1] = n1hi;
            S.hw[q2][0] = n2lo; S.hw[q2][1] = n2hi;
            S.mx[q1] = (uint8_t)k1;
            S.mx[q2] = (uint8_t)k2;
            ++moves;
            improved = done = true;
            break;
          }
        }
      }
    }
    if (!improved) break;
  }
  return moves;
}

}  // namespace plan_order

static void put16(std::vector<unsigned char>& out, unsigned v) {
  out.push_back((unsigned char)(v & 255));
  out.push_back((unsigned char)((v >> 8) & 255));
}

template <int NN, int NSPLIT, int MQ>
static int run(bool placed, bool fill_only) {
  using namespace plan_order;
  using C = Chunk<NN, NSPLIT, MQ>;
  std::vector<unsigned char> in, out;
  unsigned char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, stdin)) > 0) in.insert(in.end(), buf, buf + n);
  C* S = new C;
  size_t at = 0, chunk = 0;
  for (; at < in.size(); ++chunk) {
    if (at + 2 > in.size()) {
      fprintf(stderr, "chunk %zu: truncated header\n", chunk);
      return 2;
    }
    const int na = in[at] | (in[at + 1] << 8);
    at += 2;
    if (na < 1 || na > C::NE || at + (size_t)na * NN > in.size()) {
      fprintf(stderr, "chunk %zu: %d entries (1 .. %d), %zu bytes left\n", chunk, na, C::NE, in.size() - at);
      return 2;
    }
    const int nq = (na + C::EQ - 1) / C::EQ;
    clear_chunk(*S, nq);
    for (int j = 0; j < na; ++j) {
      uint8_t res[NN];
      for (int b = 0; b < NN; ++b) res[b] = (uint8_t)(in[at + (size_t)j * NN + b] & 15);
      if (placed) {  // position j: the fill's bookkeeping with the quarter given
        const int q = j / C::EQ;
        ++S->fill[q];
        for (int b = 0; b < C::NB; ++b) S->nib[j][b] = 0;
        for (int b = 0; b < NN; ++b) {
          S->hw[q][res[b] >> 3] += 1ull << (8 * (res[b] & 7));
          S->nib[j][b >> 1] |= (uint8_t)(res[b] << (4 * (b & 1)));
        }
        S->ent[j] = (uint16_t)j;
      } else {
        place_entry(*S, nq, na, res, j);
      }
    }
    at += (size_t)na * NN;
    const int b0 = chunk_bound(*S, nq);
    const int moves = fill_only ? 0 : balance_chunk(*S, nq);
    put16(out, (unsigned)b0);
    put16(out, (unsigned)chunk_bound(*S, nq));
    put16(out, (unsigned)moves);
    for (int p = 0; p < na; ++p) put16(out, S->ent[p]);
  }
  delete S;
  return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 2;
}

int main(int argc, char** argv) {
  const int nn = argc > 1 ? atoi(argv[1]) : 0, ns = argc > 2 ? atoi(argv[2]) : 0, mq = argc > 3 ? atoi(argv[3]) : 0;
  const bool placed = argc > 4 && !strcmp(argv[4], "placed");
  const bool fill_only = argc > 4 && !strcmp(argv[4], "fill");
#define CASE(NN_, NS_, MQ_) \
  if (nn == NN_ && ns == NS_ && mq == MQ_) return run<NN_, NS_, MQ_>(placed, fill_only)
  CASE(3, 1, 16);
  CASE(6, 2, 16);
  CASE(4, 1, 16);
  CASE(4, 2, 16);
  CASE(8, 2, 16);
  CASE(9, 1, 16);
  CASE(10, 1, 16);
  CASE(10, 2, 16);
  CASE(6, 2, 64);
  CASE(10, 2, 64);
  CASE(10, 1, 32);
#undef CASE
  fprintf(stderr, "usage: plan_balance_host NN NSPLIT MQ [placed|fill] < chunks > placements\n");
  return 2;
}
