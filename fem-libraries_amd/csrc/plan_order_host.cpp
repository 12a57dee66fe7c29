// Stand-alone host driver of plan_order.h (tests/test_plan_order_host.py; no GPU, no Python).
// usage: plan_order_host NBG [STARTS] < quarters > orders   (STARTS 2: as with FA_PLAN_ORDER_SEARCH,
//        without its chain search)
// input, per quarter:  nl (1 byte, lanes 0 .. 16), then 16 x NBG residues (1 byte each, lane-major;
//                      lanes >= nl are ignored)
// output, per quarter: 4 x uint16 (passes of order_quarter, of the descent alone, of the descent with
//                      the chain search, the bound), then 16 x NBG picks of order_quarter (lane-major:
//                      the block added at each step; lanes >= nl zero)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan_order.h"

template <int NBG>
static int run(bool two) {
  using namespace plan_order;
  constexpr int kIn = 1 + kLanes * NBG, kOut = 8 + kLanes * NBG;
  std::vector<unsigned char> in;
  unsigned char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, stdin)) > 0) in.insert(in.end(), buf, buf + n);
  if (in.size() % kIn != 0) {
    fprintf(stderr, "input is %zu bytes, not a multiple of %d\n", in.size(), kIn);
    return 2;
  }
  const size_t nq = in.size() / kIn;
  std::vector<unsigned char> out(nq * kOut, 0);
  Quarter<NBG>* S = new Quarter<NBG>;
  for (size_t i = 0; i < nq; ++i) {
    const unsigned char* p = &in[i * kIn];
    const int nl = p[0];
    if (nl > kLanes) {
      fprintf(stderr, "quarter %zu: %d lanes\n", i, nl);
      return 2;
    }
    auto load = [&]() {
      for (int q = 0; q < nl; ++q)
        for (int k = 0; k < NBG; ++k) S->st[q][k] = (unsigned char)((p[1 + q * NBG + k] & 15) | (k << 4));
    };
    uint16_t head[4];
    load();
    order_descent(*S, nl, 0);
    head[1] = (uint16_t)passes(*S);
    load();
    order_descent(*S, nl, 4);
    head[2] = (uint16_t)passes(*S);
    load();
    head[0] = (uint16_t)order_quarter(*S, nl, 0, two);
    head[3] = (uint16_t)bound(*S, nl);
    unsigned char* o = &out[i * kOut];
    for (int h = 0; h < 4; ++h) {
      o[2 * h] = (unsigned char)(head[h] & 255);
      o[2 * h + 1] = (unsigned char)(head[h] >> 8);
    }
    for (int q = 0; q < nl; ++q)
      for (int t = 0; t < NBG; ++t) o[8 + q * NBG + t] = (unsigned char)block_at(*S, q, t);
  }
  delete S;
  return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 2;
}

int main(int argc, char** argv) {
  const int nbg = argc > 1 ? atoi(argv[1]) : 0;
  const bool two = argc > 2 && atoi(argv[2]) == 2;  // starts of the alignment (1: the default plan)
  switch (nbg) {
    case 1: return run<1>(two);
    case 2: return run<2>(two);
    case 3: return run<3>(two);
    case 4: return run<4>(two);
    case 5: return run<5>(two);
    case 9: return run<9>(two);
    case 10: return run<10>(two);
  }
  fprintf(stderr, "usage: plan_order_host NBG(1|2|3|4|5|9|10) < quarters > orders\n");
  return 2;
}
