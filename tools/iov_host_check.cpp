// iov_host_check.cpp — the list forms' host side under AddressSanitizer and
// UBSan: lfa__iov_check (the sort and the overlap rule) and lfa_host_writev
// against the loop of lfa_host_write, on exactly-sized heap blocks so that
// any read or write past a segment is caught.  Host code only, no GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -ffp-contract=off -Iinclude tools/iov_host_check.cpp \
//       libfabric_amd/csrc/lfa_host.cpp libfabric_amd/csrc/lfa_valid.cpp \
//       -o /tmp/iov_host_check && /tmp/iov_host_check
//
// lfa_host.cpp asks liblfa.so's C ABI which (datatype, op) pairs exist:
// lfa_valid.cpp, the unit that answers in the library, needs no HIP either.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "lfa_atomic.h"

extern "C" int lfa__iov_check(const struct lfa_ioc *, const struct lfa_ioc *, int, size_t, size_t);

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

static unsigned g_seed = 12345;
static unsigned rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }

// one heap block per segment, exactly count * esz + off bytes
struct Blocks {
  std::vector<char *> base;
  std::vector<lfa_ioc> ioc;
  ~Blocks() {
    for (char *p : base) free(p);
  }
  void add(size_t bytes, size_t off, size_t count) {
    char *p = (char *)malloc(bytes + off ? bytes + off : 1);
    for (size_t i = 0; i < bytes + off; i++) p[i] = (char)(rnd() >> 24);
    base.push_back(p);
    ioc.push_back(lfa_ioc{p + off, count});
  }
};

static void parity(enum lfa_op op, enum lfa_datatype dt) {
  static const size_t counts[] = {0, 1, 3, 15, 16, 17, 255, 4097};
  static const size_t offs[] = {0, 1, 2, 4, 8};
  const size_t esz = lfa_reduce_datatype_size(dt);
  Blocks got, want, src;
  for (int i = 0; i < 37; i++) {
    const size_t n = counts[(i * 3 + op) % 8], off = offs[i % 5];
    const unsigned seed = g_seed;
    got.add(n * esz, off, n);
    g_seed = seed;  // the same bytes
    want.add(n * esz, off, n);
    src.add(n * esz, offs[(i + 1) % 5], n);
  }
  for (size_t i = 0; i < want.ioc.size(); i++)
    CHECK(lfa_host_write(op, dt, want.ioc[i].addr, src.ioc[i].addr, want.ioc[i].count) == 0);
  CHECK(lfa_host_writev(op, dt, got.ioc.data(), src.ioc.data(), got.ioc.size()) == 0);
  for (size_t i = 0; i < want.ioc.size(); i++)
    CHECK(memcmp(got.ioc[i].addr, want.ioc[i].addr, want.ioc[i].count * esz) == 0);
}

int main() {
  const enum lfa_datatype dts[] = {LFA_INT8, LFA_BFLOAT16, LFA_FLOAT, LFA_DOUBLE,
                                   LFA_INT128, LFA_FLOAT_COMPLEX};
  const enum lfa_op ops[] = {LFA_SUM, LFA_MIN, LFA_PROD, LFA_LXOR, LFA_BXOR};
  int ran = 0;
  for (enum lfa_datatype dt : dts)
    for (enum lfa_op op : ops)
      if (!lfa_reduce_valid(dt, op)) parity(op, dt), ran++;
  CHECK(ran == 6 * 5 - 4 - 1);  // no BXOR on the four float types, no MIN on complex

  // the overlap rule on LFA_IOV_MAX shuffled segments of one arena
  const size_t n = LFA_IOV_MAX, esz = 4;
  std::vector<char> arena(n * 64 + 64);
  std::vector<lfa_ioc> seg(n);
  for (size_t i = 0; i < n; i++) seg[i] = lfa_ioc{arena.data() + i * 64, 16};  // touching
  for (size_t i = n - 1; i > 0; i--) std::swap(seg[i], seg[rnd() % (i + 1)]);
  CHECK(lfa__iov_check(seg.data(), seg.data(), 1, n, esz) == 0);
  seg[n / 2].count = 17;  // one element into its neighbour
  CHECK(lfa__iov_check(seg.data(), seg.data(), 1, n, esz) == -LFA_EINVAL);
  seg[n / 2].count = 0;   // an empty segment overlaps nothing, wherever it points
  seg[n / 2].addr = arena.data() + 8;
  CHECK(lfa__iov_check(seg.data(), seg.data(), 1, n, esz) == 0);
  seg[3].addr = nullptr;  // a NULL address with a count
  CHECK(lfa__iov_check(seg.data(), seg.data(), 1, n, esz) == -LFA_EINVAL);
  seg[3].addr = (void *)(UINTPTR_MAX - 7);  // a range that wraps the address space
  CHECK(lfa__iov_check(seg.data(), seg.data(), 1, n, esz) == -LFA_EINVAL);
  CHECK(lfa__iov_check(seg.data(), seg.data(), 1, n + 1, esz) == -LFA_EINVAL);
  CHECK(lfa__iov_check(nullptr, seg.data(), 1, 2, esz) == -LFA_EINVAL);
  CHECK(lfa__iov_check(seg.data(), nullptr, 1, 2, esz) == -LFA_EINVAL);
  CHECK(lfa__iov_check(seg.data(), nullptr, 0, 2, esz) == 0);
  printf("iov_host_check: %d parity cases and the overlap rule pass\n", ran);
  return 0;
}
