// iov_host_check.cpp — the list forms' host side under AddressSanitizer and
// UBSan: lfa__iov_check and lfa__iov_fetch_check (the sort and the overlap
// rule over dst, and over dst and res), lfa_host_writev / lfa_host_readwritev /
// lfa_host_swapv against the loops of lfa_host_write / lfa_host_readwrite /
// lfa_host_swap, on exactly-sized heap blocks so that any read or write past a
// segment is caught, and the tables IovTable builds for the fetch and compare
// records (printed for tests/test_iov_fetch_cpu.py).  Host code only, no GPU:
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

#include "../libfabric_amd/csrc/lfa_iov_table.h"

extern "C" int lfa__iov_check(const struct lfa_ioc *, const struct lfa_ioc *, int, size_t, size_t);
extern "C" int lfa__iov_fetch_check(const struct lfa_ioc *, const struct lfa_ioc *, int,
                                    const struct lfa_ioc *, int, const struct lfa_ioc *, size_t,
                                    size_t);

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

// The fetch (swap == false) or compare list form against its loop, 37
// segments; res starts at yet another offset than dst and src.
static void fetch_parity(bool swap, enum lfa_op op, enum lfa_datatype dt) {
  static const size_t counts[] = {0, 1, 3, 15, 16, 17, 255, 4097};
  static const size_t offs[] = {0, 1, 2, 4, 8};
  const size_t esz = lfa_datatype_size(dt);
  Blocks got, want, src, cmp, gres, wres;
  for (int i = 0; i < 37; i++) {
    const size_t n = counts[(i * 3 + op) % 8], off = offs[i % 5];
    const unsigned seed = g_seed;
    got.add(n * esz, off, n);
    g_seed = seed;  // the same bytes
    want.add(n * esz, off, n);
    src.add(n * esz, offs[(i + 1) % 5], n);
    cmp.add(n * esz, offs[(i + 2) % 5], n);
    gres.add(n * esz, offs[(i + 3) % 5], n);
    wres.add(n * esz, offs[(i + 3) % 5], n);
    // compares that hold now and then: cmp and src take some of dst's elements
    for (size_t k = 0; k < n; k += 2) memcpy((char *)cmp.ioc[i].addr + k * esz,
                                             (char *)got.ioc[i].addr + k * esz, esz);
  }
  const size_t ns = want.ioc.size();
  for (size_t i = 0; i < ns; i++)
    CHECK((swap ? lfa_host_swap(op, dt, want.ioc[i].addr, src.ioc[i].addr, cmp.ioc[i].addr,
                                wres.ioc[i].addr, want.ioc[i].count)
                : lfa_host_readwrite(op, dt, want.ioc[i].addr, src.ioc[i].addr, wres.ioc[i].addr,
                                     want.ioc[i].count)) == 0);
  CHECK((swap ? lfa_host_swapv(op, dt, got.ioc.data(), src.ioc.data(), cmp.ioc.data(),
                               gres.ioc.data(), ns)
              : lfa_host_readwritev(op, dt, got.ioc.data(), src.ioc.data(), gres.ioc.data(), ns)) ==
        0);
  for (size_t i = 0; i < ns; i++) {
    CHECK(memcmp(got.ioc[i].addr, want.ioc[i].addr, want.ioc[i].count * esz) == 0);
    CHECK(memcmp(gres.ioc[i].addr, wres.ioc[i].addr, want.ioc[i].count * esz) == 0);
  }
}

// Every error of the fetch and compare list forms, through the shared check
// and through both host loops; no buffer is touched.
static void fetch_errors() {
  const size_t esz = 4;
  std::vector<char> arena(4096), keep;
  for (char &c : arena) c = (char)(rnd() >> 24);
  keep = arena;
  char *b = arena.data();
  auto two = [&](size_t o0, size_t n0, size_t o1, size_t n1) {
    return std::vector<lfa_ioc>{{b + o0, n0}, {b + o1, n1}};
  };
  const std::vector<lfa_ioc> dst = two(0, 8, 64, 8), src = two(1024, 8, 1088, 8),
                             cmp = two(2048, 8, 2112, 8), res = two(3072, 8, 3136, 8);
  // (dst, src, cmp, res) -> the code of the check, the fetch loop and the compare loop
  auto all = [&](const lfa_ioc *d, const lfa_ioc *s, const lfa_ioc *c, const lfa_ioc *r, size_t n,
                 int want) {
    CHECK(lfa__iov_fetch_check(d, s, 1, c, 1, r, n, esz) == want);
    CHECK(lfa_host_swapv(LFA_CSWAP, LFA_FLOAT, d, s, c, r, n) == want);
    if (!c) return;  // a bad cmp list is no error of the fetch form
    CHECK(lfa__iov_fetch_check(d, s, 1, nullptr, 0, r, n, esz) == want);
    CHECK(lfa_host_readwritev(LFA_SUM, LFA_FLOAT, d, s, r, n) == want);
  };
  const int bad = -LFA_EINVAL;
  all(nullptr, src.data(), cmp.data(), res.data(), 2, bad);  // NULL arrays
  all(dst.data(), nullptr, cmp.data(), res.data(), 2, bad);
  all(dst.data(), src.data(), cmp.data(), nullptr, 2, bad);
  CHECK(lfa__iov_fetch_check(dst.data(), src.data(), 1, nullptr, 1, res.data(), 2, esz) == bad);
  CHECK(lfa_host_swapv(LFA_CSWAP, LFA_FLOAT, dst.data(), src.data(), nullptr, res.data(), 2) == bad);
  for (int which = 0; which < 4; which++) {  // a NULL address, then a differing count
    for (int pass = 0; pass < 2; pass++) {
      std::vector<lfa_ioc> v[4] = {dst, src, cmp, res};
      if (pass) v[which][1].count = 7;
      else v[which][1].addr = nullptr;
      if (which == 2) {
        CHECK(lfa__iov_fetch_check(v[0].data(), v[1].data(), 1, v[2].data(), 1, v[3].data(), 2,
                                   esz) == bad);
        CHECK(lfa_host_swapv(LFA_CSWAP, LFA_FLOAT, v[0].data(), v[1].data(), v[2].data(),
                             v[3].data(), 2) == bad);
      } else {
        all(v[0].data(), v[1].data(), v[2].data(), v[3].data(), 2, bad);
      }
    }
  }
  {
    std::vector<lfa_ioc> many(LFA_IOV_MAX + 1, lfa_ioc{nullptr, 0});
    all(many.data(), many.data(), many.data(), many.data(), LFA_IOV_MAX + 1, bad);
    all(many.data(), many.data(), many.data(), many.data(), LFA_IOV_MAX, 0);  // all empty
  }
  // the overlap rule over dst and res
  all(dst.data(), src.data(), cmp.data(), two(28, 8, 3136, 8).data(), 2, bad);   // res[0] in dst[0]
  all(dst.data(), src.data(), cmp.data(), two(3072, 8, 28, 8).data(), 2, bad);   // res[1] in dst[0]
  all(dst.data(), src.data(), cmp.data(), two(3072, 8, 3100, 8).data(), 2, bad); // res[1] in res[0]
  all(two(0, 8, 28, 8).data(), src.data(), cmp.data(), res.data(), 2, bad);      // dst[1] in dst[0]
  all(dst.data(), src.data(), cmp.data(), two(3072, 64, 3080, 8).data(), 2, bad);  // count differs
  {
    std::vector<lfa_ioc> d = two(0, 64, 512, 1), r = two(3072, 64, 3100, 1);     // contained
    std::vector<lfa_ioc> s = two(1024, 64, 1500, 1), c = two(2048, 64, 2500, 1);
    all(d.data(), s.data(), c.data(), r.data(), 2, bad);
  }
  {
    std::vector<lfa_ioc> d = dst;  // a range that wraps the address space
    d[1].addr = (void *)(UINTPTR_MAX - 7);
    all(d.data(), src.data(), cmp.data(), res.data(), 2, bad);
  }
  // unsupported pairs come first, whatever the lists are
  CHECK(lfa_host_readwritev(LFA_BXOR, LFA_FLOAT, nullptr, nullptr, nullptr, 2) == -LFA_EOPNOTSUPP);
  CHECK(lfa_host_readwritev(LFA_CSWAP, LFA_FLOAT, nullptr, nullptr, nullptr, 2) == -LFA_EOPNOTSUPP);
  CHECK(lfa_host_swapv(LFA_MSWAP, LFA_FLOAT, nullptr, nullptr, nullptr, nullptr, 2) ==
        -LFA_EOPNOTSUPP);
  CHECK(lfa_host_swapv(LFA_SUM, LFA_FLOAT, nullptr, nullptr, nullptr, nullptr, 2) ==
        -LFA_EOPNOTSUPP);
  CHECK(lfa_host_swapv(LFA_CSWAP, LFA_FLOAT16, nullptr, nullptr, nullptr, nullptr, 2) ==
        -LFA_EOPNOTSUPP);
  CHECK(lfa_host_readwritev(LFA_SUM, LFA_FLOAT, nullptr, nullptr, nullptr, 0) == 0);
  CHECK(arena == keep);
  // ranges that only touch are accepted, res against dst too; ATOMIC_READ
  // takes no src list, or one of NULL addresses
  std::vector<lfa_ioc> d = two(0, 8, 32, 8), r = two(64, 8, 96, 8), none(2, lfa_ioc{nullptr, 0});
  CHECK(lfa__iov_fetch_check(d.data(), src.data(), 1, cmp.data(), 1, r.data(), 2, esz) == 0);
  CHECK(lfa_host_readwritev(LFA_ATOMIC_READ, LFA_FLOAT, d.data(), nullptr, r.data(), 2) == 0);
  CHECK(memcmp(b, keep.data(), 64) == 0 && memcmp(b + 64, b, 64) == 0);
  memset(b + 64, 0, 64);
  CHECK(lfa_host_readwritev(LFA_ATOMIC_READ, LFA_FLOAT, d.data(), none.data(), r.data(), 2) == 0);
  CHECK(memcmp(b + 64, b, 64) == 0);
  CHECK(lfa_host_readwritev(LFA_SUM, LFA_FLOAT, d.data(), nullptr, r.data(), 2) == bad);
}

// The tables of the fetch (nin 2) and compare (nin 3) records, and writev's
// (nin 1) for comparison: "tab <nin> <nseg> <direct> <words> | first... | words..."
static void fetch_tables() {
  static const size_t counts[] = {1, 4097, 3, 8192, 4096 + 5, 17};
  for (uint32_t nin = 1; nin <= 3; nin++)
    for (size_t nseg : {(size_t)1, (size_t)6, (size_t)11, (size_t)14, (size_t)15}) {
      IovTable t;
      t.reset(nin);
      for (size_t s = 0; s < nseg; s++) {
        const void *in[3];
        for (uint32_t k = 0; k < nin; k++)
          in[k] = (const void *)(0x100000000ull * (k + 1) + 0x100000u * s + 4);
        CHECK(t.add((void *)(uintptr_t)(0x10000000u + 0x100000u * s + 4), counts[s % 6], in, 4) ==
              0);
      }
      std::vector<uint64_t> w(t.words());
      t.write(w.data());
      printf("tab %u %zu %d %zu |", nin, t.nseg(), (int)t.direct, t.words());
      for (uint32_t f : t.first) printf(" %u", f);
      printf(" |");
      for (uint64_t x : w) printf(" %llx", (unsigned long long)x);
      printf("\n");
    }
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
  // the fetch and compare list forms: every pair of both tables
  int fetched = 0, compared = 0;
  for (int dt = 0; dt < LFA_DATATYPE_CNT; dt++)
    for (int op = 0; op <= LFA_MSWAP; op++) {
      if (!lfa_atomic_valid((lfa_datatype)dt, (lfa_op)op, LFA_FETCH_ATOMIC))
        fetch_parity(false, (lfa_op)op, (lfa_datatype)dt), fetched++;
      if (!lfa_atomic_valid((lfa_datatype)dt, (lfa_op)op, LFA_COMPARE_ATOMIC))
        fetch_parity(true, (lfa_op)op, (lfa_datatype)dt), compared++;
    }
  CHECK(fetched == 145 && compared == 84);
  fetch_errors();
  fetch_tables();
  printf("iov_host_check: %d fetch and %d compare parity cases and their errors pass\n", fetched,
         compared);
  printf("iov_host_check: %d parity cases and the overlap rule pass\n", ran);
  return 0;
}
