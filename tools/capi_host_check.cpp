// capi_host_check.cpp — the two pieces of liblfa.so's host side that need no
// HIP, on the host alone: the parameter registry (lfa_param.cpp) and the
// list forms' table builder (lfa_iov_table.h).  The registry is checked here;
// the tables are printed for tests/test_capi_host_cpu.py to compare with the
// layout lfa_iov.h documents.  Also built with ASan + UBSan:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/capi_host_check.cpp libfabric_amd/csrc/lfa_param.cpp \
//       -lpthread -o /tmp/capi_host_check && /tmp/capi_host_check
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../libfabric_amd/csrc/lfa_iov_table.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

// The registry keeps every string it was ever given (lfa_param.cpp): that is
// its promise, not a leak to report.  Everything else ASan checks stays on.
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

static bool is(const char *name, const char *want) {
  const char *v = lfa_param(name);
  return want ? v && !strcmp(v, want) : !v;
}

// ---- the registry ----------------------------------------------------------
constexpr int kThreads = 4, kOwn = 4, kRounds = 200;

static std::string thread_name(int t, int k) {
  return "LFA_CHECK_T" + std::to_string(t) + "_" + std::to_string(k);
}

// Each thread sets its own names and reads everyone's: a value read is unset
// or one that was written for that very name.
static void *thread_body(void *arg) {
  const int me = (int)(intptr_t)arg;
  for (int r = 0; r < kRounds; r++) {
    for (int k = 0; k < kOwn; k++) {
      char v[32];
      snprintf(v, sizeof v, "t%d k%d r%d", me, k, r);
      CHECK(lfa_param_set(thread_name(me, k).c_str(), v) == 0);
    }
    for (int t = 0; t < kThreads; t++)
      for (int k = 0; k < kOwn; k++) {
        const char *v = lfa_param(thread_name(t, k).c_str());
        int vt, vk, vr;
        if (!v) continue;
        CHECK(sscanf(v, "t%d k%d r%d", &vt, &vk, &vr) == 3);
        CHECK(vt == t && vk == k && vr >= 0 && vr < kRounds);
        if (t == me) CHECK(vr == r);
      }
  }
  return nullptr;
}

static void check_registry() {
  const char *a = "LFA_CHECK_A";
  int names = 0;  // distinct names the registry holds: it has 64 slots
  // set, reset, unset: a NULL value lets the environment show through again
  unsetenv(a);
  CHECK(is(a, nullptr));
  setenv(a, "from-env", 1);
  CHECK(is(a, "from-env"));
  CHECK(lfa_param_set(a, "one") == 0 && is(a, "one"));
  names++;
  CHECK(lfa_param_set(a, "two") == 0 && is(a, "two"));
  CHECK(lfa_param_set(a, nullptr) == 0 && is(a, "from-env"));
  unsetenv(a);
  CHECK(is(a, nullptr));
  CHECK(lfa_param(nullptr) == nullptr);
  CHECK(lfa_param_set(nullptr, "x") == -LFA_EINVAL && lfa_param_set("", "x") == -LFA_EINVAL);

  // the longest name and value, and one character more
  const std::string n47(47, 'N'), n48(48, 'N'), v79(79, 'v'), v80(80, 'v');
  CHECK(lfa_param_set(n47.c_str(), v79.c_str()) == 0 && is(n47.c_str(), v79.c_str()));
  names++;
  CHECK(lfa_param_set(n48.c_str(), "x") == -LFA_EINVAL && is(n48.c_str(), nullptr));
  CHECK(lfa_param_set(n47.c_str(), v80.c_str()) == -LFA_EINVAL && is(n47.c_str(), v79.c_str()));

  // a pointer lfa_param returned outlives every later set of its name
  CHECK(lfa_param_set(a, "first") == 0);
  const char *first = lfa_param(a);
  for (int i = 0; i < 100; i++) {
    const std::string v = "later-" + std::to_string(i);
    CHECK(lfa_param_set(a, v.c_str()) == 0 && is(a, v.c_str()));
  }
  CHECK(!strcmp(first, "first"));
  CHECK(lfa_param_set(a, nullptr) == 0 && !strcmp(first, "first"));
  CHECK(lfa_param_set(a, "last") == 0);

  pthread_t th[kThreads];
  for (int t = 0; t < kThreads; t++)
    CHECK(pthread_create(&th[t], nullptr, thread_body, (void *)(intptr_t)t) == 0);
  for (int t = 0; t < kThreads; t++) CHECK(pthread_join(th[t], nullptr) == 0);
  names += kThreads * kOwn;

  // the 65th distinct name is refused, and the 64 before it stay as they are
  int fill = 0;
  for (; names < 64; names++, fill++) {
    const std::string n = "LFA_CHECK_F" + std::to_string(fill);
    CHECK(lfa_param_set(n.c_str(), n.c_str()) == 0);
  }
  CHECK(lfa_param_set("LFA_CHECK_65", "x") == -LFA_ENOMEM && is("LFA_CHECK_65", nullptr));
  CHECK(is(a, "last") && is(n47.c_str(), v79.c_str()));
  for (int t = 0; t < kThreads; t++)
    for (int k = 0; k < kOwn; k++) {
      char v[32];
      snprintf(v, sizeof v, "t%d k%d r%d", t, k, kRounds - 1);
      CHECK(is(thread_name(t, k).c_str(), v));
    }
  for (int i = 0; i < fill; i++) {
    const std::string n = "LFA_CHECK_F" + std::to_string(i);
    CHECK(is(n.c_str(), n.c_str()));
  }
  CHECK(lfa_param_set(a, "still") == 0 && is(a, "still"));  // a held name can still change
  printf("registry ok %d names\n", names);
}

// ---- IovTable --------------------------------------------------------------
// Addresses are only classified and stored, never touched.
static uintptr_t dst_of(size_t s, size_t off) { return 0x10000000u + 0x100000u * s + off; }
static uintptr_t in_of(size_t k, size_t s, size_t off) {
  return 0x100000000ull * (k + 1) + 0x100000u * s + off;
}

static void print_table(const IovTable &t) {
  printf("table %zu %d %zu\nfirst", t.nseg(), (int)t.direct, t.words());
  for (uint32_t f : t.first) printf(" %u", f);
  std::vector<uint64_t> w(t.words(), ~0ull);
  t.write(w.data());
  printf("\nwords");
  for (uint64_t x : w) printf(" %llx", (unsigned long long)x);
  printf("\n");
}

// One call: segments of `counts` elements of esz bytes, dst and every input
// `off` bytes past a 16-byte boundary.
static void call(IovTable &t, uint32_t nin, size_t esz, size_t off, const size_t *counts,
                 size_t n) {
  t.reset(nin);
  printf("call %u %zu %zu %zu\n", nin, esz, off, n);
  for (size_t s = 0; s < n; s++) {
    const void *in[3];
    for (uint32_t k = 0; k < nin; k++) in[k] = (const void *)in_of(k, s, off);
    CHECK(t.add((void *)dst_of(s, off), counts[s], in, esz) == 0);
    printf("seg %llx %zu", (unsigned long long)dst_of(s, off), counts[s]);
    for (uint32_t k = 0; k < nin; k++) printf(" %llx", (unsigned long long)in_of(k, s, off));
    printf("\n");
  }
  print_table(t);
}

static void check_tables() {
  IovTable t;
  for (uint32_t nin : {1u, 3u})
    for (size_t esz : {(size_t)1, (size_t)4, (size_t)16})
      for (size_t off : {(size_t)0, (size_t)4, (size_t)1}) {
        // one tile; exactly LFA_IOV_TILE bytes after the head (the elements
        // before dst's first 16-byte boundary, when dst is element-aligned);
        // one element more
        const size_t head = off % esz ? 0 : (16 - off % 16) % 16 / esz;
        const size_t full = head + LFA_IOV_TILE / esz;
        const size_t mixed[] = {3, full, full + 1}, single[] = {3, full};
        call(t, nin, esz, off, mixed, 3);
        call(t, nin, esz, off, single, 2);  // every segment one tile: direct
      }

  // the grid bound: segments of 2^30 tiles until the sum would pass 2^31 - 1
  t.reset(1);
  const void *in = (const void *)in_of(0, 0, 0);
  int ok = 0, rc = 0;
  while (!(rc = t.add((void *)dst_of(0, 0), ((size_t)1 << 30) * LFA_IOV_TILE, &in, 1)) && ok < 8)
    ok++;
  printf("bound %d %d %zu %u\n", ok, rc, t.nseg(), t.first.back());

  // words() against LFA_IOV_INLINE, one one-tile segment at a time
  for (uint32_t nin : {1u, 3u}) {
    const void *ins[3] = {in, in, in};
    t.reset(nin);
    for (int s = 1; s <= 24; s++) {
      CHECK(t.add((void *)dst_of(s, 0), 4, ins, 4) == 0);
      printf("grow %u %zu %zu %d\n", nin, t.nseg(), t.words(), (int)(t.words() <= LFA_IOV_INLINE));
    }
  }
}

int main() {
  check_registry();
  check_tables();
  return 0;
}
