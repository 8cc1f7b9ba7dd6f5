// split_host_check.cpp — lfa_split.h on the host, as g++ sees it: prints the
// path and the head / nvec / body / tail split of a grid of (element size,
// dst offset, src offset, count) cases and the taper split around its tile
// boundaries, one line each, for tests/test_split_cpu.py to compare with the
// same quantities computed in Python.  Also built with ASan + UBSan:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/split_host_check.cpp -o /tmp/split_host_check && /tmp/split_host_check
#include <stdio.h>

#include "../libfabric_amd/csrc/lfa_split.h"

int main() {
  static const size_t esz_all[] = {1, 2, 4, 8, 16};
  const uintptr_t base = 0x10000;  // addresses are only classified, never touched
  for (size_t esz : esz_all) {
    // src against dst: the same offset, an odd number of bytes apart, and a
    // multiple of esz apart that is no multiple of 16 (none exists at esz 16)
    const size_t deltas[] = {0, 3, esz}, ndelta = esz < 16 ? 3 : 2;
    for (size_t doff = 0; doff < 32; doff++)
      for (size_t j = 0; j < ndelta; j++) {
        const size_t delta = deltas[j];
        const uintptr_t dst = base + doff, src = base + 4096 + doff + delta;
        const void *outs[1] = {(const void *)dst}, *ins[1] = {(const void *)src};
        const enum lfa_path path = lfa_split_path(outs, 1, ins, 1, esz);
        const size_t head = lfa_split_head(dst, 64, esz);  // counts around the head
        size_t counts[32], n = 0;
        counts[n++] = 0;
        counts[n++] = 1;
        for (size_t c = head ? head - 1 : 0; c <= head + 16 / esz + 1; c++) counts[n++] = c;
        for (size_t i = 0; i < n; i++) {
          const struct lfa_split s = lfa_split_of(path, dst, counts[i], esz);
          printf("split %zu %zu %zu %zu %d %zu %zu %zu %zu\n", esz, doff, doff + delta, counts[i],
                 (int)path, s.head, s.nvec, s.body, s.tail);
        }
      }
  }
  static const size_t ks[] = {0, 1, 7, 8, 9}, divs[] = {4, 8}, tvs[] = {256, 512};
  for (size_t k : ks)
    for (int d = -1; d <= 1; d++) {
      if (k == 0 && d < 0) continue;
      const size_t nvec = k * 4096 + d;
      for (size_t div : divs)
        for (size_t tv : tvs) {
          const struct lfa_taper t = lfa_split_taper(nvec, div, 4096, tv);
          printf("taper %zu %zu %zu %zu %u %u\n", nvec, div, tv, t.split, t.nhead, t.ntail);
        }
    }
  return 0;
}
