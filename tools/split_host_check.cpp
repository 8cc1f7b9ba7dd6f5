// split_host_check.cpp — lfa_split.h on the host, as g++ sees it: prints the
// path and the head / nvec / body / tail split of a grid of (element size,
// dst offset, src offset, count) cases and the taper split around its tile
// boundaries, and the form launch_write, launch_tree_body and launch_fetch pick
// by size (lfa_form_write, lfa_form_tree, lfa_form_fetch) around every threshold, with and without an
// as_bytes override, one line each, for tests/test_split_cpu.py to compare with
// the same quantities computed in Python.  Also built with ASan + UBSan:
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
  // The form each launcher picks by size (lfa_form_*): body sizes 16 bytes
  // either side of every threshold, one small and one huge, first as the
  // real body (as_bytes 0), then as as_bytes over a small real body.
  size_t sizes[11], nsize = 0;
  const size_t small = (size_t)2597 * 16;
  sizes[nsize++] = small;
  static const size_t mibs[] = {32, 64, 192};
  for (size_t mib : mibs)
    for (size_t d = 0; d <= 32; d += 16) sizes[nsize++] = (mib << 20) - 16 + d;
  sizes[nsize++] = (size_t)5 << 30;
  for (int forced = 0; forced <= 1; forced++)
    for (size_t i = 0; i < nsize; i++) {
      const size_t real = forced ? small : sizes[i], as = forced ? sizes[i] : 0;
      const size_t bytes = lfa_form_bytes(real / 16, as);
      for (int mapped = 0; mapped <= 1; mapped++)
        printf("form write %zu %zu %d %d\n", as, real, mapped, (int)lfa_form_write(bytes, mapped));
      // ATOMIC_READ, the other readwrite ops, the compare table
      for (int nin = 1; nin <= 3; nin++)
        printf("form fetch %zu %zu %d %d\n", as, real, nin, (int)lfa_form_fetch(bytes, nin));
      for (int nsrc = 2; nsrc <= 32; nsrc++) {
        int nleaf = 1;
        while (nleaf * 2 <= nsrc) nleaf *= 2;
        for (size_t esz : esz_all) {
          const struct lfa_tree_form f = lfa_form_tree(bytes, nsrc, nleaf, esz);
          printf("form tree %zu %zu %d %d %zu %d %d\n", as, real, nsrc, nleaf, esz, f.variant,
                 f.cap_lds);
        }
      }
    }
  return 0;
}
