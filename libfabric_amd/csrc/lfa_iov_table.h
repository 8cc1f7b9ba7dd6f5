// lfa_iov_table.h — one call's segment table under construction, on the host
// (lfa_iov.cpp).  The layout the kernels trust is lfa_iov.h's; nothing here
// needs HIP, so a host-only program can include it (tools/capi_host_check.cpp).
#ifndef LFA_IOV_TABLE_H
#define LFA_IOV_TABLE_H

#include <string.h>

#include <vector>

#include "../../include/lfa_atomic.h"
#include "lfa_iov.h"

// One call's table under construction (lfa_iov.h): the non-empty segments'
// records, then the launch.
struct IovTable {
  std::vector<uint64_t> rec;   // nseg records of 2 + nin words
  std::vector<uint32_t> first; // first_tile[nseg + 1]
  uint32_t nin = 0;
  bool direct = true;

  void reset(uint32_t n) {
    rec.clear();
    first.assign(1, 0u);
    nin = n;
    direct = true;
  }
  size_t nseg() const { return first.size() - 1; }
  // 0, or -LFA_EINVAL when the grid would pass 2^31 workgroups
  int add(void *dst, size_t count, const void *const *in, size_t esz) {
    uintptr_t any = (uintptr_t)dst;
    for (uint32_t k = 0; k < nin; k++) any |= (uintptr_t)in[k];
    // `any % esz` is what the kernels test: esz is a power of two
    const size_t tiles = lfa_iov_tiles((uintptr_t)dst, any, count, esz);
    if (tiles > 0x7fffffffu - first.back()) return -LFA_EINVAL;
    if (tiles != 1) direct = false;
    rec.push_back((uint64_t)(uintptr_t)dst);
    rec.push_back((uint64_t)count);
    for (uint32_t k = 0; k < nin; k++) rec.push_back((uint64_t)(uintptr_t)in[k]);
    first.push_back(first.back() + (uint32_t)tiles);
    return 0;
  }
  size_t words() const { return lfa_iov_prefix_words(nseg()) + rec.size(); }
  void write(uint64_t *w) const {
    const size_t p = lfa_iov_prefix_words(nseg());
    memset(w, 0, p * 8);
    memcpy(w, first.data(), first.size() * 4);
    memcpy(w + p, rec.data(), rec.size() * 8);
  }
};

#endif  // LFA_IOV_TABLE_H
