// lfa_param.cpp — the tuning-parameter registry of liblfa.so (lfa_param,
// lfa_param_set; include/lfa_atomic.h), lfa_version and the one knob the
// ABI itself exports, lfa_host_small_bytes.  No HIP.
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lfa_atomic.h"

namespace {
constexpr int kParams = 64;
constexpr size_t kParamValueMax = 80;
// A value, once set, is never written again: a new value of the same name
// is a new string and the old one is kept (a caller may still be parsing it
// on another thread), so every pointer lfa_param returned stays valid and
// unchanged for the life of the process.  Sets are rare (provider init,
// tests), so what is kept stays small.
struct ParamSlot {
  char name[48];
  const char *value;  // null: not set (the environment shows through)
};
ParamSlot g_params[kParams];
pthread_mutex_t g_param_lock = PTHREAD_MUTEX_INITIALIZER;
}  // namespace

extern "C" {

const char *lfa_param(const char *name) {
  if (!name) return nullptr;
  const char *v = nullptr;
  pthread_mutex_lock(&g_param_lock);
  for (const ParamSlot &p : g_params)
    if (p.value && !strcmp(p.name, name)) v = p.value;
  pthread_mutex_unlock(&g_param_lock);
  return v ? v : getenv(name);
}

int lfa_param_set(const char *name, const char *value) {
  if (!name || !*name || strlen(name) >= sizeof(ParamSlot::name) ||
      (value && strlen(value) >= kParamValueMax))
    return -LFA_EINVAL;
  char *copy = value ? strdup(value) : nullptr;
  if (value && !copy) return -LFA_ENOMEM;
  int ret = -LFA_ENOMEM;
  pthread_mutex_lock(&g_param_lock);
  ParamSlot *slot = nullptr;
  for (ParamSlot &p : g_params)
    if (p.name[0] && !strcmp(p.name, name)) slot = &p;
  if (!slot)
    for (ParamSlot &p : g_params)
      if (!p.name[0]) {
        slot = &p;
        strcpy(p.name, name);
        break;
      }
  if (slot) {
    slot->value = copy;  // the previous string, if any, is kept (above)
    copy = nullptr;
    ret = 0;
  }
  pthread_mutex_unlock(&g_param_lock);
  free(copy);
  return ret;
}

const char *lfa_version(void) {
  return "lfa-combine 0.2 gfx950 (LDS-DMA staged, 4 KiB/operand/wave, nt loads/stores)";
}

size_t lfa_host_small_bytes(void) {
  static size_t v = [] {
    const char *e = lfa_param("LFA_HOST_SMALL_BYTES");
    return e ? (size_t)strtoull(e, nullptr, 0) : (size_t)LFA_HOST_SMALL_DEFAULT;
  }();
  return v;
}

}  // extern "C"
