// Host-side carving of a caller-provided workspace (plain C++, no HIP include).  A layout is written once, as a sequence
// of take<T>(n) calls; run on a null base the same sequence gives the byte count *_workspace_bytes returns.
#pragma once
#include <stddef.h>
#include <stdint.h>

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct WsCarver {
  uintptr_t base;
  size_t bytes = 0;      // carved so far: after the last take, the size of the layout
  explicit WsCarver(void* ws) : base((uintptr_t)ws) {}
  // n elements of T at the next 256-byte boundary (every array starts on one: the base is the allocator's)
  template <typename T> T* take(size_t n) {
    T* p = (T*)(base + bytes);
    bytes += align_up(n * sizeof(T), 256);
    return p;
  }
};
