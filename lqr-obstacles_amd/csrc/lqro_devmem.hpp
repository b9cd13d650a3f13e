// lqro_devmem.hpp — one owner for device buffers.  A DevPool hands out
// buffers, each from its own allocation, and frees what it still holds when it
// is destroyed: the context owns one (lqro_ctx.hpp), the one-shot entry points
// keep one on the stack.  Every allocation, free and fill goes through the
// three devmem_* functions, which liblqro.so defines over hipMalloc / hipFree /
// hipMemset (lqro_runtime.hip); no HIP include here, so a host program can
// define them over malloc instead (tests/cpp/lqro_devmem_main.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace lqro {

// 0: done, else the runtime's error code (a hipError_t in liblqro.so)
int devmem_alloc(void** p, size_t bytes);
int devmem_free(void* p);
int devmem_fill(void* p, int byte, size_t bytes);

class __attribute__((visibility("hidden"))) DevPool {   // (no part of the library's ABI)
 public:
  static constexpr int kNoFill = -1;
  DevPool() = default;
  DevPool(const DevPool&) = delete;
  DevPool& operator=(const DevPool&) = delete;
  ~DevPool() { free_all(); }
  void free_all() {   // (what the destructor does, for an owner that must free before it goes; last got, first freed)
    for (auto it = held_.rbegin(); it != held_.rend(); ++it) (void)devmem_free(*it);
    held_.clear();
  }
  // p = a new buffer of n elements (at least one: a zero-element request still
  // gets a valid buffer), every byte set to `fill` unless kNoFill.  Returns 0,
  // or the failing call's code: p is then null, the pool holds what it held.
  template <class T>
  int get(T*& p, size_t n, int fill = kNoFill) {
    p = nullptr;
    const size_t bytes = sizeof(T) * std::max<size_t>(n, 1);
    void* q = nullptr;
    int e = devmem_alloc(&q, bytes);
    if (e == 0 && fill != kNoFill && (e = devmem_fill(q, fill, bytes)) != 0) (void)devmem_free(q);
    if (e != 0) return e;
    held_.push_back(q);
    p = static_cast<T*>(q);
    return 0;
  }
  // frees p now (null, or a buffer this pool handed out) and nulls it
  template <class T>
  void release(T*& p) {
    const auto it = std::find(held_.begin(), held_.end(), static_cast<void*>(p));
    if (it != held_.end()) {
      (void)devmem_free(*it);
      held_.erase(it);
    }
    p = nullptr;
  }

 private:
  std::vector<void*> held_;
};

}  // namespace lqro
