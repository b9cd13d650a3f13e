// lqro_devmem_main.cpp — csrc/lqro_devmem.hpp's pool on the host, with
// malloc-backed stand-ins for the three device-memory calls
// (tests/test_devmem_cpu.py builds it with g++, plain and with
// -fsanitize=address,undefined).  Includes nothing of the project but that
// header.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../../lqr-obstacles_amd/csrc/lqro_devmem.hpp"

static std::set<void*> g_live;   // buffers allocated and not yet freed
static int g_allocs = 0;         // allocations asked for so far
static int g_fail_at = 0;        // fail the k-th allocation (1-based); 0: none
static int g_frees = 0;          // buffers freed
static int g_bad_frees = 0;      // frees of something not live (a double free)
static size_t g_last_bytes = 0;
constexpr int kNoMem = 2, kFillError = 7;   // the stand-ins' codes (hipErrorOutOfMemory is 2)
static bool g_fill_fails = false;

namespace lqro {
int devmem_alloc(void** p, size_t bytes) {
  *p = nullptr;
  if (++g_allocs == g_fail_at) return kNoMem;
  g_last_bytes = bytes;
  *p = malloc(bytes);
  memset(*p, 0xA5, bytes);
  g_live.insert(*p);
  return 0;
}
int devmem_free(void* p) {
  if (!g_live.erase(p)) {
    ++g_bad_frees;
    return 1;
  }
  free(p);
  ++g_frees;
  return 0;
}
int devmem_fill(void* p, int byte, size_t bytes) {
  if (g_fill_fails) return kFillError;
  memset(p, byte, bytes);
  return 0;
}
}  // namespace lqro

static int g_failed = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #x); \
      ++g_failed;                                                 \
    }                                                             \
  } while (0)

using lqro::DevPool;

int main() {
  // everything is freed at scope exit; a buffer released early exactly once
  {
    DevPool pool;
    double* a = nullptr;
    int *b = nullptr, *c = nullptr;
    char* v = nullptr;
    CHECK(pool.get(a, 10) == 0 && a && g_last_bytes == 10 * sizeof(double));
    CHECK(pool.get(b, 3) == 0 && b && g_last_bytes == 3 * sizeof(int));
    CHECK(pool.get(c, 5) == 0 && c);
    CHECK(pool.get(v, 24) == 0 && v && g_last_bytes == 24);   // bytes: a char count
    CHECK(g_live.size() == 4);
    pool.release(b);
    CHECK(b == nullptr && g_live.size() == 3);
    pool.release(b);   // null: nothing
    CHECK(g_live.size() == 3 && g_bad_frees == 0);
    // release-and-get: the old buffer goes first, the new one is owned
    pool.release(c);
    CHECK(pool.get(c, 50) == 0 && c && g_frees == 2);
    CHECK(g_live.size() == 3 && g_last_bytes == 50 * sizeof(int));
  }
  CHECK(g_live.empty() && g_bad_frees == 0 && g_allocs == 5 && g_frees == 5);

  // freed by hand ahead of the destructor: still exactly once
  {
    DevPool pool;
    int *a = nullptr, *b = nullptr;
    CHECK(pool.get(a, 2) == 0 && pool.get(b, 2) == 0);
    pool.free_all();
    CHECK(g_live.empty());
  }
  CHECK(g_live.empty() && g_bad_frees == 0 && g_frees == 7);

  // the optional fill writes the whole buffer, no fill leaves it alone; a
  // zero-element request still yields a valid one-element buffer
  {
    DevPool pool;
    unsigned char *f = nullptr, *n = nullptr;
    CHECK(pool.get(f, 1000, 0xFF) == 0 && pool.get(n, 1000) == 0);
    bool all_ff = true, all_a5 = true;
    for (int k = 0; k < 1000; ++k) {
      all_ff = all_ff && f[k] == 0xFF;
      all_a5 = all_a5 && n[k] == 0xA5;
    }
    CHECK(all_ff && all_a5);
    long long* z = nullptr;
    CHECK(pool.get(z, 0, 0) == 0 && z != nullptr && g_last_bytes == sizeof(long long) && z[0] == 0);
    z[0] = 1;   // (one element is there to write)
  }
  CHECK(g_live.empty() && g_bad_frees == 0);

  // the k-th allocation fails: its code comes back, the pointer is null, every
  // earlier buffer is still owned and is freed at exit
  for (int k = 1; k <= 4; ++k) {
    {
      DevPool pool;
      float* p[4] = {nullptr, nullptr, nullptr, nullptr};
      g_allocs = 0;
      g_fail_at = k;
      for (int q = 0; q < 4; ++q) {
        const int e = pool.get(p[q], 8, 0);
        CHECK(e == (q + 1 == k ? kNoMem : 0));
        CHECK((p[q] == nullptr) == (q + 1 == k));
      }
      g_fail_at = 0;
      CHECK(g_live.size() == 3);
      for (int q = 0; q < 4; ++q)
        if (p[q]) CHECK(g_live.count(p[q]) == 1 && p[q][7] == 0.0f);
      // a failed release-and-get: the old buffer is gone, nothing replaces it
      g_allocs = 0;
      g_fail_at = 1;
      float*& victim = p[k == 1 ? 1 : 0];
      pool.release(victim);
      CHECK(pool.get(victim, 16) == kNoMem && victim == nullptr && g_live.size() == 2);
      g_fail_at = 0;
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
  }

  // a failing fill: its code, and the buffer it was for is not kept
  {
    DevPool pool;
    int *a = nullptr, *b = nullptr;
    CHECK(pool.get(a, 4) == 0);
    g_fill_fails = true;
    CHECK(pool.get(b, 4, 0) == kFillError && b == nullptr && g_live.size() == 1);
    g_fill_fails = false;
  }
  CHECK(g_live.empty() && g_bad_frees == 0);

  if (g_failed) return 1;
  printf("devmem ok\n");
  return 0;
}
