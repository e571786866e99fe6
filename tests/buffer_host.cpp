// buffer_host.cpp — mjb::Buffer and mjb::Arena (csrc/mjb_buffer.hpp) without a GPU or the HIP runtime: the four allocator entry points
// are defined here over malloc / free.  They keep a table of the live blocks (which function made each, with which flags), abort on a
// release through the wrong function or of an unknown pointer, and can be told to fail the k-th allocation from now.  Built with
// -fsanitize=address,undefined by tests/test_buffer_host.py; exit status 0 and an empty stderr mean every check held.
#include "../mujoco_template_amd/csrc/mjb_buffer.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>

namespace {
struct Block { bool pinned; unsigned flags; size_t bytes; };
std::map<void*, Block> g_live;
long g_allocs = 0, g_frees = 0;      // calls that reached an allocator / a release function
long g_fail_in = 0;                  // > 0: the g_fail_in-th allocation from now fails

[[noreturn]] void die(const char* what) { std::fprintf(stderr, "buffer_host: %s\n", what); std::abort(); }
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::abort(); } } while (0)

hipError_t make(void** out, size_t bytes, bool pinned, unsigned flags) {
  g_allocs++;
  if (g_fail_in > 0 && --g_fail_in == 0) { *out = nullptr; return hipErrorOutOfMemory; }
  void* p = std::malloc(bytes ? bytes : 1);
  if (!p) die("host malloc failed");
  std::memset(p, 0xA5, bytes);
  g_live[p] = Block{pinned, flags, bytes};
  *out = p;
  return hipSuccess;
}
hipError_t release(void* p, bool pinned) {
  g_frees++;
  auto it = g_live.find(p);
  if (it == g_live.end()) die("release of a pointer that is not live (unknown, or released twice)");
  if (it->second.pinned != pinned) die(pinned ? "hipHostFree of a hipMalloc block" : "hipFree of a hipHostMalloc block");
  g_live.erase(it);
  std::free(p);
  return hipSuccess;
}
const Block& block_of(const void* p) {
  auto it = g_live.find(const_cast<void*>(p));
  if (it == g_live.end()) die("the buffer's pointer is not a live block");
  return it->second;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return make(ptr, size, false, 0); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int flags) { return make(ptr, size, true, flags); }
hipError_t hipFree(void* ptr) { return release(ptr, false); }
hipError_t hipHostFree(void* ptr) { return release(ptr, true); }
}

using mjb::Arena;
using mjb::Buffer;
using mjb::Mem;

static_assert(!std::is_copy_constructible<Buffer<double>>::value && !std::is_copy_assignable<Buffer<double>>::value, "Buffer owns its block");
static_assert(!std::is_copy_constructible<Arena>::value && !std::is_copy_assignable<Arena>::value, "Arena owns its blocks");

static void test_reserve() {
  Buffer<double> b;
  CHECK(b.get() == nullptr && b.count() == 0 && b.kind() == Mem::Device);
  CHECK(b.reserve(0) == hipSuccess && b.get() == nullptr && g_allocs == 0);          // nothing asked for, nothing made
  CHECK(b.reserve(10) == hipSuccess);                                                // an empty buffer allocates
  CHECK(b.get() && b.count() == 10 && g_live.size() == 1 && block_of(b.get()).bytes == 10 * sizeof(double));
  double* const first = b.get();
  for (size_t i = 0; i < 10; i++) first[i] = (double)i;                              // the whole block is writable (ASan)
  const long allocs = g_allocs, frees = g_frees;
  CHECK(b.reserve(10) == hipSuccess && b.reserve(3) == hipSuccess && b.reserve(0) == hipSuccess);
  CHECK(b.get() == first && b.count() == 10 && g_allocs == allocs && g_frees == frees);   // smaller or equal: same block, no allocator call
  CHECK(b.reserve(11) == hipSuccess);                                                // larger: the old block goes exactly once
  CHECK(b.count() == 11 && g_allocs == allocs + 1 && g_frees == frees + 1 && g_live.size() == 1 && block_of(b.get()).bytes == 11 * sizeof(double));
  b.get()[10] = 1.0;
  g_fail_in = 1;                                                                     // a failed reserve leaves the buffer empty
  CHECK(b.reserve(100) == hipErrorOutOfMemory);
  CHECK(b.get() == nullptr && b.count() == 0 && g_live.empty() && g_frees == frees + 2);
  CHECK(b.reserve(4) == hipSuccess && b.count() == 4 && g_live.size() == 1);         // and the next call allocates again
  b.reset();
  CHECK(b.get() == nullptr && b.count() == 0 && g_live.empty());
  const long frees2 = g_frees;
  b.reset();                                                                         // twice is harmless
  CHECK(g_frees == frees2 && g_live.empty());
  {
    Buffer<int> scoped;
    CHECK(scoped.reserve(7) == hipSuccess && g_live.size() == 1);
  }
  CHECK(g_live.empty());                                                             // the destructor releases
}

static void test_kinds() {
  Buffer<float> dev(Mem::Device);
  Buffer<float> pin(Mem::Pinned);
  Buffer<float> coh(Mem::PinnedCoherent);
  CHECK(dev.reserve(5) == hipSuccess && pin.reserve(5) == hipSuccess && coh.reserve(5) == hipSuccess);
  CHECK(!block_of(dev.get()).pinned);
  CHECK(block_of(pin.get()).pinned && block_of(pin.get()).flags == hipHostMallocDefault);
  CHECK(block_of(coh.get()).pinned && block_of(coh.get()).flags == hipHostMallocCoherent);
  CHECK(hipHostMallocCoherent != hipHostMallocDefault);
  CHECK(dev.reserve(6) == hipSuccess && pin.reserve(6) == hipSuccess && coh.reserve(6) == hipSuccess);   // release() aborts on the wrong function
  CHECK(block_of(coh.get()).flags == hipHostMallocCoherent && g_live.size() == 3);
  Buffer<double> arr[2] = {Buffer<double>(Mem::Pinned), Buffer<double>(Mem::Pinned)};      // how the data object declares its pairs
  CHECK(arr[0].kind() == Mem::Pinned && arr[1].reserve(2) == hipSuccess && block_of(arr[1].get()).pinned);
}

static void test_slack_policy() {
  const size_t ask[3] = {1, 4000, 4096}, want[3] = {4096, 5000, 5120};               // at least 4096 bytes, otherwise a quarter more
  for (int k = 0; k < 3; k++) {
    Buffer<unsigned char> b(Mem::Pinned);
    CHECK(b.reserve(ask[k], true) == hipSuccess);
    CHECK(b.count() == want[k] && block_of(b.get()).bytes == want[k]);
    b.get()[want[k] - 1] = 1;
  }
  Buffer<unsigned char> b(Mem::Pinned);
  CHECK(b.reserve(4097, true) == hipSuccess && b.count() == 4097 + 1024);
  const long allocs = g_allocs;
  CHECK(b.reserve(5121, true) == hipSuccess && g_allocs == allocs);                   // inside the slack: no allocator call
  CHECK(b.reserve(5122, true) == hipSuccess && g_allocs == allocs + 1 && b.count() == 5122 + 5122 / 4);
}

static void test_arena() {
  const int N = 9;
  {
    Arena a;
    for (int k = 0; k < N; k++) {
      double* p = a.alloc<double>((size_t)k);                                          // count 0 still gives a block of one element
      CHECK(p && a.ok && block_of(p).bytes == (k ? k : 1) * sizeof(double) && !block_of(p).pinned);
      p[k ? k - 1 : 0] = 1.0;
    }
    CHECK(g_live.size() == (size_t)N);
  }
  CHECK(g_live.empty());                                                             // all N released
  for (int k = 1; k <= 4; k++) {                                                      // the k-th allocation fails
    {
      Arena a;
      g_fail_in = k;
      for (int i = 1; i <= 4; i++) {
        int* p = a.alloc<int>(3);
        CHECK((p == nullptr) == (i == k));
        CHECK(a.ok == (i < k));                                                        // reported, and stays reported
      }
      CHECK(g_live.size() == 3);
    }
    CHECK(g_live.empty());                                                           // what it held is still released
  }
}

int main() {
  test_reserve();
  test_kinds();
  CHECK(g_live.empty());
  test_slack_policy();
  test_arena();
  CHECK(g_live.empty() && g_fail_in == 0);                                             // nothing live at exit
  std::puts("buffer_host: ok");
  return 0;
}
