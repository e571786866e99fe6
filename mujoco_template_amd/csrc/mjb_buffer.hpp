// mjb_buffer.hpp — the two owners of device / pinned-host memory behind the C ABI (mjb_api.hip).  Host-only: no kernels, no __device__
// code.  The structs the kernels receive keep raw pointers; they borrow `.get()` from a Buffer or take an Arena allocation.
#pragma once
#include <hip/hip_runtime_api.h>
#include <vector>

namespace mjb {
enum class Mem { Device, Pinned, PinnedCoherent };   // hipMalloc / hipHostMalloc(Default) / hipHostMalloc(Coherent)

// One block of `count()` elements that can grow.  The kind is fixed at construction and decides the release function.
template <typename X> class Buffer {
 public:
  explicit Buffer(Mem kind = Mem::Device) : kind_(kind) {}
  Buffer(const Buffer&) = delete; Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { reset(); }
  X* get() const { return p_; }
  size_t count() const { return n_; }
  Mem kind() const { return kind_; }
  // At least `count` elements: a no-op when they are there, else the old block goes and a new one of exactly `count` comes (contents
  // are not kept).  With `slack` the new block is a quarter larger than asked for and at least 4096 bytes.  On failure the buffer
  // is empty.  A caller whose old block may still be in use by a stream drains that stream first.
  hipError_t reserve(size_t count, bool slack = false) {
    if (count <= n_) return hipSuccess;
    reset();
    size_t bytes = count * sizeof(X);
    if (slack) bytes = bytes + bytes / 4 < 4096 ? 4096 : bytes + bytes / 4;
    void* p = nullptr;
    const hipError_t e = kind_ == Mem::Device ? hipMalloc(&p, bytes)
                                              : hipHostMalloc(&p, bytes, kind_ == Mem::Pinned ? hipHostMallocDefault : hipHostMallocCoherent);
    if (e == hipSuccess) { p_ = (X*)p; n_ = bytes / sizeof(X); }
    return e;
  }
  void reset() {
    if (p_) (void)(kind_ == Mem::Device ? hipFree(p_) : hipHostFree(p_));
    p_ = nullptr; n_ = 0;
  }
 private:
  Mem kind_; X* p_ = nullptr; size_t n_ = 0;
};

// Device blocks of fixed lifetime: handed out one by one, released together by the destructor.
struct Arena {
  bool ok = true;                                  // false once an allocation has failed
  std::vector<void*> ptrs;
  Arena() = default;
  Arena(const Arena&) = delete; Arena& operator=(const Arena&) = delete;
  ~Arena() { for (void* p : ptrs) (void)hipFree(p); }
  template <typename X> X* alloc(size_t count) {   // never an empty block: count 0 gives one element
    void* p = nullptr;
    if (hipMalloc(&p, (count ? count : 1) * sizeof(X)) != hipSuccess) { ok = false; return nullptr; }
    ptrs.push_back(p);
    return (X*)p;
  }
};
}  // namespace mjb
