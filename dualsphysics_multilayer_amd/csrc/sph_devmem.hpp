// sph_devmem.hpp — the owners of the host code's device memory (host only: no kernel file
// includes it).  DevArena: a list of allocations that live as long as their arena.  GrowBuf:
// one buffer that is replaced by a larger one when a step needs more than it holds.
#pragma once
#include <cstddef>

namespace sphx {

// Elements a growing buffer gets for a need of `need`: half as many again plus the buffer's
// floor, or exactly the need (the SPH_SLAB_MINCAP test hook, the RCCL gather scratch).
constexpr unsigned long long grown_capacity(unsigned long long need, unsigned long long floor, bool exact) {
  return exact ? need : need + need / 2 + floor;
}

}  // namespace sphx

// (a CPU test program of the capacity rule defines SPH_DEVMEM_CAPACITY_ONLY: no HIP headers)
#ifndef SPH_DEVMEM_CAPACITY_ONLY
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace sphx {

void check_hip(hipError_t e, const char* what);  // throws SphError (sph_solver.cpp)

class DevArena {
 public:
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() { clear(); }

  // `count` elements, at least 256 bytes; not initialised
  template <class T>
  T* alloc(size_t count) {
    void* p = nullptr;
    check_hip(hipMalloc(&p, std::max<size_t>(sizeof(T) * count, 256)), "hipMalloc");
    ptrs_.push_back(p);
    return static_cast<T*>(p);
  }
  // alloc + a synchronous copy of `count` elements from the host (none: nothing copied)
  template <class T>
  T* upload(const T* src, size_t count) {
    T* p = alloc<T>(count);
    if (count) check_hip(hipMemcpy(p, src, sizeof(T) * count, hipMemcpyHostToDevice), "upload");
    return p;
  }
  // frees one allocation of this arena and forgets it
  void release(void* p) {
    if (!p) return;
    (void)hipFree(p);
    ptrs_.erase(std::remove(ptrs_.begin(), ptrs_.end(), p), ptrs_.end());
  }
  void clear() {
    for (void* p : ptrs_) (void)hipFree(p);
    ptrs_.clear();
  }
  void swap(DevArena& o) { ptrs_.swap(o.ptrs_); }

 private:
  std::vector<void*> ptrs_;
};

template <class T>
class GrowBuf {
 public:
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { clear(); }

  T* ptr() const { return p_; }
  unsigned long long cap() const { return cap_; }  // elements
  // Room for `need` elements; true when the buffer was replaced (the old contents are gone).
  // Whatever still uses the old buffer is waited for by the caller, before the call.
  bool reserve(unsigned long long need, unsigned long long floor, bool exact) {
    if (need <= cap_) return false;
    resize(grown_capacity(need, floor, exact));
    return true;
  }
  // exactly `n` elements, whatever it held
  void resize(unsigned long long n) {
    clear();
    void* p = nullptr;
    check_hip(hipMalloc(&p, sizeof(T) * n), "hipMalloc growing buffer");
    p_ = static_cast<T*>(p);
    cap_ = n;
  }
  void clear() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  unsigned long long cap_ = 0;
};

}  // namespace sphx
#endif  // SPH_DEVMEM_CAPACITY_ONLY
