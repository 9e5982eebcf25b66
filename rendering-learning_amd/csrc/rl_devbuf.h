// Internal (not part of the ABI): the owners of everything the library allocates through HIP — device buffers (DevBuf), pinned host
// memory (PinnedBuf) and events (Event).  Each frees in its destructor, so a scene, a host-buffer entry point or the BVH builder releases
// what it holds on every path out.  Plain hipMalloc / hipFree: no pooling, no stream-ordered allocation.  Every device allocation
// passes through DevBuf, which is what rl_debug_live_buffers counts.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rl_render.h"

namespace rl {

int set_err_public(int code, const std::string &m);  // rl_render.hip

// device allocations the library owns right now: {count, bytes} (rl_debug_live_buffers)
inline std::atomic<unsigned long long> g_live_buffers{0}, g_live_bytes{0};

// `size()` elements of T in device memory.  Move-only; converts to T * wherever a raw pointer is read.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) release(), p_ = std::exchange(o.p_, nullptr), n_ = std::exchange(o.n_, 0);
    return *this;
  }
  ~DevBuf() { release(); }
  operator T *() const { return p_; }
  T *get() const { return p_; }  // where nothing asks for a T * by type: casts, template argument deduction
  size_t size() const { return n_; }  // capacity in elements
  void release() {
    if (!p_) return;
    hipFree(p_);
    g_live_buffers--, g_live_bytes -= n_ * sizeof(T);
    p_ = nullptr, n_ = 0;
  }
  // grow-only: nothing when `count` elements fit; otherwise the old buffer is freed FIRST and its contents are gone.  The caller orders
  // the free behind work in flight that still uses the old buffer (hipFree itself waits for the device).
  hipError_t reserve(size_t count) {
    if (count <= n_) return hipSuccess;
    release();
    hipError_t e = hipMalloc((void **)&p_, count * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    n_ = count;
    g_live_buffers++, g_live_bytes += n_ * sizeof(T);
    return hipSuccess;
  }
  // a fresh buffer holding v (one element's room for an empty vector, so that the pointer is never null).  RL_OK / RL_E_DEVICE.
  int upload(const std::vector<T> &v) {
    release();
    hipError_t e = reserve(v.size() ? v.size() : 1);
    if (e != hipSuccess) return set_err_public(RL_E_DEVICE, std::string("hipMalloc((void **)out, bytes): ") + hipGetErrorString(e));
    if (!v.empty() && (e = hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess)
      return set_err_public(RL_E_DEVICE, std::string("hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice): ") + hipGetErrorString(e));
    return RL_OK;
  }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};

// `count` elements of T in pinned host memory, allocated once (hipHostMalloc with `flags`)
template <class T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() {
    if (p_) hipHostFree(p_);
  }
  operator T *() const { return p_; }
  hipError_t reserve(size_t count, unsigned flags) { return p_ ? hipSuccess : hipHostMalloc((void **)&p_, count * sizeof(T), flags); }

 private:
  T *p_ = nullptr;
};

class Event {
 public:
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() {
    if (e_) hipEventDestroy(e_);
  }
  operator hipEvent_t() const { return e_; }
  hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }  // once; later calls keep it

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace rl
