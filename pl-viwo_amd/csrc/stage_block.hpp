// stage_block.hpp — layout of one packed upload (jacobian_api.hip: the point and the line batch).  Arrays are added in the order
// they are to lie in the block, each starting on a 16-byte boundary, its size derived from its element type; the pinned and the
// device copy share every offset.  Fixed capacity, no allocation: the stagers run on the caller's thread in front of a launch.
// Plain C++ (tests/host_sanitize/stage_block_check.cpp compiles it on its own).
#pragma once
#include <cstddef>
#include <cstring>

namespace plv {

struct StageBlock {
  static constexpr int kMax = 48;
  template <class T> struct Slot {  // an array's place in the block; a default one is an array that is absent
    int i = -1;
    explicit operator bool() const { return i >= 0; }
  };
  static size_t padded(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

  // count elements of W values of T each, copied from src by copy_all (src null: room only, the caller fills host()); `spare`
  // more values are kept free behind them
  template <size_t W = 1, class T> Slot<T> add(const T *src, size_t count, size_t spare = 0) {
    if (n == kMax) {
      full = true;
      return {};
    }
    src_[n] = src, off_[n] = total_, copy_[n] = W * count * sizeof(T);
    total_ += padded(copy_[n] + spare * sizeof(T));
    return {n++};
  }
  template <class T, size_t W = 1> Slot<T> room(size_t count) { return add<W>((const T *)nullptr, count); }

  size_t total() const { return total_; }
  bool overflowed() const { return full; }
  template <class T> size_t offset(Slot<T> s) const { return off_[s.i]; }
  // fills the pinned block h (total() bytes); d is where its copy will lie on the device
  void copy_all(void *h, const void *d) {
    h_ = (char *)h, d_ = (const char *)d;
    for (int i = 0; i < n; ++i)
      if (src_[i] && copy_[i]) memcpy(h_ + off_[i], src_[i], copy_[i]);
  }
  const char *dev_base() const { return d_; }
  template <class T> T *host(Slot<T> s) const { return s ? (T *)(h_ + off_[s.i]) : nullptr; }
  template <class T> const T *dev(Slot<T> s) const { return s ? (const T *)(d_ + off_[s.i]) : nullptr; }

 private:
  const void *src_[kMax];
  size_t off_[kMax], copy_[kMax], total_ = 0;
  int n = 0;
  bool full = false;
  char *h_ = nullptr;
  const char *d_ = nullptr;
};

}  // namespace plv
