// match_block.hpp — device-free pieces of the point front ends (frontend_api.hip, stereo_api.hip): the layout of the temporal
// matching's block and the copy of a host image into a packed block.  Nothing of HIP is included: a plain C++ compiler checks it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace plv {

// One temporal matching of n points works on one block  [pts0 | pts1 | n0 | n1 | iters | mask | status]  — 2 floats per point in
// each of the first four fields, an int, and two bytes — on the device and in its pinned twin on the host: the host writes pts0 and
// the initial pts1, lk_kernel reads them there, and the matching's last kernel mirrors pts1 .. mask back.  With a base, the typed
// views of the fields; without one, the sizes alone.
struct MatchBlock {
  size_t n;
  char *base;
  explicit MatchBlock(size_t n_, void *base_ = nullptr) : n(n_), base((char *)base_) {}
  size_t o_pts0() const { return 0; }
  size_t o_pts1() const { return n * 8; }
  size_t o_n0() const { return n * 16; }
  size_t o_n1() const { return n * 24; }
  size_t o_iters() const { return n * 32; }
  size_t o_mask() const { return n * 36; }
  size_t o_status() const { return n * 37; }
  size_t total() const { return n * 38; }
  // pts1 .. iters: what the selection kernel copies into the pinned twin as words (it writes the twin's mask itself)
  size_t mirror_bytes() const { return o_mask() - o_pts1(); }
  // pts1 .. mask: everything the host reads back — what the copy command covers where no kernel mirrored
  size_t result_bytes() const { return o_status() - o_pts1(); }
  float *pts0() const { return (float *)(base + o_pts0()); }
  float *pts1() const { return (float *)(base + o_pts1()); }
  float *n0() const { return (float *)(base + o_n0()); }
  float *n1() const { return (float *)(base + o_n1()); }
  int *iters() const { return (int *)(base + o_iters()); }
  uint8_t *mask() const { return (uint8_t *)(base + o_mask()); }
  uint8_t *status() const { return (uint8_t *)(base + o_status()); }
};

// h rows of row_bytes each, `stride` bytes apart in src, packed into dst (nothing behind the last row's last byte is read)
inline void pack_rows(void *dst, const void *src, size_t stride, size_t row_bytes, int h) {
  if (stride == row_bytes) {
    memcpy(dst, src, row_bytes * (size_t)h);
    return;
  }
  for (int y = 0; y < h; ++y) memcpy((char *)dst + (size_t)y * row_bytes, (const char *)src + (size_t)y * stride, row_bytes);
}

}  // namespace plv
