// draw_kernels.hpp — the track image's rasteriser (draw_kernels.hip): tile shape, launch interface, the pixel predicates the kernel
// evaluates and the bounding box of a primitive, which the host uses to leave out what lies outside the image and the kernel to pick a
// tile's primitives.
#pragma once
#include <cmath>
#include <cstdint>

#include "plv_ctx.hpp"

namespace plv {

// Tile of one workgroup: 64 x 8 pixels, 256 threads, two pixels (rows r and r + 4 of one column) per thread.  A wave owns whole rows
// of 64 pixels = 192 contiguous bytes of the output.  Measured on the bench's boulevard scene (profiles/track_image.json "tile_heights"):
// a lower tile has a shorter list to paint from, but every workgroup walks the whole primitive list — 64 x 4 is the fastest at 752 x 480,
// 64 x 16 at 1280 x 720, 64 x 8 within 15 % of the better at both.
constexpr int DRAW_TILE_W = 64, DRAW_TILE_H = 8, DRAW_THREADS = 256;
// Primitives of one round in LDS (32 bytes each): 32 KB, so that four workgroups share a CU's 160 KB
constexpr int DRAW_LIST_CAP = 1024;

// pitch of the device RGB image: rows start on 4-byte boundaries so that a full tile row goes out as 48 dwords
inline size_t draw_rgb_pitch(int w) { return ((size_t)3 * w + 3) & ~(size_t)3; }

// Clipped-away test on the host and in the kernel's list stage: the inclusive bounding box of a primitive (conservative for a ring)
__host__ __device__ inline void draw_prim_bbox(const plv_draw_prim &p, long long &bx0, long long &by0, long long &bx1, long long &by1) {
  if (p.kind == PLV_DRAW_RING) {
    const long long r = p.b > 0 ? (long long)sqrtf((float)p.b) + 2 : 0;  // (>= sqrt(b): b < 2^31, the float's error is below 0.01)
    bx0 = (long long)p.x0 - r, bx1 = (long long)p.x0 + r, by0 = (long long)p.y0 - r, by1 = (long long)p.y0 + r;
    if (p.b < 0 || p.a > p.b) bx1 = bx0 - 1;  // empty
    return;
  }
  bx0 = p.x0 < p.x1 ? p.x0 : p.x1, bx1 = p.x0 < p.x1 ? p.x1 : p.x0;
  by0 = p.y0 < p.y1 ? p.y0 : p.y1, by1 = p.y0 < p.y1 ? p.y1 : p.y0;
  if (p.kind == PLV_DRAW_SEG) {
    const long long adx = bx1 - bx0, ady = by1 - by0;
    if (p.a < 1) {
      bx1 = bx0 - 1;  // no thickness: empty
      return;
    }
    if (adx >= ady)
      by1 += p.a - 1;
    else
      bx1 += p.a - 1;
  }
}

// the predicates of include/plviwo.h, one pixel against one primitive; every product is formed in 64 bits
__host__ __device__ inline bool draw_covers(int kind, int x0, int y0, int x1, int y1, int a, int b, int x, int y) {
  if (kind == PLV_DRAW_RING) {
    const long long dx = (long long)x - x0, dy = (long long)y - y0, d = dx * dx + dy * dy;
    return (long long)a <= d && d <= (long long)b;
  }
  if (kind == PLV_DRAW_BOX) {
    const int xa = x0 < x1 ? x0 : x1, xb = x0 < x1 ? x1 : x0, ya = y0 < y1 ? y0 : y1, yb = y0 < y1 ? y1 : y0;
    return ((x == xa || x == xb) && y >= ya && y <= yb) || ((y == ya || y == yb) && x >= xa && x <= xb);
  }
  // PLV_DRAW_SEG: u the major coordinate, v the minor one.  The pixel's minor offset k = floor(N / D) is tested as k D <= N < (k + 1) D
  // over the k's that the thickness allows, so no division is made.
  const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0;
  const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const bool xmajor = adx >= ady;
  const long long u = xmajor ? x : y, v = xmajor ? y : x, u0 = xmajor ? x0 : y0, u1 = xmajor ? x1 : y1, v0 = xmajor ? y0 : x0;
  const long long amaj = xmajor ? adx : ady, amin = xmajor ? ady : adx;
  const bool up = (xmajor ? dy : dx) >= 0;
  if (u < (u0 < u1 ? u0 : u1) || u > (u0 < u1 ? u1 : u0)) return false;
  const long long kl = up ? v - v0 - ((long long)a - 1) : v0 - v, kh = up ? v - v0 : v0 - v + ((long long)a - 1);
  if (amaj == 0) return kl <= 0 && 0 <= kh;
  const long long i = u < u0 ? u0 - u : u - u0, N = 2 * i * amin + amaj, D = 2 * amaj;
  return kl * D <= N && N < (kh + 1) * D;
}

// d_grey: w x h bytes, rows grey_pitch apart; d_mask: null or w x h bytes, rows mask_pitch apart; d_prims [n]; d_rgb: rows
// draw_rgb_pitch(w) apart.  Enqueued on the context's stream.
int launch_draw(plv_ctx *ctx, const uint8_t *d_grey, int grey_pitch, const uint8_t *d_mask, int mask_pitch, const plv_draw_prim *d_prims,
                int n, int w, int h, uint8_t *d_rgb);

}  // namespace plv
