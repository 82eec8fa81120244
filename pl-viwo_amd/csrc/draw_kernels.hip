// draw_kernels.hip — the track image's rasteriser for gfx950 (include/plviwo.h "track image", DESIGN.md "The track image").
//
// One workgroup per 64 x 8 tile.  The primitive list is walked FROM THE BACK in rounds: 256 threads test 256 primitives' clipped
// bounding boxes against the tile, a wave ballot + a prefix over the four waves' counts compacts the hits into an LDS list that keeps
// their order (no atomics), and once the list is full (or the primitives are used up) every thread scans it front to back — that is,
// last-painted first — for each of its two pixels and stops at the first primitive whose predicate holds.  An entry carries its box
// clipped to the tile: a wave whose rows the box misses passes it with one test, a lane whose column it misses never forms a product.
// A pixel that found its colour is final, whatever earlier primitives say, so a list that does not fit LDS costs further rounds and
// never a truncation; a tile whose pixels are all final stops reading the list.  What nothing covers takes the grey image's value, the mask rule runs in the same
// pass, and a wave writes its row of 64 pixels as 48 dwords (two cross-lane reads pack the 3-byte pixels) or, at the image's right edge,
// pixel by pixel.  The result depends on the list's order alone: no run-time scheduling enters it.
#include "draw_kernels.hpp"

namespace plv {
namespace {

// thread (wave, lane) owns column `lane` of the tile's rows wave, wave + 4, ...: PX pixels
constexpr int PX = DRAW_TILE_H / 4;

__global__ void __launch_bounds__(DRAW_THREADS) draw_tile_kernel(const uint8_t *__restrict__ grey, int grey_pitch, const uint8_t *__restrict__ mask,
                                                                 int mask_pitch, const plv_draw_prim *__restrict__ prims, int n, int W, int H,
                                                                 uint8_t *__restrict__ rgb, int rgb_pitch) {
  constexpr int TILE_H = DRAW_TILE_H;
  // entry e: {kind | the bounding box clipped to the tile (local x0, x1: 6 bits each, y0, y1: 4 bits each) << 2, x0, y0, x1}, {y1, a, b, colour}
  __shared__ int4 list[2 * DRAW_LIST_CAP];
  __shared__ int wcount[2][DRAW_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tx0 = blockIdx.x * DRAW_TILE_W, ty0 = blockIdx.y * TILE_H;
  const int tx1 = min(tx0 + DRAW_TILE_W, W) - 1, ty1 = min(ty0 + TILE_H, H) - 1;
  const int x = tx0 + lane;
  unsigned col[PX];
  int open = 0;  // bit j: pixel (x, ty0 + wave + 4 j) lies in the image and has no colour yet
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    col[j] = 0;
    if (x < W && ty0 + wave + 4 * j < H) open |= 1 << j;
  }
  const int mine = open;
  int next = n, par = 0;  // primitives [0, next) have not been looked at
  bool alive = true;
  while (next > 0 && alive) {
    int list_n = 0;
    while (next > 0 && list_n + DRAW_THREADS <= DRAW_LIST_CAP) {
      const int i = next - 1 - t;
      bool hit = false;
      int4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
      if (i >= 0) {
        const int4 *src = reinterpret_cast<const int4 *>(prims + i);
        lo = src[0], hi = src[1];
        plv_draw_prim p;
        p.kind = lo.x, p.x0 = lo.y, p.y0 = lo.z, p.x1 = lo.w, p.y1 = hi.x, p.a = hi.y, p.b = hi.z;
        long long bx0, by0, bx1, by1;
        draw_prim_bbox(p, bx0, by0, bx1, by1);
        hit = bx0 <= bx1 && bx0 <= tx1 && bx1 >= tx0 && by0 <= ty1 && by1 >= ty0;
        if (hit) {
          const int lx0 = (int)max(bx0, (long long)tx0) - tx0, lx1 = (int)min(bx1, (long long)tx1) - tx0;
          const int ly0 = (int)max(by0, (long long)ty0) - ty0, ly1 = (int)min(by1, (long long)ty1) - ty0;
          lo.x = (lo.x & 3) | lx0 << 2 | lx1 << 8 | ly0 << 14 | ly1 << 18;
          hi.w &= 0xffffff;
        }
      }
      const unsigned long long m = __ballot(hit);
      if (lane == 0) wcount[par][wave] = __popcll(m);
      __syncthreads();
      int off = list_n, total = 0;
      for (int w = 0; w < DRAW_THREADS / 64; ++w) {
        const int c = wcount[par][w];
        off += w < wave ? c : 0;
        total += c;
      }
      if (hit) {
        const int at = off + __popcll(m & ((1ull << lane) - 1ull));
        list[2 * at] = lo, list[2 * at + 1] = hi;
      }
      list_n += total;
      next -= DRAW_THREADS;
      par ^= 1;  // (the next step's counts go to the other row: one barrier per step is enough)
    }
    __syncthreads();
    for (int e = 0; e < list_n && open; ++e) {
      const int4 lo = list[2 * e];
      const int ly0 = lo.x >> 14 & 15, ly1 = lo.x >> 18 & 15;
      // the rows are the same for the whole wave: an entry whose box misses them costs the wave this test and nothing else
      int rows = 0;
#pragma unroll
      for (int j = 0; j < PX; ++j) rows |= (wave + 4 * j >= ly0 && wave + 4 * j <= ly1) ? 1 << j : 0;
      if (!rows || lane < (lo.x >> 2 & 63) || lane > (lo.x >> 8 & 63) || !(rows & open)) continue;
      const int4 hi = list[2 * e + 1];
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (((rows & open) >> j & 1) && draw_covers(lo.x & 3, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, x, ty0 + wave + 4 * j)) {
          col[j] = (unsigned)hi.w;
          open &= ~(1 << j);
        }
    }
    alive = __syncthreads_or(open != 0) != 0;  // (also: nobody reads the list any more)
  }
  const bool full_row = tx0 + DRAW_TILE_W <= W;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int y = ty0 + wave + 4 * j;  // the same for the whole wave
    if (y >= H) break;
    unsigned c = col[j];
    if (mine >> j & 1) {
      if (open >> j & 1) {
        const unsigned g = grey[(size_t)y * grey_pitch + x];
        c = g | g << 8 | g << 16;
      }
      if (mask && mask[(size_t)y * mask_pitch + x]) {
        const unsigned c2 = c >> 16;
        c = (c & 0xffffu) | min(255u, c2 + ((c2 & 1u) ? 25u : 26u)) << 16;
      }
    }
    uint8_t *row = rgb + (size_t)y * rgb_pitch + (size_t)3 * tx0;
    if (full_row) {  // 64 pixels = 48 dwords: dword d holds the bytes 4 d .. 4 d + 3 of the row, which lie in the pixels p and p + 1
      const int d = lane < 48 ? lane : 47, p = (4 * d) / 3, sh = 8 * ((4 * d) % 3);
      const unsigned a = __shfl(c, p), b = __shfl(c, p + 1);
      if (lane < 48) reinterpret_cast<unsigned *>(row)[lane] = sh ? (a >> sh) | (b << (24 - sh)) : a | (b << 24);
    } else if (x < W) {
      row[3 * lane] = (uint8_t)c, row[3 * lane + 1] = (uint8_t)(c >> 8), row[3 * lane + 2] = (uint8_t)(c >> 16);
    }
  }
}

}  // namespace

int launch_draw(plv_ctx *ctx, const uint8_t *d_grey, int grey_pitch, const uint8_t *d_mask, int mask_pitch, const plv_draw_prim *d_prims,
                int n, int w, int h, uint8_t *d_rgb) {
  if (!d_grey || !d_rgb || w < 1 || h < 1 || n < 0 || (n > 0 && !d_prims) || grey_pitch < w || (d_mask && mask_pitch < w)) {
    set_last_error("draw: a %d x %d image, %d primitives, pitches %d / %d", w, h, n, grey_pitch, mask_pitch);
    return PLV_E_BADARG;
  }
  if ((((uintptr_t)d_rgb) & 3) || (((uintptr_t)d_prims) & 15)) {
    set_last_error("draw: the output must lie on a 4-byte boundary and the primitives on a 16-byte one");
    return PLV_E_BADARG;
  }
  ProfScope ps(ctx->prof, "draw_tile_kernel", ctx->stream);
  const dim3 grid((w + DRAW_TILE_W - 1) / DRAW_TILE_W, (h + DRAW_TILE_H - 1) / DRAW_TILE_H);
  hipLaunchKernelGGL(draw_tile_kernel, grid, dim3(DRAW_THREADS), 0, ctx->stream, d_grey, grey_pitch, d_mask, mask_pitch, d_prims, n, w, h, d_rgb,
                     (int)draw_rgb_pitch(w));
  PLV_HIP_CHECK(hipGetLastError());
  return PLV_OK;
}

}  // namespace plv
