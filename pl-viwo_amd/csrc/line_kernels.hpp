// line_kernels.hpp — device buffers and launcher of the line detector (line_kernels.hip).
#pragma once
#include <cstdint>

#include "plv_ctx.hpp"

namespace plv {

struct FldChain {
  int start, len, slot;  // points [start, start+len) of the chain buffer; first output slot
};
struct FldComp {  // a component of the edge map that can hold a kept chain (plv_line_walk_mode 2)
  int root, cnt, pts_off, rec_off;  // root label, pixels, first point owned, first chain record owned
  int x0, x1, y1, n_rec;            // bounding box (its first row is the root's), chains kept
};
struct FldRec {
  int seed, start, len;  // a kept chain of a component: raster index of its seed, its points
};
const size_t kLineWalkLdsMax = 64 * 1024;  // the component walk's bit map of the half-resolution image must fit (1 bit per pixel)
struct FldParams {
  int length_threshold;      // 20   REF: TrackLSD.h:269
  float distance_threshold;  // sqrt(2)   :270
  int canny_low, canny_high; // 50, 50   :271-272 (aperture 3 is what canny_kernel implements)
};
struct FldBuffers {
  uint8_t *half, *map, *work;  // half-resolution image, Canny map (0 weak / 1 none / 2 edge), walk scratch
  int2 *pts;
  FldChain *chains;
  int chain_cap;
  int *counts;     // [0] chains, [1] segment slots, [2] points
  float4 *segs;    // segment slots, chain c writes segs[chain.slot ...]
  int *seg_count;  // [chain_cap]
  int *lab_work = nullptr;      // [w*h] union-find forest of the component labelling (null: no labels for this detection)
  int *lab_cnt = nullptr;       // [w*h] pixels per component at its root, then -(part) there
  int *lab_roots = nullptr;     // [line_label_roots_bytes()] the roots' list and its counter
  uint8_t *lab_out = nullptr;   // [w*h] parts, host-visible (0 not an edge, else 1 .. line_label_parts())
  // (nullable, host-visible) the parts' pixels in raster order, per run of 256 pixels: see ccl_flatten_kernel
  uint8_t *blk_sorted = nullptr;        // [256 * ceil(w*h / 256)]
  unsigned short *blk_bins = nullptr;   // [ceil(w*h / 256)][line_label_parts() + 1]
  // component-parallel walk (plv_line_walk_mode 2; null otherwise)
  FldComp *comps = nullptr;        // [line_walk_components_cap()]
  FldRec *recs = nullptr;          // [w*h / (length_threshold + 1) + 1] chain records, by component
  FldRec *recs_sorted = nullptr;   // [same] gathered
  int *walk_info = nullptr;        // [8] see fld_components_kernel
};

// d_hist: d_img is the RAW image and d_hist its histogram (the kernel equalises on the fly: canny_kernel); null: d_img is the equalised image
int launch_line_edges(plv_ctx *ctx, const uint8_t *d_img, int W, int H, const FldParams &fp, FldBuffers &b, hipStream_t st = nullptr /* default: the ctx stream */,
                      const unsigned *d_hist = nullptr);
int launch_line_labels(plv_ctx *ctx, int w, int h, FldBuffers &b, hipStream_t st, int length_threshold);
int line_label_parts();         // parts launch_line_labels writes (the largest components first: 1 .. 8, then 8 hashed ones)
size_t line_label_roots_bytes();
// gate (nullable, device): the kernel runs only when *gate != 0 (the fallback of the component-parallel walk)
int launch_line_walk(plv_ctx *ctx, int w, int h, const FldParams &fp, FldBuffers &b, const int *gate = nullptr);
int launch_line_fit(plv_ctx *ctx, int w, int h, const FldParams &fp, FldBuffers &b, const int *gate = nullptr);
size_t line_walk_lds_bytes(int w, int h);
int line_walk_components_cap();
int launch_line_walk_components(plv_ctx *ctx, int w, int h, const FldParams &fp, FldBuffers &b);

}  // namespace plv
