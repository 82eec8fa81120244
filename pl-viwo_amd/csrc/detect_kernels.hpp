// detect_kernels.hpp — parameters of fast_cells_kernel / subpix_kernel.
#pragma once
#include "plv_ctx.hpp"

namespace plv {

struct DetectParams {
  const uint8_t *img;   // level-0 (equalised) image, packed
  int W, H;
  const uint8_t *mask;  // optional W x H, > 127 = masked
  const int *cells;     // [n_cells][2] grid coordinates of the cells to extract from
  int cell_w, cell_h;
  int threshold, nfg;
  int cand_cap;         // keys stored per cell (global memory): at least fast_cell_bound(cell_w, cell_h), so that no maximum is dropped
  int lds_cap;          // keys fast_topk_kernel stages in LDS; a cell with more of them selects its nfg best from the stored list first
  const int *boxes;    // [n_boxes][2] integer positions of the tracked points whose +-min_px_dist box is masked
  int n_boxes, min_px_dist;
  float *out_xy;        // [n_cells * nfg][2]
  float *out_resp;      // [n_cells * nfg]
  uint8_t *out_valid;   // [n_cells * nfg]
  uint8_t *out_over;    // [n_cells] 1: the cell had more maxima than cand_cap, its slots are not to be used
};

// most local maxima a cw x ch cell can have: FAST skips a 3-pixel border and strict 3x3 suppression leaves one per 2x2 block
inline int fast_cell_bound(int cw, int ch) {
  if (cw < 7 || ch < 7) return 0;
  const long long b = (long long)((cw - 6 + 1) / 2) * ((ch - 6 + 1) / 2);
  return b > 0x7fffffff ? 0x7fffffff : (int)b;
}

int launch_fast_cells(plv_ctx *ctx, const DetectParams &P, int n_cells, unsigned long long *d_cand, int *d_cand_n);
int launch_subpix(plv_ctx *ctx, const uint8_t *d_img, int W, int H, int n, const uint8_t *d_valid, float *d_xy,
                  const float *d_mask, int win, int max_iters, double eps);

}  // namespace plv
