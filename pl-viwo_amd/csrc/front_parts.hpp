// front_parts.hpp — the pieces of the point front end (frontend_api.hip) that take the pyramid they work on as an argument, so that
// the stereo tracker (stereo_api.hip) runs them on its own two cameras' pyramids.  The monocular path calls the same functions on
// the context's one camera (FrontState).
#pragma once
#include <vector>

#include "frontend_kernels.hpp"

namespace plv {

struct DetJob {  // one top-up detection between its host stages (plv_perform_detection / _ahead)
  std::vector<uint8_t> close;        // occupancy grid of the kept points (min_px_dist cells)
  std::vector<int> boxes, cells;
  std::vector<float> pts;            // kept points
  std::vector<uint64_t> ids;
  int cw = 0, ch = 0, nfg = 0, sxp = 0, syp = 0, n_cells = 0, n_slots = 0;
  char *h_out = nullptr;             // pinned: [xy n_slots x 2 f32][resp n_slots f32][valid n_slots u8][over n_cells u8]
  // what an ahead-of-time job was started from
  bool active = false, has_mask = false;
  int fed = 0, n_in = 0;
  std::vector<float> in_pts;
  std::vector<uint64_t> in_ids;
  std::vector<uint8_t> in_mask;
};

struct DetScratch {  // detection staging of one camera
  DevBuf det_in, det_out, det_mask, subpix_tab, det_cand, det_cand_n;
  PinBuf det_pin;
  void release_detection() {
    DevBuf *bufs[] = {&det_in, &det_out, &det_mask, &subpix_tab, &det_cand, &det_cand_n};
    for (auto *b : bufs) b->release();
    det_pin.release();
  }
};

// Where perform_detection_stereo departs from perform_detection_monocular (REF: TrackKLT.cpp:530-827); null: the monocular rules.
struct DetStereoRules {
  // the top-up runs when  num_features - n  >  min(20, 0.5 num_features)  (:609, :785; the monocular test returns on  <, :470)
  bool strict_need = true;
  // right camera (:754-759): a point whose id is in this list (the left camera's) survives an occupied min_px_dist cell
  const uint64_t *spared = nullptr;
  int n_spared = 0;
};

// geometry of cv::buildOpticalFlowPyramid's levels, packed into one allocation; returns its size in bytes
int level_geometry(int W, int H, int win, int max_level, PyrDesc &p);
// equalisation (or CLAHE, or nothing: cfg.histogram_method) of the packed W x H device image d_img and its pyramid into p, enqueued;
// h_src != null: d_img is still empty and the image sits in pinned host memory at h_src
int front_feed_pyramid(plv_ctx *ctx, int W, int H, const uint8_t *d_img, const uint8_t *h_src, const PyrDesc &p, DevBuf &hist, DevBuf &clahe_lut);
int check_encoded(const char *who, const uint8_t *data, int stride, int encoding, int w);

// the three stages of a top-up detection on a w x h image (see plv_perform_detection); `mask` of det_pre is the one the points and
// the grid cells are tested against, `mask` of det_launch the one the corners are (with the kept points' boxes painted in)
int det_pre(plv_ctx *ctx, int w, int h, const uint8_t *mask, const float *pts_in, const uint64_t *ids_in, int n_in, DetJob &J,
            const DetStereoRules *stereo = nullptr);
int det_launch(plv_ctx *ctx, DetScratch &s, int w, int h, const PyrDesc &pyr, const uint8_t *mask, DetJob &J, hipStream_t stream);
int det_check(const DetJob &J);
void det_post(plv_ctx *ctx, const DetJob &J, float *pts, uint64_t *ids, int cap, uint64_t *currid, int *n_out);
// det_post's rejection near existing points without its id assignment: the accepted corners in extraction order (2 floats each)
void det_new_points(plv_ctx *ctx, const DetJob &J, std::vector<float> &out);

}  // namespace plv
