// front_parts.hpp — the pieces of the point front end (frontend_api.hip) that take the pyramid they work on as an argument, so that
// the stereo tracker (stereo_api.hip) runs them on its own two cameras' pyramids.  The monocular path calls the same functions on
// the context's one camera (FrontState).  Both keep a camera's images in a CamFront and run a temporal matching's tail through
// match_ransac_tail / match_read_back on the block of match_block.hpp.
#pragma once
#include <algorithm>
#include <vector>

#include "frontend_kernels.hpp"
#include "match_block.hpp"
#include "plv_internal.hpp"

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

// geometry of cv::buildOpticalFlowPyramid's levels, packed into one allocation; returns its size in bytes
int level_geometry(int W, int H, int win, int max_level, PyrDesc &p);

struct CamFront {  // one camera's images on the device
  int W = 0, H = 0;
  PyrDesc pyr[2];  // ping-pong pyramids
  DevBuf pyr_mem[2];
  int cur = 0;     // index of the current pyramid; last = 1 - cur
  int fed = 0;     // number of images fed so far (last is valid when fed >= 2)
  DevBuf raw;      // incoming raw image (packed)
  DevBuf hist, clahe_lut;
  DetScratch det;
  bool prepared() const { return raw.p != nullptr; }
  // pyramids for the context's window, histogram (zeroed on the stream) and raw image of W x H, once; `who` refuses an image too small
  int prepare(plv_ctx *ctx, const char *who) {
    if (prepared()) return PLV_OK;
    if (W < 16 || H < 16) {
      set_last_error("%s: image %dx%d too small", who, W, H);
      return PLV_E_BADARG;
    }
    for (int i = 0; i < 2; ++i) {
      const int bytes = level_geometry(W, H, ctx->cfg.win_size, ctx->cfg.pyr_levels, pyr[i]);
      TRY(pyr_mem[i].reserve((size_t)bytes));
      pyr[i].base = pyr_mem[i].as<uint8_t>();
    }
    TRY(hist.reserve(257 * sizeof(unsigned)));  // 256 bins + arrival counter; the pyramid launch leaves it zero for the next image
    PLV_HIP_CHECK(hipMemsetAsync(hist.p, 0, 257 * sizeof(unsigned), ctx->stream));
    return raw.reserve((size_t)W * H);
  }
  void release() {
    DevBuf *bufs[] = {&pyr_mem[0], &pyr_mem[1], &raw, &hist, &clahe_lut};
    for (auto *b : bufs) b->release();
    det.release_detection();
  }
  // the pyramid levels a win x win LK window gives on this image (the caller compares with pyr[0].levels and words the refusal)
  int levels_for(const plv_ctx *ctx, int win) const {
    PyrDesc want{};
    (void)level_geometry(W, H, win, ctx->cfg.pyr_levels, want);
    return want.levels;
  }
  // the pyramid the next image goes into; commit() once everything of that image is enqueued
  int next() const { return fed == 0 ? cur : 1 - cur; }
  void commit(int next) { cur = next, ++fed; }
  // equalised level-0 image of the current (which = PLV_PYR_CUR) or previous (PLV_PYR_LAST) frame; null before it has been fed
  const uint8_t *level0(int which, int *w, int *h) const {
    if (fed < (which == PLV_PYR_LAST ? 2 : 1)) return nullptr;
    const PyrDesc &p = pyr[which == PLV_PYR_LAST ? 1 - cur : cur];
    if (w) *w = p.w[0];
    if (h) *h = p.h[0];
    return p.base + p.off[0];
  }
};

struct RansacScratch {  // launch_ransac's device scratch
  DevBuf counts, models, info;
  int reserve(int max_iters) {
    const size_t mi = (size_t)std::max(max_iters, 1);
    TRY(counts.reserve(mi * 3 * 4));
    TRY(models.reserve(mi * 28 * 8));
    return info.reserve(16);
  }
  void release() { counts.release(), models.release(), info.release(); }
};

// A temporal matching behind its LK launch: RANSAC on the normalised points n0 / n1 of the device block (a findFundamentalMat call
// of its own in the reference: the seed of a fresh call, the camera's larger focal length), whose last kernel mirrors pts1 .. mask
// into the pinned block; where no such kernel ran, a copy command does.
inline int match_ransac_tail(plv_ctx *ctx, const CamK &K, const MatchBlock &dev, const MatchBlock &pin, RansacScratch &r) {
  const double fmax = std::max(K.v[0], K.v[1]);
  bool mirrored = false;
  TRY(launch_ransac(ctx, dev.n0(), dev.n1(), (int)dev.n, ctx->cfg.ransac_thr_px / fmax, ctx->cfg.ransac_conf, std::max(1, ctx->cfg.ransac_max_iters),
                    0u, r.counts.as<int>(), dev.status(), dev.mask(), r.info.as<int>(), r.models.as<double>(), dev.pts1(), pin.pts1(),
                    dev.mirror_bytes(), pin.mask(), &mirrored));
  if (!mirrored) PLV_HIP_CHECK(plv::memcpy_async(pin.pts1(), dev.pts1(), dev.result_bytes(), hipMemcpyDeviceToHost, ctx->stream));
  return PLV_OK;
}
// ... and once the host has waited for it: positions, inlier mask and (n0, n1 may be null) normalised points out of the pinned
// block; returns the sum of the LK iterations, counted in counters().lk_iters
inline long long match_read_back(const MatchBlock &pin, float *pts1, uint8_t *mask, float *n0, float *n1) {
  memcpy(pts1, pin.pts1(), pin.n * 8);
  if (n0) memcpy(n0, pin.n0(), pin.n * 8);
  if (n1) memcpy(n1, pin.n1(), pin.n * 8);
  memcpy(mask, pin.mask(), pin.n);
  long long t = 0;
  const int *it = pin.iters();
  for (size_t i = 0; i < pin.n; ++i) t += it[i];
  plv::counters().lk_iters += (unsigned long long)t;
  return t;
}

// Where perform_detection_stereo departs from perform_detection_monocular (REF: TrackKLT.cpp:530-827); null: the monocular rules.
struct DetStereoRules {
  // the top-up runs when  num_features - n  >  min(20, 0.5 num_features)  (:609, :785; the monocular test returns on  <, :470)
  bool strict_need = true;
  // right camera (:754-759): a point whose id is in this list (the left camera's) survives an occupied min_px_dist cell
  const uint64_t *spared = nullptr;
  int n_spared = 0;
};

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
