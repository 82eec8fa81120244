// stereo_api.hip — the stereo point tracker behind plv_stereo_* / plv_tracker_feed_stereo: host mirror of
//   TrackKLT::feed_new_camera (two images) / feed_stereo   REF: open_vins/ov_core/src/track/TrackKLT.cpp:34-94, 202-393
//   TrackKLT::perform_detection_stereo                     REF: TrackKLT.cpp:530-827
//   FeatureDatabase with ov_core::Feature's per-camera observations
// A second tracker beside the monocular one of tracker_api.hip: its own ping-pong pyramids per camera, last masks, last points, one
// id counter, one database.  The bookkeeping is the reference's, on the host; the image and point work goes through the launchers
// the monocular path uses (front_parts.hpp, frontend_kernels.hpp), with the two temporal matchings of a frame in one LK launch
// (launch_lk_pair) and one wait.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "camera_tracks.hpp"
#include "encoding_kernels.hpp"
#include "front_parts.hpp"
#include "plv_internal.hpp"
#include "update_tail.hpp"

using namespace plv;

namespace {

struct StereoCam : CamFront {  // (cur and fed move in step in both cameras)
  PinBuf img_pin;  // the host image on its way to the device (packed, in its encoding): the caller's buffer is free at return
  DevBuf io;                        // the temporal matching's block (MatchBlock)
  RansacScratch ransac;
  PinBuf flow_pin;                  // ... its host twin (points in, results out)
  std::vector<float> pts_last;      // 2 per point
  std::vector<uint64_t> ids_last;
  std::vector<uint8_t> mask_last;   // W*H or empty
  double K[8] = {};                 // camera 1 only: camera 0 is the context's (cfg.intrinsics, plv_ctx::cam_model)
  int model = PLV_CAM_RADTAN;
};

struct Stereo {
  bool configured = false;
  int W = 0, H = 0;
  StereoCam cam[2];
  int cur() const { return cam[0].cur; }  // index of the current pyramids (both cameras are fed in step); last = 1 - cur
  uint64_t currid = 0;  // REF: TrackBase::currid, shared by both cameras
  std::unordered_map<uint64_t, StereoFeature> db;
  DevBuf lr_dev;  // left-to-right LK of new left corners: [pts1 | status | iters]
  PinBuf lr_pin;  // ... [pts0 | pts1 | status]
  bool unsynced = false;  // kernels that read img_pin may still be on the stream
  std::mutex mtx;
};

std::mutex g_mtx;
Stereo *stereo_of(plv_ctx *ctx, bool create) {
  std::lock_guard<std::mutex> lk(g_mtx);
  if (!ctx->stereo_state && create) ctx->stereo_state = new Stereo();
  return (Stereo *)ctx->stereo_state;
}

int sync(plv_ctx *ctx, Stereo *S) {
  TRY(stream_wait(ctx));
  S->unsynced = false;
  return PLV_OK;
}

CamK cam_k(plv_ctx *ctx, const Stereo *S, int c) {
  CamK K;
  for (int i = 0; i < 8; ++i) K.v[i] = c == 0 ? ctx->cfg.intrinsics[i] : S->cam[1].K[i];
  K.model = c == 0 ? ctx->cam_model : S->cam[1].model;
  return K;
}

bool bad_cam(int cam, const char *who) {
  if (cam == 0 || cam == 1) return false;
  set_last_error("%s: camera %d, a stereo pair has cameras 0 and 1", who, cam);
  return true;
}

// one image of the pair: into the camera's pinned block, [conversion,] equalisation and pyramid into pyramid `next` — all enqueued
int enqueue_image(plv_ctx *ctx, Stereo *S, int c, int next, const uint8_t *img, int stride, int encoding) {
  StereoCam &C = S->cam[c];
  const size_t row = (size_t)S->W * encoding_bpp(encoding);
  TRY(C.img_pin.reserve(row * S->H));
  uint8_t *pin = C.img_pin.as<uint8_t>();
  pack_rows(pin, img, (size_t)stride, row, S->H);
  S->unsynced = true;
  if (encoding == PLV_ENC_MONO8)  // (the histogram kernel reads the pinned block and leaves the image in C.raw)
    return front_feed_pyramid(ctx, S->W, S->H, C.raw.as<uint8_t>(), pin, C.pyr[next], C.hist, C.clahe_lut);
  TRY(launch_grey_from_encoded(ctx, pin, true, C.raw.as<uint8_t>(), S->W, S->H, encoding));
  return front_feed_pyramid(ctx, S->W, S->H, C.raw.as<uint8_t>(), nullptr, C.pyr[next], C.hist, C.clahe_lut);
}

// cv::calcOpticalFlowPyrLK(left pyramid, right pyramid of the same time, p, p, USE_INITIAL_FLOW)   REF :661-672
int track_left_to_right(plv_ctx *ctx, Stereo *S, int which, const std::vector<float> &p0, std::vector<float> &p1, std::vector<uint8_t> &status) {
  const size_t n = p0.size() / 2;
  TRY(S->lr_pin.reserve(n * 17));
  TRY(S->lr_dev.reserve(n * 13 + 16));
  char *hp = S->lr_pin.as<char>(), *dp = S->lr_dev.as<char>();
  memcpy(hp, p0.data(), n * 8);
  float *d_p1 = (float *)dp;
  int *d_it = (int *)(dp + n * 8);
  uint8_t *d_st = (uint8_t *)(dp + n * 12);
  // (both cameras have the context's width x height and one window: the two pyramids have the same level geometry, which is all
  // lk_kernel asks of its (prev, cur) pair)
  TRY(launch_lk(ctx, S->cam[0].pyr[which], S->cam[1].pyr[which], (int)n, (const float *)hp, d_p1, d_st, d_it, ctx->cfg.win_size,
                ctx->cfg.lk_max_iters, ctx->cfg.lk_eps, nullptr, nullptr, nullptr, (const float *)hp));
  PLV_HIP_CHECK(plv::memcpy_async(hp + n * 8, d_p1, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(hp + n * 16, d_st, n, hipMemcpyDeviceToHost, ctx->stream));
  TRY(sync(ctx, S));
  p1.assign((const float *)(hp + n * 8), (const float *)(hp + n * 8) + 2 * n);
  status.assign((const uint8_t *)(hp + n * 16), (const uint8_t *)(hp + n * 16) + n);
  return PLV_OK;
}

// the corners one camera's top-up extracts and keeps: FAST per cell + sub-pixel on level 0 of pyramid `which`, rejection near the
// kept points (J); mask_dev is what the corners are tested against
int extract_corners(plv_ctx *ctx, Stereo *S, int c, int which, const uint8_t *mask_dev, DetJob &J, std::vector<float> &fresh) {
  fresh.clear();
  if (J.n_slots <= 0) return PLV_OK;
  TRY(det_launch(ctx, S->cam[c].det, S->W, S->H, S->cam[c].pyr[which], mask_dev, J, ctx->stream));
  TRY(sync(ctx, S));
  TRY(det_check(J));
  det_new_points(ctx, J, fresh);
  return PLV_OK;
}

// TrackKLT::perform_detection_stereo on pyramids `which` of both cameras; the four lists are pruned and topped up in place
int detection_stereo(plv_ctx *ctx, Stereo *S, int which, const uint8_t *mask0, const uint8_t *mask1, std::vector<float> &pts0,
                     std::vector<uint64_t> &ids0, std::vector<float> &pts1, std::vector<uint64_t> &ids1) {
  plv::HostPhase ph("stereo feed: perform_detection_stereo");
  const int W = S->W, H = S->H;
  auto in_image = [W, H](float x, float y) { return !((int)x < 0 || (int)x >= W || (int)y < 0 || (int)y >= H); };
  // ---- LEFT  :537-710
  DetStereoRules left;
  DetJob J0;
  TRY(det_pre(ctx, W, H, mask0, pts0.data(), ids0.data(), (int)ids0.size(), J0, &left));
  pts0 = J0.pts, ids0 = J0.ids;
  std::vector<float> fresh, tracked;
  std::vector<uint8_t> status;
  TRY(extract_corners(ctx, S, 0, which, mask0, J0, fresh));
  if (!fresh.empty()) {
    TRY(track_left_to_right(ctx, S, which, fresh, tracked, status));
    for (size_t i = 0; i < status.size(); ++i) {  // :675-708
      const bool oob_left = !in_image(fresh[2 * i], fresh[2 * i + 1]), oob_right = !in_image(tracked[2 * i], tracked[2 * i + 1]);
      if (oob_left) continue;  // (no id is spent)
      const uint64_t id = ++S->currid;
      pts0.insert(pts0.end(), {fresh[2 * i], fresh[2 * i + 1]});
      ids0.push_back(id);
      if (!oob_right && status[i] == 1) {
        pts1.insert(pts1.end(), {tracked[2 * i], tracked[2 * i + 1]});
        ids1.push_back(id);
      }
    }
  }
  // ---- RIGHT  :715-826.  A point whose id the left list holds survives an occupied cell (:754-759); the mask the corners are
  // tested against is cloned from mask0 (:721) while the points and the grid cells are tested against mask1 (:762, :794).
  DetStereoRules right;
  right.spared = ids0.data(), right.n_spared = (int)ids0.size();
  DetJob J1;
  TRY(det_pre(ctx, W, H, mask1, pts1.data(), ids1.data(), (int)ids1.size(), J1, &right));
  pts1 = J1.pts, ids1 = J1.ids;
  TRY(extract_corners(ctx, S, 1, which, mask0, J1, fresh));
  for (size_t i = 0; i < fresh.size() / 2; ++i) {
    pts1.insert(pts1.end(), {fresh[2 * i], fresh[2 * i + 1]});
    ids1.push_back(++S->currid);
  }
  return PLV_OK;
}

// what one camera's temporal matching works on and returns
struct Matching {
  int n = 0;
  bool ran = false;                // n >= 10: LK + RANSAC on the device
  std::vector<float> p_new, n_new;  // positions in the current image and their normalised coordinates (n_new: only where ran)
  std::vector<uint8_t> mask;        // empty for n == 0, all zero for n < 10 (REF :836-852)
};

// both cameras' perform_matching (REF :260-268, :829-886): one LK launch over both point sets (each camera's own pyramids and
// intrinsics), the two RANSACs behind it, one wait
int matching_pair(plv_ctx *ctx, Stereo *S, const std::vector<float> *pts_old[2], Matching M[2]) {
  plv::HostPhase ph("stereo feed: perform_matching x 2");
  LkPair jobs{};
  for (int c = 0; c < 2; ++c) {
    Matching &m = M[c];
    m.n = (int)pts_old[c]->size() / 2;
    m.p_new = *pts_old[c];  // (the initial flow; fewer than 10 points stay where they were)
    m.mask.assign((size_t)m.n, 0);
    m.ran = m.n >= 10;
    jobs.job[c].n = 0;
    if (!m.ran) continue;
    StereoCam &C = S->cam[c];
    const size_t total = MatchBlock((size_t)m.n).total();
    TRY(C.io.reserve(total));
    TRY(C.flow_pin.reserve(total));
    TRY(C.ransac.reserve(ctx->cfg.ransac_max_iters));
    const MatchBlock dev((size_t)m.n, C.io.p), pin((size_t)m.n, C.flow_pin.p);
    memcpy(pin.pts0(), pts_old[c]->data(), (size_t)m.n * 8);
    memcpy(pin.pts1(), pts_old[c]->data(), (size_t)m.n * 8);
    LkJob &j = jobs.job[c];
    j.prev = C.pyr[1 - C.cur], j.cur = C.pyr[C.cur], j.n = m.n;
    j.pts0 = pin.pts0(), j.pts1_init = pin.pts1();  // (read from the pinned block, once)
    j.pts1 = dev.pts1(), j.n0 = dev.n0(), j.n1 = dev.n1();
    j.iters = dev.iters(), j.status = dev.status();
    j.K = cam_k(ctx, S, c);
  }
  if (!M[0].ran && !M[1].ran) return PLV_OK;
  TRY(launch_lk_pair(ctx, jobs, ctx->cfg.win_size, ctx->cfg.lk_max_iters, ctx->cfg.lk_eps));
  for (int c = 0; c < 2; ++c) {
    if (!M[c].ran) continue;
    StereoCam &C = S->cam[c];
    TRY(match_ransac_tail(ctx, jobs.job[c].K, MatchBlock((size_t)M[c].n, C.io.p), MatchBlock((size_t)M[c].n, C.flow_pin.p), C.ransac));
  }
  {
    plv::NsScope ns_wait(plv::counters().flow_wait_ns);
    TRY(sync(ctx, S));
  }
  for (int c = 0; c < 2; ++c) {
    if (!M[c].ran) continue;
    M[c].n_new.resize(2 * (size_t)M[c].n);  // (p_new and mask have their sizes)
    (void)match_read_back(MatchBlock((size_t)M[c].n, S->cam[c].flow_pin.p), M[c].p_new.data(), M[c].mask.data(), nullptr, M[c].n_new.data());
  }
  return PLV_OK;
}

// the rest of TrackKLT::feed_stereo once both images are equalised and their pyramids built
int feed_fed(plv_ctx *ctx, Stereo *S, double timestamp, const uint8_t *mask_l, const uint8_t *mask_r) {
  const int W = S->W, H = S->H;
  StereoCam &L = S->cam[0], &R = S->cam[1];
  auto move_forward = [&](std::vector<float> &pl, std::vector<uint64_t> &il, std::vector<float> &pr, std::vector<uint64_t> &ir) {
    L.pts_last.swap(pl), L.ids_last.swap(il), R.pts_last.swap(pr), R.ids_last.swap(ir);
    const uint8_t *m[2] = {mask_l, mask_r};
    for (int c = 0; c < 2; ++c)
      if (m[c])
        S->cam[c].mask_last.assign(m[c], m[c] + (size_t)W * H);
      else
        S->cam[c].mask_last.clear();
    return S->unsynced ? sync(ctx, S) : PLV_OK;  // (the pinned image blocks are written again by the next pair)
  };
  std::vector<float> pl, pr;
  std::vector<uint64_t> il, ir;
  if (L.pts_last.empty() && R.pts_last.empty()) {  // :221-240 first pair / lost everything: detect on the current pair
    TRY(detection_stereo(ctx, S, S->cur(), mask_l, mask_r, pl, il, pr, ir));
    return move_forward(pl, il, pr, ir);
  }
  // :244-251 top-up on the LAST pair, with the last masks
  pl = L.pts_last, il = L.ids_last, pr = R.pts_last, ir = R.ids_last;
  TRY(detection_stereo(ctx, S, 1 - S->cur(), L.mask_last.empty() ? nullptr : L.mask_last.data(),
                       R.mask_last.empty() ? nullptr : R.mask_last.data(), pl, il, pr, ir));
  // :254-268 temporal KLT per camera, the old positions as the initial flow
  Matching M[2];
  const std::vector<float> *old[2] = {&pl, &pr};
  TRY(matching_pair(ctx, S, old, M));
  std::vector<float> good_l, good_r;
  std::vector<uint64_t> gid_l, gid_r;
  if (M[0].mask.empty() && M[1].mask.empty())  // :285-299 nothing to match in either camera: reset
    return move_forward(good_l, gid_l, good_r, gid_r);
  plv::HostPhase ph_db("stereo feed: pairing + database update");
  std::vector<int> src_l, src_r;  // where in the matched lists a good point came from (its normalised coordinates)
  // :306-338 left points, with their partner in the right list when both were tracked
  for (int i = 0; i < M[0].n; ++i) {
    const float x = M[0].p_new[2 * i], y = M[0].p_new[2 * i + 1];
    if (x < 0 || y < 0 || (int)x > W || (int)y > H) continue;  // (:308-309: `>`, unlike the right side's `>=`)
    const auto it = std::find(ir.begin(), ir.end(), il[i]);
    const int k = it == ir.end() ? -1 : (int)(it - ir.begin());
    if (M[0].mask[i] && k >= 0 && M[1].mask[k]) {
      const float xr = M[1].p_new[2 * k], yr = M[1].p_new[2 * k + 1];
      if (xr < 0 || yr < 0 || (int)xr >= W || (int)yr >= H) continue;  // :325-327 dropped from both lists
      good_l.insert(good_l.end(), {x, y}), gid_l.push_back(il[i]), src_l.push_back(i);
      good_r.insert(good_r.end(), {xr, yr}), gid_r.push_back(ir[k]), src_r.push_back(k);
    } else if (M[0].mask[i]) {
      good_l.insert(good_l.end(), {x, y}), gid_l.push_back(il[i]), src_l.push_back(i);
    }
  }
  // :341-354 right points that were not added with their partner
  for (int i = 0; i < M[1].n; ++i) {
    const float x = M[1].p_new[2 * i], y = M[1].p_new[2 * i + 1];
    if (x < 0 || y < 0 || (int)x >= W || (int)y >= H) continue;
    if (!M[1].mask[i] || std::find(gid_r.begin(), gid_r.end(), ir[i]) != gid_r.end()) continue;
    good_r.insert(good_r.end(), {x, y}), gid_r.push_back(ir[i]), src_r.push_back(i);
  }
  // :357-366 database: the left list under camera 0, then the right list under camera 1 (a good point passed its camera's matching,
  // whose launch undistorted it with that camera's intrinsics: undistort_cv of the same point)
  const std::vector<float> *good[2] = {&good_l, &good_r};
  const std::vector<uint64_t> *gid[2] = {&gid_l, &gid_r};
  const std::vector<int> *src[2] = {&src_l, &src_r};
  for (int c = 0; c < 2; ++c)
    for (size_t i = 0; i < gid[c]->size(); ++i) {
      Track &tr = S->db[(*gid[c])[i]].cam[c];
      const int k = (*src[c])[i];
      tr.t.push_back(timestamp);
      tr.uv.push_back((*good[c])[2 * i]), tr.uv.push_back((*good[c])[2 * i + 1]);
      tr.uvn.push_back(M[c].n_new[2 * k]), tr.uvn.push_back(M[c].n_new[2 * k + 1]);
    }
  return move_forward(good_l, gid_l, good_r, gid_r);  // :369-381
}

// a configured stereo tracker, or null with the error text
Stereo *configured(plv_ctx *ctx, const char *who) {
  Stereo *S = stereo_of(ctx, false);
  if (S && S->configured) return S;
  set_last_error("%s: no stereo pair on this context (plv_stereo_configure comes first)", who);
  return nullptr;
}

}  // namespace

namespace plv {
void plv_stereo_destroy(plv_ctx *ctx) {
  Stereo *S = (Stereo *)ctx->stereo_state;
  if (!S) return;
  for (StereoCam &C : S->cam) {
    C.release();
    C.io.release();
    C.ransac.release();
    C.img_pin.release();
    C.flow_pin.release();
  }
  S->lr_dev.release();
  S->lr_pin.release();
  delete S;
  ctx->stereo_state = nullptr;
}

const CamFront *plv_stereo_front0(plv_ctx *ctx) {
  Stereo *S = stereo_of(ctx, false);
  return S && S->configured ? &S->cam[0] : nullptr;
}

int plv_tracker_kind_check(plv_ctx *ctx, int kind, const char *who) {
  if (ctx->tracker_kind == PLV_TRACKER_NONE || ctx->tracker_kind == kind) return PLV_OK;
  set_last_error("%s: this context has been fed through the %s tracker; the two trackers do not share a context", who,
                 ctx->tracker_kind == PLV_TRACKER_STEREO ? "stereo" : "monocular");
  return PLV_E_BADARG;
}
}  // namespace plv

extern "C" {

int plv_stereo_configure(plv_ctx *ctx, const double *K8_right, int model_right) {
  if (!ctx || !K8_right || (model_right != PLV_CAM_RADTAN && model_right != PLV_CAM_EQUIDISTANT)) {
    set_last_error("plv_stereo_configure: no context, no intrinsics or camera model %d unknown", model_right);
    return PLV_E_BADARG;
  }
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(K8_right[i])) {
      set_last_error("plv_stereo_configure: intrinsic value %d of the right camera is not finite", i);
      return PLV_E_BADARG;
    }
  (void)hipSetDevice(ctx->device);
  Stereo *S = stereo_of(ctx, true);
  std::lock_guard<std::mutex> lk(S->mtx);
  if (!S->configured) {
    S->W = ctx->cfg.width, S->H = ctx->cfg.height;
    for (StereoCam &C : S->cam) {
      C.W = S->W, C.H = S->H;
      TRY(C.prepare(ctx, "plv_stereo_configure"));
      TRY(C.img_pin.reserve((size_t)S->W * S->H));
    }
  }
  std::copy(K8_right, K8_right + 8, S->cam[1].K);
  S->cam[1].model = model_right;
  S->configured = true;
  return PLV_OK;
}

int plv_stereo_set_intrinsics(plv_ctx *ctx, int cam, const double *K8) {
  if (!ctx || !K8) {
    set_last_error("plv_stereo_set_intrinsics: no context or no intrinsics");
    return PLV_E_BADARG;
  }
  if (bad_cam(cam, "plv_stereo_set_intrinsics")) return PLV_E_BADARG;
  Stereo *S = configured(ctx, "plv_stereo_set_intrinsics");
  if (!S) return PLV_E_BADARG;
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(K8[i])) {
      set_last_error("plv_stereo_set_intrinsics: intrinsic value %d is not finite", i);
      return PLV_E_BADARG;
    }
  if (cam == 0) return plv_set_camera_intrinsics(ctx, K8);
  std::lock_guard<std::mutex> lk(S->mtx);
  std::copy(K8, K8 + 8, S->cam[1].K);
  return PLV_OK;
}

int plv_tracker_feed_stereo(plv_ctx *ctx, double timestamp, const uint8_t *left, int stride_left, const uint8_t *right, int stride_right,
                            int encoding, const uint8_t *mask_left, const uint8_t *mask_right) {
  if (!ctx) {
    set_last_error("plv_tracker_feed_stereo: no context");
    return PLV_E_BADARG;
  }
  // every refusal comes before anything is enqueued or written
  TRY(plv_tracker_kind_check(ctx, PLV_TRACKER_STEREO, "plv_tracker_feed_stereo"));
  Stereo *S = configured(ctx, "plv_tracker_feed_stereo");
  if (!S) return PLV_E_BADARG;
  TRY(check_encoded("plv_tracker_feed_stereo (left)", left, stride_left, encoding, S->W));
  TRY(check_encoded("plv_tracker_feed_stereo (right)", right, stride_right, encoding, S->W));
  std::lock_guard<std::mutex> lk(S->mtx);  // REF: mtx_feeds of both cameras, TrackKLT.cpp:207-208
  {
    const int want = S->cam[0].levels_for(ctx, ctx->cfg.win_size);
    if (want != S->cam[0].pyr[0].levels) {
      set_last_error("plv_tracker_feed_stereo: a %d x %d window gives %d pyramid levels, the stereo pyramids have %d", ctx->cfg.win_size,
                     ctx->cfg.win_size, want, S->cam[0].pyr[0].levels);
      return PLV_E_BADARG;
    }
    if (ctx->cfg.histogram_method == PLV_HIST_CLAHE && (S->W % 8 != 0 || S->H % 8 != 0)) {
      set_last_error("plv_tracker_feed_stereo: CLAHE needs a width and height divisible into 8 x 8 tiles, not %dx%d", S->W, S->H);
      return PLV_E_BADARG;
    }
    if (ctx->cfg.histogram_method != PLV_HIST_HISTOGRAM && ctx->cfg.histogram_method != PLV_HIST_NONE && ctx->cfg.histogram_method != PLV_HIST_CLAHE) {
      set_last_error("plv_tracker_feed_stereo: unknown histogram method %d", ctx->cfg.histogram_method);
      return PLV_E_BADARG;
    }
  }
  (void)hipSetDevice(ctx->device);
  ctx->tracker_kind = PLV_TRACKER_STEREO;
  // :50-76 equalisation and pyramid per image, back to back on the stream (no wait between them)
  const int next = S->cam[0].next();
  {
    plv::HostPhase ph("stereo feed: two images enqueued");
    TRY(enqueue_image(ctx, S, 0, next, left, stride_left, encoding));
    TRY(enqueue_image(ctx, S, 1, next, right, stride_right, encoding));
  }
  for (StereoCam &C : S->cam) C.commit(next);  // (only now: a pair of which one image was refused leaves both cameras where they were)
  return feed_fed(ctx, S, timestamp, mask_left, mask_right);
}

// TrackBase::get_last_obs / get_last_ids of one camera
int plv_stereo_last(plv_ctx *ctx, int cam, float *pts, uint64_t *ids, int cap, int *n) {
  if (!ctx || !n) {
    set_last_error("plv_stereo_last: no context or no count");
    return PLV_E_BADARG;
  }
  if (bad_cam(cam, "plv_stereo_last")) return PLV_E_BADARG;
  Stereo *S = configured(ctx, "plv_stereo_last");
  if (!S) return PLV_E_BADARG;
  std::lock_guard<std::mutex> lk(S->mtx);
  const StereoCam &C = S->cam[cam];
  *n = (int)C.ids_last.size();
  if (*n > cap) return PLV_E_CAPACITY;
  if (pts) std::copy(C.pts_last.begin(), C.pts_last.end(), pts);
  if (ids) std::copy(C.ids_last.begin(), C.ids_last.end(), ids);
  return PLV_OK;
}

int plv_stereo_db_size(plv_ctx *ctx) {
  Stereo *S = ctx ? stereo_of(ctx, false) : nullptr;
  if (!S) return 0;
  std::lock_guard<std::mutex> lk(S->mtx);
  return (int)S->db.size();
}

int plv_stereo_db_ids(plv_ctx *ctx, uint64_t *ids, int cap, int *n) {
  if (!ctx || !n) return PLV_E_BADARG;
  Stereo *S = configured(ctx, "plv_stereo_db_ids");
  if (!S) return PLV_E_BADARG;
  std::lock_guard<std::mutex> lk(S->mtx);
  return export_sorted_ids(S->db, ids, cap, n);
}

int plv_stereo_db_export_tracks(plv_ctx *ctx, const uint64_t *ids, int n, int cam, int *obs_ptr, double *obs_time, float *obs_uv,
                                float *obs_uvn, int cap_obs) {
  if (!ctx || n < 0 || (n > 0 && !ids) || !obs_ptr) return PLV_E_BADARG;
  if (bad_cam(cam, "plv_stereo_db_export_tracks")) return PLV_E_BADARG;
  Stereo *S = configured(ctx, "plv_stereo_db_export_tracks");
  if (!S) return PLV_E_BADARG;
  std::lock_guard<std::mutex> lk(S->mtx);
  auto track_of = [S, cam](uint64_t id) -> const Track * {
    const auto it = S->db.find(id);
    return it == S->db.end() ? nullptr : &it->second.cam[cam];
  };
  return export_tracks(ids, n, track_of, obs_ptr, obs_time, obs_uv, obs_uvn, cap_obs);
}

// FeatureDatabase::cleanup_measurements(t) (REF: FeatureDatabase.cpp:286-323): Feature::clean_older_measurements over every
// camera, the feature erased when nothing is left
int plv_stereo_db_cleanup_measurements(plv_ctx *ctx, double t) {
  if (!ctx) return PLV_E_BADARG;
  Stereo *S = configured(ctx, "plv_stereo_db_cleanup_measurements");
  if (!S) return PLV_E_BADARG;
  std::lock_guard<std::mutex> lk(S->mtx);
  cleanup_measurements(S->db, t, [](StereoFeature &f, double t_) { return drop_before(f.cam[0], t_) + drop_before(f.cam[1], t_); });
  return PLV_OK;
}

int plv_stereo_db_remove(plv_ctx *ctx, const uint64_t *ids, int n) {
  if (!ctx || n < 0 || (n > 0 && !ids)) return PLV_E_BADARG;
  Stereo *S = configured(ctx, "plv_stereo_db_remove");
  if (!S) return PLV_E_BADARG;
  std::lock_guard<std::mutex> lk(S->mtx);
  erase_ids(S->db, ids, n);
  return PLV_OK;
}

int plv_stereo_db_append_measurements(plv_ctx *ctx, uint64_t id, int cam, int n, const double *t, const float *uv, const float *uvn) {
  if (!ctx || n < 0 || (n > 0 && (!t || !uv || !uvn))) {
    set_last_error("plv_stereo_db_append_measurements: no context, a negative count or a missing array");
    return PLV_E_BADARG;
  }
  if (bad_cam(cam, "plv_stereo_db_append_measurements")) return PLV_E_BADARG;
  Stereo *S = configured(ctx, "plv_stereo_db_append_measurements");
  if (!S) return PLV_E_BADARG;
  std::lock_guard<std::mutex> lk(S->mtx);
  Track &tr = S->db[id].cam[cam];
  tr.t.insert(tr.t.end(), t, t + n);
  tr.uv.insert(tr.uv.end(), uv, uv + 2 * (size_t)n);
  tr.uvn.insert(tr.uvn.end(), uvn, uvn + 2 * (size_t)n);
  return PLV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the stereo point update
namespace {
typedef PoolCand<StereoFeature> StereoCand;

// One plv_stereo_update_points / plv_stereo_try_update call (stereo_points_run).  The pool mechanics are camera_tracks.hpp's: a candidate holds the two cameras' tracks, and what
// goes back to the database (db_unused) is kept per camera, so that every per-track template serves one camera of a feature.
struct StereoPointsUpdate {
  plv_ctx *ctx;
  Stereo *S;
  const plv_state_view *st;
  const plv_camera_side *right;
  const plv_update_options *opt;
  double *dx;
  plv_update_result *res;
  const double dt = st->cam_dt, t_oldest = st->clone_time[0], t_oldest2 = st->clone_time[1];  // one time offset for the pair (REF State.cpp:102-103)
  BoundingMemo start_of{*st};
  std::vector<StereoCand> pool;
  TrackMap<Track> unused[2];
  std::vector<int> valid_n;
  // use_imu_res (opt->cpi, plv_stereo_try_update): the distinct times the table serves, listed once for both cameras — the pair shares
  // dt, a left and a right observation of one frame share one pose — and per pool candidate and camera every observation's index
  bool cpi_on = false;
  std::vector<double> cpi_times;
  std::vector<std::array<std::vector<int>, 2>> pose_idx;

  // REF CamHelper.cpp:702-703 / :709-738: db_unused returns to the tracker's database; cleanup_features runs on every call
  int finish(int rc) {
    std::lock_guard<std::mutex> lk(S->mtx);
    res->n_returned = (int)unused[0].size();
    for (const auto &kv : unused[1]) res->n_returned += unused[0].find(kv.first) == unused[0].end();
    for (int c = 0; c < 2; ++c)
      for (auto &kv : unused[c]) append_track(S->db[kv.first].cam[c], kv.second);
    if (opt->window_full)
      cleanup_measurements(S->db, t_oldest, [](StereoFeature &f, double t_) { return drop_before(f.cam[0], t_) + drop_before(f.cam[1], t_); });
    return rc;
  }
  int finish_early() {
    std::fill(dx, dx + ctx->cov_n, 0.0);
    return finish(PLV_OK);
  }
  void back_all(StereoCand &c) {
    for (int q = 0; q < 2; ++q) {
      if (c.tr.cam[q].t.empty()) continue;
      PoolCand<Track> one{c.id, std::move(c.tr.cam[q])};
      give_back_all(unused[q], one);
      c.tr.cam[q] = Track{};
    }
  }
  int abandon(int rc) {
    for (StereoCand &c : pool) back_all(c);
    return finish(rc);
  }
  // observations with bounding clones (get_imu_poses, REF :327-372), over both cameras
  int usable(const StereoCand &c) { return usable_views(c.tr.cam[0], dt, start_of) + usable_views(c.tr.cam[1], dt, start_of); }

  void take_pool_of_window() {
    {
      std::lock_guard<std::mutex> lk(S->mtx);
      take_pool(S->db, t_oldest2 - dt, opt->t_prev_frame - dt, pool);  // REF :631-637, over the observations of both cameras
    }
    res->n_pool = (int)pool.size();
    size_t kept = 0;
    for (size_t ci = 0; ci < pool.size(); ++ci) {  // REF :740-775 remove_unusable_measurements, per camera
      StereoCand &c = pool[ci];
      size_t keep = 0;
      for (int q = 0; q < 2; ++q) keep += trim_to_window(unused[q], c.id, c.tr.cam[q], dt, opt->state_time + st->dt_exp, t_oldest - st->dt_exp);
      if (keep < 2) continue;  // REF :766-771
      if (kept != ci) pool[kept] = std::move(c);
      ++kept;
    }
    pool.resize(kept);
    sort_long_first(pool);  // REF :640, by the observations of both cameras; ties by ascending id
  }

  // REF CamHelper.cpp get_imu_poses (:356-365), per camera: what the table cannot serve returns to its own camera's track
  void attach_cpi() {
    cpi_on = true;
    pose_idx.resize(pool.size());
    CpiTimes M{*st, *opt->cpi, cpi_times};
    for (size_t f = 0; f < pool.size(); ++f)
      for (int q = 1; q >= 0; --q) cpi_attach_track(M, dt, pool[f].id, pool[f].tr.cam[q], unused[q], pose_idx[f][q]);
  }

  // candidates [sel] in the layout of plv_stereo_tracks: camera 1's observations, then camera 0's (the reference's iteration order);
  // valid_only: without the observations that have no bounding clones
  struct Flat {
    std::vector<int> ptr;
    std::vector<double> t;
    std::vector<float> uv, uvn;
    std::vector<uint8_t> cam;
    std::vector<int> pose_of;  // (cpi_on) index into cpi_times
  };
  CpiStage cpi_stage(const Flat &F) const { return CpiStage{opt->cpi, (int)cpi_times.size(), cpi_times.data(), F.pose_of.data(), nullptr, nullptr}; }
  void flatten(const std::vector<int> &sel, bool valid_only, Flat &F) {
    F.ptr.assign(1, 0);
    for (int f : sel) {
      for (int q = 1; q >= 0; --q) {
        const Track &tr = pool[f].tr.cam[q];
        for (size_t i = 0; i < tr.t.size(); ++i) {
          if (valid_only && start_of(tr.t[i] + dt) < 0) continue;
          F.t.push_back(tr.t[i]);
          F.uv.insert(F.uv.end(), tr.uv.begin() + 2 * i, tr.uv.begin() + 2 * i + 2);
          F.uvn.insert(F.uvn.end(), tr.uvn.begin() + 2 * i, tr.uvn.begin() + 2 * i + 2);
          F.cam.push_back((uint8_t)q);
          if (cpi_on) F.pose_of.push_back(pose_idx[f][q][i]);
        }
      }
      F.ptr.push_back((int)F.t.size());
    }
  }
  static plv_stereo_tracks view(const Flat &F, const double *p) {
    plv_stereo_tracks v{};
    v.tracks.n_feat = (int)F.ptr.size() - 1, v.tracks.obs_ptr = F.ptr.data(), v.tracks.obs_time = F.t.data(), v.tracks.obs_uv = F.uv.data();
    v.tracks.obs_uvn = F.uvn.data(), v.tracks.p_FinG = v.tracks.p_FinG_fej = p;
    v.obs_cam = F.cam.data();
    return v;
  }
};
}  // namespace

namespace {
// plv_stereo_update_points behind its refusals.  try_update (plv_stereo_try_update): opt->cpi is honoured and every feature the
// reference copies to point_used is recorded (REF CamHelper.cpp:648-699: triangulated, dynamic or not, until the cap ends the loop).
int stereo_points_run(const char *who, plv_ctx *ctx, Stereo *S, const plv_state_view *st, const plv_camera_side *right, const plv_update_options *opt,
                      double *dx, plv_update_result *res, uint64_t *msckf_ids, uint8_t *accepted_out, double *p_out, bool try_update) {
  *res = plv_update_result{0, 0, 0, 0, 0, PLV_OK, 0, 0, 0};
  (void)hipSetDevice(ctx->device);
  StereoPointsUpdate U{ctx, S, st, right, opt, dx, res};
  U.take_pool_of_window();
  if (try_update && opt->cpi) U.attach_cpi();
  const int Fp = (int)U.pool.size();
  if (Fp == 0) return U.finish_early();
  U.valid_n.resize(Fp);
  bool any = false;
  for (int f = 0; f < Fp; ++f) {
    U.valid_n[f] = U.usable(U.pool[f]);
    any = any || U.valid_n[f] >= 2;
    if (U.valid_n[f] > opt->max_obs) {
      set_last_error("%s: feature %llu has %d usable observations over both cameras, the batch holds max_obs = %d", who,
                     (unsigned long long)U.pool[f].id, U.valid_n[f], opt->max_obs);
      return U.abandon(PLV_E_CAPACITY);
    }
  }
  // ---- launch 1: every pool candidate triangulated (the reference goes feature by feature until the cap; a feature it never
  // reaches keeps its observations either way).  With a CPI table cpi_pose_kernel runs in front of it on the stream.
  std::vector<double> pf(3 * (size_t)Fp, 0.0), err(Fp, 0.0);
  std::vector<uint8_t> ok(Fp, 0);
  if (any) {
    std::vector<int> everyone(Fp);
    for (int f = 0; f < Fp; ++f) everyone[f] = f;
    StereoPointsUpdate::Flat A;
    U.flatten(everyone, false, A);
    const plv_stereo_tracks all = StereoPointsUpdate::view(A, nullptr);
    const CpiStage cs = U.cpi_stage(A);
    const int rc_t = stereo_triangulate(ctx, st, right, &all, &opt->tri, U.cpi_on ? &cs : nullptr, pf.data(), ok.data(), err.data());
    if (rc_t != PLV_OK) return U.abandon(rc_t);
  }
  // ---- REF :648-699 the selection loop, on the host
  std::vector<int> sel;
  for (int f = 0; f < Fp; ++f) {
    StereoCand &c = U.pool[f];
    if ((int)sel.size() >= opt->max_msckf) {
      U.back_all(c);
      continue;
    }
    if (try_update && U.valid_n[f] >= 2 && ok[f]) {  // copy_to_db(db_used, feat): dynamic (:677) and MSCKF (:697) features
      double newest = 0;
      for (const Track &tr : c.tr.cam)
        if (!tr.t.empty()) newest = std::max(newest, tr.t.back());
      (void)plv_point_used_insert(ctx, c.id, &pf[3 * (size_t)f], newest);
    }
    if (U.valid_n[f] < 2 || !ok[f] || !(err[f] < 3.0)) {
      U.back_all(c);
      continue;
    }
    sel.push_back(f);
  }
  res->n_msckf = (int)sel.size();
  if (sel.empty()) return U.finish_early();
  // ---- launch 2 + the resident tail: UpdaterCamera::msckf_update on the selected features (their CPI poses are the ones launch 1
  // formed: the batch's index points into the same buffer)
  std::vector<double> feat(3 * sel.size());
  for (size_t q = 0; q < sel.size(); ++q) {
    std::copy(pf.begin() + 3 * (size_t)sel[q], pf.begin() + 3 * (size_t)sel[q] + 3, feat.begin() + 3 * q);
    if (msckf_ids) msckf_ids[q] = U.pool[sel[q]].id;
    for (int cq = 0; cq < 2; ++cq) {  // observations without bounding clones go back (get_imu_poses)
      const Track &tr = U.pool[sel[q]].tr.cam[cq];
      for (size_t i = 0; i < tr.t.size(); ++i)
        if (U.start_of(tr.t[i] + U.dt) < 0) give_back(U.unused[cq], U.pool[sel[q]].id, tr, i);
    }
  }
  if (p_out) std::copy(feat.begin(), feat.end(), p_out);
  StereoPointsUpdate::Flat B;
  U.flatten(sel, true, B);
  const plv_stereo_tracks chosen = StereoPointsUpdate::view(B, feat.data());
  const CpiStage cs_b = U.cpi_stage(B);
  std::vector<int> cols(ctx->cfg.max_state_dim > 0 ? ctx->cfg.max_state_dim : 1024);
  std::vector<uint8_t> acc(sel.size(), 0);
  int k = 0, n_rows = 0;
  int rc = plv_stereo_jacobian_columns(st, right, &chosen, cols.data(), (int)cols.size(), &k);
  if (rc == PLV_OK) rc = stereo_jacobians_resident(ctx, st, right, &chosen, k, cols.data(), 2 * opt->max_obs, U.cpi_on ? &cs_b : nullptr);
  if (rc == PLV_OK) {
    rc = plv_msckf_update_resident(ctx, st->sigma_pix * st->sigma_pix, opt->chi2_mult, 3.0, acc.data(), &n_rows, dx);
    rc = ekf_returned_false(rc, &res->status, dx, ctx->cov_n);
  }
  auto back_valid = [&](int f) {
    for (int cq = 0; cq < 2; ++cq) {
      const Track &tr = U.pool[f].tr.cam[cq];
      for (size_t i = 0; i < tr.t.size(); ++i)
        if (U.start_of(tr.t[i] + U.dt) >= 0) give_back(U.unused[cq], U.pool[f].id, tr, i);
    }
  };
  if (rc != PLV_OK) {  // a failing update returns the selected tracks
    for (int f : sel) back_valid(f);
    return U.finish(rc);
  }
  res->n_rows = n_rows;
  // REF UpdaterCamera.cpp:266-268: only what the gate rejected goes back
  for (size_t q = 0; q < sel.size(); ++q) {
    res->n_accepted += acc[q];
    if (accepted_out) accepted_out[q] = acc[q];
    if (!acc[q]) back_valid(sel[q]);
  }
  return U.finish(PLV_OK);
}
}  // namespace

extern "C" {

int plv_stereo_update_points(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_update_options *opt, double *dx,
                             plv_update_result *res, uint64_t *msckf_ids, uint8_t *accepted_out, double *p_out) {
  const char *who = "plv_stereo_update_points";
  if (!ctx || !st || !opt || !dx || !res || st->n_clones < 2 || !st->clone_time || opt->max_msckf < 1 || opt->max_obs < 2) {
    set_last_error("%s: a missing argument, fewer than 2 clones, max_msckf < 1 or max_obs < 2", who);
    return PLV_E_BADARG;
  }
  // ---- every refusal comes before the database, the covariance or the staged batch is touched
  auto refuse = [who](const char *why) {
    set_last_error("%s: %s", who, why);
    return (int)PLV_E_BADARG;
  };
  if (opt->max_slam != 0) return refuse("in-state landmarks (max_slam != 0) are not built for the stereo update");
  if (opt->cpi) return refuse("use_imu_res (plv_update_options::cpi) is not built for the stereo update");
  if (st->use_imu_cov) return refuse("use_imu_cov is not built for the stereo update");
  if (ctx->decision_trace) return refuse("the decision trace does not cover the stereo update (plv_decision_trace off first)");
  Stereo *S = configured(ctx, who);
  if (!S) return PLV_E_BADARG;
  TRY(plv_stereo_side_check(who, st, right));
  return stereo_points_run(who, ctx, S, st, right, opt, dx, res, msckf_ids, accepted_out, p_out, false);
}

// UpdaterCamera::try_update for the pair (REF UpdaterCamera.cpp:139-195 with cam_id = sensor_ids.at(0)): the point half over both
// cameras, the line half on camera 0 — a composition of the calls a caller would make one after the other.
int plv_stereo_try_update(plv_ctx *ctx, const plv_state_view *st, plv_camera_side *right, plv_try_update *io) {
  const char *who = "plv_stereo_try_update";
  if (!ctx || !st || !io || !io->opt_points || !io->dx_points || !io->res_points || (io->n_var > 0 && !io->vars) ||
      (io->opt_lines && (!io->dx_lines || !io->res_lines)) || st->n_clones < 2 || !st->clone_time || io->opt_points->max_msckf < 1 ||
      io->opt_points->max_obs < 2) {
    set_last_error("%s: a missing argument, fewer than 2 clones, max_msckf < 1 or max_obs < 2", who);
    return PLV_E_BADARG;
  }
  // ---- every refusal comes before the databases, the covariance, the variables or the staged batch are touched
  auto refuse = [who](const char *why) {
    set_last_error("%s: %s", who, why);
    return (int)PLV_E_BADARG;
  };
  const plv_update_options *op = io->opt_points, *ol = io->opt_lines;
  if (op->max_slam != 0 || (ol && ol->max_slam != 0)) return refuse("in-state landmarks (max_slam != 0) are not built for the stereo update");
  if (st->use_imu_cov) return refuse("use_imu_cov is not built for the stereo update");
  if (ctx->decision_trace) return refuse("the decision trace does not cover the stereo update (plv_decision_trace off first)");
  Stereo *S = configured(ctx, who);
  if (!S) return PLV_E_BADARG;
  TRY(plv_stereo_side_check(who, st, right));
  if ((op->cpi && !cpi_table_usable(op->cpi)) || (ol && ol->cpi && !cpi_table_usable(ol->cpi)))
    return refuse("a CPI table (plv_update_options::cpi) with a missing array or times that do not ascend");
  if (plv_state_vars_check(io->n_var, io->vars, ctx->cov_n) != PLV_OK) {  // (the test plv_state_boxplus makes when dx is applied)
    set_last_error("%s: a variable of the list has an unknown kind, no values or an index beyond the covariance (%d)", who, ctx->cov_n);
    return PLV_E_BADARG;
  }
  // StateHelper::EKFUpdate's mean update (:156-168); `right` and st's calibration fields are mirrors of the variables, the tracker
  // undistorts the next pair with the calibrated intrinsics of both cameras
  auto apply = [&](const plv_update_result &r, const double *dx) {
    if (r.status != PLV_OK || r.n_accepted < 1 || io->n_var < 1) return (int)PLV_OK;
    TRY(plv_state_boxplus(io->n_var, io->vars, dx, ctx->cov_n));
    if (st->intrinsic_state_id >= 0) TRY(plv_set_camera_intrinsics(ctx, st->intrinsics));
    if (right->intrinsic_state_id >= 0) TRY(plv_stereo_set_intrinsics(ctx, 1, right->intrinsics));
    return (int)PLV_OK;
  };
  int rc = stereo_points_run(who, ctx, S, st, right, op, io->dx_points, io->res_points, io->msckf_ids, io->msckf_accepted, io->p_FinG, true);
  // REF :148-152: the line pool is formed and triangulated on the state as it is before the point update's correction is applied
  const int rc_lf = rc == PLV_OK && ol ? plv_camera_get_line_features(ctx, st) : PLV_OK;
  if (rc == PLV_OK) rc = apply(*io->res_points, io->dx_points);  // (the covariance holds the point update: so does the state)
  if (rc == PLV_OK) rc = rc_lf;
  if (rc == PLV_OK && ol) {
    rc = plv_line_tracker_feed_wait(ctx);
    io->line_db_size = plv_line_db_size_after_feed(ctx);
    // camera 0's calibration, on the updated state; point_used is cleaned in there when the window is full (:187-189)
    if (rc == PLV_OK) rc = plv_camera_update_lines(ctx, st, ol, io->dx_lines, io->res_lines, io->line_ids, io->line_accepted, io->line_FinG, io->line_cap);
    if (rc == PLV_OK) rc = apply(*io->res_lines, io->dx_lines);
  }
  if (rc != PLV_OK && ol) plv_line_pool_discard(ctx);
  return rc;
}

}  // extern "C"
