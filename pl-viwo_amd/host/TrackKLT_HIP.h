// TrackKLT_HIP.h — ov_core::TrackBase implementation on libplviwo_hip.so.
// REF: open_vins/ov_core/src/track/TrackBase.h:72-196 (interface), TrackKLT.cpp:34-200 (feed_new_camera / feed_monocular),
//      :202-393 (feed_stereo), :395-528 / :530-827 (perform_detection_monocular / _stereo), :829-886 (perform_matching),
//      feat/FeatureDatabase.cpp:60-120 (update_feature)
//
// The whole frame logic runs behind plv_tracker_feed (first-frame detection, top-up on the last image, pyramidal LK with the
// previous positions as the initial flow, undistortion, 7-point RANSAC, bounds / mask filter, id hand-over).  The adapter keeps
// TrackBase's observable state current: pts_last / ids_last (get_last_obs / get_last_ids, read by TrackLSD and the display code),
// img_last / img_mask_last, and the ov_core::FeatureDatabase (update_feature with the frame's observations), so code that walks
// `get_feature_database()` keeps working.  UpdaterCameraHIP.h uses the library's own track store instead and does not need it.
//
// Stereo (`use_stereo` with cameras 0 and 1, the shipped KAIST configuration): a message with two images goes to
// plv_tracker_feed_stereo — TrackKLT::feed_stereo behind one call — and the mirror follows feed_stereo :356-381: update_feature for
// the left list under the left camera's id and for the right list under the right one's, pts_last / ids_last / img_last /
// img_mask_last of both ids.  The reference's own UpdaterCamera reads that FeatureDatabase; UpdaterCameraHIP (the update on the
// device) is monocular.  Two images without use_stereo (binocular: feed_monocular per camera) are refused.
//
// Two constructors.  The first has TrackKLT's own signature (TrackKLT.h:54-58), so the reference's call site
//   new TrackKLT(state->cam_intrinsic_model, op->n_pts, 0, op->use_stereo, op->histogram, op->fast, op->grid_x, op->grid_y, op->min_px_dist)
// (UpdaterCamera.cpp:41,63) compiles with the class name changed and nothing else: the tracker creates and owns its plv_ctx
// (image size and intrinsics from the CamBase of its camera, everything else from the arguments / the reference's constants) and
// TrackLSD_HIP / UpdaterCameraHIP / StateHelperHIP find it through context().  The second takes a ctx the caller made (PlvContext.h).
#pragma once
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "plviwo.h"
#include "track/TrackBase.h"
#include "utils/print.h"

namespace ov_core {

class TrackKLT_HIP : public TrackBase {
public:
  // REF: TrackKLT.h:54-58 — the reference's signature; the context is created here and destroyed with the tracker
  explicit TrackKLT_HIP(std::unordered_map<size_t, std::shared_ptr<CamBase>> cameras, int numfeats, int numaruco, bool stereo,
                        HistogramMethod histmethod, int fast_threshold, int gridx, int gridy, int minpxdist)
      : TrackBase(cameras, numfeats, numaruco, stereo, histmethod), ctx(nullptr), mirror_db(true), stereo_pair(stereo) {
    if (cameras.empty() || (stereo && (cameras.count(0) == 0 || cameras.count(1) == 0))) {
      PRINT_ERROR(RED "[TrackKLT_HIP]: one monocular camera, or cameras 0 and 1 of a stereo pair\n" RESET);
      std::exit(EXIT_FAILURE);
    }
    const std::shared_ptr<CamBase> &cam = stereo ? cameras.at(0) : cameras.begin()->second;
    plv_config cfg;
    plv_config_default(&cfg, cam->w(), cam->h());  // CamBase.h:190-193
    cfg.num_features = numfeats;
    cfg.fast_threshold = fast_threshold;
    cfg.grid_x = gridx, cfg.grid_y = gridy;
    cfg.min_px_dist = minpxdist;
    cfg.histogram_method = (int)histmethod;  // PLV_HIST_* follow TrackBase::HistogramMethod (TrackBase.h:78)
    const Eigen::MatrixXd K = cam->get_value();  // fx fy cx cy k1 k2 p1 p2 (CamBase.h:56-82,181)
    for (int i = 0; i < 8; ++i) cfg.intrinsics[i] = K(i, 0);
    if (const char *dev = std::getenv("PLV_DEVICE")) cfg.device = std::atoi(dev);
    plv_ctx *c = nullptr;
    if (plv_ctx_create(&cfg, &c) != PLV_OK) {
      PRINT_ERROR(RED "[TrackKLT_HIP]: %s\n" RESET, plv_last_error());
      std::exit(EXIT_FAILURE);  // no CPU fallback: the library needs a gfx950 device
    }
    owned = std::shared_ptr<plv_ctx>(c, plv_ctx_destroy);
    ctx = c;
    if (stereo) configure_right(cam, cameras.at(1));
  }

  // a context the caller created (PlvContext.h: sized from the estimator's options as well)
  TrackKLT_HIP(std::unordered_map<size_t, std::shared_ptr<CamBase>> cameras, int numfeats, int numaruco, bool stereo,
               HistogramMethod histmethod, plv_ctx *ctx_, bool mirror_database = true)
      : TrackBase(cameras, numfeats, numaruco, stereo, histmethod), ctx(ctx_), mirror_db(mirror_database), stereo_pair(stereo) {
    if (stereo) {
      if (cameras.count(0) == 0 || cameras.count(1) == 0) {
        PRINT_ERROR(RED "[TrackKLT_HIP]: a stereo pair is cameras 0 and 1\n" RESET);
        std::exit(EXIT_FAILURE);
      }
      configure_right(cameras.at(0), cameras.at(1));
    }
  }

  // the library keeps its own track store (plv_db_*); UpdaterCameraHIP turns the ov_core::FeatureDatabase mirror off
  void mirror_database(bool on) { mirror_db = on; }

  void feed_new_camera(const CameraData &message) override {
    if (message.sensor_ids.size() == 2 && message.images.size() == 2 && message.masks.size() == 2) {  // TrackKLT.cpp:82-83
      if (!stereo_pair) {  // (:84-89 binocular: a feed_monocular per camera, each with its own tracker state)
        PRINT_ERROR(RED "[TrackKLT_HIP]: two images without use_stereo (binocular tracking) are not built: one tracker per camera\n" RESET);
        std::exit(EXIT_FAILURE);
      }
      feed_stereo(message);
      return;
    }
    if (message.sensor_ids.size() != 1) {
      PRINT_ERROR(RED "[TrackKLT_HIP]: one image, or the two of a stereo pair\n" RESET);
      std::exit(EXIT_FAILURE);
    }
    const size_t cam_id = message.sensor_ids.at(0);
    std::lock_guard<std::mutex> lck(mtx_feeds.at(cam_id));
    const cv::Mat &img = message.images.at(0), &mask = message.masks.at(0);
    if (img.type() != CV_8UC1 || !mask.isContinuous() ||
        plv_tracker_feed(ctx, message.timestamp, img.data, (int)img.step, mask.empty() ? nullptr : mask.data) != PLV_OK) {
      PRINT_ERROR(RED "[TrackKLT_HIP]: %s\n" RESET, plv_last_error());  // TrackKLT.cpp:37-43 exits on bad sizes as well
      std::exit(EXIT_FAILURE);
    }
    after_feed(cam_id, message.timestamp, img, mask);
  }

  // feed_new_camera for a sensor_msgs/Image as it arrives — `data`, `step` and `encoding` of the message ("mono8", "bayer_rggb8",
  // "bgr8", ...: plv_encoding_from_name) — instead of the MONO8 image cv_bridge::toCvShare would make of it on the host
  // (REF: PL-VIWO/src/core/ROSHelper.cpp:151-173).  The bytes go into one of the library's page-locked raw blocks, the conversion
  // kernel reads them there into an HBM slot, and the frame takes the staged path.  img_last stays empty: there is no host grey image.
  void feed_new_camera(double timestamp, size_t cam_id, const uint8_t *data, int step, const std::string &encoding, const cv::Mat &mask) {
    std::lock_guard<std::mutex> lck(mtx_feeds.at(cam_id));
    const int slot = stage_encoded(data, step, encoding);
    if (slot < 0 || !mask.isContinuous() || plv_tracker_feed_staged(ctx, timestamp, slot, mask.empty() ? nullptr : mask.data) != PLV_OK) {
      PRINT_ERROR(RED "[TrackKLT_HIP]: %s\n" RESET, plv_last_error());
      std::exit(EXIT_FAILURE);
    }
    after_feed(cam_id, timestamp, cv::Mat(), mask);
  }

  // the message's bytes -> raw block (alternating) -> plv_image_stage_encoded: the HBM slot that holds the grey image, or -1
  // (plv_last_error says why; an encoding the library does not take among the reasons)
  int stage_encoded(const uint8_t *data, int step, const std::string &encoding) {
    const int enc = plv_encoding_from_name(encoding.c_str());
    uint8_t *blk = nullptr;
    int bstride = 0;
    if (!data || step < 0 || plv_raw_image_buffer(ctx, raw_index, enc, &blk, &bstride) != PLV_OK) return -1;
    if (step < bstride) return plv_image_stage_encoded(ctx, raw_index, data, step, enc) == PLV_OK ? raw_index : -1;  // (refused: the library names the cause)
    const int rows = camera_calib.begin()->second->h();
    for (int y = 0; y < rows; ++y) std::memcpy(blk + (size_t)y * bstride, data + (size_t)y * step, (size_t)bstride);
    const int slot = raw_index;
    raw_index = (raw_index + 1) & 3;
    return plv_image_stage_encoded(ctx, slot, blk, bstride, enc) == PLV_OK ? slot : -1;
  }

  plv_ctx *context() const { return ctx; }

protected:
  // camera 1 of the pair: its own intrinsics, the context's image size
  void configure_right(const std::shared_ptr<CamBase> &left, const std::shared_ptr<CamBase> &right) {
    double k8[8];
    const Eigen::MatrixXd K = right->get_value();
    for (int i = 0; i < 8; ++i) k8[i] = K(i, 0);
    if (left->w() != right->w() || left->h() != right->h() || plv_stereo_configure(ctx, k8, PLV_CAM_RADTAN) != PLV_OK) {
      PRINT_ERROR(RED "[TrackKLT_HIP]: the two cameras of a pair have one image size; %s\n" RESET, plv_last_error());
      std::exit(EXIT_FAILURE);
    }
  }

  // TrackKLT::feed_stereo(message, 0, 1) behind plv_tracker_feed_stereo, then TrackBase's state for both camera ids
  void feed_stereo(const CameraData &message) {
    const size_t id[2] = {(size_t)message.sensor_ids.at(0), (size_t)message.sensor_ids.at(1)};
    std::lock_guard<std::mutex> lck1(mtx_feeds.at(id[0]));  // TrackKLT.cpp:207-208
    std::lock_guard<std::mutex> lck2(mtx_feeds.at(id[1]));
    const cv::Mat *img[2] = {&message.images.at(0), &message.images.at(1)}, *mask[2] = {&message.masks.at(0), &message.masks.at(1)};
    bool ok = true;
    for (int c = 0; c < 2; ++c) {  // the reference tracks with camera_calib's values of the moment (the state's estimate under do_calib_int)
      double k8[8];
      const Eigen::MatrixXd K = camera_calib.at(id[c])->get_value();
      for (int i = 0; i < 8; ++i) k8[i] = K(i, 0);
      ok = ok && plv_stereo_set_intrinsics(ctx, c, k8) == PLV_OK && img[c]->type() == CV_8UC1 && mask[c]->isContinuous();
    }
    // :221 with both lists empty the pair is only detected on: nothing goes to the database
    const bool tracked = !(pts_last[id[0]].empty() && pts_last[id[1]].empty());
    if (!ok || plv_tracker_feed_stereo(ctx, message.timestamp, img[0]->data, (int)img[0]->step, img[1]->data, (int)img[1]->step, PLV_ENC_MONO8,
                                       mask[0]->empty() ? nullptr : mask[0]->data, mask[1]->empty() ? nullptr : mask[1]->data) != PLV_OK) {
      PRINT_ERROR(RED "[TrackKLT_HIP]: %s\n" RESET, plv_last_error());
      std::exit(EXIT_FAILURE);
    }
    std::vector<cv::KeyPoint> kps[2];
    std::vector<size_t> kid[2];
    for (int c = 0; c < 2; ++c) {  // :357-366 the left list under the left id, then the right list under the right id
      fetch_last(c, kps[c], kid[c]);
      if (mirror_db && tracked) mirror(id[c], message.timestamp, kps[c], kid[c]);
    }
    std::lock_guard<std::mutex> lckv(mtx_last_vars);  // :369-381
    for (int c = 0; c < 2; ++c) {
      img_last[id[c]] = *img[c];
      img_mask_last[id[c]] = *mask[c];
      pts_last[id[c]] = kps[c];
      ids_last[id[c]] = kid[c];
    }
  }

  // the library's last points and ids as TrackBase keeps them (cam < 0: the monocular tracker's, else camera `cam` of the pair)
  void fetch_last(int cam, std::vector<cv::KeyPoint> &kps, std::vector<size_t> &kid) {
    int n = 0;
    if (cam < 0)
      plv_tracker_last(ctx, nullptr, nullptr, 1 << 30, &n);
    else
      plv_stereo_last(ctx, cam, nullptr, nullptr, 1 << 30, &n);
    std::vector<float> xy(2 * (size_t)n + 2);
    std::vector<uint64_t> ids((size_t)n + 1);
    if (cam < 0)
      plv_tracker_last(ctx, xy.data(), ids.data(), n, &n);
    else
      plv_stereo_last(ctx, cam, xy.data(), ids.data(), n, &n);
    kps.assign((size_t)n, cv::KeyPoint());
    kid.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
      kps[i].pt = cv::Point2f(xy[2 * i], xy[2 * i + 1]);
      kid[i] = (size_t)ids[i];
    }
  }

  // TrackKLT.cpp:176-179 / :357-366: every point of the list is an observation of this frame by camera cam_id
  void mirror(size_t cam_id, double timestamp, const std::vector<cv::KeyPoint> &kps, const std::vector<size_t> &kid) {
    for (size_t i = 0; i < kid.size(); ++i) {
      const cv::Point2f npt = camera_calib.at(cam_id)->undistort_cv(kps[i].pt);
      database->update_feature(kid[i], timestamp, cam_id, kps[i].pt.x, kps[i].pt.y, npt.x, npt.y);
    }
  }

  // TrackBase's observable state after a monocular feed: pts_last / ids_last, the database mirror, img_last / img_mask_last
  void after_feed(size_t cam_id, double timestamp, const cv::Mat &img, const cv::Mat &mask) {
    std::vector<cv::KeyPoint> kps;
    std::vector<size_t> kid;
    fetch_last(-1, kps, kid);
    if (mirror_db && have_last) mirror(cam_id, timestamp, kps, kid);
    have_last = true;
    std::lock_guard<std::mutex> lckv(mtx_last_vars);  // TrackKLT.cpp:182-189
    img_last[cam_id] = img;
    img_mask_last[cam_id] = mask;
    pts_last[cam_id] = kps;
    ids_last[cam_id] = kid;
  }

  std::shared_ptr<plv_ctx> owned;  // (first constructor)
  plv_ctx *ctx;
  bool mirror_db, have_last = false;
  bool stereo_pair;   // TrackBase::use_stereo as the constructor was given it
  int raw_index = 0;  // the raw block (and HBM slot) the next encoded message goes into: 0 .. 3
};

}  // namespace ov_core
