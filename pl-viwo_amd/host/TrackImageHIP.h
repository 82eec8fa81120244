// TrackImageHIP.h — the track picture of TrackBase::display_history / UpdaterCamera::get_track_img, drawn by libplviwo_hip.so.
// REF: open_vins/ov_core/src/track/TrackBase.cpp:119-265 (display_history), PL-VIWO/src/update/cam/UpdaterCamera.cpp:486-500
//      (get_track_img), PL-VIWO/src/update/cam/TrackLSD.cpp:832-887 (DrawFeatures)
//
// The image the tracker works on is the equalised level 0 of its pyramid in HBM; on the encoded-image route (TrackKLT_HIP::feed_new_camera
// with an encoding) there is no host grey image at all, so the inherited display_history has nothing to draw on.  plv_track_image
// paints the histories, the last lines with the points on them and the mask over that image on the device and returns the RGB
// picture with one copy.  An override of display_history / get_track_img calls track_image() and then cv::putText for the overlay
// ("init", "CAM:0"), which the library leaves to the caller (INTEGRATION.md "Track image").
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include <opencv2/core.hpp>

#include "plviwo.h"

#ifndef CV_8UC3
#define CV_8UC3 16  // CV_MAKETYPE(CV_8U, 3), OpenCV's own value: only for a core.hpp that does not define it (the test stand-in)
#endif

namespace plv_host {

// The layers (PLV_VIZ_* bits) over the newest image of `ctx`, with the features `highlighted` boxed (get_track_img passes the ids of
// State::cam_SLAM_features), into `out`: a CV_8UC3 matrix of the camera's size that the CALLER owns — nothing is allocated here, so a
// node can draw into the sensor_msgs/Image it is about to publish.  Returns the library's status: PLV_E_BADARG for a matrix of another
// type or size and before the first image was fed (plv_last_error says which).
inline int track_image(plv_ctx *ctx, const std::vector<size_t> &highlighted, int layers, cv::Mat &out) {
  int w = 0, h = 0;
  const int rc = plv_pyramid_download(ctx, PLV_PYR_CUR, 0, &w, &h, nullptr);
  if (rc != PLV_OK) return rc;
  if (out.empty() || out.type() != CV_8UC3 || out.cols != w || out.rows != h) return PLV_E_BADARG;
  const std::vector<uint64_t> ids(highlighted.begin(), highlighted.end());
  plv_track_image_options opt;
  plv_track_image_options_default(&opt);  // get_track_img's colours (255, 255, 0) / (255, 255, 255), 50 tracks
  opt.layers = layers;
  opt.n_highlighted = (int)ids.size();
  opt.highlighted = ids.empty() ? nullptr : ids.data();
  return plv_track_image(ctx, &opt, out.data, (int)(size_t)out.step);
}

}  // namespace plv_host
