// frontend_api.hip — point front-end entry points of include/plviwo.h (product code, no CPU path).
#include <algorithm>
#include <cmath>
#include <vector>

#include "detect_kernels.hpp"
#include "encoding_kernels.hpp"
#include "front_parts.hpp"
#include "frontend_kernels.hpp"
#include "line_kernels.hpp"
#include "plv_internal.hpp"

using namespace plv;

namespace {

struct FrontState : CamFront {  // the context's one camera, and what only the monocular path has
  int pending_n = -1;      // plv_perform_matching_launch .. _wait
  bool pending_ran = false;
  DevBuf slots[8];
  DevBuf ds_src, ds_dst;   // full-resolution staging of plv_downsample / plv_feed_image_downsampled
  // per-call point buffers
  DevBuf pts0, pts1, n0, n1, status, iters, mask, io;
  RansacScratch ransac;
  PinBuf img_pin[6];       // host images on their way to the device (plv_feed_image_enqueue): the caller's buffer is free at return
  int img_pin_next = 0;
  // images in their sensor encoding (plv_image_stage_encoded ...): nothing here is allocated before the first of them arrives
  PinBuf raw_pin[6];       // packed encoded images the conversion kernel reads in place: [0] [1] the library's own, [2 ..] plv_raw_image_buffer
  hipEvent_t raw_done[2] = {nullptr, nullptr};  // behind the conversion that read own block i: the block is free once it has passed
  int raw_pin_next = 0;
  DevBuf cv_src, cv_dst;   // staging of plv_image_convert
  DetJob det_pending;
  hipStream_t det_stream = nullptr;
  hipEvent_t det_done = nullptr;
  unsigned long long flow_done_stamp = 0;  // plv_ctx::gather_stamp when flow_done was recorded
  hipEvent_t flow_done = nullptr;  // behind the result copy of plv_perform_matching_launch: the wait does not cover what is enqueued after it
};

}  // namespace
namespace plv {
int level_geometry(int W, int H, int win, int max_level, PyrDesc &p) {
  p.levels = 0;
  unsigned off = 0;
  int w = W, h = H;
  for (int l = 0; l <= max_level && l < PLV_MAX_LEVELS; ++l) {
    if (l > 0) {
      int nw = (w + 1) / 2, nh = (h + 1) / 2;
      if (nw <= win || nh <= win) break;  // cv::buildOpticalFlowPyramid stops here
      w = nw;
      h = nh;
    }
    p.w[l] = w;
    p.h[l] = h;
    p.off[l] = off;
    off += (unsigned)(((size_t)w * h + 255) & ~(size_t)255);
    p.levels = l + 1;
  }
  return (int)off;
}
}  // namespace plv
extern "C" int plv_set_lk_window(plv_ctx *ctx, int win) {
  if (!ctx || win < 3 || win > 21 || (win & 1) == 0) {
    set_last_error("plv_set_lk_window: odd window sizes 3 .. 21");
    return PLV_E_BADARG;
  }
  if (ctx->fe_state) {
    FrontState *s = (FrontState *)ctx->fe_state;
    if (s->prepared() && s->levels_for(ctx, win) != s->pyr[0].levels) {
      set_last_error("plv_set_lk_window: a %d x %d window gives %d pyramid levels, the pyramids of this context have %d", win, win,
                     s->levels_for(ctx, win), s->pyr[0].levels);
      return PLV_E_BADARG;
    }
  }
  ctx->cfg.win_size = win;
  return PLV_OK;
}
namespace {
FrontState *fe(plv_ctx *ctx) {
  if (!ctx->fe_state) {
    auto *s = new FrontState();
    s->W = ctx->cfg.width;
    s->H = ctx->cfg.height;
    ctx->fe_state = s;
  }
  return (FrontState *)ctx->fe_state;
}

int ensure_pyramids(plv_ctx *ctx, FrontState *s) {
  if (s->prepared()) return PLV_OK;
  TRY(s->prepare(ctx, "front-end"));
  TRY(s->img_pin[0].reserve((size_t)s->W * s->H));  // (pinned blocks of plv_feed_image_enqueue: not allocated inside a frame)
  return s->img_pin[1].reserve((size_t)s->W * s->H);
}

// equalize + pyramid of the packed device image d_img into the next "current" pyramid
// h_src != null: d_img is still empty and the image sits in pinned host memory at h_src (the first kernel that reads it brings it in)
int feed_device(plv_ctx *ctx, FrontState *s, const uint8_t *d_img, const uint8_t *h_src = nullptr) {
  plv::HostPhase ph("feed image (enqueue hist + pyramid)");
  const int next = s->next();
  TRY(front_feed_pyramid(ctx, s->W, s->H, d_img, h_src, s->pyr[next], s->hist, s->clahe_lut));
  s->commit(next);
  return PLV_OK;
}
}  // namespace

int plv::front_feed_pyramid(plv_ctx *ctx, int W, int H, const uint8_t *d_img, const uint8_t *h_src, const PyrDesc &p, DevBuf &hist,
                            DevBuf &clahe_lut) {
  const int npix = W * H;
  switch (ctx->cfg.histogram_method) {
    case PLV_HIST_HISTOGRAM:  // (the equalisation rides on the first pyramid launch)
      return launch_equalize_pyramid(ctx, d_img, p, hist.as<unsigned>(), h_src);
    case PLV_HIST_NONE:
      if (h_src) PLV_HIP_CHECK(plv::memcpy_async((void *)d_img, h_src, (size_t)npix, hipMemcpyHostToDevice, ctx->stream));
      PLV_HIP_CHECK(plv::memcpy_async(p.base + p.off[0], d_img, (size_t)npix, hipMemcpyDeviceToDevice, ctx->stream));
      break;
    case PLV_HIST_CLAHE:  // REF: TrackKLT.cpp:60-64 — clip 10.0, 8x8 tiles
      if (h_src) PLV_HIP_CHECK(plv::memcpy_async((void *)d_img, h_src, (size_t)npix, hipMemcpyHostToDevice, ctx->stream));
      TRY(clahe_lut.reserve(64 * 256));
      TRY(launch_clahe(ctx, d_img, p.base + p.off[0], W, H, 10.0, 8, clahe_lut.as<uint8_t>()));
      break;
    default:
      set_last_error("front-end: unknown histogram method %d", ctx->cfg.histogram_method);
      return PLV_E_BADARG;
  }
  return launch_pyramid(ctx, p);
}

namespace {
int upload_image(plv_ctx *ctx, FrontState *s, void *dst, const uint8_t *img, int stride) {
  if (!img || stride < s->W) {
    set_last_error("front-end: null image or stride %d < width %d", stride, s->W);
    return PLV_E_BADARG;
  }
  PLV_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)s->W, img, (size_t)stride, (size_t)s->W, (size_t)s->H, hipMemcpyHostToDevice,
                                 ctx->stream));
  return PLV_OK;
}

}  // namespace

// ---- images in their sensor encoding
int plv::check_encoded(const char *who, const uint8_t *data, int stride, int encoding, int w) {
  const int bpp = encoding_bpp(encoding);
  if (bpp == 0) {
    set_last_error("%s: %d is no PLV_ENC_* encoding", who, encoding);
    return PLV_E_BADARG;
  }
  if (!data) {
    set_last_error("%s: null image", who);
    return PLV_E_BADARG;
  }
  if (stride < w * bpp) {
    set_last_error("%s: stride %d < width %d x %d bytes per pixel", who, stride, w, bpp);
    return PLV_E_BADARG;
  }
  return PLV_OK;
}

namespace {
// Where the conversion kernel reads a W x H image from: `data` itself when it lies (packed) in one of the library's page-locked raw
// blocks, else one of the library's own two blocks, into which the image is copied here.  *own: that block's index, or -1.
int encoded_source(FrontState *s, const uint8_t *data, int stride, int bpp, const uint8_t **h_src, int *own) {
  const size_t row = (size_t)s->W * bpp, bytes = row * s->H;
  *own = -1;
  if ((size_t)stride == row)
    for (auto &b : s->raw_pin)
      if (b.p && data >= b.as<uint8_t>() && data + bytes <= b.as<uint8_t>() + b.cap && ((data - b.as<uint8_t>()) & 15) == 0) {
        *h_src = data;
        return PLV_OK;
      }
  plv::HostPhase ph("encoded image: host copy into the pinned block");
  TRY(s->raw_pin[0].reserve(bytes));  // (both at the first image: the second call must not allocate)
  TRY(s->raw_pin[1].reserve(bytes));
  const int i = s->raw_pin_next;
  s->raw_pin_next ^= 1;
  // the conversion that read this block two images ago: normally long finished
  if (s->raw_done[i] && hipEventQuery(s->raw_done[i]) == hipErrorNotReady) PLV_HIP_CHECK(plv::event_sync(s->raw_done[i]));
  uint8_t *dst = s->raw_pin[i].as<uint8_t>();
  pack_rows(dst, data, (size_t)stride, row, s->H);
  *h_src = dst;
  *own = i;
  return PLV_OK;
}

// the conversion of a host image into d_dst (W x H grey bytes in HBM), enqueued on the ctx stream; arguments checked by the caller
int convert_enqueue(plv_ctx *ctx, FrontState *s, const uint8_t *data, int stride, int encoding, uint8_t *d_dst) {
  const uint8_t *h_src = nullptr;
  int own = -1;
  TRY(encoded_source(s, data, stride, encoding_bpp(encoding), &h_src, &own));
  TRY(launch_grey_from_encoded(ctx, h_src, true, d_dst, s->W, s->H, encoding));
  if (own >= 0) {
    if (!s->raw_done[own]) PLV_HIP_CHECK(hipEventCreateWithFlags(&s->raw_done[own], hipEventDisableTiming));
    PLV_HIP_CHECK(hipEventRecord(s->raw_done[own], ctx->stream));
  }
  return PLV_OK;
}

}  // namespace

namespace plv {
void plv_frontend_destroy(plv_ctx *ctx) {
  auto *s = (FrontState *)ctx->fe_state;
  if (!s) return;
  if (s->det_pending.active) (void)hipEventSynchronize(s->det_done);
  if (s->det_done) (void)hipEventDestroy(s->det_done);
  if (s->flow_done) (void)hipEventDestroy(s->flow_done);
  if (s->det_stream) (void)hipStreamDestroy(s->det_stream);
  for (auto &b : s->img_pin) b.release();
  for (auto &b : s->raw_pin) b.release();
  for (auto &e : s->raw_done)
    if (e) (void)hipEventDestroy(e);
  s->cv_src.release();
  s->cv_dst.release();
  DevBuf *bufs[] = {&s->ds_src, &s->ds_dst, &s->pts0, &s->pts1, &s->n0, &s->n1, &s->status, &s->iters, &s->mask, &s->io};
  for (auto *b : bufs) b->release();
  for (auto &b : s->slots) b.release();
  s->ransac.release();
  s->release();
  delete s;
  ctx->fe_state = nullptr;
}

// plv_feed_image without the wait at its end (the tracker's path: plv_tracker_feed goes on to enqueue the flow and waits there).
// The image is copied into one of two pinned blocks of the library first, so the caller's buffer is free when the call returns
// although the transfer and the kernels are only enqueued.
int plv_feed_image_enqueue(plv_ctx *ctx, const uint8_t *img, int stride) {
  if (!ctx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(ensure_pyramids(ctx, s));
  if (!img || stride < s->W) {
    set_last_error("front-end: null image or stride %d < width %d", stride, s->W);
    return PLV_E_BADARG;
  }
  const size_t bytes = (size_t)s->W * s->H;
  // an image the caller wrote straight into one of the library's pinned blocks (plv_image_buffer): nothing to copy on the host
  const uint8_t *h_src = nullptr;
  if (stride == s->W)
    for (auto &b : s->img_pin)
      if (b.p && img >= b.as<uint8_t>() && img + bytes <= b.as<uint8_t>() + b.cap) h_src = img;
  if (!h_src) {
    plv::HostPhase ph("feed image: host copy into the pinned block");
    PinBuf &pin = s->img_pin[s->img_pin_next];
    s->img_pin_next ^= 1;
    TRY(pin.reserve(bytes));
    pack_rows(pin.p, img, (size_t)stride, (size_t)s->W, s->H);
    h_src = pin.as<uint8_t>();  // (a block is reused two images later: the wait for that image's flow lies in between)
  }
  // no copy command: the histogram kernel reads the pinned block over PCIe (16 bytes per lane) and leaves the image in s->raw
  return feed_device(ctx, s, s->raw.as<uint8_t>(), h_src);
}

// plv_tracker_feed_encoded's image feed: the conversion into the frame's raw image, then the device feed, all enqueued
int plv_feed_encoded_enqueue(plv_ctx *ctx, const uint8_t *data, int stride, int encoding) {
  if (!ctx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(check_encoded("plv_tracker_feed_encoded", data, stride, encoding, s->W));
  if (encoding == PLV_ENC_MONO8) return plv_feed_image_enqueue(ctx, data, stride);  // (already grey: the host route's feed)
  TRY(ensure_pyramids(ctx, s));
  TRY(convert_enqueue(ctx, s, data, stride, encoding, s->raw.as<uint8_t>()));
  return feed_device(ctx, s, s->raw.as<uint8_t>());
}
}  // namespace plv
extern "C" {

int plv_image_stage_encoded(plv_ctx *ctx, int slot, const uint8_t *data, int stride, int encoding) {
  if (!ctx || slot < 0 || slot >= 8) {
    set_last_error("plv_image_stage_encoded: no context or slot %d outside 0 .. 7", slot);
    return PLV_E_BADARG;
  }
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(check_encoded("plv_image_stage_encoded", data, stride, encoding, s->W));
  TRY(ensure_pyramids(ctx, s));
  TRY(s->slots[slot].reserve((size_t)s->W * s->H));
  // stream-ordered, no host sync: the next call on this ctx that returns data synchronises
  return convert_enqueue(ctx, s, data, stride, encoding, s->slots[slot].as<uint8_t>());
}

// The encoded twin of plv_image_buffer: the conversion kernel reads an image written here where it lies.  The pointer stands until
// the same index is asked for with an encoding of more bytes per pixel (the block then grows).
int plv_raw_image_buffer(plv_ctx *ctx, int index, int encoding, uint8_t **ptr, int *stride) {
  const int bpp = encoding_bpp(encoding);
  if (!ctx || !ptr || index < 0 || index >= 4 || bpp == 0) {
    set_last_error("plv_raw_image_buffer: no context / pointer, index %d outside 0 .. 3 or encoding %d unknown", index, encoding);
    return PLV_E_BADARG;
  }
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(s->raw_pin[2 + index].reserve((size_t)s->W * s->H * bpp));  // (blocks 0 and 1 are the library's own)
  *ptr = s->raw_pin[2 + index].as<uint8_t>();
  if (stride) *stride = s->W * bpp;
  return PLV_OK;
}

int plv_image_convert(plv_ctx *ctx, const uint8_t *data, int stride, int encoding, int w, int h, uint8_t *grey, int grey_stride) {
  if (!ctx || !grey || w < 1 || h < 1 || grey_stride < w) {
    set_last_error("plv_image_convert: no context / output, or a %d x %d image with output stride %d", w, h, grey_stride);
    return PLV_E_BADARG;
  }
  TRY(check_encoded("plv_image_convert", data, stride, encoding, w));
  const int bpp = encoding_bpp(encoding);
  if (bpp == 1 && encoding != PLV_ENC_MONO8 && (w < 3 || h < 3)) {
    set_last_error("plv_image_convert: a Bayer mosaic is 3 x 3 at least, not %d x %d", w, h);
    return PLV_E_BADARG;
  }
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  const size_t row = (size_t)w * bpp;
  TRY(s->cv_src.reserve(row * h));
  TRY(s->cv_dst.reserve((size_t)w * h));
  PLV_HIP_CHECK(hipMemcpy2DAsync(s->cv_src.p, row, data, (size_t)stride, row, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
  TRY(launch_grey_from_encoded(ctx, s->cv_src.as<uint8_t>(), false, s->cv_dst.as<uint8_t>(), w, h, encoding));
  PLV_HIP_CHECK(hipMemcpy2DAsync(grey, (size_t)grey_stride, s->cv_dst.p, (size_t)w, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, ctx->stream));
  return stream_wait(ctx);
}

// A pinned host block of the library for the caller to write the next image into (a camera driver's DMA target, cv_bridge's copy
// target: `cv::Mat(h, w, CV_8UC1, ptr)`): plv_tracker_feed / plv_camera_frame recognise a pointer into it and skip their own host
// copy.  index 0 .. 3; packed rows (stride = width).  The block must not be overwritten before the call it was handed to has returned.
int plv_image_buffer(plv_ctx *ctx, int index, uint8_t **ptr, int *stride) {
  if (!ctx || !ptr || index < 0 || index >= 4) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(ensure_pyramids(ctx, s));
  TRY(s->img_pin[2 + index].reserve((size_t)s->W * s->H));  // (blocks 0 and 1 are the library's own)
  *ptr = s->img_pin[2 + index].as<uint8_t>();
  if (stride) *stride = s->W;
  return PLV_OK;
}

int plv_feed_image(plv_ctx *ctx, const uint8_t *img, int stride) {
  if (!ctx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(ensure_pyramids(ctx, s));
  TRY(upload_image(ctx, s, s->raw.p, img, stride));
  TRY(feed_device(ctx, s, s->raw.as<uint8_t>()));
  return stream_wait(ctx);
}

// cv::pyrDown(img, out, Size(cols / 2.0, rows / 2.0)) on the device: the Size_<int> constructor truncates, so an
// odd dimension halves downwards (the default would be (n + 1) / 2).  REF: UpdaterCamera.cpp:85-98
static int downsample_to(plv_ctx *ctx, FrontState *s, const uint8_t *src, int stride, int sw, int sh, uint8_t *d_dst) {
  if (!src || sw < 2 || sh < 2 || stride < sw) {
    set_last_error("downsample: bad source %dx%d stride %d", sw, sh, stride);
    return PLV_E_BADARG;
  }
  TRY(s->ds_src.reserve((size_t)sw * sh));
  PLV_HIP_CHECK(hipMemcpy2DAsync(s->ds_src.p, (size_t)sw, src, (size_t)stride, (size_t)sw, (size_t)sh, hipMemcpyHostToDevice,
                                 ctx->stream));
  return launch_pyrdown(ctx, s->ds_src.as<uint8_t>(), sw, sh, d_dst, sw / 2, sh / 2);
}

int plv_downsample(plv_ctx *ctx, const uint8_t *src, int stride, int src_w, int src_h, uint8_t *dst, int dstride) {
  if (!ctx || !dst || dstride < src_w / 2) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  const int dw = src_w / 2, dh = src_h / 2;
  TRY(s->ds_dst.reserve((size_t)dw * dh));
  TRY(downsample_to(ctx, s, src, stride, src_w, src_h, s->ds_dst.as<uint8_t>()));
  PLV_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dstride, s->ds_dst.p, (size_t)dw, (size_t)dw, (size_t)dh, hipMemcpyDeviceToHost,
                                 ctx->stream));
  return stream_wait(ctx);
}

int plv_feed_image_downsampled(plv_ctx *ctx, const uint8_t *img, int stride, int src_w, int src_h) {
  if (!ctx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(ensure_pyramids(ctx, s));
  if (src_w / 2 != s->W || src_h / 2 != s->H) {
    set_last_error("feed_image_downsampled: %dx%d halves to %dx%d, the context tracks %dx%d", src_w, src_h, src_w / 2, src_h / 2,
                   s->W, s->H);
    return PLV_E_BADARG;
  }
  TRY(downsample_to(ctx, s, img, stride, src_w, src_h, s->raw.as<uint8_t>()));
  TRY(feed_device(ctx, s, s->raw.as<uint8_t>()));
  return stream_wait(ctx);
}

int plv_image_stage(plv_ctx *ctx, int slot, const uint8_t *img, int stride) {
  if (!ctx || slot < 0 || slot >= 8) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(ensure_pyramids(ctx, s));
  TRY(s->slots[slot].reserve((size_t)s->W * s->H));
  TRY(upload_image(ctx, s, s->slots[slot].p, img, stride));
  return stream_wait(ctx);
}

int plv_feed_staged(plv_ctx *ctx, int slot) {
  if (!ctx || slot < 0 || slot >= 8) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  if (!s->slots[slot].p) {
    set_last_error("plv_feed_staged: slot %d is empty", slot);
    return PLV_E_BADARG;
  }
  // stream-ordered, no host sync: the next call on this ctx that returns data synchronises
  return feed_device(ctx, s, s->slots[slot].as<uint8_t>());
}

}  // extern "C"
namespace plv {
// The images the line code works on: the context's one camera, or camera 0 of the pair once the stereo tracker has taken the
// context (plv_ctx::tracker_kind).  Both are a CamFront; null while nothing has been fed.
static const CamFront *front_of(plv_ctx *ctx) {
  if (!ctx) return nullptr;
  if (ctx->tracker_kind == PLV_TRACKER_STEREO) return plv_stereo_front0(ctx);
  return ctx->fe_state ? fe(ctx) : nullptr;
}
int plv_front_fed_count(plv_ctx *ctx) {
  const CamFront *s = front_of(ctx);
  return s ? s->fed : 0;
}
// TrackBase::get_last_obs / get_last_ids of the camera the lines are tracked on
int plv_front_last_points(plv_ctx *ctx, float *pts, uint64_t *ids, int cap, int *n) {
  if (ctx && ctx->tracker_kind == PLV_TRACKER_STEREO) return plv_stereo_last(ctx, 0, pts, ids, cap, n);
  return plv_tracker_last(ctx, pts, ids, cap, n);
}
// where the flow launched last (plv_perform_matching_launch, not waited for yet) leaves its results on the device: tracked positions
// and their normalised coordinates [n][2], the inlier mask [n] (LK status and RANSAC)
int plv_front_match_device(plv_ctx *ctx, const float **d_p1, const float **d_n1, const uint8_t **d_mask, int *n) {
  if (!ctx || !ctx->fe_state) return PLV_E_BADARG;
  FrontState *s = fe(ctx);
  if (s->pending_n < 10 || !s->pending_ran || !s->io.p) return PLV_E_BADARG;
  const MatchBlock dev((size_t)s->pending_n, s->io.p);
  *d_p1 = dev.pts1(), *d_n1 = dev.n1(), *d_mask = dev.mask(), *n = s->pending_n;
  return PLV_OK;
}
const uint8_t *plv_front_level0(plv_ctx *ctx, int which, int *w, int *h) {
  const CamFront *s = front_of(ctx);
  return s ? s->level0(which, w, h) : nullptr;
}
}  // namespace plv
extern "C" {

int plv_pyramid_levels(plv_ctx *ctx, int which) {
  if (!ctx || !ctx->fe_state) return 0;
  FrontState *s = fe(ctx);
  if (s->fed < (which == PLV_PYR_LAST ? 2 : 1)) return 0;
  return s->pyr[which == PLV_PYR_LAST ? 1 - s->cur : s->cur].levels;
}

int plv_pyramid_download(plv_ctx *ctx, int which, int level, int *w, int *h, uint8_t *out) {
  if (!ctx || !ctx->fe_state) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  if (s->fed < (which == PLV_PYR_LAST ? 2 : 1)) return PLV_E_BADARG;
  const PyrDesc &p = s->pyr[which == PLV_PYR_LAST ? 1 - s->cur : s->cur];
  if (level < 0 || level >= p.levels) return PLV_E_BADARG;
  if (w) *w = p.w[level];
  if (h) *h = p.h[level];
  if (out) {
    PLV_HIP_CHECK(plv::memcpy_async(out, p.base + p.off[level], (size_t)p.w[level] * p.h[level], hipMemcpyDeviceToHost,
                                 ctx->stream));
    return stream_wait(ctx);
  }
  return PLV_OK;
}

static int need_two(plv_ctx *ctx, FrontState *s, const char *who) {
  if (s->fed < 2) {
    set_last_error("%s: needs two fed images (last and current pyramid)", who);
    return PLV_E_BADARG;
  }
  (void)ctx;
  return PLV_OK;
}

static int reserve_points(FrontState *s, int n, int ransac_iters) {
  size_t nn = (size_t)std::max(n, 1);
  TRY(s->pts0.reserve(nn * 8));
  TRY(s->pts1.reserve(nn * 8));
  TRY(s->n0.reserve(nn * 8));
  TRY(s->n1.reserve(nn * 8));
  TRY(s->status.reserve(nn));
  TRY(s->mask.reserve(nn));
  TRY(s->iters.reserve(nn * 4));
  return s->ransac.reserve(ransac_iters);
}

int plv_lk_track(plv_ctx *ctx, int n, const float *pts0, float *pts1, uint8_t *status, int *iters) {
  if (!ctx || n < 0 || (n > 0 && (!pts0 || !pts1 || !status))) return PLV_E_BADARG;
  if (n == 0) return PLV_OK;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(need_two(ctx, s, "plv_lk_track"));
  TRY(reserve_points(s, n, 1));
  PLV_HIP_CHECK(plv::memcpy_async(s->pts0.p, pts0, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(s->pts1.p, pts1, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  TRY(launch_lk(ctx, s->pyr[1 - s->cur], s->pyr[s->cur], n, s->pts0.as<float>(), s->pts1.as<float>(),
                s->status.as<uint8_t>(), s->iters.as<int>(), ctx->cfg.win_size, ctx->cfg.lk_max_iters, ctx->cfg.lk_eps));
  PLV_HIP_CHECK(plv::memcpy_async(pts1, s->pts1.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(status, s->status.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (iters) PLV_HIP_CHECK(plv::memcpy_async(iters, s->iters.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  return stream_wait(ctx);
}

static CamK cam_of(plv_ctx *ctx) {
  CamK K;
  for (int i = 0; i < 8; ++i) K.v[i] = ctx->cfg.intrinsics[i];
  K.model = ctx->cam_model;
  return K;
}

int plv_undistort(plv_ctx *ctx, int n, const float *uv, float *xy) {
  if (!ctx || n < 0 || (n > 0 && (!uv || !xy))) return PLV_E_BADARG;
  if (n == 0) return PLV_OK;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(reserve_points(s, n, 1));
  PLV_HIP_CHECK(plv::memcpy_async(s->pts0.p, uv, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  TRY(launch_undistort(ctx, cam_of(ctx), n, s->pts0.as<float>(), s->n0.as<float>()));
  PLV_HIP_CHECK(plv::memcpy_async(xy, s->n0.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  return stream_wait(ctx);
}

int plv_ransac_fundamental(plv_ctx *ctx, int n, const float *m1, const float *m2, double thr, uint32_t seed,
                           uint8_t *mask, int *n_inliers, int *iters_used) {
  if (!ctx || n < 0 || (n > 0 && (!m1 || !m2 || !mask))) return PLV_E_BADARG;
  if (n_inliers) *n_inliers = 0;
  if (iters_used) *iters_used = 0;
  if (n == 0) return PLV_OK;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  const int mi = std::max(1, ctx->cfg.ransac_max_iters);
  TRY(reserve_points(s, n, mi));
  PLV_HIP_CHECK(plv::memcpy_async(s->n0.p, m1, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(s->n1.p, m2, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  TRY(launch_ransac(ctx, s->n0.as<float>(), s->n1.as<float>(), n, thr, ctx->cfg.ransac_conf, mi, seed, s->ransac.counts.as<int>(),
                    nullptr, s->mask.as<uint8_t>(), s->ransac.info.as<int>(), s->ransac.models.as<double>()));
  int info[2] = {0, 0};
  PLV_HIP_CHECK(plv::memcpy_async(mask, s->mask.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(info, s->ransac.info.p, sizeof(info), hipMemcpyDeviceToHost, ctx->stream));
  TRY(stream_wait(ctx));
  if (n_inliers) *n_inliers = info[0];
  if (iters_used) *iters_used = info[1];
  return PLV_OK;
}

int plv_ransac_hypotheses(plv_ctx *ctx, int n, const float *m1, const float *m2, double thr, uint32_t seed, int nhyp, double *models,
                          int *counts) {
  if (!ctx || n < 7 || nhyp < 1 || nhyp > 4096 || !m1 || !m2 || !models || !counts) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  TRY(reserve_points(s, n, nhyp));
  PLV_HIP_CHECK(plv::memcpy_async(s->n0.p, m1, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(s->n1.p, m2, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  TRY(launch_ransac_hyp(ctx, s->n0.as<float>(), s->n1.as<float>(), n, thr, seed, nhyp, s->ransac.counts.as<int>(), s->ransac.models.as<double>()));
  PLV_HIP_CHECK(plv::memcpy_async(models, s->ransac.models.p, (size_t)nhyp * 28 * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(counts, s->ransac.counts.p, (size_t)nhyp * 3 * 4, hipMemcpyDeviceToHost, ctx->stream));
  return stream_wait(ctx);
}

int plv_perform_matching_launch(plv_ctx *ctx, int n, const float *pts0, const float *pts1_init) {
  if (!ctx || n < 0 || (n > 0 && (!pts0 || !pts1_init))) return PLV_E_BADARG;
  FrontState *s0 = fe(ctx);
  s0->pending_n = -1;
  if (n < 10) {  // REF: TrackKLT.cpp:848-852 (nothing to run: the wait returns an all-zero mask)
    s0->pending_n = n;
    s0->pending_ran = false;
    return PLV_OK;
  }
  (void)hipSetDevice(ctx->device);
  FrontState *s = s0;
  TRY(need_two(ctx, s, "plv_perform_matching"));
  TRY(reserve_points(s, n, ctx->cfg.ransac_max_iters));
  // one device block (MatchBlock) and its pinned twin: no H2D and one D2H (pts1 .. mask) per call at the most
  const size_t total = MatchBlock((size_t)n).total();
  TRY(s->io.reserve(total));
  TRY(ctx->h_pin_flow.reserve(total));
  const MatchBlock dev((size_t)n, s->io.p), pin((size_t)n, ctx->h_pin_flow.p);
  // No copy commands around the two kernels: lk_kernel reads the points and the initial guesses straight from the pinned buffer
  // (16 B per point, once) and the last kernel of the call copies the results back into it (ransac_select_kernel).
  memcpy(pin.pts0(), pts0, (size_t)n * 8);
  memcpy(pin.pts1(), pts1_init, (size_t)n * 8);
  const CamK camk = cam_of(ctx);
  TRY(launch_lk(ctx, s->pyr[1 - s->cur], s->pyr[s->cur], n, pin.pts0(), dev.pts1(), dev.status(), dev.iters(), ctx->cfg.win_size,
                ctx->cfg.lk_max_iters, ctx->cfg.lk_eps, &camk, dev.n0(), dev.n1(),
                pin.pts1()));  // (+ the undistortion of both point sets on the same launch)
  TRY(match_ransac_tail(ctx, camk, dev, pin, s->ransac));
  if (!s->flow_done) PLV_HIP_CHECK(hipEventCreateWithFlags(&s->flow_done, hipEventDisableTiming));
  PLV_HIP_CHECK(hipEventRecord(s->flow_done, ctx->stream));
  s->flow_done_stamp = ctx->gather_stamp;
  s->pending_n = n;
  s->pending_ran = true;
  return PLV_OK;
}

int plv_perform_matching_wait(plv_ctx *ctx, float *pts1, uint8_t *mask_out, float *n0, float *n1, long long *lk_iters) {
  if (!ctx) return PLV_E_BADARG;
  FrontState *s = fe(ctx);
  const int n = s->pending_n;
  if (n < 0) {
    set_last_error("plv_perform_matching_wait: nothing was launched");
    return PLV_E_BADARG;
  }
  s->pending_n = -1;
  if (lk_iters) *lk_iters = 0;
  if (n == 0) return PLV_OK;
  if (!pts1 || !mask_out) return PLV_E_BADARG;
  if (!s->pending_ran) {
    memset(mask_out, 0, (size_t)n);
    return PLV_OK;
  }
  (void)hipSetDevice(ctx->device);
  if (ctx->prof.on)
    TRY(stream_wait(ctx));  // (the per-kernel timer reads every event recorded so far)
  else
  {
    // not the whole stream: the caller may have enqueued more behind the flow
    PLV_HIP_CHECK(plv::event_sync(s->flow_done));
    if (s->flow_done_stamp > ctx->cov_host_synced) ctx->cov_host_synced = s->flow_done_stamp;
  }
  const long long t = match_read_back(MatchBlock((size_t)n, ctx->h_pin_flow.p), pts1, mask_out, n0, n1);
  if (lk_iters) *lk_iters = t;
  return PLV_OK;
}

int plv_perform_matching(plv_ctx *ctx, int n, const float *pts0, float *pts1, uint8_t *mask_out, float *n0, float *n1,
                         long long *lk_iters) {
  if (!ctx || n < 0 || (n > 0 && (!pts0 || !pts1 || !mask_out))) return PLV_E_BADARG;
  if (lk_iters) *lk_iters = 0;
  if (n == 0) return PLV_OK;
  TRY(plv_perform_matching_launch(ctx, n, pts0, pts1));
  return plv_perform_matching_wait(ctx, pts1, mask_out, n0, n1, lk_iters);
}


// plv_perform_detection replaces TrackKLT::perform_detection_monocular (REF: open_vins/ov_core/src/
// track/TrackKLT.cpp:395-528).  The occupancy-grid bookkeeping is host logic exactly as in the
// reference (a few hundred integer operations); the per-cell FAST + top-k (Grider_GRID.h:108-151)
// and the sub-pixel refinement (:163-174) run on the device on level 0 of the chosen pyramid.
// Three stages: det_pre (host: grids, cells that need features), det_launch (device, on any stream), det_post (host: reject
// near existing points, ids in extraction order).  plv_perform_detection runs them back to back; plv_perform_detection_ahead runs
// the first two on a side stream as soon as a frame's points are known, so that the top-up the NEXT frame starts with (it works on
// the then-last image with these very points, TrackKLT.cpp:127-131) is waiting for it instead of sitting on its critical path.
}  // extern "C"
namespace plv {
int det_pre(plv_ctx *ctx, int w, int h, const uint8_t *mask, const float *pts_in, const uint64_t *ids_in, int n_in, DetJob &J,
            const DetStereoRules *stereo) {
  const plv_config &c = ctx->cfg;
  const int min_px = c.min_px_dist, grid_x = c.grid_x, grid_y = c.grid_y, num_features = c.num_features;
  if (min_px < 1 || grid_x < 1 || grid_y < 1) return PLV_E_BADARG;
  // ---- REF :401-464: occupancy grids, drop edge / masked / too-close points, remember the painted boxes
  J.cw = (int)((float)w / (float)min_px), J.ch = (int)((float)h / (float)min_px);
  J.close.assign((size_t)J.cw * J.ch, 0);
  std::vector<uint8_t> grid((size_t)grid_x * grid_y, 0);
  const float size_x = (float)w / (float)grid_x, size_y = (float)h / (float)grid_y;
  J.boxes.clear();
  J.pts.clear();
  J.ids.clear();
  for (int i = 0; i < n_in; ++i) {
    const float fx = pts_in[2 * i], fy = pts_in[2 * i + 1];
    const int x = (int)fx, y = (int)fy;
    const int edge = 10;
    if (x < edge || x >= w - edge || y < edge || y >= h - edge) continue;
    const int xc = (int)(fx / (float)min_px), yc = (int)(fy / (float)min_px);
    if (xc < 0 || xc >= J.cw || yc < 0 || yc >= J.ch) continue;
    const int xg = (int)std::floor(fx / size_x), yg = (int)std::floor(fy / size_y);
    if (xg < 0 || xg >= grid_x || yg < 0 || yg >= grid_y) continue;
    if (J.close[(size_t)yc * J.cw + xc] > 127 &&
        !(stereo && std::find(stereo->spared, stereo->spared + stereo->n_spared, ids_in[i]) != stereo->spared + stereo->n_spared))
      continue;
    if (mask && mask[(size_t)y * w + x] > 127) continue;
    J.close[(size_t)yc * J.cw + xc] = 255;
    if (grid[(size_t)yg * grid_x + xg] < 255) grid[(size_t)yg * grid_x + xg] += 1;
    if (x - min_px >= 0 && x + min_px < w && y - min_px >= 0 && y + min_px < h) {
      J.boxes.push_back(x);
      J.boxes.push_back(y);
    }
    J.pts.push_back(fx);
    J.pts.push_back(fy);
    J.ids.push_back(ids_in[i]);
  }
  J.n_cells = 0;
  J.n_slots = 0;
  // ---- REF :466-471
  const double min_feat_percent = 0.50;
  const int n = (int)J.ids.size();
  const int needed = num_features - n, least = std::min(20, (int)(min_feat_percent * num_features));
  if (stereo && stereo->strict_need ? needed <= least : needed < least) return PLV_OK;
  // ---- REF :478-492 cells that still need features and are not fully masked
  const int nfg_req = std::max(1, (int)(min_feat_percent * ((int)((double)num_features / (double)(grid_x * grid_y)) + 1)));
  // REF Grider_GRID.h:88-98 grid actually used for extraction
  int gx = grid_x, gy = grid_y;
  if (num_features < gx * gy) {
    double ratio = (double)gx / (double)gy;
    gy = (int)std::ceil(std::sqrt(num_features / ratio));
    gx = (int)std::ceil(gy * ratio);
  }
  J.nfg = (int)((double)num_features / (double)(gx * gy)) + 1;
  J.sxp = w / gx, J.syp = h / gy;
  J.cells.clear();
  for (int x = 0; x < grid_x; ++x)
    for (int y = 0; y < grid_y; ++y) {
      const int sx = std::min((int)std::floor(x * (double)w / grid_x), w - 1), sy = std::min((int)std::floor(y * (double)h / grid_y), h - 1);
      const bool masked = mask && mask[(size_t)sy * w + sx] == 255;
      if ((int)grid[(size_t)y * grid_x + x] < nfg_req && !masked) {
        if (x * J.sxp + J.sxp > w || y * J.syp + J.syp > h) continue;  // REF Grider_GRID.h:117-118
        J.cells.push_back(x);
        J.cells.push_back(y);
      }
    }
  const int n_cells = (int)J.cells.size() / 2;
  if (n_cells == 0 || J.sxp < 7 || J.syp < 7) return PLV_OK;
  J.n_cells = n_cells;
  J.n_slots = n_cells * J.nfg;
  return PLV_OK;
}

// FAST per cell + sub-pixel refinement of every kept slot + the copy of the slots to pinned memory, all on `stream`
int det_launch(plv_ctx *ctx, DetScratch &scratch, int w, int h, const PyrDesc &pyr, const uint8_t *mask, DetJob &J, hipStream_t stream) {
  DetScratch *s = &scratch;
  const plv_config &c = ctx->cfg;
  const int n_cells = J.n_cells, n_slots = J.n_slots;
  const size_t o_cells = 0, o_boxes = ((size_t)n_cells * 8 + 15) & ~(size_t)15, in_total = o_boxes + ((J.boxes.size() * 4 + 15) & ~(size_t)15);
  TRY(s->det_pin.reserve(in_total + (size_t)n_slots * 13 + (size_t)n_cells + 128));
  TRY(s->det_in.reserve(in_total + 16));
  const size_t o_xy = 0, o_resp = (size_t)n_slots * 8, o_valid = (size_t)n_slots * 12, o_over = (size_t)n_slots * 13, out_total = o_over + (size_t)n_cells;
  TRY(s->det_out.reserve(out_total + 16));
  char *hp = s->det_pin.as<char>();
  J.h_out = hp + ((in_total + 63) & ~(size_t)63);  // results land behind the inputs (both may be in flight at once)
  memcpy(hp + o_cells, J.cells.data(), J.cells.size() * 4);
  if (!J.boxes.empty()) memcpy(hp + o_boxes, J.boxes.data(), J.boxes.size() * 4);
  PLV_HIP_CHECK(plv::memcpy_async(s->det_in.p, hp, in_total, hipMemcpyHostToDevice, stream));
  const uint8_t *d_mask = nullptr;
  if (mask) {
    TRY(s->det_mask.reserve((size_t)w * h));
    PLV_HIP_CHECK(plv::memcpy_async(s->det_mask.p, mask, (size_t)w * h, hipMemcpyHostToDevice, stream));
    d_mask = s->det_mask.as<uint8_t>();
  }
  if (!s->subpix_tab.p) {  // cv::cornerSubPix window weights exp(-(x/5)^2) exp(-(y/5)^2)
    float tab[121];
    for (int i = 0; i < 11; ++i) {
      float y = (float)(i - 5) / 5;
      float vy = std::exp(-y * y);
      for (int j = 0; j < 11; ++j) {
        float x = (float)(j - 5) / 5;
        tab[i * 11 + j] = (float)(vy * std::exp(-x * x));
      }
    }
    TRY(s->subpix_tab.reserve(sizeof(tab)));
    PLV_HIP_CHECK(hipMemcpy(s->subpix_tab.p, tab, sizeof(tab), hipMemcpyHostToDevice));
  }
  DetectParams P{};
  P.img = pyr.base + pyr.off[0];
  P.W = w;
  P.H = h;
  P.mask = d_mask;
  P.cells = (const int *)(s->det_in.as<char>() + o_cells);
  P.cell_w = J.sxp;
  P.cell_h = J.syp;
  P.threshold = c.fast_threshold;
  P.nfg = J.nfg;
  // every local maximum a cell can have is stored: none is dropped, whatever the image (in whole blocks of 4096 keys: the lists of
  // the default shape, 3 240 keys at most, lie where they always did)
  P.cand_cap = (int)std::min<long long>(((long long)fast_cell_bound(J.sxp, J.syp) + 4095) / 4096 * 4096, 0x7fffffff);
  P.lds_cap = 4096;
  P.boxes = (const int *)(s->det_in.as<char>() + o_boxes);
  P.n_boxes = (int)J.boxes.size() / 2;
  P.min_px_dist = c.min_px_dist;
  P.out_xy = (float *)(s->det_out.as<char>() + o_xy);
  P.out_resp = (float *)(s->det_out.as<char>() + o_resp);
  P.out_valid = (uint8_t *)(s->det_out.as<char>() + o_valid);
  P.out_over = (uint8_t *)(s->det_out.as<char>() + o_over);
  {  // per-cell candidate lists of fast_tiles_kernel; the counters start at zero and fast_topk_kernel leaves them at zero
    const size_t all_cells = (size_t)c.grid_x * c.grid_y;
    if (s->det_cand_n.cap < all_cells * 4) {
      TRY(s->det_cand_n.reserve(all_cells * 4));
      PLV_HIP_CHECK(hipMemsetAsync(s->det_cand_n.p, 0, s->det_cand_n.cap, stream));
    }
    TRY(s->det_cand.reserve(all_cells * (size_t)P.cand_cap * 8));
  }
  hipStream_t keep = ctx->stream;
  ctx->stream = stream;  // (the launchers take the stream from the ctx)
  int rc = launch_fast_cells(ctx, P, n_cells, s->det_cand.as<unsigned long long>(), s->det_cand_n.as<int>());
  if (rc == PLV_OK) rc = launch_subpix(ctx, P.img, w, h, n_slots, P.out_valid, P.out_xy, s->subpix_tab.as<float>(), 5, 20, 0.001);
  ctx->stream = keep;
  TRY(rc);
  PLV_HIP_CHECK(plv::memcpy_async(J.h_out, s->det_out.p, out_total, hipMemcpyDeviceToHost, stream));
  return PLV_OK;
}

// The backstop behind the candidate storage: a cell that counted more maxima than were stored (its counter was not at zero when the
// frame began, say) has no trustworthy top-k.  The whole detection is refused, before det_post has written anything.
int det_check(const DetJob &J) {
  if (J.n_slots <= 0) return PLV_OK;
  const uint8_t *over = (const uint8_t *)(J.h_out + (size_t)J.n_slots * 13);
  for (int i = 0; i < J.n_cells; ++i)
    if (over[i]) {
      set_last_error("plv_perform_detection: cell (%d, %d) of %dx%d pixels had more corner candidates than were stored", J.cells[2 * i],
                     J.cells[2 * i + 1], J.sxp, J.syp);
      return PLV_E_CAPACITY;
    }
  return PLV_OK;
}

// ---- REF :497-527 reject near existing points: take(x, y) for every corner that stays, in extraction order, while room() holds
template <class Room, class Take> static void accept_corners(plv_ctx *ctx, const DetJob &J, Room room, Take take) {
  if (J.n_slots <= 0) return;
  const int min_px = ctx->cfg.min_px_dist;
  std::vector<uint8_t> close = J.close;
  const float *oxy = (const float *)(J.h_out);
  const uint8_t *oval = (const uint8_t *)(J.h_out + (size_t)J.n_slots * 12);
  for (int sl = 0; sl < J.n_slots && room(); ++sl) {
    if (!oval[sl]) continue;
    const float px = oxy[2 * sl], py = oxy[2 * sl + 1];
    const int xg = (int)(px / (float)min_px), yg = (int)(py / (float)min_px);
    if (xg < 0 || xg >= J.cw || yg < 0 || yg >= J.ch) continue;
    if (close[(size_t)yg * J.cw + xg] > 127) continue;
    close[(size_t)yg * J.cw + xg] = 255;
    take(px, py);
  }
}

// ... and ids in extraction order
void det_post(plv_ctx *ctx, const DetJob &J, float *pts, uint64_t *ids, int cap, uint64_t *currid, int *n_out) {
  int n = (int)J.ids.size();
  std::copy(J.pts.begin(), J.pts.end(), pts);
  std::copy(J.ids.begin(), J.ids.end(), ids);
  accept_corners(ctx, J, [&] { return n < cap; }, [&](float px, float py) {
    pts[2 * n] = px;
    pts[2 * n + 1] = py;
    ids[n] = ++*currid;
    ++n;
  });
  *n_out = n;
}

void det_new_points(plv_ctx *ctx, const DetJob &J, std::vector<float> &out) {
  out.clear();
  accept_corners(ctx, J, [] { return true; }, [&](float px, float py) {
    out.push_back(px);
    out.push_back(py);
  });
}
}  // namespace plv

namespace {
// a detection that was started ahead of time and has not been collected: wait for it so that its buffers can be reused
void det_drop_pending(FrontState *s);
}  // namespace
namespace plv {
// plv_ctx_synchronize: the side stream's work belongs to the frame that started it — wait for it too (the job stays collectable)
int plv_front_quiesce(plv_ctx *ctx) {
  if (!ctx || !ctx->fe_state) return PLV_OK;
  FrontState *s = (FrontState *)ctx->fe_state;
  if (s->det_pending.active && s->det_done) PLV_HIP_CHECK(plv::event_sync(s->det_done));
  return PLV_OK;
}
}  // namespace plv
extern "C" {
namespace {
void det_drop_pending(FrontState *s) {
  if (s->det_pending.active) {
    (void)plv::event_sync(s->det_done);
    s->det_pending.active = false;
  }
}
}  // namespace

int plv_perform_detection(plv_ctx *ctx, int which, const uint8_t *mask, float *pts, uint64_t *ids, int n_in, int cap,
                          uint64_t *currid, int *n_out) {
  if (!ctx || !pts || !ids || !currid || !n_out || n_in < 0 || cap < n_in) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  if (s->fed < (which == PLV_PYR_LAST ? 2 : 1)) {
    set_last_error("plv_perform_detection: no %s pyramid yet", which == PLV_PYR_LAST ? "last" : "current");
    return PLV_E_BADARG;
  }
  // ---- a detection started ahead of time on what is now the last image, with these very points (and mask)?
  DetJob &A = s->det_pending;
  if (A.active) {
    const bool same = which == PLV_PYR_LAST && A.fed + 1 == s->fed && A.n_in == n_in && A.has_mask == (mask != nullptr) &&
                      (n_in == 0 || (!memcmp(A.in_pts.data(), pts, (size_t)n_in * 8) && !memcmp(A.in_ids.data(), ids, (size_t)n_in * 8))) &&
                      (!mask || !memcmp(A.in_mask.data(), mask, (size_t)s->W * s->H));
    (void)plv::event_sync(s->det_done);
    A.active = false;
    if (same) {
      if ((int)A.ids.size() > cap) return PLV_E_CAPACITY;
      TRY(det_check(A));
      det_post(ctx, A, pts, ids, cap, currid, n_out);
      return PLV_OK;
    }
  }
  const PyrDesc &pyr = s->pyr[which == PLV_PYR_LAST ? 1 - s->cur : s->cur];
  DetJob J;
  TRY(det_pre(ctx, s->W, s->H, mask, pts, ids, n_in, J));
  if (J.n_slots > 0) {
    TRY(det_launch(ctx, s->det, s->W, s->H, pyr, mask, J, ctx->stream));
    TRY(stream_wait(ctx));
    TRY(det_check(J));
  }
  det_post(ctx, J, pts, ids, cap, currid, n_out);
  return PLV_OK;
}

}  // extern "C"

namespace plv {

// The top-up detection of the NEXT frame, started now: on the current image (the next frame's last image) with the points this frame
// ended with.  Runs on a side stream next to whatever the caller enqueues on the ctx stream (the updates); plv_perform_detection of
// the next frame finds it finished (the per-kernel profiler follows it onto the side stream: Profiler::collect).
int plv_perform_detection_ahead(plv_ctx *ctx, const uint8_t *mask, const float *pts, const uint64_t *ids, int n_in) {
  if (!ctx || n_in < 0 || (n_in > 0 && (!pts || !ids))) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  FrontState *s = fe(ctx);
  if (s->fed < 1) return PLV_OK;
  det_drop_pending(s);
  DetJob &A = s->det_pending;
  TRY(det_pre(ctx, s->W, s->H, mask, pts, ids, n_in, A));
  A.fed = s->fed;
  A.n_in = n_in;
  A.has_mask = mask != nullptr;
  A.in_pts.assign(pts, pts + 2 * (size_t)n_in);
  A.in_ids.assign(ids, ids + n_in);
  if (mask)
    A.in_mask.assign(mask, mask + (size_t)s->W * s->H);
  else
    A.in_mask.clear();
  if (!s->det_stream) {
    PLV_HIP_CHECK(hipStreamCreateWithFlags(&s->det_stream, hipStreamNonBlocking));
    PLV_HIP_CHECK(hipEventCreateWithFlags(&s->det_done, hipEventDisableTiming));
  }
  if (A.n_slots > 0) TRY(det_launch(ctx, s->det, s->W, s->H, s->pyr[s->cur], mask ? A.in_mask.data() : nullptr, A, s->det_stream));  // (the job's own copy of the mask)
  PLV_HIP_CHECK(hipEventRecord(s->det_done, s->det_stream));
  A.active = true;
  return PLV_OK;
}

}  // namespace plv
