// draw_api.hip — the display path behind the C-ABI (include/plviwo.h "track image"): the rasteriser's entry point and the layers that turn
// tracker state into its primitive list.
//   TrackBase::display_active / display_history   REF: open_vins/ov_core/src/track/TrackBase.cpp:90-100, 119-265
//   UpdaterCamera::get_track_img                   REF: PL-VIWO/src/update/cam/UpdaterCamera.cpp:486-500
//   TrackLSD::DrawFeatures                         REF: PL-VIWO/src/update/cam/TrackLSD.cpp:832-887
// The layers are host bookkeeping over what the tracker's own entry points export (plv_tracker_last, plv_db_export_tracks,
// plv_line_tracker_last, plv_line_tracker_last_points, plv_line_db_ids): nothing here writes tracker state.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "draw_kernels.hpp"
#include "plv_internal.hpp"

using namespace plv;

namespace {

struct DrawState {
  DevBuf d_grey, d_mask, d_prims, d_rgb;
  PinBuf pin;                  // [primitives][mask]: what the host builds goes up from here
  hipEvent_t done = nullptr;   // behind the result copy: the call waits for this and for nothing enqueued after it
};

std::mutex g_mtx;
std::unordered_map<plv_ctx *, DrawState *> g_draw;
DrawState *ds(plv_ctx *ctx) {
  std::lock_guard<std::mutex> lk(g_mtx);
  auto it = g_draw.find(ctx);
  if (it != g_draw.end()) return it->second;
  DrawState *s = new DrawState();
  g_draw[ctx] = s;
  return s;
}

constexpr int COORD_MAX = 1 << 24;        // plv_draw_primitives refuses anything beyond
constexpr float FLOAT_COORD_MAX = 1048576.f;  // 2^20: a layer drops the primitive

bool coord_ok(int v) { return v >= -COORD_MAX && v <= COORD_MAX; }

int check_prims(const plv_draw_prim *prims, int n) {
  for (int i = 0; i < n; ++i) {
    const plv_draw_prim &p = prims[i];
    if (p.kind != PLV_DRAW_RING && p.kind != PLV_DRAW_BOX && p.kind != PLV_DRAW_SEG) {
      set_last_error("draw: primitive %d has the unknown kind %d", i, p.kind);
      return PLV_E_BADARG;
    }
    if (!coord_ok(p.x0) || !coord_ok(p.y0) || (p.kind != PLV_DRAW_RING && (!coord_ok(p.x1) || !coord_ok(p.y1)))) {
      set_last_error("draw: primitive %d has a coordinate beyond +-2^24", i);
      return PLV_E_BADARG;
    }
  }
  return PLV_OK;
}

// room in the staging block for n primitives
size_t stage_bytes(int n) { return ((size_t)std::max(n, 1) * sizeof(plv_draw_prim) + 255) & ~(size_t)255; }

// grey / mask: device pointers (mask may be null).  Stages the primitives that meet the image at the start of the pinned block
// (stage_bytes(n) reserved by the caller), enqueues their copy, the kernel and the copy of the result, waits for that copy.
int draw_and_fetch(plv_ctx *ctx, DrawState *s, const uint8_t *d_grey, int grey_pitch, const uint8_t *d_mask, int mask_pitch,
                   const plv_draw_prim *prims, int n, int w, int h, uint8_t *rgb, int rgb_stride) {
  plv_draw_prim *stage = s->pin.as<plv_draw_prim>();
  int kept = 0;
  for (int i = 0; i < n; ++i) {  // in order: what lies wholly outside never travels
    long long bx0, by0, bx1, by1;
    draw_prim_bbox(prims[i], bx0, by0, bx1, by1);
    if (bx0 <= bx1 && bx0 < w && bx1 >= 0 && by0 < h && by1 >= 0) stage[kept++] = prims[i];
  }
  const size_t pitch = draw_rgb_pitch(w);
  TRY(s->d_rgb.reserve(pitch * h));
  TRY(s->d_prims.reserve(stage_bytes(kept)));
  if (!s->done) PLV_HIP_CHECK(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
  if (kept) PLV_HIP_CHECK(plv::memcpy_async(s->d_prims.p, stage, (size_t)kept * sizeof(plv_draw_prim), hipMemcpyHostToDevice, ctx->stream));
  TRY(launch_draw(ctx, d_grey, grey_pitch, d_mask, mask_pitch, s->d_prims.as<plv_draw_prim>(), kept, w, h, s->d_rgb.as<uint8_t>()));
  ++counters().copies;
  counters().copy_bytes += (size_t)3 * w * h;
  PLV_HIP_CHECK(hipMemcpy2DAsync(rgb, (size_t)rgb_stride, s->d_rgb.p, pitch, (size_t)3 * w, (size_t)h, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(hipEventRecord(s->done, ctx->stream));
  PLV_HIP_CHECK(plv::event_sync(s->done));
  ctx->prof.collect();
  return PLV_OK;
}

// ---- layers
bool to_px(float v, int &out) {  // rne of the float32 value; false: the primitive is dropped
  if (!std::isfinite(v) || std::fabs(v) > FLOAT_COORD_MAX) return false;
  out = (int)std::nearbyintf(v);  // (the default rounding mode: to nearest, ties to even)
  return true;
}
bool to_px_trunc(float v, int &out) {  // TrackLSD.cpp:865-866: (int)(v + 0.5), the sum in double
  if (!std::isfinite(v) || std::fabs(v) > FLOAT_COORD_MAX) return false;
  out = (int)((double)v + 0.5);
  return true;
}
uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

struct Rgb {
  uint8_t c[3];
};
void push(std::vector<plv_draw_prim> &out, int kind, int x0, int y0, int x1, int y1, int a, int b, Rgb col) {
  plv_draw_prim p;
  memset(&p, 0, sizeof(p));
  p.kind = kind, p.x0 = x0, p.y0 = y0, p.x1 = x1, p.y1 = y1, p.a = a, p.b = b;
  p.rgb[0] = col.c[0], p.rgb[1] = col.c[1], p.rgb[2] = col.c[2];
  out.push_back(p);
}
void push_disc(std::vector<plv_draw_prim> &out, float x, float y, int r, Rgb col) {
  int px, py;
  if (to_px(x, px) && to_px(y, py)) push(out, PLV_DRAW_RING, px, py, 0, 0, 0, r * r, col);
}
void push_box(std::vector<plv_draw_prim> &out, float x, float y, float d, Rgb col) {
  int xa, ya, xb, yb;
  if (to_px(x - d, xa) && to_px(y - d, ya) && to_px(x + d, xb) && to_px(y + d, yb)) push(out, PLV_DRAW_BOX, xa, ya, xb, yb, 0, 0, col);
}
void push_seg(std::vector<plv_draw_prim> &out, float x0, float y0, float x1, float y1, Rgb col) {
  int xa, ya, xb, yb;
  if (to_px(x0, xa) && to_px(y0, ya) && to_px(x1, xb) && to_px(y1, yb)) push(out, PLV_DRAW_SEG, xa, ya, xb, yb, 1, 0, col);
}

int check_options(const plv_track_image_options *opt) {
  if (!opt || (opt->layers & ~(PLV_VIZ_HISTORY | PLV_VIZ_ACTIVE | PLV_VIZ_LINES | PLV_VIZ_MASK)) || opt->n_highlighted < 0 || opt->n_flagged < 0 ||
      (opt->n_highlighted > 0 && !opt->highlighted) || (opt->n_flagged > 0 && !opt->flagged)) {
    set_last_error("track image: no options, an unknown layer bit, or a list without its ids");
    return PLV_E_BADARG;
  }
  return PLV_OK;
}

int build_list(plv_ctx *ctx, const plv_track_image_options *opt, std::vector<plv_draw_prim> &out) {
  const int W = ctx->cfg.width, H = ctx->cfg.height;
  const bool small = std::min(W, H) < 400;  // TrackBase.cpp:127
  const int rad = small ? 1 : 2;
  int np = 0;
  TRY(plv_tracker_last(ctx, nullptr, nullptr, INT_MAX, &np));
  std::vector<float> pts(2 * (size_t)std::max(np, 1));
  std::vector<uint64_t> ids((size_t)std::max(np, 1));
  TRY(plv_tracker_last(ctx, pts.data(), ids.data(), np, &np));

  if (opt->layers & PLV_VIZ_HISTORY) {
    const std::unordered_set<uint64_t> high(opt->highlighted, opt->highlighted + opt->n_highlighted);
    const std::unordered_set<uint64_t> flagged(opt->flagged, opt->flagged + opt->n_flagged);
    std::vector<int> ptr((size_t)np + 1, 0);
    TRY(plv_db_export_tracks(ctx, ids.data(), np, ptr.data(), nullptr, nullptr, nullptr, INT_MAX));  // the lengths
    std::vector<float> uv(2 * (size_t)std::max(ptr[np], 1));
    TRY(plv_db_export_tracks(ctx, ids.data(), np, ptr.data(), nullptr, uv.data(), nullptr, ptr[np]));
    const Rgb green{{0, 255, 0}};
    const int c1[3] = {opt->r1, opt->g1, opt->b1}, c2[3] = {opt->r2, opt->g2, opt->b2};
    const long long max_tracks = opt->max_tracks;
    for (int i = 0; i < np; ++i) {
      const float x = pts[2 * i], y = pts[2 * i + 1];
      if (high.count(ids[i])) {  // :161-167
        push_box(out, x, y, small ? 3.f : 5.f, green);
        push_disc(out, x, y, rad, green);
      }
      const int n = ptr[i + 1] - ptr[i];
      if (n <= 0) continue;  // :170-173
      const float *tuv = uv.data() + 2 * (size_t)ptr[i];
      const bool flag = flagged.count(ids[i]) != 0;
      for (int z = n - 1; z > 0; --z) {
        if ((long long)n - z > max_tracks) break;
        Rgb col;
        if (flag) {  // Chi_test == false, :176-192
          col = Rgb{{0, 255, (uint8_t)(255 - (int)(1.0 * 255 / n * z))}};
        } else {  // :199-201
          for (int k = 0; k < 3; ++k) col.c[k] = clamp8(c2[k] - (int)(1.0 * c1[k] / n * z));
        }
        push_disc(out, tuv[2 * z], tuv[2 * z + 1], flag ? 2 : rad, col);
        if (z + 1 < n) push_seg(out, tuv[2 * z], tuv[2 * z + 1], tuv[2 * z + 2], tuv[2 * z + 3], col);
      }
    }
  }
  if (opt->layers & PLV_VIZ_ACTIVE) {  // TrackBase.cpp:90-100
    const Rgb ca{{clamp8(opt->r1), clamp8(opt->g1), clamp8(opt->b1)}}, cb{{clamp8(opt->r2), clamp8(opt->g2), clamp8(opt->b2)}};
    for (int i = 0; i < np; ++i) {
      push_disc(out, pts[2 * i], pts[2 * i + 1], rad, ca);
      push_box(out, pts[2 * i], pts[2 * i + 1], 3.f, cb);
    }
  }
  if (opt->layers & PLV_VIZ_LINES) {  // TrackLSD.cpp:832-887
    int nl = 0, ndb = 0;
    TRY(plv_line_tracker_last(ctx, nullptr, nullptr, INT_MAX, &nl));
    std::vector<float> lines(4 * (size_t)std::max(nl, 1));
    std::vector<uint64_t> lids((size_t)std::max(nl, 1));
    TRY(plv_line_tracker_last(ctx, lines.data(), lids.data(), nl, &nl));
    TRY(plv_line_db_ids(ctx, nullptr, INT_MAX, &ndb));
    std::vector<uint64_t> dbv((size_t)std::max(ndb, 1));
    TRY(plv_line_db_ids(ctx, dbv.data(), ndb, &ndb));
    const std::unordered_set<uint64_t> in_db(dbv.begin(), dbv.begin() + ndb);
    std::vector<int> rel_ptr((size_t)nl + 1, 0);
    int nl2 = 0;
    const int rc = plv_line_tracker_last_points(ctx, rel_ptr.data(), nullptr, nl, 0, &nl2);
    if (rc != PLV_OK && rc != PLV_E_CAPACITY) return rc;
    std::vector<uint64_t> rel_id((size_t)std::max(rel_ptr[nl], 1));
    TRY(plv_line_tracker_last_points(ctx, rel_ptr.data(), rel_id.data(), nl, rel_ptr[nl], &nl2));
    std::unordered_map<uint64_t, int> at;  // point id -> index among the last points
    for (int i = 0; i < np; ++i) at[ids[i]] = i;
    for (int i = 0; i < nl; ++i) {
      if (!in_db.count(lids[i])) continue;
      const Rgb col{{(uint8_t)(((long long)i * 128) % 255), (uint8_t)(((long long)i * 53) % 255), (uint8_t)(((long long)i * 23) % 255)}};
      int xa, ya, xb, yb;
      if (to_px_trunc(lines[4 * i], xa) && to_px_trunc(lines[4 * i + 1], ya) && to_px_trunc(lines[4 * i + 2], xb) && to_px_trunc(lines[4 * i + 3], yb))
        push(out, PLV_DRAW_SEG, xa, ya, xb, yb, 2, 0, col);
      for (int q = rel_ptr[i]; q < rel_ptr[i + 1]; ++q) {
        auto it = at.find(rel_id[q]);
        if (it == at.end()) continue;
        int px, py;
        if (to_px(pts[2 * it->second], px) && to_px(pts[2 * it->second + 1], py)) push(out, PLV_DRAW_RING, px, py, 0, 0, 49, 81, col);
      }
    }
  }
  return PLV_OK;
}

}  // namespace

namespace plv {
void plv_draw_destroy(plv_ctx *ctx) {
  std::lock_guard<std::mutex> lk(g_mtx);
  auto it = g_draw.find(ctx);
  if (it == g_draw.end()) return;
  DrawState *s = it->second;
  s->d_grey.release(), s->d_mask.release(), s->d_prims.release(), s->d_rgb.release(), s->pin.release();
  if (s->done) (void)hipEventDestroy(s->done);
  delete s;
  g_draw.erase(it);
}
}  // namespace plv

extern "C" {

void plv_track_image_options_default(plv_track_image_options *opt) {
  if (!opt) return;
  memset(opt, 0, sizeof(*opt));
  opt->layers = PLV_VIZ_HISTORY;
  opt->r1 = 255, opt->g1 = 255, opt->b1 = 0;  // UpdaterCamera.cpp:495
  opt->r2 = 255, opt->g2 = 255, opt->b2 = 255;
  opt->max_tracks = 50;
}

int plv_draw_primitives(plv_ctx *ctx, const uint8_t *grey, int stride, int w, int h, const plv_draw_prim *prims, int n,
                        const uint8_t *mask, int mask_stride, uint8_t *rgb, int rgb_stride) {
  if (!ctx || !grey || !rgb || w < 1 || h < 1 || n < 0 || (n > 0 && !prims) || stride < w || (long long)rgb_stride < 3LL * w ||
      (mask && mask_stride < w) || 3LL * w * h > INT_MAX) {
    set_last_error("plv_draw_primitives: no context / image / output / list, or a %d x %d image with strides %d, %d (mask), %d (rgb)", w, h, stride,
                   mask_stride, rgb_stride);
    return PLV_E_BADARG;
  }
  TRY(check_prims(prims, n));
  (void)hipSetDevice(ctx->device);
  DrawState *s = ds(ctx);
  TRY(s->pin.reserve(stage_bytes(n)));
  TRY(s->d_grey.reserve((size_t)w * h));
  PLV_HIP_CHECK(hipMemcpy2DAsync(s->d_grey.p, (size_t)w, grey, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
  if (mask) {
    TRY(s->d_mask.reserve((size_t)w * h));
    PLV_HIP_CHECK(hipMemcpy2DAsync(s->d_mask.p, (size_t)w, mask, (size_t)mask_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
  }
  return draw_and_fetch(ctx, s, s->d_grey.as<uint8_t>(), w, mask ? s->d_mask.as<uint8_t>() : nullptr, w, prims, n, w, h, rgb, rgb_stride);
}

int plv_track_image_primitives(plv_ctx *ctx, const plv_track_image_options *opt, plv_draw_prim *prims, int cap, int *n) {
  if (!ctx || !n || cap < 0 || (cap > 0 && !prims)) return PLV_E_BADARG;
  TRY(check_options(opt));
  std::vector<plv_draw_prim> list;
  TRY(build_list(ctx, opt, list));
  *n = (int)list.size();
  if (*n > cap) {
    set_last_error("plv_track_image_primitives: %d primitives, room for %d", *n, cap);
    return PLV_E_BADARG;
  }
  if (*n) memcpy(prims, list.data(), list.size() * sizeof(plv_draw_prim));
  return PLV_OK;
}

int plv_track_image(plv_ctx *ctx, const plv_track_image_options *opt, uint8_t *rgb, int rgb_stride) {
  if (!ctx) return PLV_E_BADARG;
  int w = 0, h = 0;
  TRY(plv_pyramid_download(ctx, PLV_PYR_CUR, 0, &w, &h, nullptr));  // (no image yet: its code)
  const uint8_t *d_grey = plv_front_level0(ctx, PLV_PYR_CUR, &w, &h);
  if (!d_grey || !rgb || (long long)rgb_stride < 3LL * w) {
    set_last_error("plv_track_image: no output, or rows %d bytes apart for a %d x %d image", rgb_stride, w, h);
    return PLV_E_BADARG;
  }
  TRY(check_options(opt));
  (void)hipSetDevice(ctx->device);
  std::vector<plv_draw_prim> list;
  TRY(build_list(ctx, opt, list));
  std::vector<uint8_t> mask;
  if (opt->layers & PLV_VIZ_MASK) plv_tracker_mask_last(ctx, mask);
  const bool masked = mask.size() == (size_t)w * h;
  DrawState *s = ds(ctx);
  const size_t prim_bytes = stage_bytes((int)list.size());
  TRY(s->pin.reserve(prim_bytes + (masked ? mask.size() : 0)));
  if (masked) {
    TRY(s->d_mask.reserve(mask.size()));
    memcpy(s->pin.as<char>() + prim_bytes, mask.data(), mask.size());
    PLV_HIP_CHECK(plv::memcpy_async(s->d_mask.p, s->pin.as<char>() + prim_bytes, mask.size(), hipMemcpyHostToDevice, ctx->stream));
  }
  return draw_and_fetch(ctx, s, d_grey, w, masked ? s->d_mask.as<uint8_t>() : nullptr, w, list.data(), (int)list.size(), w, h, rgb, rgb_stride);
}

}  // extern "C"
