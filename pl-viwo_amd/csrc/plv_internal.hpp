// plv_internal.hpp — the library's cross-file internals: every function one translation unit defines and another calls that
// include/plviwo.h does not declare.  C++ linkage in namespace plv, so that a declaration here that drifts from its definition is a
// compile or link error (C linkage carries no types), and hidden from the shared library's export table (Makefile, plviwo.map).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/plviwo.h"

struct plv_ctx_update_state;  // update_state.hpp
namespace plv {  // update_state.hpp, update_kernels.hpp, gate_stage.hpp, camera_tracks.hpp
struct UpdateRiders; struct CovSave; struct GateStage; struct CpiStage; struct CamFront;  // (front_parts.hpp)
}

// Speculative submission of the point update (round 6): host arrays per candidate + where the flow leaves its results on the device
// (SpecSelectArgs, jacobian_kernels.hpp).  The candidates' observation ranges end with a slot for the frame's own observation when
// li >= 0 (time staged, image point and normalised point written by the device).
struct plv_points_spec {
  int n_flow;
  const int *li;
  const uint8_t *meta, *prevalid;
  const float *d_flow_p1, *d_flow_n1;
  const uint8_t *d_flow_mask;
};

// a PLV_* code other than PLV_OK leaves the calling function as it is
#define TRY(expr)                  \
  do {                             \
    int _rc = (expr);              \
    if (_rc != PLV_OK) return _rc; \
  } while (0)

namespace plv {

// ---- plv_api.hip
// the host waits for everything on the ctx's stream: plv_ctx::cov_host_synced moves up to the stamp of the moment the wait began,
// and the per-kernel timer reads its events
int stream_wait(plv_ctx *ctx);
// the ctx's update-side state (update_state.hpp); null for a ctx plv_ctx_create did not make
plv_ctx_update_state *plv_update_state(plv_ctx *ctx);
// fills *gate so that the projected Jacobian launch ends with the gate of every entry (the one-submission updates; off: the update
// launch runs its own).  rows_hint: most rows any entry of the batch can have (0: unknown, the batch's row capacity counts)
int plv_update_gate_prepare(plv_ctx *ctx, int F, int fdim, int k, int ld, double sigma2, double chi2_mult, double res_norm_gate, int probe,
                            int rows_hint, GateStage *gate);
// plv_msckf_update_resident_launch / _wait with what internal callers hand them (the public functions: empty riders, no save)
int update_resident_launch(plv_ctx *ctx, double sigma2, double chi2_mult, double res_norm_gate, UpdateRiders &riders);
int update_resident_wait(plv_ctx *ctx, uint8_t *accepted, int *n_accepted_rows, double *dx, const CovSave &save);
// the prior factor of the update on the side stream, next to triangulation, Jacobians and gate (phase 0 / 1)
int plv_prior_prefetch(plv_ctx *ctx, int phase, const int *d_cols, int k, int F, int mp_max);

// ---- jacobian_api.hip
// what every stereo call refuses of the pair's camera 1: no side, an unknown model, a state id that collides with camera 0's or the
// time offset's.  Host logic; `what` leads the error text.
int plv_stereo_side_check(const char *what, const plv_state_view *st, const plv_camera_side *right);
// plv_triangulate_stereo / plv_build_jacobians_stereo_resident with the residual poses from a CPI table (cpi; null: as the public
// calls).  The triangulation stages the table and forms the pose of every distinct time on the stream in front of its kernel
// (cpi_pose_kernel); the Jacobian batch that follows is a part of the triangulated pool and reads the same poses: its cpi->pose_of
// points into them, nothing is formed again and no pose reaches the host.
int stereo_triangulate(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *tracks,
                       const plv_tri_options *opt, const CpiStage *cpi, double *p_FinG, uint8_t *ok, double *reproj_err);
int stereo_jacobians_resident(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *tracks, int k,
                              const int *col_to_state, int ld, const CpiStage *cpi);

// ---- init_api.cpp
// the test plv_state_boxplus makes of a variable list, made before anything is enqueued (plv_camera_try_update / plv_camera_frame)
int plv_state_vars_check(int n_var, const plv_state_var *vars, int n_dx);

// ---- frontend_api.hip
// plv_ctx_destroy: the ctx's image front end
void plv_frontend_destroy(plv_ctx *ctx);
// plv_feed_image without the wait at its end (the tracker's path: the feed goes on to enqueue the flow and waits there)
int plv_feed_image_enqueue(plv_ctx *ctx, const uint8_t *img, int stride);
// plv_tracker_feed_encoded's image feed: conversion of the encoded host image into the frame's raw image + the device feed, enqueued
int plv_feed_encoded_enqueue(plv_ctx *ctx, const uint8_t *data, int stride, int encoding);
// The next three answer for whichever tracker owns the context (plv_ctx::tracker_kind): the context's one camera, or camera 0 of
// a stereo pair — the camera the lines are tracked on (REF: TrackLSD.cpp:54-57).
// images fed so far: identifies the frame a cached detection belongs to
int plv_front_fed_count(plv_ctx *ctx);
// the point tracker's current observations and their ids (plv_tracker_last / plv_stereo_last of camera 0)
int plv_front_last_points(plv_ctx *ctx, float *pts, uint64_t *ids, int cap, int *n);
// where the flow launched last leaves its results on the device: positions, normalised coordinates [n][2], inlier mask [n]
int plv_front_match_device(plv_ctx *ctx, const float **d_p1, const float **d_n1, const uint8_t **d_mask, int *n);
// equalised level-0 image of the current (which = 0) or previous (1) frame
const uint8_t *plv_front_level0(plv_ctx *ctx, int which, int *w, int *h);
// plv_ctx_synchronize: waits for a detection started ahead of time on the side stream (the job stays collectable)
int plv_front_quiesce(plv_ctx *ctx);
// starts the next frame's top-up detection ahead of time, on the side stream
int plv_perform_detection_ahead(plv_ctx *ctx, const uint8_t *mask, const float *pts, const uint64_t *ids, int n_in);

// ---- tracker_api.hip
// plv_ctx_destroy: the ctx's point tracker and feature database
void plv_tracker_destroy(plv_ctx *ctx);
// index of a feature in the running point update's pool, or -1
int plv_point_chain_lookup(plv_ctx *ctx, uint64_t id);
// FeatureDatabase::get_feature(id) on point_used (triangulated features only): 1 and p [3] when it holds the point
int plv_point_used_lookup(plv_ctx *ctx, uint64_t id, double *p);
// the anchors of a pool of lines in one pass under one lock (plv_ctx::chain's candidates when chained)
void plv_point_anchor_fill(plv_ctx *ctx, int Lp, const int *pt_ptr, const int *pt_ids, int chained, double *anchor, uint8_t *has);
// point_used->cleanup_measurements(oldest_clone_time)
void plv_point_used_cleanup(plv_ctx *ctx, double t_oldest);
// the database hand-back a point update left behind; runs inside the line update's wait (a void (*)(void *) callback)
void plv_tracker_run_deferred(void *ctx);
// a copy of the mask of the last feed (W x H bytes; empty: that feed had none)
void plv_tracker_mask_last(plv_ctx *ctx, std::vector<uint8_t> &out);

// ---- stereo_api.hip
// plv_ctx_destroy: the ctx's stereo tracker, its pyramids and its database
void plv_stereo_destroy(plv_ctx *ctx);
// camera 0's images of a configured stereo tracker (null: none on this context)
const CamFront *plv_stereo_front0(plv_ctx *ctx);
// plv_ctx::tracker_kind: PLV_OK unless the other tracker has taken an image on this context (then PLV_E_BADARG, with the error text)
enum { PLV_TRACKER_NONE = 0, PLV_TRACKER_MONO = 1, PLV_TRACKER_STEREO = 2 };
int plv_tracker_kind_check(plv_ctx *ctx, int kind, const char *who);

// ---- draw_api.hip
// plv_ctx_destroy: the buffers of the track image
void plv_draw_destroy(plv_ctx *ctx);

// ---- line_api.hip
// plv_ctx_destroy: the ctx's line tracker and its worker
void plv_line_tracker_destroy(plv_ctx *ctx);
// whether the frame's lines are detected ahead of the line tracker's feed
int plv_line_prefetch_enabled(plv_ctx *ctx);
// the tracker feed's hook into the image feed (plv_ctx::edges_hook): the edge kernel between histogram and pyramid
void plv_line_edges_early(plv_ctx *ctx, const uint8_t *d_raw, int W, int H, const unsigned *d_hist);
// plv_line_tracker_feed_async with the frame's tracked points handed in, posted the moment the point list stands
int plv_line_tracker_feed_async_points(plv_ctx *ctx, double timestamp, const double *vps, int np, const float *pts, const uint64_t *pids);
// plv_camera_try_update turns the deferral on around its line update; the tracker feed runs what was left behind
void plv_line_defer_finish(plv_ctx *ctx, int on);
void plv_line_run_deferred(plv_ctx *ctx);
// forms the line pool now if the frame's line feed has finished: 0 while the feed is still on the worker, 1 otherwise (never blocks)
int plv_line_pool_prepare(plv_ctx *ctx, const plv_state_view *st, const plv_update_options *opt);
// a line update follows the feed about to be posted: the worker forms that update's pool at the end of the feed
void plv_line_feed_pool_args(plv_ctx *ctx, const plv_state_view *st, const plv_update_options *opt);
// drops a pool formed ahead of time
void plv_line_pool_discard(plv_ctx *ctx);
// the line database's size once the running feed has finished
int plv_line_db_size_after_feed(plv_ctx *ctx);
// the chained first half of the line update, inside the point update's wait: 1 when the line launch is on the stream behind it
int plv_camera_lines_submit_chained(plv_ctx *ctx, const plv_state_view *st, const plv_update_options *opt, int cap);
// whether a chained first half waits for its second half
int plv_camera_lines_job_pending(plv_ctx *ctx);
// a chained first half whose second half will not run: its launch is waited for and dropped (keep_pool: the pool stays formed)
void plv_camera_lines_job_abort2(plv_ctx *ctx, int keep_pool);
void plv_camera_lines_job_abort(plv_ctx *ctx);

// ---- jacobian_api.hip: the one-call camera updates (tracker_api.hip, line_api.hip)
// The point update = plv_points_update_submit (everything enqueued: upload, [spec_select,] triangulation + Jacobians + null space +
// gate, compression, EKFUpdate) + plv_points_update_collect (host work inside the wait, the wait, results).  With `spec` the batch is
// the speculative one; collect then also returns the device's membership (member [F], may be null) and *spec_over (1: the pool exceeded
// max_sel and every candidate was left empty — nothing was updated, the caller runs the update the long way).
// rows_hint: as plv_update_gate_prepare takes it.  cpi: the batch's residual poses come from the CPI table on the device (null: the tracks'
// own, if any).  wait_poll: host work that becomes possible while the update runs, polled inside the wait until it returns nonzero.
// plv_cpi_poses with the poses left on the device (*d_R [n_q][9], *d_p [n_q][3]: valid until the ctx's next point update or
// triangulation); ok [n_q] comes back
int plv_cpi_poses_resident(plv_ctx *ctx, const plv_state_view *st, const plv_cpi_table *cpi, int n_q, const double *t_q, uint8_t *ok,
                           const double **d_R, const double **d_p);
int plv_points_update_submit(plv_ctx *ctx, const plv_state_view *st, const plv_tracks *all, const plv_tri_options *tri,
                             const uint8_t *flags, int max_sel, int k, const int *col_to_state, int ld, double sigma2,
                             double chi2_mult, double res_norm_gate, const plv_points_spec *spec, int rows_hint, const CpiStage *cpi);
int plv_points_update_collect(plv_ctx *ctx, double *p_out, uint8_t *ok_out, double *err_out, uint8_t *accepted, int *n_rows, double *dx,
                              void (*before_wait)(void *), void *before_wait_arg, int (*wait_poll)(void *), void *wait_poll_arg, uint8_t *member,
                              int *spec_count, int *spec_over);
// a collected speculative batch whose update nobody uses: the covariance as it found it (a chained line launch aborted first)
int plv_points_spec_undo(plv_ctx *ctx);
// the line update in two halves: `submit` enqueues up to the gate, `finish` waits for it, updates and collects
int plv_lines_update_fused_submit(plv_ctx *ctx, const plv_state_view *st, const plv_state_view *st_tri, const plv_line_tracks *all,
                                  const uint8_t *flags, int max_sel, int k, const int *col_to_state, int ld, double sigma2, double chi2_mult,
                                  int rows_hint, const CpiStage *cpi);
int plv_lines_update_fused_finish(plv_ctx *ctx, double sigma2, double chi2_mult, double *lines_out, uint8_t *ok_out, uint8_t *accepted,
                                  int *n_rows, double *dx, void (*before_wait)(void *), void *before_wait_arg);

}  // namespace plv
