// update_tail.hpp — the part of the batch tail (camera_tracks.hpp) that calls the library: the two-step route's build and update of
// the selected tracks, for points (tracker_api.hip) and lines (line_api.hip), and what both updates make of an EKFUpdate that
// returned false.  What differs per kind sits in overloads and BatchKind: the view struct and its field names, the columns / build
// calls and the residual-norm gate.
#pragma once
#include <algorithm>
#include <vector>

#include "camera_tracks.hpp"

namespace plv {

// EKFUpdate returned false (PLV_E_NOT_PSD): nothing changed and dx is zero; the call itself succeeded and says so in *status
inline int ekf_returned_false(int rc, int *status, double *dx, int n) {
  *status = rc == PLV_E_NOT_PSD ? rc : PLV_OK;
  if (rc != PLV_E_NOT_PSD) return rc;
  std::fill(dx, dx + n, 0.0);
  return PLV_OK;
}

// per kind — UpdaterCamera::msckf_update / lines_update: the view of the gathered tracks, its columns + Jacobians, the residual-norm gate
inline void selected_view(const Selection<Track> &S, plv_tracks &v) {
  v.n_feat = (int)S.sel.size(), v.obs_uv = S.g.uv.data();
  v.p_FinG = v.p_FinG_fej = S.feat.data();  // MSCKF features: FEJ value = estimate (REF CamHelper.cpp:556-557)
}
inline void selected_view(const Selection<LineTrack> &S, plv_line_tracks &v) { v.n_lines = (int)S.sel.size(), v.seg_uv = S.g.uv.data(), v.line_FinG = S.feat.data(); }
inline int build_resident(plv_ctx *ctx, const plv_state_view *st, const plv_tracks &v, std::vector<int> &cols, int ld) {
  int k = 0;
  const int rc = plv_jacobian_columns(st, &v, cols.data(), (int)cols.size(), &k);
  return rc != PLV_OK ? rc : plv_build_jacobians_resident(ctx, st, &v, k, cols.data(), ld);
}
inline int build_resident(plv_ctx *ctx, const plv_state_view *st, const plv_line_tracks &v, std::vector<int> &cols, int ld) {
  int k = 0;
  const int rc = plv_line_jacobian_columns(st, &v, cols.data(), (int)cols.size(), &k);
  return rc != PLV_OK ? rc : plv_build_line_jacobians_resident(ctx, st, &v, k, cols.data(), ld);
}
template <class TrackT> struct BatchKind;
template <> struct BatchKind<Track> {
  typedef plv_tracks View;
  static constexpr double kResNormGate = 3.0;
};
template <> struct BatchKind<LineTrack> {
  typedef plv_line_tracks View;
  static constexpr double kResNormGate = 0.0;
};

// the gate's verdicts of the selected tracks (S.acc): read from the fused launch's (acc_all, per pool candidate), or — the two-step
// route — columns, Jacobians and update of the gathered tracks (gather_selected).  A failing update returns the selected tracks.
template <class TrackT>
int update_selected(plv_ctx *ctx, const plv_state_view *st, const plv_update_options *opt, const CpiPoses &cpi, std::vector<PoolCand<TrackT>> &pool,
                    TrackMap<TrackT> &unused, Selection<TrackT> &S, const std::vector<uint8_t> &acc_all, bool fused_ran, std::vector<int> &cols,
                    int n_dx, int *status, int *n_rows, double *dx) {
  S.acc.assign(S.sel.size(), 0);
  if (fused_ran) {
    for (size_t q = 0; q < S.sel.size(); ++q) S.acc[q] = acc_all[S.sel[q]];
    return PLV_OK;
  }
  typename BatchKind<TrackT>::View v{};
  selected_view(S, v);
  v.obs_ptr = S.sptr.data();
  v.obs_time = S.g.t.data();
  if (cpi.on) {
    v.res_R = S.g.R.data();
    v.res_p = S.g.p.data();
    if (cpi.noise) {
      v.res_Q = S.g.Q.data();
      v.res_clone = S.g.C.data();
    }
  }
  int rc = build_resident(ctx, st, v, cols, 2 * opt->max_obs);
  if (rc == PLV_OK) {
    rc = plv_msckf_update_resident(ctx, st->sigma_pix * st->sigma_pix, opt->chi2_mult, BatchKind<TrackT>::kResNormGate, S.acc.data(), n_rows, dx);
    rc = ekf_returned_false(rc, status, dx, n_dx);
  }
  if (rc != PLV_OK)
    for (int f : S.sel) give_back_all(unused, pool[f]);
  return rc;
}

}  // namespace plv
