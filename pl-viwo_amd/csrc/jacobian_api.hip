// jacobian_api.hip — plv_jacobian_columns / plv_build_jacobians[_resident] (include/plviwo.h).
// Host side: integer bookkeeping only (column order, CSR -> per-observation feature index, one
// packed upload); all arithmetic is in jacobian_kernel.  No CPU compute path.
#include <algorithm>
#include <vector>

#include <chrono>
#include "jacobian_kernels.hpp"
#include "line_map_kernels.hpp"
#include "nullspace_core.hpp"
#include "update_kernels.hpp"
#include "update_state.hpp"
#include "camera_tracks.hpp"
#include "stage_block.hpp"

using namespace plv;

namespace {

typedef plv::StageBlock StageBlock;
typedef plv_ctx_update_state::Staging Staging;

// the checks a point and a line batch share; tracks_ok: the caller's test of its own arrays.  `what` leads the error text
template <class Tracks, class Ok> int check_views(const char *what, const plv_state_view *st, const Tracks *tr, Ok tracks_ok) {
  if (!st || !tr || st->n_clones < 1 || !st->clone_time || !st->clone_R || !st->clone_p || !st->clone_R_fej ||
      !st->clone_p_fej || !st->clone_state_id || !tracks_ok(*tr)) {
    set_last_error("%s: null view field", what);
    return PLV_E_BADARG;
  }
  if (st->intr_order != 3) {
    set_last_error("%s: only intr_order = 3 is built (got %d)", what, st->intr_order);
    return PLV_E_BADARG;
  }
  if ((tr->res_R == nullptr) != (tr->res_p == nullptr)) return PLV_E_BADARG;
  return PLV_OK;
}
int check_views(const plv_state_view *st, const plv_tracks *tr) {
  return check_views("jacobians", st, tr, [](const plv_tracks &t) {
    return t.n_feat >= 1 && t.obs_ptr && t.obs_time && t.obs_uv && t.p_FinG && t.p_FinG_fej;
  });
}

// Column order of a batch: every clone an observation interpolates over, in first-seen order.  Points (lines = false) put the
// calibration blocks in front, lines the time offset behind each new window.
int jacobian_columns(const plv_state_view *st, int n, const int *obs_ptr, const double *obs_time, bool lines, int *col_to_state, int cap,
                     int *k_out, const plv_camera_side *right = nullptr) {
  int k = 0;
  auto push = [&](int id, int size) {
    if (id < 0) return true;
    for (int j = 0; j < k; ++j)
      if (col_to_state[j] == id) return true;
    if (k + size > cap) return false;
    for (int d = 0; d < size; ++d) col_to_state[k++] = id + d;
    return true;
  };
  // REF: CamHelper.cpp:74-95 calibration blocks first, then :98-110 interpolation poses in first-seen order
  if (!lines && (!push(st->extrinsic_state_id, 6) || !push(st->intrinsic_state_id, 8) || !push(st->dt_state_id, 1))) return PLV_E_CAPACITY;
  // a stereo pair (plv_stereo_jacobian_columns): camera 1's calibration blocks behind camera 0's and the shared time offset
  if (right && (!push(right->extrinsic_state_id, 6) || !push(right->intrinsic_state_id, 8))) return PLV_E_CAPACITY;
  // (a window start that has been seen adds nothing: 700 observations meet ~14 distinct windows, and the search through the
  // column list per pose was 29 us of the caller's thread in front of the point launch at configs[2])
  std::vector<uint8_t> seen_s0((size_t)std::max(st->n_clones, 1), 0);
  BoundingMemo start_of(*st);
  for (int f = 0; f < n; ++f)
    for (int o = obs_ptr[f]; o < obs_ptr[f + 1]; ++o) {
      const int s0 = start_of(obs_time[o] + st->cam_dt);
      if (s0 < 0 || seen_s0[s0]) continue;
      seen_s0[s0] = 1;
      for (int w = 0; w < 4; ++w)
        if (!push(st->clone_state_id[s0 + w], 6)) return PLV_E_CAPACITY;
      // REF: LineHelper.cpp:757-788 — `order` of get_interpolated_jacobian: four poses, then the time offset
      if (lines && !push(st->dt_state_id, 1)) return PLV_E_CAPACITY;
    }
  *k_out = k;
  return PLV_OK;
}

int max_obs(const int *obs_ptr, int n) {  // (sizes a launch's LDS)
  int m = 1;
  for (int f = 0; f < n; ++f) m = std::max(m, obs_ptr[f + 1] - obs_ptr[f]);
  return m;
}

// The part of a packed block both batches carry: the clones of the state view, the residual poses with their covariances, the
// column map.  The stager of a batch adds its own arrays in between, in the order of the block; pack() fills the pinned block,
// fill() hands the device addresses and the view's scalars to the kernels' parameters.
struct StateStage {
  StageBlock &B;
  const plv_state_view *st;
  int k;
  const int *col_to_state;
  StageBlock::Slot<double> time, R, p, Rf, pf, rR, rp, rQ;
  StageBlock::Slot<int> ccol, cols, rc;
  // residual poses from the CPI table on the device (plv::CpiStage): the table, the batch's distinct observation times and every
  // observation's index into them ride in the block; cpi_pose_kernel writes [n_times][9] + [n_times][3] into the staging's own
  // buffer (a second set on the clone poses of the lines' triangulation state), and the batch reads them through res_pose_of
  const CpiStage *cs = nullptr;
  StageBlock::Slot<double> c_t, c_ct, c_dt, c_R, c_a, c_v, c_tq;
  StageBlock::Slot<int> c_of;
  const double *cpi_R[2] = {nullptr, nullptr}, *cpi_p[2] = {nullptr, nullptr};
  int col_of(int sid) const {
    if (sid < 0) return -1;
    for (int j = 0; j < k; ++j)
      if (col_to_state[j] == sid) return j;
    return -1;
  }
  void add_clones() {
    const size_t N = (size_t)st->n_clones;
    time = B.add(st->clone_time, N), R = B.add<9>(st->clone_R, N), p = B.add<3>(st->clone_p, N);
    Rf = B.add<9>(st->clone_R_fej, N), pf = B.add<3>(st->clone_p_fej, N), ccol = B.room<int>(N);
  }
  void add_res_poses(const double *res_R, const double *res_p, size_t nobs) {
    if (res_R) rR = B.add<9>(res_R, nobs), rp = B.add<3>(res_p, nobs);
  }
  int add_res_noise(const double *res_Q, const int *res_clone, size_t nobs) {
    if (res_Q && !res_clone) return PLV_E_BADARG;
    if (res_Q) rQ = B.add<36>(res_Q, nobs), rc = B.add(res_clone, nobs);
    return PLV_OK;
  }
  int add_cpi(const CpiStage *c, size_t nobs) {
    if (!c->table || c->table->n < 1 || c->n_times < 1 || !c->times || !c->pose_of || (c->Q && !c->clone)) return PLV_E_BADARG;
    const plv_cpi_table &T = *c->table;
    const size_t n = (size_t)T.n, nt = (size_t)c->n_times;
    for (size_t o = 0; o < nobs; ++o)
      if (c->pose_of[o] < 0 || c->pose_of[o] >= c->n_times) return PLV_E_BADARG;
    cs = c;
    c_t = B.add(T.t, n), c_ct = B.add(T.clone_t, n), c_dt = B.add(T.dt, n), c_R = B.add<9>(T.R_I0toIk, n), c_a = B.add<3>(T.alpha, n);
    c_v = B.add<3>(T.v, n), c_tq = B.add(c->times, nt), c_of = B.add(c->pose_of, nobs);
    if (c->Q) rQ = B.add<36>(c->Q, nt), rc = B.add(c->clone, nt);
    return PLV_OK;
  }
  // The poses of c's times stand in the staging's buffer already — formed by launch_cpi for an earlier batch of the same update, of
  // which this one is a part (the stereo update's selection out of its triangulated pool): only the pose index rides in the block.
  int add_cpi_formed(const CpiStage *c, size_t nobs, Staging &sg) {
    if (c->n_times < 1 || !c->pose_of || c->Q || sg.cpi.cap < 2 * 12 * (size_t)c->n_times * sizeof(double)) return PLV_E_BADARG;
    for (size_t o = 0; o < nobs; ++o)
      if (c->pose_of[o] < 0 || c->pose_of[o] >= c->n_times) return PLV_E_BADARG;
    cs = c;
    c_of = B.add(c->pose_of, nobs);
    cpi_R[0] = sg.cpi.as<double>(), cpi_p[0] = cpi_R[0] + 9 * (size_t)c->n_times;  // (launch_cpi's layout)
    return PLV_OK;
  }
  // behind the block's upload on the ctx stream; tri_R / tri_p: the clone poses (device) of a second state to form the poses on as well
  int launch_cpi(plv_ctx *ctx, Staging &sg, const double *tri_R, const double *tri_p) {
    const size_t nt = (size_t)cs->n_times, ok_room = StageBlock::padded(nt);
    TRY(sg.cpi.reserve(2 * 12 * nt * sizeof(double) + 2 * ok_room));
    for (int s = 0; s < (tri_R ? 2 : 1); ++s) {
      CpiParams C{};
      C.n = cs->table->n, C.n_clones = st->n_clones, C.n_q = cs->n_times;
      C.t = B.dev(c_t), C.clone_t = B.dev(c_ct), C.dt = B.dev(c_dt), C.R = B.dev(c_R), C.alpha = B.dev(c_a), C.v = B.dev(c_v);
      C.clone_time = B.dev(time), C.clone_R = s ? tri_R : B.dev(R), C.clone_p = s ? tri_p : B.dev(p);
      std::copy(cs->table->gravity, cs->table->gravity + 3, C.gravity);
      double *dR = sg.cpi.as<double>() + 12 * nt * (size_t)s, *dp = dR + 9 * nt;
      unsigned char *dok = sg.cpi.as<unsigned char>() + 2 * 12 * nt * sizeof(double) + ok_room * (size_t)s;
      TRY(launch_cpi_poses(ctx, C, B.dev(c_tq), dR, dp, dok));
      cpi_R[s] = dR, cpi_p[s] = dp;
    }
    return PLV_OK;
  }
  void add_cols() { cols = B.add(col_to_state, (size_t)k); }
  int pack(Staging &sg) {  // (the caller enqueues the upload)
    if (B.overflowed()) return PLV_E_CAPACITY;
    TRY(sg.h_jin.reserve(B.total()));
    TRY(sg.jin.reserve(B.total()));
    B.copy_all(sg.h_jin.p, sg.jin.p);
    int *ccol_h = B.host(ccol);
    for (int i = 0; i < st->n_clones; ++i) ccol_h[i] = col_of(st->clone_state_id[i]);
    return PLV_OK;
  }
  void fill(JacParams &P, const plv_ctx *ctx, int ld) const {
    P.n_clones = st->n_clones;
    P.clone_time = B.dev(time), P.clone_R = B.dev(R), P.clone_p = B.dev(p);
    P.clone_R_fej = B.dev(Rf), P.clone_p_fej = B.dev(pf), P.clone_col = B.dev(ccol);
    memcpy(P.R_ItoC, st->R_ItoC, sizeof P.R_ItoC);
    memcpy(P.p_IinC, st->p_IinC, sizeof P.p_IinC);
    memcpy(P.K, st->intrinsics, sizeof P.K);
    P.cam_model = ctx->cam_model;
    P.cam_dt = st->cam_dt;
    P.dt_exp = st->dt_exp;
    P.sigma_pix = st->sigma_pix;
    P.intr_ori_cov = st->intr_ori_cov;
    P.intr_pos_cov = st->intr_pos_cov;
    P.use_pol_cov = st->use_pol_cov;
    P.use_imu_cov = st->use_imu_cov && rQ ? 1 : 0;
    P.intr_err_mlt = st->intr_err_mlt;
    P.res_R = B.dev(rR), P.res_p = B.dev(rp), P.res_Q = B.dev(rQ), P.res_clone = B.dev(rc);
    P.res_pose_of = nullptr;
    if (cs) P.res_R = cpi_R[0], P.res_p = cpi_p[0], P.res_pose_of = B.dev(c_of);
    P.feat_rep = st->feat_rep;
    P.col_dt = col_of(st->dt_state_id);
    P.k = k;
    P.ld = ld;
    P.cols_in = B.dev(cols);
    P.cols_out = nullptr;
    P.in_base = B.dev_base();
    P.in_bytes = (int)B.total();
  }
};

// Packs every input array into one pinned block, uploads it with one copy and fills JacParams.
struct StageExtra {  // optional riders of the packed block (one-submission update): normalised coordinates, admissibility flags
  const float *uvn = nullptr;
  const uint8_t *flags = nullptr;
  const float *d_uvn = nullptr;
  const uint8_t *d_flags = nullptr;
  // speculative submission (plv_points_spec): per candidate the flow index, the meta bits and the count of valid older observations
  // (SpecSelectArgs, jacobian_kernels.hpp); out: where they, the ranges' ends the device writes and the staged arrays it patches sit
  const int *spec_li = nullptr;
  const uint8_t *spec_meta = nullptr, *spec_prevalid = nullptr;
  const int *d_spec_li = nullptr;
  const uint8_t *d_spec_meta = nullptr, *d_spec_prevalid = nullptr;
  int *d_obs_end = nullptr;
  float *d_obs_uv = nullptr;
  // a stereo pair (plv_stereo_tracks): the two cameras' table and every observation's camera
  const CamSide *cams = nullptr;
  const uint8_t *obs_cam = nullptr;
  const CamSide *d_cams = nullptr;
  const uint8_t *d_obs_cam = nullptr;
  // residual poses of the batch come from the CPI table on the device (null: the tracks' own res_R / res_p, if any);
  // cpi_formed: they are the ones the previous staging formed (StateStage::add_cpi_formed), nothing is launched
  const CpiStage *cpi = nullptr;
  bool cpi_formed = false;
};
int stage_inputs(plv_ctx *ctx, plv_ctx_update_state *us, const plv_state_view *st, const plv_tracks *tr, int k,
                 const int *col_to_state, int ld, JacParams &P, StageExtra *ex = nullptr) {
  const int F = tr->n_feat, nobs = tr->obs_ptr[F];
  if (nobs < 1) {
    set_last_error("jacobians: no observations");
    return PLV_E_BADARG;
  }
  const bool spec = ex && ex->spec_li;
  StageBlock B;
  StateStage S{B, st, k, col_to_state};
  S.add_clones();
  const auto ptr = B.add(tr->obs_ptr, F + 1), of = B.room<int>(nobs);
  const auto ot = B.add(tr->obs_time, nobs);
  const auto uv = B.add<2>(tr->obs_uv, nobs);
  const auto pg = B.add<3>(tr->p_FinG, F), pgf = B.add<3>(tr->p_FinG_fej, F);
  const CpiStage *cs = tr->res_R || !ex ? nullptr : ex->cpi;
  const bool formed = cs && ex->cpi_formed;
  if (formed) TRY(S.add_cpi_formed(cs, (size_t)nobs, us->staging_of(3)));
  else if (cs) TRY(S.add_cpi(cs, (size_t)nobs));
  else S.add_res_poses(tr->res_R, tr->res_p, nobs);
  S.add_cols();
  StageBlock::Slot<float> xuvn;
  StageBlock::Slot<uint8_t> xfl, sme, spv;
  StageBlock::Slot<int> sli, send;
  if (ex && ex->uvn) xuvn = B.add<2>(ex->uvn, nobs);
  if (ex && ex->flags) xfl = B.add(ex->flags, F);
  if (!cs) TRY(S.add_res_noise(tr->res_Q, tr->res_clone, nobs));
  StageBlock::Slot<CamSide> xcam;
  StageBlock::Slot<uint8_t> xoc;
  if (ex && ex->cams) xcam = B.add(ex->cams, 2), xoc = B.add(ex->obs_cam, nobs);
  if (spec) {
    sli = B.add(ex->spec_li, F), sme = B.add(ex->spec_meta, F), spv = B.add(ex->spec_prevalid, F);
    send = B.add(tr->obs_ptr + 1, F);  // (overwritten by spec_select_kernel)
  }
  Staging &sg = us->staging_of(3);
  TRY(S.pack(sg));
  int *of_h = B.host(of);
  for (int f = 0; f < F; ++f) {
    if (tr->obs_ptr[f + 1] < tr->obs_ptr[f]) return PLV_E_BADARG;
    for (int o = tr->obs_ptr[f]; o < tr->obs_ptr[f + 1]; ++o) of_h[o] = f;
  }
  // (an upload by a kernel of the ctx stream instead of the copy command was measured, alternating frame by frame: no difference)
  if (spec) {
    // the speculative batch is staged while the frame's flow occupies the ctx stream: its upload goes onto a stream of its own at once
    // (a copy command behind the flow would sit between the flow's last kernel and the update's first); the ctx stream waits for it
    if (!us->spec_stream) {
      PLV_HIP_CHECK(hipStreamCreateWithFlags(&us->spec_stream, hipStreamNonBlocking));
      PLV_HIP_CHECK(hipEventCreateWithFlags(&us->spec_ev, hipEventDisableTiming));
    }
    PLV_HIP_CHECK(plv::memcpy_async(sg.jin.p, sg.h_jin.p, B.total(), hipMemcpyHostToDevice, us->spec_stream));
    PLV_HIP_CHECK(hipEventRecord(us->spec_ev, us->spec_stream));
    PLV_HIP_CHECK(hipStreamWaitEvent(ctx->stream, us->spec_ev, 0));
  } else
    PLV_HIP_CHECK(plv::memcpy_async(sg.jin.p, sg.h_jin.p, B.total(), hipMemcpyHostToDevice, ctx->stream));
  if (cs && !formed) TRY(S.launch_cpi(ctx, sg, nullptr, nullptr));
  S.fill(P, ctx, ld);
  P.col_ext = S.col_of(st->extrinsic_state_id);
  P.col_int = S.col_of(st->intrinsic_state_id);
  P.n_feat = F;
  P.n_obs = nobs;
  P.obs_ptr = B.dev(ptr), P.obs_feat = B.dev(of), P.obs_time = B.dev(ot), P.obs_uv = B.dev(uv);
  P.p_FinG = B.dev(pg), P.p_FinG_fej = B.dev(pgf);
  // (what every workgroup touches first thing: the whole block — or, of a speculative batch, whose block holds every candidate's
  //  observations, the state and the ranges in front of them)
  if (spec) P.in_bytes = (int)B.offset(of);
  if (ex) {
    ex->d_uvn = B.dev(xuvn), ex->d_flags = B.dev(xfl);
    ex->d_cams = B.dev(xcam), ex->d_obs_cam = B.dev(xoc);
    if (spec) {
      ex->d_spec_li = B.dev(sli), ex->d_spec_meta = B.dev(sme), ex->d_spec_prevalid = B.dev(spv);
      ex->d_obs_end = const_cast<int *>(B.dev(send)), ex->d_obs_uv = const_cast<float *>(B.dev(uv));
      P.obs_end = ex->d_obs_end;
    }
  }
  return PLV_OK;
}

// the column map as the host staged it: same offset in the pinned block as in the device copy (or the pinned block itself)
const int *host_copy_of(plv_ctx_update_state *us, const int *cols_in, int fdim) {
  Staging &sg = us->staging_of(fdim);
  const char *c = (const char *)cols_in, *hj = sg.h_jin.as<char>();
  if (c >= hj && c < hj + sg.h_jin.cap) return cols_in;
  return (const int *)(hj + (c - sg.jin.as<char>()));
}

// A batch of n features of measurement size fdim (3 points, 6 lines) is built into us->bHf ([Hf | Hx | res]) and us->brows on the device
int reserve_batch(plv_ctx *ctx, plv_ctx_update_state *us, int n, int fdim, int k, int ld) {
  TRY(us->bHf.reserve_units((size_t)n, (size_t)std::max(ctx->cfg.num_features, 64), (size_t)(fdim + k + 1) * ld * 8));
  TRY(us->brows.reserve((size_t)n * 4));
  return us->bcols_of(fdim).reserve((size_t)k * 4);
}
// Launches the staged batch and books it in us->b*.  project (resident update path): build + null-space projection in one launch,
// launch_projected(gather, gblocks, gate) — `gate` (plv_update_gate_prepare; off: none) rides on it and is booked with the batch when
// the launch took it; the column map is published by its workgroup 0, and when a covariance of matching size is
// resident its gathers ride along; prior_ahead: the prior factor's second phase follows on the side stream.  Else launch_plain().
// ph_launch / ph_prior: labels of the two host phases (null: not timed).
template <class Projected, class Plain>
int launch_batch(plv_ctx *ctx, plv_ctx_update_state *us, JacParams &P, int n, int fdim, int k, const int *col_to_state, int ld, bool project,
                 bool prior_ahead, GateStage gate, const char *ph_launch, const char *ph_prior, Projected launch_projected, Plain launch_plain) {
  P.rows = us->brows.as<int>();
  P.Hf = us->bHf.as<double>();
  P.Hx = P.Hf + (size_t)n * fdim * ld;
  P.res = P.Hx + (size_t)n * k * ld;
  us->b_projected = false;
  us->b_gather_token = 0;
  us->b_gate.on = 0;
  if (project) {
    P.cols_out = us->bcols_of(fdim).as<int>();
    bool can_gather = ctx->cov_n > 0;
    for (int j = 0; j < k && can_gather; ++j) can_gather = col_to_state[j] >= 0 && col_to_state[j] < ctx->cov_n;
    GatherArgs g{};
    int gblocks = 0;
    plv::HostPhase ph_l(ph_launch);
    if (can_gather) {
      const int cn = ctx->cov_n;
      TRY(gather_args(ctx, ctx->d_P.as<double>(), cn, cn, P.cols_in, k, g));
      gblocks = (std::max(k * cn, std::max(k * k, cn)) + 255) / 256;
    }
    TRY(launch_projected(can_gather ? &g : nullptr, gblocks, gate));
    ph_l.stop();
    plv::HostPhase ph_p1(ph_prior);
    if (can_gather && prior_ahead) TRY(plv_prior_prefetch(ctx, 1, host_copy_of(us, P.cols_in, fdim), k, n, ld - fdim));
    ph_p1.stop();
    us->b_projected = true;
    us->b_gather_token = can_gather ? ctx->gather_stamp : 0;
    us->b_gate = gate;
  } else {
    TRY(launch_plain());
  }
  us->bF = n;
  us->bfdim = fdim;
  us->bk = k;
  us->bld = ld;
  us->bmaxrows = ld;
  us->b_on_device_rows = true;
  return PLV_OK;
}
// host out: the un-projected systems of the batch just built
int download_batch(plv_ctx *ctx, plv_ctx_update_state *us, int n, int fdim, int k, int ld, int *rows, double *Hf, double *Hx, double *res) {
  const size_t nHf = (size_t)n * fdim * ld, nHx = (size_t)n * k * ld, nr = (size_t)n * ld;
  const double *d = us->bHf.as<double>();
  PLV_HIP_CHECK(plv::memcpy_async(Hf, d, nHf * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(Hx, d + nHf, nHx * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(res, d + nHf + nHx, nr * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(rows, us->brows.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  return PLV_OK;
}

struct FusedTri {  // triangulate on the device first and let the Jacobian launch take its candidates from the result
  const plv_tri_options *opt;
  const float *uvn;
  const uint8_t *flags;
  int max_sel;
  size_t o_p, o_err, o_ok;  // out: where the results sit in the point staging's tri (p [F][3], err [F], ok [F], contiguous)
  const plv_points_spec *spec = nullptr;  // speculative submission: the candidates' membership is decided on the device (spec_select_kernel)
  size_t o_member = 0, o_words = 0;       // out (spec): member [F] and the words (SpecSelectArgs) behind ok, part of the mirrored result block
  const int *d_words = nullptr;           // out (spec): the words on the device
  GateStage gate{};                       // the gate the Jacobian launch is to end with (plv_update_gate_prepare)
  const CpiStage *cpi = nullptr;          // StageExtra::cpi
};
int build_on_device(plv_ctx *ctx, plv_ctx_update_state *us, const plv_state_view *st, const plv_tracks *tr, int k,
                    const int *col_to_state, int ld, bool project, FusedTri *ft = nullptr) {
  TRY(check_views(st, tr));
  if (k < 1 || ld < 2 || !col_to_state) return PLV_E_BADARG;
  const int F = tr->n_feat;
  TRY(reserve_batch(ctx, us, F, 3, k, ld));
  const bool prior_ahead = project && ctx->cov_n > 0;
  {
    plv::HostPhase ph("build: prior prefetch, phase 0");
    if (prior_ahead) TRY(plv_prior_prefetch(ctx, 0, nullptr, k, F, ld - 3));  // (before the upload goes onto the stream)
  }
  plv::HostPhase ph_stage("build: inputs staged + upload enqueued");
  JacParams P{};
  bool fuse_tri = false;
  double *tri_poses = nullptr, *tri_p = nullptr, *tri_err = nullptr;
  unsigned char *tri_valid = nullptr, *tri_ok = nullptr;
  const float *tri_uvn = nullptr;
  const plv_tri_options *tri_opt = nullptr;
  const int tri_max_obs = max_obs(tr->obs_ptr, F);
  if (ft) {
    StageExtra ex;
    ex.uvn = ft->uvn;
    ex.flags = ft->flags;
    ex.cpi = ft->cpi;
    if (ft->spec) ex.spec_li = ft->spec->li, ex.spec_meta = ft->spec->meta, ex.spec_prevalid = ft->spec->prevalid;
    TRY(stage_inputs(ctx, us, st, tr, k, col_to_state, ld, P, &ex));
    const int nobs = tr->obs_ptr[F];
    const size_t o_pose = 0, o_valid = (size_t)nobs * 96, o_p = (o_valid + nobs + 15) & ~(size_t)15, o_err = o_p + (size_t)F * 24,
                 o_ok = o_err + (size_t)F * 8, o_member = o_ok + F, o_words = (o_member + F + 7) & ~(size_t)7, o_order = o_words + 32,
                 total = o_order + 4 * (size_t)spec_grid(ft->max_sel) + 16;
    plv::DevBuf &tri = us->staging_of(3).tri;
    TRY(tri.reserve(total));
    char *d = tri.as<char>();
    ft->o_member = o_member, ft->o_words = o_words;
    // one launch for triangulation + Jacobians + null space while the selection has no cap to enforce (see the kernel); a speculative
    // batch holds more candidates than the cap, but its pool does not (spec_select_kernel empties every candidate otherwise)
    fuse_tri = project && (F <= ft->max_sel || ft->spec);
    if (ft->spec) {
      if (!fuse_tri) {
        set_last_error("speculative point submission needs the fused triangulation launch");
        return PLV_E_BADARG;
      }
      SpecSelectArgs A{};
      A.F = F, A.n_flow = ft->spec->n_flow, A.W = ctx->cfg.width, A.H = ctx->cfg.height, A.max_sel = ft->max_sel, A.grid = spec_grid(ft->max_sel);
      A.obs_ptr = P.obs_ptr, A.li = ex.d_spec_li, A.meta = ex.d_spec_meta, A.prevalid = ex.d_spec_prevalid;
      A.flow_p1 = ft->spec->d_flow_p1, A.flow_n1 = ft->spec->d_flow_n1, A.flow_mask = ft->spec->d_flow_mask;
      A.obs_uv = ex.d_obs_uv, A.obs_uvn = const_cast<float *>(ex.d_uvn), A.obs_end = ex.d_obs_end;
      A.sel_flags = const_cast<unsigned char *>(ex.d_flags), A.member = (unsigned char *)(d + o_member), A.words = (int *)(d + o_words);
      if (!ft->gate.on) {
        set_last_error("speculative point submission needs the gate inside the Jacobian launch");
        return PLV_E_BADARG;
      }
      A.order = (int *)(d + o_order), A.rows_out = us->brows.as<int>();
      A.tri_p = (double *)(d + o_p), A.tri_err = (double *)(d + o_err), A.tri_ok = (unsigned char *)(d + o_ok);
      A.chi2 = ft->gate.chi2, A.accepted = ft->gate.accepted, A.acc_rows = ft->gate.acc_rows;
      A.zero_word = ft->gate.n_acc_next, A.cols_out = us->bcols.as<int>(), A.cols_in = P.cols_in, A.k = k;
      TRY(launch_spec_select(ctx, A));
      P.spec_order = A.order, P.spec_count = A.words + 2, P.spec_pass = A.words + 4;
      ft->d_words = A.words;
    }
    tri_poses = (double *)(d + o_pose), tri_valid = (unsigned char *)(d + o_valid), tri_uvn = ex.d_uvn;
    tri_p = (double *)(d + o_p), tri_ok = (unsigned char *)(d + o_ok), tri_err = (double *)(d + o_err);
    tri_opt = ft->opt;
    if (ctx->decision_trace) {
      TRY(ctx->d_tri_dbg.reserve((size_t)F * 32));
      P.tri_dbg = ctx->d_tri_dbg.as<double>();
      ctx->dec_F = F;
    }
    if (!fuse_tri) TRY(launch_triangulate(ctx, P, tri_poses, tri_valid, tri_uvn, *ft->opt, tri_p, tri_ok, tri_err, tri_max_obs));
    P.p_FinG = P.p_FinG_fej = (const double *)(d + o_p);  // MSCKF features: FEJ value = estimate (REF CamHelper.cpp:556-557)
    P.sel_flags = ex.d_flags;
    P.tri_ok = (const unsigned char *)(d + o_ok);
    P.tri_err = (const double *)(d + o_err);
    P.max_sel = ft->max_sel;
    ft->o_p = o_p, ft->o_err = o_err, ft->o_ok = o_ok;
  } else {
    TRY(stage_inputs(ctx, us, st, tr, k, col_to_state, ld, P));
  }
  ph_stage.stop();
  return launch_batch(
      ctx, us, P, F, 3, k, col_to_state, ld, project, prior_ahead, ft ? ft->gate : GateStage{}, "build: gather arguments + Jacobian launch",
      "build: prior prefetch, phase 1 (side stream)",
      [&](const GatherArgs *g, int gblocks, GateStage &gt) {
        if (fuse_tri)
          return launch_jacobians_projected(ctx, P, g, gblocks, gt, tri_opt, tri_poses, tri_valid, tri_uvn, tri_p, tri_ok, tri_err, tri_max_obs);
        return launch_jacobians_projected(ctx, P, g, gblocks, gt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tri_max_obs);
      },
      [&] {
        P.cols_out = us->bcols.as<int>();
        return launch_jacobians(ctx, P);
      });
}

}  // namespace

extern "C" {

int plv_jacobian_columns(const plv_state_view *st, const plv_tracks *tr, int *col_to_state, int cap, int *k_out) {
  if (!col_to_state || !k_out) return PLV_E_BADARG;
  TRY(check_views(st, tr));
  return jacobian_columns(st, tr->n_feat, tr->obs_ptr, tr->obs_time, false, col_to_state, cap, k_out);
}
}  // extern "C"
namespace plv {

// One-submission point update (plv_camera_update_points): triangulation of every pool candidate, the selection loop, Jacobians +
// null-space projection, gate, compression and EKFUpdate are enqueued back to back; one upload, one result download, one host
// synchronisation.  `all` carries obs_uvn; flags[f] = the host's part of the selection test.  Returns as plv_msckf_update_resident
// (PLV_E_NOT_PSD: covariance untouched); p / ok / err (per candidate) and accepted (per candidate, 0 for unselected ones) are filled
// in both cases.
typedef plv_ctx_update_state::PointJob PointJob;
static PointJob &point_job(plv_ctx *ctx) { return plv_update_state(ctx)->point_job; }
static hipEvent_t g_ce[3] = {nullptr, nullptr, nullptr};

int plv_points_update_submit(plv_ctx *ctx, const plv_state_view *st, const plv_tracks *all, const plv_tri_options *tri, const uint8_t *flags,
                             int max_sel, int k, const int *col_to_state, int ld, double sigma2, double chi2_mult, double res_norm_gate,
                             const plv_points_spec *spec, int rows_hint, const CpiStage *cpi) {
  if (!ctx || !all || !tri || !flags || !all->obs_uvn) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  auto &sg = us->staging_of(3);
  PointJob &J = point_job(ctx);
  J = PointJob();
  std::vector<double> p_dummy(3 * (size_t)std::max(all->n_feat, 1), 0.0);
  plv_tracks t2 = *all;
  t2.p_FinG = t2.p_FinG_fej = p_dummy.data();  // (outputs of the triangulation: the staged copy is never read)
  FusedTri ft{tri, all->obs_uvn, flags, max_sel, 0, 0, 0};
  ft.spec = spec;
  ft.cpi = cpi;
  // PLV_KNOB_CHAIN_EVENTS (with PLV_KNOB_HOST_TIMING): three timed events on the stream — at entry (the stream is idle: stamped at once),
  // behind the Jacobian launch, behind the update's last kernel — to set the device's view of the chain against the host's phases
  J.chain_events = plv::knob(plv::PLV_KNOB_CHAIN_EVENTS) && plv::host_phases().on;
  J.t_entry = std::chrono::steady_clock::now();
  if (J.chain_events) {
    for (auto &e : g_ce)
      if (!e) (void)hipEventCreate(&e);
    (void)hipEventRecord(g_ce[0], ctx->stream);
  }
  plv::HostPhase ph_a("points fused: stage + triangulate + jacobians enqueued");
  TRY(plv_update_gate_prepare(ctx, all->n_feat, 3, k, ld, sigma2, chi2_mult, res_norm_gate, 0, rows_hint, &ft.gate));
  TRY(build_on_device(ctx, us, st, &t2, k, col_to_state, ld, true, &ft));
  ph_a.stop();
  plv::frame_mark("@ point Jacobian launch enqueued");
  if (J.chain_events) (void)hipEventRecord(g_ce[1], ctx->stream);
  us->b_single_use = true;
  const int F = all->n_feat;
  const size_t mirror_bytes = spec ? (ft.o_words + 20 - ft.o_p) : (size_t)F * 33;
  TRY(sg.h_tri.reserve(mirror_bytes + 16));
  plv::HostPhase ph_b("points fused: gate .. EKF enqueued");
  // the triangulation results reach the host with the update's result block (copied by its last kernel), or by a copy command when
  // the chain ended another way; either lands before the wait below returns
  UpdateRiders riders;
  EkfRiders &ekf = riders.ekf;
  ekf.mirror2_src = sg.tri.as<char>() + ft.o_p, ekf.mirror2_dst = sg.h_tri.p, ekf.mirror2_bytes = mirror_bytes;
  // (for a line launch chained behind this update, plv_camera_try_update: the commit kernel leaves "state changed" in a device word)
  TRY(us->chain_words.reserve(64));
  us->applied_word = us->chain_words.as<int>();
  ekf.applied_word = us->applied_word;
  ekf.cap_words = spec ? ft.d_words + 3 : nullptr, ekf.cap = max_sel;
  us->spec_save_seq = 0;
  if (spec) {  // (the commit saves what it overwrites: plv_points_spec_undo)
    TRY(us->spec_save.reserve((size_t)ctx->cov_n * ctx->cov_n * 8));
    if (++us->spec_save_count == 0) ++us->spec_save_count;  // (0: no batch)
    us->spec_save_seq = us->spec_save_count;
    us->spec_save_n = ctx->cov_n;
    // (its launch's commit, and that of a re-run inside the wait, save the covariance they overwrite)
    J.save = CovSave{us->spec_save.as<double>(), us->chain_words.as<unsigned>() + 1, us->spec_save_seq};
  }
  ekf.save = J.save;
  int rc = update_resident_launch(ctx, sigma2, chi2_mult, res_norm_gate, riders);
  us->applied_armed = rc == PLV_OK && riders.applied_used;
  us->pt_tri_p = (const double *)(sg.tri.as<char>() + ft.o_p), us->pt_tri_ok = (const unsigned char *)(sg.tri.as<char>() + ft.o_ok), us->pt_tri_F = F;
  const bool mirrored = riders.mirror2_taken;
  if (!mirrored)
    PLV_HIP_CHECK(plv::memcpy_async(sg.h_tri.p, sg.tri.as<char>() + ft.o_p, mirror_bytes, hipMemcpyDeviceToHost, ctx->stream));
  ph_b.stop();
  plv::frame_mark("@ point chain enqueued");
  if (J.chain_events) (void)hipEventRecord(g_ce[2], ctx->stream);
  J.pending = true, J.mirrored = mirrored, J.rc = rc, J.F = F, J.spec = spec != nullptr, J.max_sel = max_sel;
  J.o_p = ft.o_p, J.o_member = ft.o_member, J.o_words = ft.o_words;
  return PLV_OK;
}

int plv_points_update_collect(plv_ctx *ctx, double *p_out, uint8_t *ok_out, double *err_out, uint8_t *accepted, int *n_rows, double *dx,
                              void (*before_wait)(void *), void *before_wait_arg, int (*wait_poll)(void *), void *wait_poll_arg, uint8_t *member,
                              int *spec_count, int *spec_over) {
  if (!ctx || !p_out || !ok_out || !err_out || !accepted || !dx) return PLV_E_BADARG;
  auto *us = plv_update_state(ctx);
  PointJob &J = point_job(ctx);
  if (!J.pending) {
    set_last_error("plv_points_update_collect: no point update was submitted");
    return PLV_E_BADARG;
  }
  J.pending = false;
  int rc = J.rc;
  const int F = J.F;
  plv::HostPhase ph_c("points fused: host work inside the wait");
  if (before_wait) before_wait(before_wait_arg);  // host work of the caller that fits into the wait
  // ... and work that becomes possible DURING the wait (the line pool, once the line worker has finished the frame's feed): the
  // caller's poll function is tried until it reports that nothing is left, or the update is done
  if (rc == PLV_OK && wait_poll && us->done_ev) {
    while (hipEventQuery(us->done_ev) == hipErrorNotReady || plv::knob(plv::PLV_KNOB_CHAIN_ALWAYS)) {
      if (wait_poll(wait_poll_arg)) break;
      for (int i = 0; i < 32; ++i) __builtin_ia32_pause();
    }
  }
  ph_c.stop();
  plv::frame_mark("@ host work inside the point wait done");
  plv::NsScope ns_pw(plv::counters().points_wait_ns);
  plv::HostPhase ph_d("points fused: wait");
  if (rc == PLV_OK) rc = update_resident_wait(ctx, accepted, n_rows, dx, J.save);  // (ends at the update's last kernel)
  if (rc != PLV_OK || !J.mirrored) PLV_HIP_CHECK(plv::stream_sync(ctx->stream));    // (the copy command enqueued behind it)
  ph_d.stop();
  plv::frame_mark("@ point update collected");
  if (J.chain_events) {
    const double host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - J.t_entry).count();
    (void)hipEventSynchronize(g_ce[2]);
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, g_ce[0], g_ce[1]) == hipSuccess && hipEventElapsedTime(&b, g_ce[1], g_ce[2]) == hipSuccess) {
      plv::host_phases().add("points fused: DEVICE entry -> Jacobian launch done", a * 1e3);
      plv::host_phases().add("points fused: DEVICE Jacobian done -> last kernel done", b * 1e3);
      plv::host_phases().add("points fused: HOST entry -> results read", host_us);
    }
  }
  const char *h = us->staging_of(3).h_tri.as<char>();
  memcpy(p_out, h, (size_t)F * 24);
  memcpy(err_out, h + (size_t)F * 24, (size_t)F * 8);
  memcpy(ok_out, h + (size_t)F * 32, (size_t)F);
  if (J.spec) {
    if (member) memcpy(member, h + (J.o_member - J.o_p), (size_t)F);
    const int *w = (const int *)(h + (J.o_words - J.o_p));
    if (spec_count) *spec_count = w[0];
    if (spec_over) *spec_over = w[1] ? 1 : ((w[3] && w[4] >= J.max_sel) ? 2 : 0);  // (2: worked on, but the selection loop's cap would have cut the pool)
  } else {
    if (spec_count) *spec_count = 0;
    if (spec_over) *spec_over = 0;
  }
  return rc;
}

// (internal, tracker_api.hip) the speculative point batch was collected and nobody will use its update: the covariance as the batch found
// it.  The stream is waited for and a line launch chained behind the batch is aborted first (its commit sits on top of the batch's: the
// saved covariance undoes both).  Nothing is restored when the batch committed nothing (rejected, capped, skipped, ended at the gate).
int plv_points_spec_undo(plv_ctx *ctx) {
  auto *us = plv_update_state(ctx);
  const unsigned seq = us->spec_save_seq;
  us->spec_save_seq = 0;
  if (!seq) return PLV_OK;
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  if (plv_camera_lines_job_pending(ctx)) plv_camera_lines_job_abort(ctx);
  if (us->spec_save_n != ctx->cov_n) {
    set_last_error("plv_points_spec_undo: the covariance changed size under a speculative point update");
    return PLV_E_DEVICE;
  }
  TRY(launch_cov_restore(ctx, ctx->d_P.as<double>(), ctx->cov_n, us->spec_save.as<double>(), us->chain_words.as<unsigned>() + 1, seq));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ++ctx->gather_stamp;
  ctx->cov_host_synced = ctx->gather_stamp;
  return PLV_OK;
}
}  // namespace plv
extern "C" {

int plv_build_jacobians_resident(plv_ctx *ctx, const plv_state_view *st, const plv_tracks *tr, int k,
                                 const int *col_to_state, int ld) {
  if (!ctx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(build_on_device(ctx, us, st, tr, k, col_to_state, ld, true));
  us->b_single_use = true;  // consumed in place by the next plv_msckf_update_resident
  return PLV_OK;            // stream-ordered; no host synchronisation
}

int plv_build_jacobians(plv_ctx *ctx, const plv_state_view *st, const plv_tracks *tr, int k, const int *col_to_state,
                        int ld, int *rows, double *Hf, double *Hx, double *res) {
  if (!ctx || !rows || !Hf || !Hx || !res) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(build_on_device(ctx, us, st, tr, k, col_to_state, ld, false));
  us->b_single_use = false;
  return download_batch(ctx, us, tr->n_feat, 3, k, ld, rows, Hf, Hx, res);
}


int plv_triangulate(plv_ctx *ctx, const plv_state_view *st, const plv_tracks *tr, const plv_tri_options *opt, double *p_FinG,
                    uint8_t *ok, double *reproj_err) {
  if (!ctx || !opt || !p_FinG || !ok) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  // p_FinG of the view is an OUTPUT here: allow it to be missing by pointing the checks at the output
  plv_tracks t2 = *tr;
  if (!t2.p_FinG) t2.p_FinG = p_FinG;
  if (!t2.p_FinG_fej) t2.p_FinG_fej = t2.p_FinG;
  TRY(check_views(st, &t2));
  if (!tr->obs_uvn) {
    set_last_error("plv_triangulate: plv_tracks.obs_uvn is required");
    return PLV_E_BADARG;
  }
  const int F = tr->n_feat, nobs = tr->obs_ptr[F];
  int dummy_cols[1] = {-1};
  JacParams P{};
  TRY(stage_inputs(ctx, us, st, &t2, 0, dummy_cols, 2, P));
  const size_t o_pose = 0, o_valid = (size_t)nobs * 96, o_uvn = (o_valid + nobs + 15) & ~(size_t)15, o_p = o_uvn + (size_t)nobs * 8,
               o_err = o_p + (size_t)F * 24, o_ok = o_err + (size_t)F * 8, total = o_ok + F + 16;
  TRY(us->staging_of(3).tri.reserve(total));
  char *d = us->staging_of(3).tri.as<char>();
  PLV_HIP_CHECK(plv::memcpy_async(d + o_uvn, tr->obs_uvn, (size_t)nobs * 8, hipMemcpyHostToDevice, ctx->stream));
  TRY(launch_triangulate(ctx, P, (double *)(d + o_pose), (unsigned char *)(d + o_valid), (const float *)(d + o_uvn), *opt,
                         (double *)(d + o_p), (unsigned char *)(d + o_ok), (double *)(d + o_err), max_obs(tr->obs_ptr, F)));
  PLV_HIP_CHECK(plv::memcpy_async(p_FinG, d + o_p, (size_t)F * 24, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(ok, d + o_ok, (size_t)F, hipMemcpyDeviceToHost, ctx->stream));
  if (reproj_err) PLV_HIP_CHECK(plv::memcpy_async(reproj_err, d + o_err, (size_t)F * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  return PLV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ stereo pair (plv_stereo_tracks)
namespace {

bool ids_overlap(int a, int na, int b, int nb) { return a >= 0 && b >= 0 && a < b + nb && b < a + na; }

}  // namespace
namespace plv {
int plv_stereo_side_check(const char *what, const plv_state_view *st, const plv_camera_side *right) {
  if (!st || !right) {
    set_last_error("%s: no state view or no plv_camera_side for camera 1", what);
    return PLV_E_BADARG;
  }
  if (right->model != PLV_CAM_RADTAN && right->model != PLV_CAM_EQUIDISTANT) {
    set_last_error("%s: camera model %d of camera 1 unknown", what, right->model);
    return PLV_E_BADARG;
  }
  const int e1 = right->extrinsic_state_id, i1 = right->intrinsic_state_id;
  if (ids_overlap(e1, 6, i1, 8) || ids_overlap(e1, 6, st->extrinsic_state_id, 6) || ids_overlap(e1, 6, st->intrinsic_state_id, 8) ||
      ids_overlap(e1, 6, st->dt_state_id, 1) || ids_overlap(i1, 8, st->extrinsic_state_id, 6) || ids_overlap(i1, 8, st->intrinsic_state_id, 8) ||
      ids_overlap(i1, 8, st->dt_state_id, 1)) {
    set_last_error("%s: a state id of camera 1 (extrinsics %d, intrinsics %d) collides with camera 0's or the time offset's", what, e1, i1);
    return PLV_E_BADARG;
  }
  return PLV_OK;
}
}  // namespace plv
namespace {
// ... and of the tracks, before anything is staged: an observation camera above 1, a camera-0 observation in front of a camera-1 one
int check_stereo(const char *what, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *s) {
  TRY(plv_stereo_side_check(what, st, right));
  if (!s || !s->obs_cam) {
    set_last_error("%s: no tracks or no obs_cam", what);
    return PLV_E_BADARG;
  }
  const plv_tracks &t = s->tracks;
  if (t.n_feat < 1 || !t.obs_ptr) {
    set_last_error("%s: no features", what);
    return PLV_E_BADARG;
  }
  for (int f = 0; f < t.n_feat; ++f) {
    if (t.obs_ptr[f + 1] < t.obs_ptr[f]) return PLV_E_BADARG;
    for (int o = t.obs_ptr[f]; o < t.obs_ptr[f + 1]; ++o) {
      if (s->obs_cam[o] > 1) {
        set_last_error("%s: observation %d is of camera %d, a stereo pair has cameras 0 and 1", what, o, (int)s->obs_cam[o]);
        return PLV_E_BADARG;
      }
      if (o > t.obs_ptr[f] && s->obs_cam[o] > s->obs_cam[o - 1]) {
        set_last_error("%s: feature %d lists a camera-0 observation in front of a camera-1 observation (camera 1 comes first)", what, f);
        return PLV_E_BADARG;
      }
    }
  }
  return PLV_OK;
}

void fill_cam_sides(const plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, int k, const int *col_to_state, CamSide *cams) {
  auto col_of = [&](int sid) {
    for (int j = 0; sid >= 0 && j < k; ++j)
      if (col_to_state[j] == sid) return j;
    return -1;
  };
  memset(cams, 0, 2 * sizeof(CamSide));
  memcpy(cams[0].R_ItoC, st->R_ItoC, sizeof cams[0].R_ItoC), memcpy(cams[1].R_ItoC, right->R_ItoC, sizeof cams[1].R_ItoC);
  memcpy(cams[0].p_IinC, st->p_IinC, sizeof cams[0].p_IinC), memcpy(cams[1].p_IinC, right->p_IinC, sizeof cams[1].p_IinC);
  memcpy(cams[0].K, st->intrinsics, sizeof cams[0].K), memcpy(cams[1].K, right->intrinsics, sizeof cams[1].K);
  cams[0].cam_model = ctx->cam_model, cams[1].cam_model = right->model;
  cams[0].col_ext = col_of(st->extrinsic_state_id), cams[1].col_ext = col_of(right->extrinsic_state_id);
  cams[0].col_int = col_of(st->intrinsic_state_id), cams[1].col_int = col_of(right->intrinsic_state_id);
}

// cpi (optional): the batch's residual poses are the ones the update's triangulation formed from the CPI table (cpi->pose_of: every
// observation's index into them)
int build_stereo_on_device(plv_ctx *ctx, plv_ctx_update_state *us, const plv_state_view *st, const plv_camera_side *right,
                           const plv_stereo_tracks *s, int k, const int *col_to_state, int ld, const CpiStage *cpi = nullptr) {
  TRY(check_stereo("stereo jacobians", st, right, s));
  TRY(check_views(st, &s->tracks));
  if (k < 1 || ld < 2 || !col_to_state) return PLV_E_BADARG;
  const int F = s->tracks.n_feat;
  TRY(reserve_batch(ctx, us, F, 3, k, ld));
  CamSide cams[2];
  fill_cam_sides(ctx, st, right, k, col_to_state, cams);
  StageExtra ex;
  ex.cams = cams, ex.obs_cam = s->obs_cam;
  ex.cpi = cpi, ex.cpi_formed = cpi != nullptr;
  JacParams P{};
  TRY(stage_inputs(ctx, us, st, &s->tracks, k, col_to_state, ld, P, &ex));
  return launch_batch(
      ctx, us, P, F, 3, k, col_to_state, ld, false, false, GateStage{}, nullptr, nullptr,
      [](const GatherArgs *, int, GateStage &) { return (int)PLV_E_BADARG; },
      [&] {
        P.cols_out = us->bcols.as<int>();
        return launch_jacobians_stereo(ctx, P, ex.d_cams, ex.d_obs_cam);
      });
}

}  // namespace

extern "C" {

int plv_stereo_jacobian_columns(const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *s, int *col_to_state, int cap,
                                int *k_out) {
  if (!col_to_state || !k_out) return PLV_E_BADARG;
  TRY(check_stereo("plv_stereo_jacobian_columns", st, right, s));
  plv_tracks t2 = s->tracks;  // (the columns read times only)
  if (!t2.p_FinG) t2.p_FinG = t2.p_FinG_fej = st->clone_p;
  if (!t2.p_FinG_fej) t2.p_FinG_fej = t2.p_FinG;
  TRY(check_views(st, &t2));
  return jacobian_columns(st, t2.n_feat, t2.obs_ptr, t2.obs_time, false, col_to_state, cap, k_out, right);
}

int plv_build_jacobians_stereo_resident(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *s,
                                        int k, const int *col_to_state, int ld) {
  return plv::stereo_jacobians_resident(ctx, st, right, s, k, col_to_state, ld, nullptr);
}

int plv_build_jacobians_stereo(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *s, int k,
                               const int *col_to_state, int ld, int *rows, double *Hf, double *Hx, double *res) {
  if (!ctx || !rows || !Hf || !Hx || !res) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(build_stereo_on_device(ctx, us, st, right, s, k, col_to_state, ld));
  us->b_single_use = false;
  return download_batch(ctx, us, s->tracks.n_feat, 3, k, ld, rows, Hf, Hx, res);
}

int plv_triangulate_stereo(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *s,
                           const plv_tri_options *opt, double *p_FinG, uint8_t *ok, double *reproj_err) {
  return plv::stereo_triangulate(ctx, st, right, s, opt, nullptr, p_FinG, ok, reproj_err);
}

}  // extern "C"
namespace plv {

int stereo_jacobians_resident(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *s, int k,
                              const int *col_to_state, int ld, const CpiStage *cpi) {
  if (!ctx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(build_stereo_on_device(ctx, us, st, right, s, k, col_to_state, ld, cpi));
  us->b_single_use = true;  // consumed in place by the next plv_msckf_update_resident (which projects it first)
  return PLV_OK;            // stream-ordered; no host synchronisation
}

int stereo_triangulate(plv_ctx *ctx, const plv_state_view *st, const plv_camera_side *right, const plv_stereo_tracks *s,
                       const plv_tri_options *opt, const CpiStage *cpi, double *p_FinG, uint8_t *ok, double *reproj_err) {
  if (!ctx || !opt || !p_FinG || !ok) return PLV_E_BADARG;
  TRY(check_stereo("plv_triangulate_stereo", st, right, s));
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  plv_tracks t2 = s->tracks;  // p_FinG of the view is an OUTPUT here, as in plv_triangulate
  if (!t2.p_FinG) t2.p_FinG = p_FinG;
  if (!t2.p_FinG_fej) t2.p_FinG_fej = t2.p_FinG;
  TRY(check_views(st, &t2));
  if (!t2.obs_uvn) {
    set_last_error("plv_triangulate_stereo: plv_tracks.obs_uvn is required");
    return PLV_E_BADARG;
  }
  const int F = t2.n_feat, nobs = t2.obs_ptr[F];
  // The kernel anchors on a feature's last observation with bounding clones.  The reference's anchor is the last observation of the
  // camera with strictly more of them, camera 1 on a tie (FeatureInitializer.cpp:36-46): where that is camera 1, the feature's two
  // blocks change places in the staged copy — camera 0's observations, then camera 1's.  The sums over the observations then run in
  // that order: a difference by rounding.
  std::vector<int> src((size_t)nobs);
  BoundingMemo start_of(*st);
  for (int f = 0; f < F; ++f) {
    const int a = t2.obs_ptr[f], b = t2.obs_ptr[f + 1];
    int m = a, n_valid[2] = {0, 0};
    while (m < b && s->obs_cam[m] == 1) ++m;  // [a, m) camera 1, [m, b) camera 0
    for (int o = a; o < b; ++o) n_valid[s->obs_cam[o]] += start_of(t2.obs_time[o] + st->cam_dt) >= 0;
    const bool anchor_right = n_valid[1] >= n_valid[0];
    int at = a;
    if (anchor_right) {
      for (int o = m; o < b; ++o) src[at++] = o;
      for (int o = a; o < m; ++o) src[at++] = o;
    } else {
      for (int o = a; o < b; ++o) src[at++] = o;
    }
  }
  std::vector<double> ot((size_t)nobs), rR, rp;
  std::vector<float> uv(2 * (size_t)nobs), uvn(2 * (size_t)nobs);
  std::vector<uint8_t> oc((size_t)nobs);
  std::vector<int> pose_of(cpi ? (size_t)nobs : 0);  // (the CPI poses' indices move with their observations)
  if (t2.res_R) rR.resize(9 * (size_t)nobs), rp.resize(3 * (size_t)nobs);
  for (int o = 0; o < nobs; ++o) {
    const int q = src[o];
    ot[o] = t2.obs_time[q], oc[o] = s->obs_cam[q];
    if (cpi) pose_of[o] = cpi->pose_of[q];
    std::copy(t2.obs_uv + 2 * (size_t)q, t2.obs_uv + 2 * (size_t)q + 2, &uv[2 * (size_t)o]);
    std::copy(t2.obs_uvn + 2 * (size_t)q, t2.obs_uvn + 2 * (size_t)q + 2, &uvn[2 * (size_t)o]);
    if (t2.res_R) {
      std::copy(t2.res_R + 9 * (size_t)q, t2.res_R + 9 * (size_t)q + 9, &rR[9 * (size_t)o]);
      std::copy(t2.res_p + 3 * (size_t)q, t2.res_p + 3 * (size_t)q + 3, &rp[3 * (size_t)o]);
    }
  }
  t2.obs_time = ot.data(), t2.obs_uv = uv.data(), t2.obs_uvn = uvn.data();
  if (t2.res_R) t2.res_R = rR.data(), t2.res_p = rp.data();
  t2.res_Q = nullptr, t2.res_clone = nullptr;  // (the triangulation reads no noise)
  CamSide cams[2];
  int dummy_cols[1] = {-1};
  fill_cam_sides(ctx, st, right, 0, dummy_cols, cams);
  StageExtra ex;
  ex.cams = cams, ex.obs_cam = oc.data(), ex.uvn = uvn.data();
  CpiStage moved{};
  if (cpi) moved = *cpi, moved.pose_of = pose_of.data(), ex.cpi = &moved;
  JacParams P{};
  TRY(stage_inputs(ctx, us, st, &t2, 0, dummy_cols, 2, P, &ex));
  const size_t o_pose = 0, o_valid = (size_t)nobs * 96, o_p = (o_valid + nobs + 15) & ~(size_t)15, o_err = o_p + (size_t)F * 24,
               o_ok = o_err + (size_t)F * 8, total = o_ok + F + 16;
  TRY(us->staging_of(3).tri.reserve(total));
  char *d = us->staging_of(3).tri.as<char>();
  TRY(launch_triangulate_stereo(ctx, P, ex.d_cams, ex.d_obs_cam, (double *)(d + o_pose), (unsigned char *)(d + o_valid), ex.d_uvn, *opt,
                                (double *)(d + o_p), (unsigned char *)(d + o_ok), (double *)(d + o_err), max_obs(t2.obs_ptr, F)));
  PLV_HIP_CHECK(plv::memcpy_async(p_FinG, d + o_p, (size_t)F * 24, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(ok, d + o_ok, (size_t)F, hipMemcpyDeviceToHost, ctx->stream));
  if (reproj_err) PLV_HIP_CHECK(plv::memcpy_async(reproj_err, d + o_err, (size_t)F * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  return PLV_OK;
}

}  // namespace plv

namespace {

// ------------------------------------------------------------------------------------------ lines
int check_line_views(const plv_state_view *st, const plv_line_tracks *lt, bool need_lines, bool need_uvn) {
  TRY(check_views("line jacobians", st, lt, [=](const plv_line_tracks &t) {
    return t.n_lines >= 1 && t.obs_ptr && t.obs_time && t.seg_uv && !(need_lines && !t.line_FinG) && !(need_uvn && !t.seg_uvn);
  }));
  if (lt->has_pt && !lt->anchor_pt) return PLV_E_BADARG;
  return PLV_OK;
}

// one packed upload of the state view and the line tracks; fills JacParams (n_feat = n_lines)
// st_tri (optional): a second state whose clone poses ride in the same block; *Pt then is P with the poses, extrinsics and time
// offset of that state (the view the line triangulation works on when it differs from the one the Jacobians are taken at)
int stage_line_inputs(plv_ctx *ctx, plv_ctx_update_state *us, const plv_state_view *st, const plv_line_tracks *lt, int k,
                      const int *col_to_state, int ld, JacParams &P, StageExtra *ex = nullptr, const plv_state_view *st_tri = nullptr,
                      JacParams *Pt = nullptr) {
  const int N = st->n_clones, L = lt->n_lines, nobs = lt->obs_ptr[L];
  if (nobs < 1) {
    set_last_error("line jacobians: no observations");
    return PLV_E_BADARG;
  }
  for (int l = 0; l < L; ++l)
    if (lt->obs_ptr[l + 1] < lt->obs_ptr[l]) return PLV_E_BADARG;
  StageBlock B;
  StateStage S{B, st, k, col_to_state};
  S.add_clones();
  const auto ptr = B.add(lt->obs_ptr, L + 1);
  const auto ot = B.add(lt->obs_time, nobs);
  const auto uv = B.add<4>(lt->seg_uv, nobs);
  StageBlock::Slot<float> uvn;
  StageBlock::Slot<double> lg, ap, tR, tp, cq, aold;
  StageBlock::Slot<int> D, cid, aptr, af;
  StageBlock::Slot<uint8_t> hp, xfl, aho;
  if (lt->seg_uvn) uvn = B.add<4>(lt->seg_uvn, nobs);
  if (lt->line_FinG) lg = B.add<6>(lt->line_FinG, L);
  if (lt->D) D = B.add(lt->D, L);
  if (lt->has_pt) ap = B.add<3>(lt->anchor_pt, L), hp = B.add(lt->has_pt, L);
  const CpiStage *cs = lt->res_R || !ex ? nullptr : ex->cpi;
  if (cs) TRY(S.add_cpi(cs, (size_t)nobs));
  else {
    S.add_res_poses(lt->res_R, lt->res_p, nobs);
    TRY(S.add_res_noise(lt->res_Q, lt->res_clone, nobs));
  }
  S.add_cols();
  if (ex && ex->flags) xfl = B.add(ex->flags, L);
  const bool two_states = st_tri && Pt && st_tri != st && st_tri->n_clones == N;
  if (two_states) tR = B.add<9>(st_tri->clone_R, N), tp = B.add<3>(st_tri->clone_p, N);
  // chained launch (plv_ctx::chain): quaternions + covariance indices for the kernel's own x (+) dx, anchor candidates
  const plv_ctx::ChainState &ch = ctx->chain;
  const bool chained = ch.on && ch.ready && !two_states && (int)ch.q.size() == 4 * N && (int)ch.ids.size() == N + 3 && (int)ch.anc_ptr.size() == L + 1;
  if (ch.on && !chained) {
    set_last_error("line jacobians: chained launch asked for without its state");
    return PLV_E_BADARG;
  }
  if (chained) {
    const size_t n_anc = ch.anc_f.size();  // (possibly none: a spare value keeps the three arrays apart)
    cq = B.add<4>(ch.q.data(), N), cid = B.add(ch.ids.data(), N + 3), aptr = B.add(ch.anc_ptr.data(), L + 1);
    af = B.add(ch.anc_f.data(), n_anc, 1), aho = B.add(ch.anc_has_old.data(), n_anc, 4), aold = B.add<3>(ch.anc_old.data(), n_anc, 1);
  }
  Staging &sg = us->staging_of(6);
  TRY(S.pack(sg));
  // (an upload by a kernel of the ctx stream instead of the copy command was measured, alternating frame by frame: no difference)
  PLV_HIP_CHECK(plv::memcpy_async(sg.jin.p, sg.h_jin.p, B.total(), hipMemcpyHostToDevice, ctx->stream));
  // (CPI poses: the triangulation's on the clone poses of its own state, the rows' on st's — both from the one table)
  if (cs) TRY(S.launch_cpi(ctx, sg, two_states ? B.dev(tR) : nullptr, two_states ? B.dev(tp) : nullptr));
  S.fill(P, ctx, ld);
  P.col_ext = P.col_int = -1;
  P.n_feat = L;
  P.n_obs = nobs;
  P.obs_ptr = B.dev(ptr), P.obs_time = B.dev(ot), P.seg_uv = B.dev(uv), P.seg_uvn = B.dev(uvn);
  P.line_FinG = B.dev(lg), P.lineD = B.dev(D), P.anchor_pt = B.dev(ap), P.has_pt = B.dev(hp);
  if (chained) {
    P.chain_dx = us->result.as<double>();  // (dx leads the status block of the update launched last: the point update)
    P.chain_applied = us->applied_word;
    P.chain_status = ResultBlock(ctx->cov_n, 0).status((const void *)us->result.p);
    P.chain_q = B.dev(cq), P.chain_id = B.dev(cid);
    memcpy(P.chain_qe, ch.qe, sizeof P.chain_qe);
    P.anc_ptr = B.dev(aptr), P.anc_f = B.dev(af), P.anc_has_old = B.dev(aho), P.anc_old = B.dev(aold);
    P.anc_tri_p = us->pt_tri_p;
    P.anc_tri_ok = us->pt_tri_ok;
  }
  if (ex) ex->d_flags = B.dev(xfl);
  if (Pt) {
    *Pt = P;
    if (two_states) {
      Pt->clone_R = B.dev(tR), Pt->clone_p = B.dev(tp);
      if (cs) Pt->res_R = S.cpi_R[1], Pt->res_p = S.cpi_p[1];
      memcpy(Pt->R_ItoC, st_tri->R_ItoC, sizeof Pt->R_ItoC);
      memcpy(Pt->p_IinC, st_tri->p_IinC, sizeof Pt->p_IinC);
      Pt->cam_dt = st_tri->cam_dt;
    }
  }
  return PLV_OK;
}

struct FusedLineTri {
  const uint8_t *flags;
  int max_sel;
  size_t o_lines, o_ok;  // out: results in the line staging's tri (lines [L][6], ok [L])
  const plv_state_view *st_tri = nullptr;  // the state of the triangulation when it is not the one of the Jacobians
  GateStage gate{};                        // the gate the Jacobian launch is to end with (plv_update_gate_prepare)
  const CpiStage *cpi = nullptr;           // StageExtra::cpi
};
int build_lines_on_device(plv_ctx *ctx, plv_ctx_update_state *us, const plv_state_view *st, const plv_line_tracks *lt, int k,
                          const int *col_to_state, int ld, bool project, FusedLineTri *ft = nullptr) {
  TRY(check_line_views(st, lt, ft == nullptr, ft != nullptr));
  if (k < 1 || ld < 2 || !col_to_state) return PLV_E_BADARG;
  const int L = lt->n_lines;
  TRY(reserve_batch(ctx, us, L, 6, k, ld));
  // The prior factor of the whitened update, ahead of time on the side stream — not for the one-submission line update (gate probe): it
  // accepts a line or two, fewer rows than columns, and then goes through EKFUpdate on the rows themselves (plv_api.hip, round 6); the
  // four enqueue calls were 8-10 us of the caller's thread in front of the line launch, the factor 50 us of side-stream work per frame
  // that nothing read.  (A probed update that does accept more rows than columns starts the factor when it knows.)
  GateStage gate = ft ? ft->gate : GateStage{};
  const bool prior_ahead = project && ctx->cov_n > 0 && !(gate.on && gate.probe_dst);
  if (prior_ahead) TRY(plv_prior_prefetch(ctx, 0, nullptr, k, L, ld - 6));  // (before the upload goes onto the stream)
  JacParams P{}, Pt{};
  bool fuse_tri = false;
  double *tri_cam = nullptr, *tri_imu = nullptr, *tri_lines = nullptr;
  unsigned char *tri_valid = nullptr, *tri_ok = nullptr;
  StageExtra ex;
  if (ft) ex.flags = ft->flags, ex.cpi = ft->cpi;
  {
    plv::HostPhase ph_stage("build lines: inputs staged + upload enqueued");
    TRY(stage_line_inputs(ctx, us, st, lt, k, col_to_state, ld, P, &ex, ft ? ft->st_tri : nullptr, &Pt));
  }
  plv::HostPhase ph_rest("build lines: gather arguments + launch + prior prefetch");
  if (ft) {
    const int nobs = lt->obs_ptr[L];
    const size_t o_cam = 0, o_imu = (size_t)nobs * 96, o_lines = o_imu + (size_t)nobs * 96, o_ok = o_lines + (size_t)L * 48,
                 o_valid = (o_ok + L + 15) & ~(size_t)15, total = o_valid + nobs + 16;
    plv::DevBuf &tri = us->staging_of(6).tri;
    TRY(tri.reserve(total));
    char *d = tri.as<char>();
    // one launch for triangulation + Jacobians + null space while the selection has no cap to enforce (see the kernel)
    fuse_tri = project && L <= ft->max_sel;
    tri_cam = (double *)(d + o_cam), tri_imu = (double *)(d + o_imu), tri_valid = (unsigned char *)(d + o_valid);
    tri_lines = (double *)(d + o_lines), tri_ok = (unsigned char *)(d + o_ok);
    if (!fuse_tri) TRY(launch_triangulate_lines(ctx, Pt, tri_cam, tri_imu, tri_valid, tri_lines, tri_ok));
    P.line_FinG = (const double *)(d + o_lines);
    P.sel_flags = ex.d_flags;
    P.tri_ok = (const unsigned char *)(d + o_ok);
    P.tri_err = nullptr;
    P.max_sel = ft->max_sel;
    ft->o_lines = o_lines, ft->o_ok = o_ok;
    if (gate.on && gate.probe_dst) {  // the gate inside the launch also carries the triangulated lines to the host
      gate.probe_src = (const unsigned char *)(d + o_lines);
      gate.probe_stride_a = 48, gate.probe_off_b = L * 48, gate.probe_stride_b = 1;
    }
  }
  return launch_batch(
      ctx, us, P, L, 6, k, col_to_state, ld, project, prior_ahead, gate, nullptr, nullptr,
      [&](const GatherArgs *g, int gblocks, GateStage &gt) {
        const int line_max_obs = max_obs(lt->obs_ptr, L);
        if (fuse_tri) return launch_line_jacobians_projected(ctx, P, g, gblocks, gt, &Pt, tri_cam, tri_imu, tri_valid, tri_lines, tri_ok, line_max_obs);
        return launch_line_jacobians_projected(ctx, P, g, gblocks, gt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, line_max_obs);
      },
      [&]() -> int {  // (nothing publishes the column map on this route)
        PLV_HIP_CHECK(plv::memcpy_async(us->bcols_l.p, col_to_state, (size_t)k * 4, hipMemcpyHostToDevice, ctx->stream));
        return launch_line_jacobians(ctx, P);
      });
}

}  // namespace

namespace plv {
// The line twin (plv_camera_update_lines): line triangulation, selection, Pluecker Jacobians, null space, gate, compression, EKF.
// st_tri: the state the lines are triangulated on (the one before the point update, plv_camera_get_line_features); the Jacobians
// are taken at st.
// The line half's one-submission update in two steps: `submit` stages the pool and enqueues triangulation + Jacobians + null space +
// gate (one launch, the gate's verdicts and the triangulated lines go to pinned memory); `finish` waits for the gate, enqueues
// compression + EKFUpdate only when something was accepted, and collects.  plv_camera_try_update calls `submit` while the point
// update of the frame is still running (plv_ctx::chain.on: the launch then forms the corrected state itself, JacParams::chain_dx).
int plv_lines_update_fused_submit(plv_ctx *ctx, const plv_state_view *st, const plv_state_view *st_tri, const plv_line_tracks *all,
                                  const uint8_t *flags, int max_sel, int k, const int *col_to_state, int ld, double sigma2, double chi2_mult,
                                  int rows_hint, const CpiStage *cpi) {
  if (!ctx || !all || !flags) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  auto &sg = us->staging_of(6);
  FusedLineTri ft{flags, max_sel, 0, 0, st_tri};
  ft.cpi = cpi;
  const int L = all->n_lines;
  TRY(sg.h_tri.reserve((size_t)L * 49 + 16));
  TRY(plv_update_gate_prepare(ctx, L, 6, k, ld, sigma2, chi2_mult, 0.0, 1, rows_hint, &ft.gate));
  ft.gate.probe_dst = (unsigned char *)sg.h_tri.p;  // (probe_src and the strides: build_lines_on_device, where the results' place is decided)
  TRY(build_lines_on_device(ctx, us, st, all, k, col_to_state, ld, true, &ft));
  us->b_single_use = true;
  us->lt_o_lines = ft.o_lines, us->lt_L = L;
  return PLV_OK;
}
int plv_lines_update_fused_finish(plv_ctx *ctx, double sigma2, double chi2_mult, double *lines_out, uint8_t *ok_out, uint8_t *accepted, int *n_rows,
                                  double *dx, void (*before_wait)(void *), void *before_wait_arg) {
  if (!ctx || !lines_out || !ok_out || !accepted || !dx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  auto &sg = us->staging_of(6);
  const int L = us->lt_L;
  // the gate's workgroups leave their verdicts and the triangulated lines in pinned memory and the launch function looks at them
  // before it enqueues compression + EKF (UpdateRiders::probe): a line update in which nothing passes the gate ends there
  UpdateRiders riders;
  riders.probe = true;
  riders.probe_src = sg.tri.as<char>() + us->lt_o_lines, riders.probe_dst = sg.h_tri.p;
  riders.probe_stride_a = 48, riders.probe_off_b = L * 48, riders.probe_stride_b = 1;
  riders.probe_hook = before_wait, riders.probe_hook_arg = before_wait_arg;
  int rc = update_resident_launch(ctx, sigma2, chi2_mult, 0.0, riders);
  if (rc == PLV_OK) rc = plv_msckf_update_resident_wait(ctx, accepted, n_rows, dx);
  else PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  const char *h = sg.h_tri.as<char>();
  memcpy(lines_out, h, (size_t)L * 48);
  memcpy(ok_out, h + (size_t)L * 48, (size_t)L);
  return rc;
}
}  // namespace plv

extern "C" {

int plv_line_jacobian_columns(const plv_state_view *st, const plv_line_tracks *lt, int *col_to_state, int cap, int *k_out) {
  if (!col_to_state || !k_out) return PLV_E_BADARG;
  TRY(check_line_views(st, lt, false, false));
  return jacobian_columns(st, lt->n_lines, lt->obs_ptr, lt->obs_time, true, col_to_state, cap, k_out);
}

int plv_build_line_jacobians_resident(plv_ctx *ctx, const plv_state_view *st, const plv_line_tracks *lt, int k,
                                      const int *col_to_state, int ld) {
  if (!ctx) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(build_lines_on_device(ctx, us, st, lt, k, col_to_state, ld, true));
  us->b_single_use = true;
  return PLV_OK;
}

int plv_build_line_jacobians(plv_ctx *ctx, const plv_state_view *st, const plv_line_tracks *lt, int k,
                             const int *col_to_state, int ld, int *rows, double *Hf, double *Hx, double *res) {
  if (!ctx || !rows || !Hf || !Hx || !res) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(build_lines_on_device(ctx, us, st, lt, k, col_to_state, ld, false));
  us->b_single_use = false;
  return download_batch(ctx, us, lt->n_lines, 6, k, ld, rows, Hf, Hx, res);
}

int plv_triangulate_lines(plv_ctx *ctx, const plv_state_view *st, const plv_line_tracks *lt, double *line_FinG,
                          uint8_t *ok) {
  if (!ctx || !line_FinG || !ok) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(check_line_views(st, lt, false, true));
  const int L = lt->n_lines, nobs = lt->obs_ptr[L];
  int dummy_cols[1] = {-1};
  JacParams P{};
  TRY(stage_line_inputs(ctx, us, st, lt, 0, dummy_cols, 2, P));
  const size_t o_cam = 0, o_imu = (size_t)nobs * 96, o_lines = o_imu + (size_t)nobs * 96, o_valid = o_lines + (size_t)L * 48,
               o_ok = o_valid + ((nobs + 15) & ~(size_t)15), total = o_ok + L + 16;
  TRY(us->staging_of(3).tri.reserve(total));
  char *d = us->staging_of(3).tri.as<char>();
  TRY(launch_triangulate_lines(ctx, P, (double *)(d + o_cam), (double *)(d + o_imu), (unsigned char *)(d + o_valid),
                               (double *)(d + o_lines), (unsigned char *)(d + o_ok)));
  PLV_HIP_CHECK(plv::memcpy_async(line_FinG, d + o_lines, (size_t)L * 48, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(ok, d + o_ok, (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  return PLV_OK;
}

// The line map's end points (DESIGN.md "The line map"): the tracks staged as plv_triangulate_lines stages them — the poses of the
// observations are the ones that call forms —, one launch, one copy back.
int plv_line_segments(plv_ctx *ctx, const plv_state_view *st, const plv_line_tracks *lt, double *end_points, double *extent, int *n_views,
                      uint8_t *ok) {
  if (!ctx || !end_points || !ok) return PLV_E_BADARG;
  if (st && lt && lt->n_lines == 0) return PLV_OK;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  TRY(check_line_views(st, lt, true, true));
  const int L = lt->n_lines;
  int dummy_cols[1] = {-1};
  JacParams P{};
  TRY(stage_line_inputs(ctx, us, st, lt, 0, dummy_cols, 2, P));
  const size_t o_seg = 0, o_views = (size_t)L * 64, o_ok = o_views + (size_t)L * 4, total = o_ok + L;
  TRY(us->staging_of(3).tri.reserve(total + 16));
  char *d = us->staging_of(3).tri.as<char>();
  TRY(launch_line_segments(ctx, P, (double *)(d + o_seg), (int *)(d + o_views), (unsigned char *)(d + o_ok)));
  std::vector<char> h(total);
  PLV_HIP_CHECK(plv::memcpy_async(h.data(), d, total, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  const double *seg = (const double *)(h.data() + o_seg);
  for (int l = 0; l < L; ++l) {
    std::copy(seg + 8 * (size_t)l, seg + 8 * (size_t)l + 6, end_points + 6 * (size_t)l);
    if (extent) extent[2 * l] = seg[8 * (size_t)l + 6], extent[2 * l + 1] = seg[8 * (size_t)l + 7];
  }
  if (n_views) memcpy(n_views, h.data() + o_views, (size_t)L * 4);
  memcpy(ok, h.data() + o_ok, (size_t)L);
  return PLV_OK;
}

// The record behind a query time, as cpi_pose_kernel finds it (cpi_servable, camera_tracks.hpp), for its covariance (host arithmetic:
// a search and one blend).
int plv_cpi_noise(const plv_state_view *st, const plv_cpi_table *cpi, int n_q, const double *t_q, double *Q, int *clone_index, uint8_t *ok) {
  if (!st || !cpi || n_q < 0 || (n_q > 0 && (!t_q || !Q || !clone_index || !ok)) || st->n_clones < 1) return PLV_E_BADARG;
  if (cpi->n > 0 && (!cpi->t || !cpi->clone_t || !cpi->Q)) {
    set_last_error("plv_cpi_noise: the table carries no covariances (plv_cpi_table::Q)");
    return PLV_E_BADARG;
  }
  for (int q = 0; q < n_q; ++q) {
    ok[q] = 0;
    clone_index[q] = -1;
    double *Qq = Q + 36 * (size_t)q;
    std::fill(Qq, Qq + 36, 0.0);
    const CpiHit h = cpi_servable(*st, *cpi, t_q[q]);
    if (h.e >= 0) {  // REF State.cpp:275-277
      std::copy(cpi->Q + 36 * (size_t)h.e, cpi->Q + 36 * (size_t)h.e + 36, Qq);
    } else if (h.i0 >= 0) {  // create_new_cpi_linear :286-355
      const double lambda = (t_q[q] - cpi->t[h.i0]) / (cpi->t[h.i1] - cpi->t[h.i0]);
      for (int j = 0; j < 36; ++j) Qq[j] = (1 - lambda) * cpi->Q[36 * (size_t)h.i0 + j] + lambda * cpi->Q[36 * (size_t)h.i1 + j];
    }
    if (!h.ok) continue;
    clone_index[q] = h.clone;
    ok[q] = 1;
  }
  return PLV_OK;
}

}  // extern "C"
// resident (null R_GtoI / p_IinG): the poses stay on the device, *d_R_out / *d_p_out say where (the point staging's triangulation
// block: valid until the next point update or triangulation of the ctx); only ok comes back
static int cpi_poses_impl(plv_ctx *ctx, const plv_state_view *st, const plv_cpi_table *cpi, int n_q, const double *t_q, double *R_GtoI,
                          double *p_IinG, uint8_t *ok, const double **d_R_out, const double **d_p_out) {
  const bool resident = !R_GtoI && !p_IinG && d_R_out && d_p_out;
  if (!ctx || !st || !cpi || n_q < 0 || (n_q > 0 && (!t_q || (!resident && (!R_GtoI || !p_IinG)) || !ok)) || cpi->n < 0 || st->n_clones < 1)
    return PLV_E_BADARG;
  if (cpi->n > 0 && (!cpi->t || !cpi->clone_t || !cpi->dt || !cpi->R_I0toIk || !cpi->alpha || !cpi->v)) return PLV_E_BADARG;
  for (int i = 1; i < cpi->n; ++i)
    if (!(cpi->t[i - 1] < cpi->t[i])) {
      set_last_error("plv_cpi_poses: the table must be strictly ascending in time (record %d)", i);
      return PLV_E_BADARG;
    }
  if (n_q == 0) return PLV_OK;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  const size_t n = (size_t)cpi->n, nc = (size_t)st->n_clones, nq = (size_t)n_q;
  // one packed upload: [t n][clone_t n][dt n][R 9n][alpha 3n][v 3n][clone_time nc][clone_R 9nc][clone_p 3nc][t_q nq]
  const size_t in_d = 18 * n + 13 * nc + nq, out_d = 12 * nq;
  std::vector<double> h(in_d);
  double *w = h.data();
  auto put = [&](const double *src, size_t cnt) {
    if (cnt) std::copy(src, src + cnt, w);
    w += cnt;
  };
  put(cpi->t, n), put(cpi->clone_t, n), put(cpi->dt, n), put(cpi->R_I0toIk, 9 * n), put(cpi->alpha, 3 * n), put(cpi->v, 3 * n);
  put(st->clone_time, nc), put(st->clone_R, 9 * nc), put(st->clone_p, 3 * nc), put(t_q, nq);
  TRY(us->staging_of(3).tri.reserve((in_d + out_d) * sizeof(double) + nq + 16));
  double *d = us->staging_of(3).tri.as<double>();
  PLV_HIP_CHECK(plv::memcpy_async(d, h.data(), in_d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  CpiParams C{};
  C.n = cpi->n, C.n_clones = st->n_clones, C.n_q = n_q;
  C.t = d, C.clone_t = d + n, C.dt = d + 2 * n, C.R = d + 3 * n, C.alpha = d + 12 * n, C.v = d + 15 * n;
  C.clone_time = d + 18 * n, C.clone_R = C.clone_time + nc, C.clone_p = C.clone_R + 9 * nc;
  const double *d_tq = C.clone_p + 3 * nc;
  double *d_R = d + in_d, *d_p = d_R + 9 * nq;
  unsigned char *d_ok = (unsigned char *)(d_p + 3 * nq);
  std::copy(cpi->gravity, cpi->gravity + 3, C.gravity);
  TRY(launch_cpi_poses(ctx, C, d_tq, d_R, d_p, d_ok));
  if (!resident) {
    PLV_HIP_CHECK(plv::memcpy_async(R_GtoI, d_R, 9 * nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PLV_HIP_CHECK(plv::memcpy_async(p_IinG, d_p, 3 * nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  PLV_HIP_CHECK(plv::memcpy_async(ok, d_ok, nq, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  if (resident) {
    *d_R_out = d_R, *d_p_out = d_p;
    return PLV_OK;
  }
  for (size_t q = 0; q < nq; ++q)
    if (!ok[q]) {
      std::fill(R_GtoI + 9 * q, R_GtoI + 9 * q + 9, 0.0);
      std::fill(p_IinG + 3 * q, p_IinG + 3 * q + 3, 0.0);
    }
  return PLV_OK;
}
namespace plv {
int plv_cpi_poses_resident(plv_ctx *ctx, const plv_state_view *st, const plv_cpi_table *cpi, int n_q, const double *t_q, uint8_t *ok,
                           const double **d_R, const double **d_p) {
  if (!d_R || !d_p) return PLV_E_BADARG;
  return cpi_poses_impl(ctx, st, cpi, n_q, t_q, nullptr, nullptr, ok, d_R, d_p);
}
}  // namespace plv

extern "C" {
int plv_cpi_poses(plv_ctx *ctx, const plv_state_view *st, const plv_cpi_table *cpi, int n_q, const double *t_q, double *R_GtoI,
                  double *p_IinG, uint8_t *ok) {
  return cpi_poses_impl(ctx, st, cpi, n_q, t_q, R_GtoI, p_IinG, ok, nullptr, nullptr);
}
}  // extern "C"
