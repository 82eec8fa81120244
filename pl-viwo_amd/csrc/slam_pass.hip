// slam_pass.hip — in-state landmarks a list at a time (include/plviwo.h: plv_camera_update_slam / plv_camera_init_slam, and the
// representation helpers).
//   UpdaterCamera::slam_update / slam_init          REF: PL-VIWO/src/update/cam/UpdaterCamera.cpp:296-369
//   Landmark::get_xyz / set_from_xyz                REF: open_vins/ov_core/src/types/Landmark.cpp:26-44, 65-101
// The reference relinearises after every landmark, so a pass is a chain of small fp64 steps and what it costs is the host's part in
// each of them.  A pass therefore stages once what no landmark changes (clone times and first estimates, every entry's observations,
// poses of the CPI table, column maps) and per landmark only what the previous correction moved (clone poses, the landmark itself);
// landmark_system_kernel writes the rows where the gate and the EKF step read them, the gate's verdict stays on the device (the EKF
// kernels return at once behind a rejection: EkfRiders::skip_word), and one small block — dx, status, verdict — comes back.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "camera_tracks.hpp"
#include "jacobian_kernels.hpp"
#include "plv_internal.hpp"
#include "update_kernels.hpp"
#include "update_state.hpp"

using namespace plv;

namespace {

const int Q95_ENTRIES = 1024;  // plv_ctx_update_state::q95 (plv_ctx_create)
const int GATE_MAX_ROWS = 63;  // chi2_gate_kernel's S tile
const double NO_TIME = -1e300;  // observation time no clone window holds

// cov_init_invertible_kernel reports 1 = rejected; the EKF kernels behind it skip on 0 (EkfRiders::skip_word)
__global__ void init_skip_word_kernel(const int *__restrict__ rejected, int *__restrict__ skip) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *skip = *rejected ? 0 : 1;
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

bool rep_known(int rep) { return rep == PLV_FEAT_GLOBAL_3D || rep == PLV_FEAT_GLOBAL_FULL_INVERSE_DEPTH; }

struct Entry {
  uint64_t id = 0;
  int a = 0, b = 0;    // its observations in the list as it came
  int o0 = 0, o1 = 0;  // those with bounding clones, in the staged arrays
  int m = 0;           // ... of which usable (0: the entry is not worked on)
  int k = 0;
  std::vector<int> cols;  // col_to_state (update: the landmark's three behind)
  size_t off_cols = 0, off_ccol = 0;
  double p[3] = {0, 0, 0};
};

struct Pass {
  plv_ctx *ctx;
  plv_ctx_update_state *us;
  const plv_state_view *st;
  const plv_update_options *opt;
  bool own_list = false;
  int ld = 0, kmax = 0;
  // the list as it came (own list: copies; caller's tracks: copies as well — a few hundred bytes)
  std::vector<uint64_t> ids;
  std::vector<int> ptr;
  std::vector<double> t, pf;
  std::vector<float> uv, uvn;
  // usable observations, compacted
  std::vector<double> ot, rR, rp, rQ;
  std::vector<float> ouv;
  std::vector<int> rc;
  bool have_res = false, have_noise = false;
  const double *d_cpi_R = nullptr, *d_cpi_p = nullptr;  // poses of the CPI table, on the device (plv_cpi_poses_resident)
  std::vector<Entry> ent;
  // device addresses
  size_t o_time = 0, o_Rf = 0, o_pf = 0, o_ot = 0, o_uv = 0, o_rR = 0, o_rp = 0, o_rQ = 0, o_rc = 0;
  double *d_block = nullptr, *d_out = nullptr, *d_dx = nullptr;
  int *d_rows = nullptr, *d_initflag = nullptr, *d_skip = nullptr, *d_flag = nullptr, *d_acc_rows = nullptr;
  unsigned char *d_acc = nullptr;
  size_t res_bytes = 0;

  int col_of(const Entry &e, int sid) const {
    if (sid < 0) return -1;
    for (int j = 0; j < e.k; ++j)
      if (e.cols[j] == sid) return j;
    return -1;
  }

  // ---- the list, the usable observations and the column maps: host only, nothing enqueued
  int read_list(int which, const plv_tracks *tracks, uint64_t *ids_io) {
    if (!tracks) {
      own_list = true;
      int F = 0;
      TRY(plv_camera_update_list(ctx, which, 0, 0, &F, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
      ids.assign((size_t)F, 0), ptr.assign((size_t)F + 1, 0), pf.assign(3 * (size_t)F, 0.0);
      if (F == 0) return PLV_OK;
      // (the size of the observation arrays is not part of the query: ask with room for every track at its longest)
      const int cap = F * std::max(4 * opt->max_obs, 256);
      t.resize((size_t)cap), uv.resize(2 * (size_t)cap), uvn.resize(2 * (size_t)cap);
      TRY(plv_camera_update_list(ctx, which, F, cap, &F, ids.data(), ptr.data(), t.data(), uv.data(), uvn.data(), pf.data()));
      std::copy(ids.begin(), ids.end(), ids_io);
      return PLV_OK;
    }
    const int F = tracks->n_feat;
    if (F < 0 || (F > 0 && (!tracks->obs_ptr || !tracks->obs_time || !tracks->obs_uv))) return PLV_E_BADARG;
    if ((tracks->res_R == nullptr) != (tracks->res_p == nullptr)) return PLV_E_BADARG;
    if (which == PLV_LIST_INIT && F > 0 && !tracks->p_FinG) return PLV_E_BADARG;
    ids.assign(ids_io, ids_io + F), ptr.assign((size_t)F + 1, 0), pf.assign(3 * (size_t)F, 0.0);
    if (F == 0) return PLV_OK;
    if (tracks->obs_ptr[0] != 0) return PLV_E_BADARG;
    for (int f = 0; f < F; ++f)
      if (tracks->obs_ptr[f + 1] < tracks->obs_ptr[f]) return PLV_E_BADARG;
    ptr.assign(tracks->obs_ptr, tracks->obs_ptr + F + 1);
    const size_t n = (size_t)ptr[F];
    t.assign(tracks->obs_time, tracks->obs_time + n), uv.assign(tracks->obs_uv, tracks->obs_uv + 2 * n);
    if (tracks->obs_uvn) uvn.assign(tracks->obs_uvn, tracks->obs_uvn + 2 * n);
    if (which == PLV_LIST_INIT) pf.assign(tracks->p_FinG, tracks->p_FinG + 3 * (size_t)F);
    if (tracks->res_R) {
      have_res = true;
      rR.assign(tracks->res_R, tracks->res_R + 9 * n), rp.assign(tracks->res_p, tracks->res_p + 3 * n);
      if (tracks->res_Q && tracks->res_clone && st->use_imu_cov) {
        have_noise = true;
        rQ.assign(tracks->res_Q, tracks->res_Q + 36 * n), rc.assign(tracks->res_clone, tracks->res_clone + n);
      }
    }
    return PLV_OK;
  }

  // REF CamHelper.cpp get_imu_poses (:327-372): an observation is used when its time + dt has bounding clones and, with the CPI table,
  // a pose from it (taken here, once, as plv_camera_update_points takes the pool's).  The table's poses stay on the device where
  // plv_cpi_poses left them; an observation it cannot serve keeps its slot with a time no window holds, which the kernel drops.
  int select_observations(int fdim_cols) {
    const int F = (int)ids.size();
    std::vector<double> cR, cp, cQ;
    std::vector<int> cc;
    ent.assign((size_t)F, Entry());
    for (int f = 0; f < F; ++f) {
      Entry &e = ent[f];
      e.id = ids[f], e.a = ptr[f], e.b = ptr[f + 1];
      std::copy(pf.begin() + 3 * f, pf.begin() + 3 * f + 3, e.p);
      e.o0 = (int)ot.size();
      for (int o = e.a; o < e.b; ++o) {
        if (!has_bounding_poses(*st, t[o] + st->cam_dt)) continue;
        ot.push_back(t[o]);
        ouv.insert(ouv.end(), &uv[2 * (size_t)o], &uv[2 * (size_t)o] + 2);
        if (have_res) cR.insert(cR.end(), &rR[9 * (size_t)o], &rR[9 * (size_t)o] + 9), cp.insert(cp.end(), &rp[3 * (size_t)o], &rp[3 * (size_t)o] + 3);
        if (have_noise) cQ.insert(cQ.end(), &rQ[36 * (size_t)o], &rQ[36 * (size_t)o] + 36), cc.push_back(rc[o]);
      }
      e.o1 = (int)ot.size();
      e.m = e.o1 - e.o0;
    }
    rR.swap(cR), rp.swap(cp), rQ.swap(cQ), rc.swap(cc);
    const size_t nobs = ot.size();
    if (opt->cpi && !have_res && nobs > 0) {
      std::vector<double> tq(nobs);
      for (size_t o = 0; o < nobs; ++o) tq[o] = ot[o] + st->cam_dt;
      std::vector<uint8_t> okq(nobs);
      TRY(plv_cpi_poses_resident(ctx, st, opt->cpi, (int)nobs, tq.data(), okq.data(), &d_cpi_R, &d_cpi_p));
      if (st->use_imu_cov && !st->use_pol_cov && opt->cpi->Q) {
        std::vector<uint8_t> okn(nobs);
        rQ.assign(36 * nobs, 0.0), rc.assign(nobs, 0);
        TRY(plv_cpi_noise(st, opt->cpi, (int)nobs, tq.data(), rQ.data(), rc.data(), okn.data()));
        have_noise = true;
        for (size_t o = 0; o < nobs; ++o) okq[o] = okq[o] && okn[o];
      }
      for (Entry &e : ent)
        for (int o = e.o0; o < e.o1; ++o)
          if (!okq[o]) ot[o] = NO_TIME, --e.m;
    }
    const double dummy_p[3] = {0, 0, 0};
    for (Entry &e : ent) {
      if (e.m < 1) continue;
      // the column order of get_feature_jacobian_full (plv_jacobian_columns) over the usable observations
      const int one_ptr[2] = {0, e.o1 - e.o0};
      plv_tracks one{};
      one.n_feat = 1, one.obs_ptr = one_ptr, one.obs_time = ot.data() + e.o0, one.obs_uv = ouv.data() + 2 * (size_t)e.o0;
      one.p_FinG = one.p_FinG_fej = dummy_p;
      e.cols.assign((size_t)15 + 6 * (size_t)st->n_clones + 3, -1);
      TRY(plv_jacobian_columns(st, &one, e.cols.data(), (int)e.cols.size() - 3, &e.k));
      e.cols.resize((size_t)e.k + fdim_cols);
      kmax = std::max(kmax, e.k + fdim_cols);
    }
    return PLV_OK;
  }

  // ---- what no landmark of the pass changes, in one upload; the buffers of the per-landmark steps
  int stage_static(int n_cap) {
    const int N = st->n_clones;
    const size_t nobs = ot.size();
    size_t off = 0;
    auto room = [&off](size_t bytes) {
      const size_t at = off;
      off = align16(off + bytes);
      return at;
    };
    o_time = room((size_t)N * 8), o_Rf = room((size_t)N * 72), o_pf = room((size_t)N * 24);
    o_ot = room(nobs * 8), o_uv = room(nobs * 8);
    if (have_res) o_rR = room(nobs * 72), o_rp = room(nobs * 24);
    if (have_noise) o_rQ = room(nobs * 288), o_rc = room(nobs * 4);
    for (Entry &e : ent) {
      if (e.m < 1) continue;
      e.off_ccol = room((size_t)N * 4), e.off_cols = room(e.cols.size() * 4);
    }
    plv_ctx_update_state::SlamPass &S = us->slam;
    TRY(S.h_stat.reserve(off));
    TRY(S.stat.reserve(off));
    char *h = S.h_stat.as<char>();
    memcpy(h + o_time, st->clone_time, (size_t)N * 8);
    memcpy(h + o_Rf, st->clone_R_fej, (size_t)N * 72);
    memcpy(h + o_pf, st->clone_p_fej, (size_t)N * 24);
    if (nobs) {
      memcpy(h + o_ot, ot.data(), nobs * 8), memcpy(h + o_uv, ouv.data(), nobs * 8);
      if (have_res) memcpy(h + o_rR, rR.data(), nobs * 72), memcpy(h + o_rp, rp.data(), nobs * 24);
      if (have_noise) memcpy(h + o_rQ, rQ.data(), nobs * 288), memcpy(h + o_rc, rc.data(), nobs * 4);
    }
    for (const Entry &e : ent) {
      if (e.m < 1) continue;
      int *ccol = (int *)(h + e.off_ccol);
      for (int i = 0; i < N; ++i) ccol[i] = col_of(e, st->clone_state_id[i]);
      memcpy(h + e.off_cols, e.cols.data(), e.cols.size() * 4);
    }
    PLV_HIP_CHECK(plv::memcpy_async(S.stat.p, S.h_stat.p, off, hipMemcpyHostToDevice, ctx->stream));
    // per landmark: clone poses + the landmark (dyn), its system + the words around it (sys), the result block (res)
    const size_t dyn_bytes = (size_t)N * 96 + 48;
    TRY(S.h_dyn.reserve(dyn_bytes));
    TRY(S.dyn.reserve(dyn_bytes));
    const size_t blk = align16((size_t)(kmax + 4) * ld * 8);
    TRY(S.sys.reserve(blk + 128));
    d_block = S.sys.as<double>();
    char *w = S.sys.as<char>() + blk;
    d_rows = (int *)w, d_initflag = (int *)(w + 16), d_skip = (int *)(w + 32), d_out = (double *)(w + 64);
    // (the shared head of plv::ResultBlock — dx, status words, accepted — and a tail of its own: one verdict padded to 8, its rows)
    const ResultBlock head(n_cap, 0);
    res_bytes = head.head_bytes() + 8 + 8;
    const void *before = S.res.p;
    TRY(S.res.reserve(res_bytes));
    if (S.res.p != before) PLV_HIP_CHECK(hipMemsetAsync(S.res.p, 0, S.res.cap, ctx->stream));
    TRY(S.h_res.reserve(res_bytes + 64));
    char *r = S.res.as<char>();
    d_dx = head.dx(r), d_flag = head.status(r), d_acc = head.accepted(r);
    d_acc_rows = (int *)(r + head.head_bytes() + 8);
    TRY(ctx->d_chi2.reserve(64));
    TRY(ctx->d_stack.reserve((size_t)(kmax + 4) * ld * 8));
    return PLV_OK;
  }

  // the clone poses as the corrections so far left them, and the landmark: one small upload
  int stage_dynamic(const double *xyz, const double *xyz_fej) {
    const int N = st->n_clones;
    plv_ctx_update_state::SlamPass &S = us->slam;
    double *h = S.h_dyn.as<double>();
    memcpy(h, st->clone_R, (size_t)N * 72);
    memcpy(h + 9 * (size_t)N, st->clone_p, (size_t)N * 24);
    memcpy(h + 12 * (size_t)N, xyz, 24);
    memcpy(h + 12 * (size_t)N + 3, xyz_fej, 24);
    PLV_HIP_CHECK(plv::memcpy_async(S.dyn.p, S.h_dyn.p, (size_t)N * 96 + 48, hipMemcpyHostToDevice, ctx->stream));
    return PLV_OK;
  }

  void fill(JacParams &P, const Entry &e, int k, int feat_rep) const {
    const int N = st->n_clones;
    const char *s = us->slam.stat.as<char>();
    const double *d = us->slam.dyn.as<double>();
    P.n_clones = N;
    P.clone_time = (const double *)(s + o_time), P.clone_R_fej = (const double *)(s + o_Rf), P.clone_p_fej = (const double *)(s + o_pf);
    P.clone_R = d, P.clone_p = d + 9 * (size_t)N;
    P.clone_col = (const int *)(s + e.off_ccol);
    memcpy(P.R_ItoC, st->R_ItoC, sizeof P.R_ItoC);
    memcpy(P.p_IinC, st->p_IinC, sizeof P.p_IinC);
    memcpy(P.K, st->intrinsics, sizeof P.K);
    P.cam_model = ctx->cam_model;
    P.cam_dt = st->cam_dt, P.dt_exp = st->dt_exp, P.sigma_pix = st->sigma_pix;
    P.intr_ori_cov = st->intr_ori_cov, P.intr_pos_cov = st->intr_pos_cov, P.use_pol_cov = st->use_pol_cov;
    P.use_imu_cov = st->use_imu_cov && have_noise ? 1 : 0;
    P.intr_err_mlt = st->intr_err_mlt;
    P.feat_rep = feat_rep;
    P.col_ext = col_of(e, st->extrinsic_state_id), P.col_int = col_of(e, st->intrinsic_state_id), P.col_dt = col_of(e, st->dt_state_id);
    P.n_feat = 1, P.n_obs = (int)ot.size();
    P.obs_time = (const double *)(s + o_ot), P.obs_uv = (const float *)(s + o_uv);
    P.p_FinG = d + 12 * (size_t)N, P.p_FinG_fej = d + 12 * (size_t)N + 3;
    if (have_res) P.res_R = (const double *)(s + o_rR), P.res_p = (const double *)(s + o_rp);
    if (d_cpi_R) P.res_R = d_cpi_R, P.res_p = d_cpi_p;
    if (have_noise) P.res_Q = (const double *)(s + o_rQ), P.res_clone = (const int *)(s + o_rc);
    P.k = k, P.ld = ld;
  }

  // StateHelper::EKFUpdate's mean update (:156-168) over the caller's variables and landmarks
  int apply(int n_var, const plv_state_var *vars, int n_lm, plv_landmark *lms, const double *dx, int n) {
    if (n_var > 0) TRY(plv_state_boxplus(n_var, vars, dx, n));
    for (int i = 0; i < n_lm; ++i)
      for (int q = 0; q < 3; ++q) lms[i].value[q] += dx[lms[i].id + q];
    if (st->intrinsic_state_id >= 0) TRY(plv_set_camera_intrinsics(ctx, st->intrinsics));
    return PLV_OK;
  }

  int give_back(const Entry &e) {
    if (!own_list || e.b == e.a || uvn.empty()) return PLV_OK;
    return plv_db_append_measurements(ctx, e.id, e.b - e.a, &t[e.a], &uv[2 * (size_t)e.a], &uvn[2 * (size_t)e.a]);
  }
};

// the checks both passes make before anything is enqueued
int check_common(plv_ctx *ctx, const plv_state_view *st, const plv_update_options *opt, int n_var, const plv_state_var *vars, int n_lm,
                 const plv_landmark *lms, const plv_slam_result *res, const uint64_t *ids, const uint8_t *verdict) {
  if (!ctx || !st || !opt || !res || !ids || !verdict || n_var < 0 || n_lm < 0 || (n_var > 0 && !vars) || (n_lm > 0 && !lms)) {
    set_last_error("landmark pass: null argument");
    return PLV_E_BADARG;
  }
  if (st->n_clones < 1 || !st->clone_time || !st->clone_R || !st->clone_p || !st->clone_R_fej || !st->clone_p_fej || !st->clone_state_id ||
      st->intr_order != 3 || ctx->cov_n < 1 || opt->max_obs < 1) {
    set_last_error("landmark pass: bad state view, options or no resident covariance");
    return PLV_E_BADARG;
  }
  if (2 * opt->max_obs > GATE_MAX_ROWS) {
    set_last_error("landmark pass: max_obs %d exceeds the gate's %d rows", opt->max_obs, GATE_MAX_ROWS);
    return PLV_E_CAPACITY;
  }
  const int n = ctx->cov_n;
  if (plv_state_vars_check(n_var, vars, n) != PLV_OK) return PLV_E_BADARG;
  for (int i = 0; i < n_lm; ++i)
    if (!rep_known(lms[i].rep) || lms[i].id < 0 || lms[i].id + 3 > n) {
      set_last_error("landmark pass: landmark %d has rep %d, id %d (covariance %d)", i, lms[i].rep, lms[i].id, n);
      return PLV_E_BADARG;
    }
  for (int i = 0; i < st->n_clones; ++i)
    if (st->clone_state_id[i] < 0 || st->clone_state_id[i] + 6 > n) return PLV_E_BADARG;
  const int cal[3][2] = {{st->extrinsic_state_id, 6}, {st->intrinsic_state_id, 8}, {st->dt_state_id, 1}};
  for (const auto &c : cal)
    if (c[0] >= 0 && c[0] + c[1] > n) return PLV_E_BADARG;
  return PLV_OK;
}

void count(plv_slam_result *res, const uint8_t *verdict, int n_list, int cov_n) {
  res->n_list = n_list;
  for (int j = 0; j < n_list; ++j) {
    if (verdict[j] == 1) ++res->n_applied;
    else if (verdict[j] == 2) ++res->n_gate;
    else if (verdict[j] == 3) ++res->n_not_psd;
    else ++res->n_skipped;
  }
  res->cov_n = cov_n;
}

}  // namespace

extern "C" {

int plv_landmark_from_xyz(int rep, const double *p, double *out) {
  if (!p || !out || !rep_known(rep)) return PLV_E_BADARG;
  if (rep == PLV_FEAT_GLOBAL_3D) {
    const double v[3] = {p[0], p[1], p[2]};
    std::copy(v, v + 3, out);
    return PLV_OK;
  }
  const double g_rho = 1 / std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);  // REF Landmark.cpp:86-93
  const double g_phi = std::acos(g_rho * p[2]);
  const double g_theta = std::atan2(p[1], p[0]);
  out[0] = g_theta, out[1] = g_phi, out[2] = g_rho;
  return PLV_OK;
}

int plv_landmark_xyz(int rep, const double *v, double *out) {
  if (!v || !out || !rep_known(rep)) return PLV_E_BADARG;
  if (rep == PLV_FEAT_GLOBAL_3D) {
    const double p[3] = {v[0], v[1], v[2]};
    std::copy(p, p + 3, out);
    return PLV_OK;
  }
  const double th = v[0], ph = v[1], ir = 1 / v[2];  // REF Landmark.cpp:39-43
  const double p[3] = {ir * std::cos(th) * std::sin(ph), ir * std::sin(th) * std::sin(ph), ir * std::cos(ph)};
  std::copy(p, p + 3, out);
  return PLV_OK;
}

int plv_camera_update_slam(plv_ctx *ctx, const plv_state_view *st, const plv_update_options *opt, int n_var, const plv_state_var *vars,
                           int n_lm, plv_landmark *lms, const plv_tracks *tracks, plv_slam_result *res, uint64_t *ids, uint8_t *verdict,
                           double *dx_each) {
  TRY(check_common(ctx, st, opt, n_var, vars, n_lm, lms, res, ids, verdict));
  (void)hipSetDevice(ctx->device);
  *res = plv_slam_result();
  const int n = ctx->cov_n;
  Pass W{ctx, plv_update_state(ctx), st, opt};
  if (!W.us) return PLV_E_BADARG;
  W.ld = 2 * opt->max_obs;
  TRY(W.read_list(PLV_LIST_SLAM, tracks, ids));
  const int F = (int)W.ids.size();
  std::fill(verdict, verdict + F, (uint8_t)0);
  if (dx_each) std::fill(dx_each, dx_each + (size_t)F * n, 0.0);
  if (F == 0) {
    count(res, verdict, 0, n);
    return PLV_OK;
  }
  TRY(W.select_observations(3));
  // the landmark of every entry; its three columns close the entry's column map
  std::vector<int> lm_of((size_t)F, -1);
  bool any = false;
  for (int f = 0; f < F; ++f) {
    Entry &e = W.ent[f];
    for (int i = 0; i < n_lm; ++i)
      if (lms[i].featid == e.id) {
        lm_of[f] = i;
        break;
      }
    if (lm_of[f] < 0 || e.m < 1 || e.m > opt->max_obs) {  // REF :314-317 (fewer than 2 rows); no landmark; beyond the batch capacity
      e.m = 0;
      continue;
    }
    for (int q = 0; q < 3; ++q) e.cols[(size_t)e.k + q] = lms[lm_of[f]].id + q;
    any = true;
  }
  if (!any) {
    count(res, verdict, F, n);
    return PLV_OK;
  }
  TRY(W.stage_static(n));
  const ResultBlock head(n, 0);
  const size_t rb = head.head_bytes() + 8;  // (+ the verdict)
  char *hres = W.us->slam.h_res.as<char>();
  for (int f = 0; f < F; ++f) {
    const Entry &e = W.ent[f];
    if (e.m < 1) continue;
    plv_landmark &lm = lms[lm_of[f]];
    double xyz[3], xyz_fej[3];
    plv_landmark_xyz(lm.rep, lm.value, xyz), plv_landmark_xyz(lm.rep, lm.fej, xyz_fej);
    TRY(W.stage_dynamic(xyz, xyz_fej));
    const int k = e.k, kx = k + 3, r = 2 * e.m;
    JacParams P{};
    W.fill(P, e, k, lm.rep);
    LandmarkSys L{W.d_block, W.d_rows, e.o0, e.o1, 0};
    TRY(launch_landmark_system(ctx, P, L));
    // Chi2Check (REF :329, UpdaterStatistics.cpp:94-117 with R = I) then EKFUpdate, which returns at once behind a rejection
    const int *d_cols = (const int *)(W.us->slam.stat.as<char>() + e.off_cols);
    double *d_P = ctx->d_P.as<double>();
    ++ctx->gather_stamp;
    TRY(launch_gather_cov(ctx, d_P, n, n, d_cols, kx));
    Chi2Args a{};
    a.P = d_P, a.ldp = n, a.k = kx, a.ld = W.ld, a.fdim_off = 0;
    a.rows = W.d_rows, a.Hx = W.d_block, a.res = W.d_block + (size_t)kx * W.ld, a.cols = d_cols;
    a.sigma2 = 1.0, a.chi2 = ctx->d_chi2.as<double>();
    a.stack = ctx->d_stack.as<double>(), a.lds = W.ld, a.mp_max = W.ld, a.stack_accepted_only = 1;
    a.chi2_mult = opt->chi2_mult, a.res_norm_gate = 0.0;
    a.q95 = W.us->q95.as<double>(), a.q95_n = Q95_ENTRIES, a.min_rows = 2;
    a.accepted = W.d_acc, a.acc_rows = W.d_acc_rows, a.n_acc = W.d_flag + 1;
    TRY(launch_chi2(ctx, 1, a, r));
    TRY(launch_ekf_fast(ctx, EkfRiders{W.d_flag + 1}, d_P, n, n, W.d_block, r, kx, W.ld, d_cols, a.res, nullptr, W.d_dx, W.d_flag, /*gathered*/ true));
    PLV_HIP_CHECK(plv::memcpy_async(hres, W.us->slam.res.p, rb, hipMemcpyDeviceToHost, ctx->stream));
    TRY(plv::stream_wait(ctx));
    const int flag = *head.status(hres);
    const bool passed = *head.accepted(hres) != 0;
    if (!passed) {
      verdict[f] = 2;
    } else if (flag != 0) {
      verdict[f] = 3;  // (the commit kernel left covariance and dx alone)
    } else {
      const double *dx = head.dx(hres);
      TRY(W.apply(n_var, vars, n_lm, lms, dx, n));
      if (dx_each) std::copy(dx, dx + n, dx_each + (size_t)f * n);
      verdict[f] = 1;
    }
  }
  count(res, verdict, F, n);
  return PLV_OK;
}

int plv_camera_init_slam(plv_ctx *ctx, const plv_state_view *st, const plv_update_options *opt, int n_var, const plv_state_var *vars,
                         int *n_lm_io, int cap_lm, plv_landmark *lms, const plv_tracks *tracks, plv_slam_result *res, uint64_t *ids,
                         uint8_t *verdict, double *dx_each) {
  if (!n_lm_io || !lms || *n_lm_io < 0 || cap_lm < *n_lm_io) return PLV_E_BADARG;
  TRY(check_common(ctx, st, opt, n_var, vars, *n_lm_io, lms, res, ids, verdict));
  if (!rep_known(st->feat_rep) || (opt->n_slam > 0 && !opt->slam_ids)) return PLV_E_BADARG;
  (void)hipSetDevice(ctx->device);
  const int n0 = ctx->cov_n;
  Pass W{ctx, plv_update_state(ctx), st, opt};
  if (!W.us) return PLV_E_BADARG;
  W.ld = 2 * opt->max_obs;
  TRY(W.read_list(PLV_LIST_INIT, tracks, ids));
  const int F = (int)W.ids.size();
  if (cap_lm < *n_lm_io + F) {
    set_last_error("plv_camera_init_slam: room for %d landmarks, %d held and %d candidates", cap_lm, *n_lm_io, F);
    return PLV_E_BADARG;
  }
  *res = plv_slam_result();
  const size_t stride = 3 + (size_t)n0 + 3 * (size_t)F;
  std::fill(verdict, verdict + F, (uint8_t)0);
  if (dx_each) std::fill(dx_each, dx_each + (size_t)F * stride, 0.0);
  if (F == 0) {
    count(res, verdict, 0, n0);
    return PLV_OK;
  }
  TRY(W.select_observations(0));
  TRY(W.stage_static(n0 + 3 * F));
  char *hres = W.us->slam.h_res.as<char>();
  const int n_cap = n0 + 3 * F;
  for (int f = 0; f < F; ++f) {
    const Entry &e = W.ent[f];
    // A landmark of the state stays in the tracker's database (CamHelper.cpp:621-628) and can come back through the pool as a
    // candidate: consumed without growing the state (the SLAM branch)
    bool in_state = false;
    for (int i = 0; i < opt->n_slam; ++i) in_state = in_state || opt->slam_ids[i] == e.id;
    for (int i = 0; i < *n_lm_io; ++i) in_state = in_state || lms[i].featid == e.id;
    if (in_state) continue;
    const int m = e.m;
    if (m < 2 || m > opt->max_obs) {  // REF :354-357 needs more than one measurement
      TRY(W.give_back(e));
      ++res->n_returned;
      continue;
    }
    const int n = ctx->cov_n, n2 = n + 3, k = e.k, r = 2 * m, mup = r - 3;
    TRY(W.stage_dynamic(e.p, e.p));
    JacParams P{};
    W.fill(P, e, k, st->feat_rep);
    LandmarkSys L{W.d_block, W.d_rows, e.o0, e.o1, 1};
    TRY(launch_landmark_system(ctx, P, L));
    // ---- StateHelper::initialize: Givens split with all rows kept (:391), the gate on the updating rows (:409-424)
    double *dHf = W.d_block, *dHx = dHf + (size_t)3 * W.ld, *dres = dHx + (size_t)k * W.ld;
    const int *d_cols = (const int *)(W.us->slam.stat.as<char>() + e.off_cols);
    double *d_P = ctx->d_P.as<double>();
    TRY(launch_nullspace(ctx, 1, 3, k, W.ld, W.d_rows, dHf, dHx, dres, nullptr, 0, 0, nullptr, /*shift*/ 0));
    ++ctx->gather_stamp;
    TRY(launch_gather_cov(ctx, d_P, n, n, d_cols, k));
    Chi2Args a{};
    a.P = d_P, a.ldp = n, a.k = k, a.ld = W.ld, a.fdim_off = 3;
    a.rows = W.d_rows, a.Hx = dHx + 3, a.res = dres + 3, a.cols = d_cols;
    a.sigma2 = 1.0, a.chi2 = ctx->d_chi2.as<double>();
    a.q95 = W.us->q95.as<double>(), a.q95_n = Q95_ENTRIES, a.min_rows = 4;
    TRY(launch_chi2(ctx, 1, a, mup));
    double chi = 0.0;
    PLV_HIP_CHECK(plv::memcpy_async(hres, ctx->d_chi2.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
    ctx->cov_host_synced = ctx->gather_stamp;
    memcpy(&chi, hres, 8);
    if (!(chi <= opt->chi2_mult * plv_chi2_quantile95(r))) {  // the threshold uses ALL rows (:415)
      verdict[f] = 2;
      TRY(W.give_back(e));
      ++res->n_returned;
      continue;
    }
    // ---- initialize_invertible into the second buffer, EKFUpdate with the updating rows on it (skipped behind a rejection)
    TRY(ctx->d_P2.reserve((size_t)n2 * n2 * 8));
    d_P = ctx->d_P.as<double>();
    TRY(launch_cov_init_invertible(ctx, d_P, n, d_cols, k, dHx, dHf, dres, W.ld, ctx->d_P2.as<double>(), W.d_out, W.d_initflag));
    ++counters().launches;
    hipLaunchKernelGGL(init_skip_word_kernel, dim3(1), dim3(64), 0, ctx->stream, W.d_initflag, W.d_skip);
    PLV_HIP_CHECK(hipGetLastError());
    TRY(launch_ekf_fast(ctx, EkfRiders{W.d_skip}, ctx->d_P2.as<double>(), n2, n2, dHx + 3, mup, k, W.ld, d_cols, dres + 3, nullptr, W.d_dx, W.d_flag));
    const ResultBlock head(n_cap, 0);
    const size_t rb = head.head_bytes();
    PLV_HIP_CHECK(plv::memcpy_async(hres, W.us->slam.res.p, rb, hipMemcpyDeviceToHost, ctx->stream));
    PLV_HIP_CHECK(plv::memcpy_async(hres + rb, W.d_initflag, 16 + 32 + 24, hipMemcpyDeviceToHost, ctx->stream));  // flag .. skip .. v
    PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
    ctx->prof.collect();
    const int rejected = *(const int *)(hres + rb), flag = *head.status(hres);
    if (rejected || flag != 0) {  // :572-587 / the update failed: the initialisation is reverted (:430-435) — nothing was swapped in
      verdict[f] = rejected ? 2 : 3;
      TRY(W.give_back(e));
      ++res->n_returned;
      continue;
    }
    std::swap(ctx->d_P, ctx->d_P2);
    ctx->cov_n = n2;
    ++ctx->gather_stamp;
    ctx->cov_host_synced = ctx->gather_stamp;
    const double *dx = head.dx(hres), *v = (const double *)(hres + rb + 48);
    plv_landmark &lm = lms[*n_lm_io];
    lm.featid = e.id, lm.id = n, lm.rep = st->feat_rep;
    plv_landmark_from_xyz(lm.rep, e.p, lm.fej);  // create_landmark: value = fej (CamHelper.cpp create_landmark)
    for (int q = 0; q < 3; ++q) lm.value[q] = lm.fej[q] + v[q];
    ++*n_lm_io;
    TRY(W.apply(n_var, vars, *n_lm_io, lms, dx, n2));
    if (dx_each) {
      double *row = dx_each + (size_t)f * stride;
      std::copy(v, v + 3, row);
      std::copy(dx, dx + n2, row + 3);
    }
    verdict[f] = 1;
  }
  count(res, verdict, F, ctx->cov_n);
  return PLV_OK;
}

}  // extern "C"
