// camera_tracks.hpp — host bookkeeping the point update (tracker_api.hip) and the line update (line_api.hip) share: the
// bounding-pose test, and the mechanics that move a feature track between its database, the update's pool and the hand-back to
// the database (db_unused).  A track keeps its observations in t (one time each) and uv / uvn (W floats each); the decisions —
// window margins, which tracks stay in the pool, what goes back — are the callers'.
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/plviwo.h"

namespace plv {

// State::bounding_times + bounding_poses_n (order 3): the first of the four clones that interpolate time t, -1 when there is none.
// REF: PL-VIWO/src/state/State.cpp:1023-1136 (same test as the kernels' bounding_start)
inline int bounding_start_host(const plv_state_view &st, double t) {
  const int N = st.n_clones;
  if (N < 4) return -1;
  const double *ct = st.clone_time;
  if (t < ct[0] - st.dt_exp || t > ct[N - 1] + st.dt_exp) return -1;
  if (t > ct[N - 1]) return -1;
  int n_b = -1;
  for (int i = 0; i < N - 1; ++i)
    if (ct[i] - st.dt_exp <= t && t <= ct[i + 1] + st.dt_exp) {
      n_b = i;
      break;
    }
  if (n_b < 0) return -1;
  int start = n_b - 1;
  if (n_b - 1 < 0)
    start = 0;
  else if (n_b + 2 >= N)
    start = N - 4;
  if (start < 0 || start + 4 > N) return -1;
  return start;
}
// is there an interpolation window for time t?
inline bool has_bounding_poses(const plv_state_view &st, double t) { return bounding_start_host(st, t) >= 0; }

// bounding_start_host answered from a small memo: the observations of a window carry the time stamps of the last few frames (~16
// distinct values), asked for thousands of times per update
struct BoundingMemo {
  const plv_state_view &st;
  double t[40];
  int s0[40];
  int n = 0;
  explicit BoundingMemo(const plv_state_view &s) : st(s) {}
  int operator()(double tq) {
    for (int i = n - 1; i >= 0; --i)
      if (t[i] == tq) return s0[i];
    const int r = bounding_start_host(st, tq);
    if (n < 40) t[n] = tq, s0[n++] = r;
    return r;
  }
};

struct Track {  // ov_core::Feature, one camera  (REF: open_vins/ov_core/src/feat/Feature.h:43-77)
  static constexpr int W = 2;  // floats of uv / uvn per observation: an image point
  static constexpr int P = 3;  // doubles of the triangulated feature: p_FinG
  std::vector<double> t;
  std::vector<float> uv, uvn;
  // (transient, Tracker::Spec) index of the track's point in the flow's batch of feed number li_seq
  int li = -1;
  unsigned long long li_seq = 0;
};

struct LineTrack {  // LineFeature, one camera   REF: linefeat/LineFeature.h:22-107
  static constexpr int W = 4;  // floats of uv / uvn per observation: the segment's two end points
  static constexpr int P = 6;  // doubles of the triangulated feature: line_FinG
  std::vector<double> t;
  std::vector<float> uv, uvn;
  std::vector<int> points;     // ids of the point features assigned at every observation (appended, REF :50-52)
  int D = 0;
};

struct StereoFeature {  // ov_core::Feature of a stereo pair: the observations of one id, per camera
  Track cam[2];
};

// the observation times of a feature, over all its cameras, and how many there are (feat_sort's track length, REF CamHelper.cpp:777-787)
template <class TrackT, class Fn> void each_time(const TrackT &tr, Fn fn) {
  for (double t : tr.t) fn(t);
}
template <class Fn> void each_time(const StereoFeature &f, Fn fn) {
  each_time(f.cam[0], fn);
  each_time(f.cam[1], fn);
}
template <class TrackT> size_t n_meas(const TrackT &tr) { return tr.t.size(); }
inline size_t n_meas(const StereoFeature &f) { return f.cam[0].t.size() + f.cam[1].t.size(); }

// what a track that starts from another one's observations takes along besides them: nothing for a point; a line's direction class
// and point list (copy_to_db copies the feature's point list)
inline void copy_track_meta(Track &, const Track &) {}
inline void copy_track_meta(LineTrack &dst, const LineTrack &src) {
  if (dst.t.empty() && dst.points.empty()) {
    dst.D = src.D;
    dst.points = src.points;
  }
}

template <class TrackT> struct PoolCand {
  uint64_t id;
  TrackT tr;
};
template <class TrackT> using TrackMap = std::unordered_map<uint64_t, TrackT>;

// observation i of src appended to dst
template <class TrackT> void append_obs(TrackT &dst, const TrackT &src, size_t i) {
  constexpr size_t W = TrackT::W;
  dst.t.push_back(src.t[i]);
  dst.uv.insert(dst.uv.end(), src.uv.begin() + W * i, src.uv.begin() + W * (i + 1));
  dst.uvn.insert(dst.uvn.end(), src.uvn.begin() + W * i, src.uvn.begin() + W * (i + 1));
}

// observation i of feature id's track src goes back to the database later (db_unused)
template <class TrackT> void give_back(TrackMap<TrackT> &unused, uint64_t id, const TrackT &src, size_t i) {
  TrackT &u = unused[id];
  copy_track_meta(u, src);
  append_obs(u, src, i);
}

// a whole candidate goes back: nothing of it went back earlier — the track is handed over as it is; else behind what did
template <class TrackT> void give_back_all(TrackMap<TrackT> &unused, PoolCand<TrackT> &c) {
  if (unused.find(c.id) == unused.end()) {
    unused.emplace(c.id, std::move(c.tr));
    c.tr = TrackT{};
    return;
  }
  for (size_t i = 0; i < c.tr.t.size(); ++i) give_back(unused, c.id, c.tr, i);
}

// the observations i with keep(i) stay, in order (keep may read observation i of tr: it is still in place); returns how many
template <class TrackT, class Keep> size_t trim_track(TrackT &tr, Keep keep) {
  constexpr size_t W = TrackT::W;
  size_t n = 0;
  for (size_t i = 0; i < tr.t.size(); ++i) {
    if (!keep(i)) continue;
    if (n != i) {
      tr.t[n] = tr.t[i];
      std::copy(tr.uv.begin() + W * i, tr.uv.begin() + W * (i + 1), tr.uv.begin() + W * n);
      std::copy(tr.uvn.begin() + W * i, tr.uvn.begin() + W * (i + 1), tr.uvn.begin() + W * n);
    }
    ++n;
  }
  tr.t.resize(n);
  tr.uv.resize(W * n);
  tr.uvn.resize(W * n);
  return n;
}

// cleanup_measurements on one track (REF FeatureDatabase.cpp:286-323): observations older than t go; returns how many stay
template <class TrackT> size_t drop_before(TrackT &tr, double t) {
  return trim_track(tr, [&tr, t](size_t i) { return !(tr.t[i] < t); });
}

// ---- what the point, stereo and line databases answer their accessors with (plv_db_* / plv_stereo_db_* / plv_line_db_*): the entry
// points keep their own argument checks and locks.  A database is any map from id to feature; where a feature is not itself a
// track (the stereo pair's two cameras), the caller says how to get at one.

// the ids in ascending order (the reference iterates an unordered_map), as many as `cap` holds: *n is set either way
template <class Map> int export_sorted_ids(const Map &db, uint64_t *ids, int cap, int *n) {
  std::vector<uint64_t> out;
  out.reserve(db.size());
  for (const auto &kv : db) out.push_back(kv.first);
  std::sort(out.begin(), out.end());
  *n = (int)out.size();
  if (*n > cap) return PLV_E_CAPACITY;
  if (ids) std::copy(out.begin(), out.end(), ids);
  return PLV_OK;
}

// CSR export of the tracks of ids [n] in the layout of plv_tracks / plv_line_tracks: obs_ptr [n + 1], and (each may be null) times,
// uv and uvn with TrackT::W floats per observation.  track_of(id): the track or null — a missing id gets no observations.  A
// track that does not fit cap_obs ends the export with PLV_E_CAPACITY before anything of it is written (obs_ptr of it neither).
// extra(f, track or null) runs per id behind the observations and may end the export with a code of its own.
template <class TrackOf, class Extra>
int export_tracks(const uint64_t *ids, int n, TrackOf track_of, int *obs_ptr, double *obs_time, float *obs_uv, float *obs_uvn, int cap_obs,
                  Extra extra) {
  int at = 0;
  obs_ptr[0] = 0;
  for (int f = 0; f < n; ++f) {
    const auto *tr = track_of(ids[f]);
    if (tr) {
      constexpr size_t W = std::remove_pointer_t<decltype(tr)>::W;
      const int m = (int)tr->t.size();
      if (at + m > cap_obs) return PLV_E_CAPACITY;
      if (obs_time) std::copy(tr->t.begin(), tr->t.end(), obs_time + at);
      if (obs_uv) std::copy(tr->uv.begin(), tr->uv.end(), obs_uv + W * (size_t)at);
      if (obs_uvn) std::copy(tr->uvn.begin(), tr->uvn.end(), obs_uvn + W * (size_t)at);
      at += m;
    }
    const int rc = extra(f, tr);
    if (rc != PLV_OK) return rc;
    obs_ptr[f + 1] = at;
  }
  return PLV_OK;
}
template <class TrackOf>
int export_tracks(const uint64_t *ids, int n, TrackOf track_of, int *obs_ptr, double *obs_time, float *obs_uv, float *obs_uvn, int cap_obs) {
  return export_tracks(ids, n, track_of, obs_ptr, obs_time, obs_uv, obs_uvn, cap_obs, [](int, const void *) { return (int)PLV_OK; });
}
// ... of a database whose features are tracks
template <class TrackT> auto track_in(const TrackMap<TrackT> &db) {
  return [&db](uint64_t id) -> const TrackT * {
    const auto it = db.find(id);
    return it == db.end() ? nullptr : &it->second;
  };
}

// the features of ids [n] leave the database (an id it does not hold: nothing happens)
template <class Map> void erase_ids(Map &db, const uint64_t *ids, int n) {
  for (int i = 0; i < n; ++i) db.erase(ids[i]);
}

// FeatureDatabase::cleanup_measurements(t) (REF FeatureDatabase.cpp:286-323): observations older than t go, a feature with none
// left is erased.  drop(feature, t): how many the feature keeps, over all its cameras.
template <class Map, class Drop> void cleanup_measurements(Map &db, double t, Drop drop) {
  for (auto it = db.begin(); it != db.end();) it = drop(it->second, t) == 0 ? db.erase(it) : std::next(it);
}
template <class TrackT> void cleanup_measurements(TrackMap<TrackT> &db, double t) {
  cleanup_measurements(db, t, [](TrackT &tr, double t_) { return drop_before(tr, t_); });
}

// remove_unusable_measurements on one track (REF CamHelper.cpp:740-775): with tm = time + dt, observations with tm > t_new go back
// (unused), those with tm < t_old are dropped; returns how many stay
template <class TrackT> size_t trim_to_window(TrackMap<TrackT> &unused, uint64_t id, TrackT &tr, double dt, double t_new, double t_old) {
  return trim_track(tr, [&unused, id, &tr, dt, t_new, t_old](size_t i) {
    const double tm = tr.t[i] + dt;
    if (tm > t_new) {
      give_back(unused, id, tr, i);
      return false;
    }
    return !(tm < t_old);
  });
}

// features_containing_older(t_old) + features_not_containing_newer(t_new) (REF CamHelper.cpp:631-637, LineHelper.cpp:33-38): every
// track with an observation older than t_old or none newer than t_new leaves the database for the pool, in ascending id order.  The
// caller holds the database's lock.
template <class TrackT> void take_pool(TrackMap<TrackT> &db, double t_old, double t_new, std::vector<PoolCand<TrackT>> &pool) {
  // (the tracks to take are remembered by position: extracting by iterator needs no second look-up — 180 hash look-ups were 8 of the
  //  line pool's 15 us on the worker's path in front of the line launch)
  static thread_local std::vector<std::pair<uint64_t, typename TrackMap<TrackT>::iterator>> take;
  take.clear();
  for (auto it = db.begin(); it != db.end(); ++it) {
    bool older = false, newer = false;
    each_time(it->second, [&](double t) {
      older = older || t < t_old;
      newer = newer || t > t_new;
    });
    if (older || !newer) take.emplace_back(it->first, it);
  }
  std::sort(take.begin(), take.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
  pool.reserve(pool.size() + take.size());
  for (auto &tk : take) pool.push_back(PoolCand<TrackT>{tk.first, std::move(db.extract(tk.second).mapped())});
}

// REF CamHelper.cpp:640 sort(feats_pool, feat_sort): long tracks first, ties in the order they stand.  The order is found on
// (length, position) pairs and every candidate moved once — a stable sort of the candidates themselves moves each ~8 times
template <class TrackT> void sort_long_first(std::vector<PoolCand<TrackT>> &pool) {
  static thread_local std::vector<std::pair<int, int>> ord;
  ord.clear();
  for (size_t i = 0; i < pool.size(); ++i) ord.emplace_back(-(int)n_meas(pool[i].tr), (int)i);
  std::sort(ord.begin(), ord.end());
  std::vector<PoolCand<TrackT>> sorted;
  sorted.reserve(pool.size());
  for (const auto &o : ord) sorted.push_back(std::move(pool[(size_t)o.second]));
  pool.swap(sorted);
}

// the pool in the layout of the device batch (plv_tracks / plv_line_tracks): ptr (CSR over the candidates), times, uv, uvn
template <class TrackT>
void flatten_pool(const std::vector<PoolCand<TrackT>> &pool, std::vector<int> &ptr, std::vector<double> &t, std::vector<float> &uv, std::vector<float> &uvn) {
  constexpr size_t W = TrackT::W;
  ptr.assign(pool.size() + 1, 0);
  for (size_t f = 0; f < pool.size(); ++f) ptr[f + 1] = ptr[f] + (int)pool[f].tr.t.size();
  const size_t nobs = (size_t)ptr.back();
  t.resize(nobs), uv.resize(W * nobs), uvn.resize(W * nobs);
  for (size_t f = 0; f < pool.size(); ++f) {
    const TrackT &tr = pool[f].tr;
    std::copy(tr.t.begin(), tr.t.end(), t.begin() + ptr[f]);
    std::copy(tr.uv.begin(), tr.uv.end(), uv.begin() + W * ptr[f]);
    std::copy(tr.uvn.begin(), tr.uvn.end(), uvn.begin() + W * ptr[f]);
  }
}

// ---- use_imu_res (plv_update_options::cpi)
// use_imu_res on the one-submission updates (plv_update_options::cpi): what the stagers of a Jacobian batch (jacobian_api.hip) add to
// the packed block so that cpi_pose_kernel, on the stream ahead of the fused launch, forms the pose of every DISTINCT observation
// time — host arrays, valid for the duration of the submitting call.  Every time is one the table serves (cpi_servable).
struct CpiStage {
  const plv_cpi_table *table;
  int n_times;
  const double *times;  // [n_times] distinct observation time + camera time offset
  const int *pose_of;   // [observations of the batch] index into times
  const double *Q;      // (use_imu_cov, else null) [n_times][36] plv_cpi_noise of the times
  const int *clone;     // ... and [n_times] the clone each hangs on
};
// Whether the CPI table serves query time t, and from which records — the rule of cpi_pose_kernel's `ok` (jacobian_kernels.hip;
// REF State.cpp:273-355 have_cpi's first two stages), which reads times only: a record stored at exactly t whose clone is in the
// window (e >= 0), else two neighbouring records i0 / i1 of one clone that has not left the window; and that clone (clone: its index
// in the window) with its own record in the table.  Nothing is launched.
struct CpiHit {
  bool ok = false;
  int e = -1, i0 = -1, i1 = -1, clone = -1;
};
inline CpiHit cpi_servable(const plv_state_view &st, const plv_cpi_table &cpi, double t) {
  CpiHit h;
  const int n = cpi.n;
  auto find_t = [&](double x) {
    const double *e = std::lower_bound(cpi.t, cpi.t + n, x);
    return (e != cpi.t + n && *e == x) ? (int)(e - cpi.t) : -1;
  };
  auto find_clone = [&](double x) {
    for (int i = 0; i < st.n_clones; ++i)
      if (st.clone_time[i] == x) return i;
    return -1;
  };
  double clone_t;
  const int e = n > 0 ? find_t(t) : -1;
  if (e >= 0 && find_clone(cpi.clone_t[e]) >= 0) {  // REF State.cpp:275-277
    h.e = e;
    clone_t = cpi.clone_t[e];
  } else {  // create_new_cpi_linear :286-355
    if (n == 0 || t < cpi.t[0] || t > cpi.t[n - 1]) return h;
    const int lo = (int)(std::lower_bound(cpi.t, cpi.t + n, t) - cpi.t);
    const int i0 = (t == cpi.t[0]) ? 0 : lo - 1;
    const int up = (int)(std::upper_bound(cpi.t, cpi.t + n, t) - cpi.t);
    const int i1 = (t == cpi.t[n - 1]) ? n - 1 : up;
    if (cpi.clone_t[i0] != cpi.clone_t[i1] || cpi.clone_t[i0] < st.clone_time[0]) return h;
    h.i0 = i0, h.i1 = i1;
    clone_t = cpi.clone_t[i0];
  }
  const int ci = find_clone(clone_t);
  if (ci < 0 || find_t(clone_t) < 0) return h;  // clones.at / cpis.at would throw
  h.clone = ci;
  h.ok = true;
  return h;
}
// what plv_cpi_poses refuses of a table
inline bool cpi_table_usable(const plv_cpi_table *cpi) {
  if (!cpi || cpi->n < 0) return false;
  if (cpi->n > 0 && (!cpi->t || !cpi->clone_t || !cpi->dt || !cpi->R_I0toIk || !cpi->alpha || !cpi->v)) return false;
  for (int i = 1; i < cpi->n; ++i)
    if (!(cpi->t[i - 1] < cpi->t[i])) return false;
  return true;
}

// The poses of the pool's observations from the CPI table, in the order of the flattened pool (flatten_pool).  One-submission route:
// the distinct observation times (time + dt) and every observation's index into them — cpi_pose_kernel forms the poses on the stream
// (plv::CpiStage), nothing of them reaches the host; noise: the table's covariances Qt 36 and the clone index Ct per time (host
// arithmetic, plv_cpi_noise).  Two-step route (expand): R 9 and p 3 per observation on the host, with Q 36 and C.
struct CpiPoses {
  bool on = false, noise = false;
  std::vector<double> times, Qt;
  std::vector<int> pose_of, Ct;
  std::vector<double> R, p, Q;
  std::vector<int> C;
  CpiStage stage(const plv_cpi_table *table) const {
    return CpiStage{table, (int)times.size(), times.data(), pose_of.data(), noise ? Qt.data() : nullptr, noise ? Ct.data() : nullptr};
  }
};

// Which query times the table serves and where each served one stands in `times`, the list of the DISTINCT served times
// (cpi_servable: decided on the host from times, no launch and no synchronisation).  A window's observations carry the stamps of
// its last few frames: the memo of what was asked, servable or not.
struct CpiTimes {
  const plv_state_view &st;
  const plv_cpi_table &cpi;
  std::vector<double> &times;
  std::vector<double> asked;
  std::vector<int> answer;  // index into times, -1: not served
  int index_of(double tq) {
    for (size_t i = asked.size(); i-- > 0;)
      if (asked[i] == tq) return answer[i];
    const bool ok = cpi_servable(st, cpi, tq).ok;
    asked.push_back(tq), answer.push_back(ok ? (int)times.size() : -1);
    if (ok) times.push_back(tq);
    return answer.back();
  }
};
// REF CamHelper.cpp get_imu_poses (:356-365) on one track: an observation whose time + dt the table cannot serve leaves the track
// for `unused`; the pose index of every observation that stays is appended to pose_of
template <class TrackT> void cpi_attach_track(CpiTimes &M, double dt, uint64_t id, TrackT &tr, TrackMap<TrackT> &unused, std::vector<int> &pose_of) {
  bool all = true;
  for (double t : tr.t) all = (M.index_of(t + dt) >= 0) && all;
  if (all) {
    for (double t : tr.t) pose_of.push_back(M.index_of(t + dt));
    return;
  }
  TrackT kept;
  copy_track_meta(kept, tr);
  for (size_t i = 0; i < tr.t.size(); ++i) {
    const int q = M.index_of(tr.t[i] + dt);
    if (q < 0) {
      give_back(unused, id, tr, i);
      continue;
    }
    append_obs(kept, tr, i);
    pose_of.push_back(q);
  }
  tr = std::move(kept);
}
// ... on a pool: the others' distinct times are listed, the pose indices stand in the order of the flattened pool.  A table
// plv_cpi_poses would refuse returns PLV_E_BADARG with the pool as it was.
template <class TrackT>
int cpi_attach(const plv_state_view *st, const plv_cpi_table *cpi, bool noise, double dt, std::vector<PoolCand<TrackT>> &pool,
               TrackMap<TrackT> &unused, CpiPoses &out) {
  if (!cpi_table_usable(cpi) || st->n_clones < 1 || (noise && cpi->n > 0 && !cpi->Q)) return PLV_E_BADARG;
  out = CpiPoses();
  out.on = true, out.noise = noise;
  CpiTimes M{*st, *cpi, out.times};
  for (PoolCand<TrackT> &c : pool) cpi_attach_track(M, dt, c.id, c.tr, unused, out.pose_of);
  if (noise && !out.times.empty()) {
    const size_t nt = out.times.size();
    out.Qt.resize(36 * nt), out.Ct.resize(nt);
    std::vector<uint8_t> okn(nt);
    const int rc = plv_cpi_noise(st, cpi, (int)nt, out.times.data(), out.Qt.data(), out.Ct.data(), okn.data());
    if (rc != PLV_OK) return rc;
  }
  return PLV_OK;
}
// the two-step route: the poses of the listed times come to the host (plv_cpi_poses: a launch and a synchronisation) and are laid
// out per observation
inline int cpi_expand(plv_ctx *ctx, const plv_state_view *st, const plv_cpi_table *cpi, CpiPoses &out) {
  const size_t nt = out.times.size(), nobs = out.pose_of.size();
  std::vector<double> Rt(9 * nt), pt(3 * nt);
  std::vector<uint8_t> okt(nt);
  const int rc = plv_cpi_poses(ctx, st, cpi, (int)nt, out.times.data(), Rt.data(), pt.data(), okt.data());
  if (rc != PLV_OK) return rc;
  out.R.resize(9 * nobs), out.p.resize(3 * nobs);
  if (out.noise) out.Q.resize(36 * nobs), out.C.resize(nobs);
  for (size_t o = 0; o < nobs; ++o) {
    const size_t q = (size_t)out.pose_of[o];
    std::copy(&Rt[9 * q], &Rt[9 * q] + 9, &out.R[9 * o]);
    std::copy(&pt[3 * q], &pt[3 * q] + 3, &out.p[3 * o]);
    if (out.noise) {
      std::copy(&out.Qt[36 * q], &out.Qt[36 * q] + 36, &out.Q[36 * o]);
      out.C[o] = out.Ct[q];
    }
  }
  return PLV_OK;
}

// the observations the two-step route builds its update from (the selected tracks' plv_tracks / plv_line_tracks): times, uv and,
// with CPI poses, theirs
struct ObsGather {
  std::vector<double> t, R, p, Q;
  std::vector<int> C;
  std::vector<float> uv;
};
// observation i of tr, the flattened pool's observation o (CpiPoses' index)
template <class TrackT> void gather_obs(ObsGather &g, const TrackT &tr, size_t i, const CpiPoses &cpi, size_t o) {
  constexpr size_t W = TrackT::W;
  g.t.push_back(tr.t[i]);
  g.uv.insert(g.uv.end(), tr.uv.begin() + W * i, tr.uv.begin() + W * (i + 1));
  if (!cpi.on) return;
  g.R.insert(g.R.end(), &cpi.R[9 * o], &cpi.R[9 * o] + 9);
  g.p.insert(g.p.end(), &cpi.p[3 * o], &cpi.p[3 * o] + 3);
  if (cpi.noise) {
    g.Q.insert(g.Q.end(), &cpi.Q[36 * o], &cpi.Q[36 * o] + 36);
    g.C.push_back(cpi.C[o]);
  }
}

// ---- the batch tail of an update: what follows the triangulation and gate results of the pool.  start_of: BoundingMemo (or the
// like); an observation is usable when its time + dt has bounding clones (get_imu_poses, REF CamHelper.cpp:327-372)

template <class TrackT, class StartOf> int usable_views(const TrackT &tr, double dt, StartOf &start_of) {
  return (int)std::count_if(tr.t.begin(), tr.t.end(), [&](double t) { return start_of(t + dt) >= 0; });
}
// usable views of every pool candidate; returns the largest count
template <class TrackT, class StartOf>
int count_usable(const std::vector<PoolCand<TrackT>> &pool, double dt, StartOf &start_of, std::vector<int> &valid_n) {
  valid_n.assign(pool.size(), 0);
  int most = 0;
  for (size_t f = 0; f < pool.size(); ++f) most = std::max(most, valid_n[f] = usable_views(pool[f].tr, dt, start_of));
  return most;
}

// the selection loop's result, and the two-step route's arrays of the selected tracks (plv_tracks / plv_line_tracks)
template <class TrackT> struct Selection {
  std::vector<int> sel;       // pool indices, in the order they were taken
  std::vector<int> n_skip;    // per pool candidate: usable observations a truncated track leaves out (its oldest)
  std::vector<int> sptr;      // CSR over sel of g's observations
  std::vector<double> feat;   // TrackT::P per selected track
  ObsGather g;
  std::vector<uint8_t> acc;   // the gate's verdict per selected track
  explicit Selection(size_t n_pool) : n_skip(n_pool, 0) {}
  // batch capacity of the update (the reference has none): candidate f is taken; of `valid` usable observations the newest max_obs
  // are used, the older ones are consumed with the feature — counted in n_truncated
  void take(int f, int valid, int max_obs, int &n_truncated) {
    if (valid > max_obs) n_skip[f] = valid - max_obs, ++n_truncated;
    sel.push_back(f);
  }
};

// the selected tracks, in order: views without bounding clones go back, the n_skip oldest usable ones are left out, the rest is
// gathered for the two-step route (ptr: flatten_pool's, the index of CpiPoses); the feature values (feat_all: P per pool candidate)
// and ids of the selected.  Behind a fused launch the batch was built on the device: nothing is gathered, and a track whose views
// all counted as usable is not walked at all.
template <class TrackT, class StartOf>
void gather_selected(const std::vector<PoolCand<TrackT>> &pool, const std::vector<int> &valid_n, const std::vector<int> &ptr, const CpiPoses &cpi,
                     const double *feat_all, bool fused_ran, double dt, StartOf &start_of, TrackMap<TrackT> &unused, Selection<TrackT> &S,
                     uint64_t *ids_out) {
  constexpr size_t P = TrackT::P;
  const size_t n = S.sel.size();
  S.sptr.assign(n + 1, 0), S.feat.resize(P * n);
  for (size_t q = 0; q < n; ++q) {
    const int f = S.sel[q];
    const PoolCand<TrackT> &c = pool[f];
    int seen = 0;
    const bool nothing_to_do = fused_ran && valid_n[f] == (int)c.tr.t.size();
    for (size_t i = 0; !nothing_to_do && i < c.tr.t.size(); ++i) {
      if (start_of(c.tr.t[i] + dt) < 0) {
        give_back(unused, c.id, c.tr, i);
        continue;
      }
      if (seen++ < S.n_skip[f] || fused_ran) continue;
      gather_obs(S.g, c.tr, i, cpi, ptr[f] + i);
    }
    S.sptr[q + 1] = (int)S.g.t.size();
    std::copy(feat_all + P * f, feat_all + P * (f + 1), S.feat.begin() + P * q);
    if (ids_out) ids_out[q] = c.id;
  }
}

// REF UpdaterCamera.cpp:266-268 / :441-444: only what the gate rejected goes back (what EKFUpdate then rejects is consumed all the
// same) — every usable view, the skipped oldest of a truncated track included.  whole(f): the caller returns candidate f's track
// itself (true), or leaves it to the view-by-view copy.  Writes the verdicts to accepted_out (may be null); returns how many passed.
template <class TrackT, class StartOf, class Whole>
int return_rejected(const std::vector<PoolCand<TrackT>> &pool, const Selection<TrackT> &S, double dt, StartOf &start_of, TrackMap<TrackT> &unused,
                    uint8_t *accepted_out, Whole whole) {
  int n_accepted = 0;
  for (size_t q = 0; q < S.sel.size(); ++q) {
    n_accepted += S.acc[q];
    if (accepted_out) accepted_out[q] = S.acc[q];
    if (S.acc[q] || whole(S.sel[q])) continue;
    const PoolCand<TrackT> &c = pool[S.sel[q]];
    for (size_t i = 0; i < c.tr.t.size(); ++i)
      if (start_of(c.tr.t[i] + dt) >= 0) give_back(unused, c.id, c.tr, i);
  }
  return n_accepted;
}

// tr's observations behind d's
template <class TrackT> void append_track(TrackT &d, const TrackT &tr) {
  d.t.insert(d.t.end(), tr.t.begin(), tr.t.end());
  d.uv.insert(d.uv.end(), tr.uv.begin(), tr.uv.end());
  d.uvn.insert(d.uvn.end(), tr.uvn.begin(), tr.uvn.end());
}
// append_new_measurements (REF FeatureDatabase.cpp): tr's observations appended to the database's track of id — tr itself when the
// database has none.  The caller holds the database's lock.
template <class TrackT> typename TrackMap<TrackT>::iterator put_track(TrackMap<TrackT> &db, uint64_t id, TrackT &tr) {
  auto ins = db.try_emplace(id);
  TrackT &d = ins.first->second;
  if (ins.second) {
    d = std::move(tr);
  } else {
    append_track(d, tr);
  }
  return ins.first;
}

}  // namespace plv
