// use_imu_res on the host (pl-viwo_amd/csrc/camera_tracks.hpp: cpi_servable, cpi_attach) on its own, for AddressSanitizer + UBSan: a
// hand-made CPI table over a window of four clones — one record at every clone time and three behind it, the oldest clone's records
// left in the table although the clone is gone — asked at every kind of time (stored record, between two records of one clone,
// between the records of two clones, before the first and beyond the last record, a record of the clone that left), then a pool of
// point and line tracks through cpi_attach: every observation ends in the pool or in `unused`, in order, and every kept one carries
// the index of its own time.  No GPU, no library.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pl-viwo_amd/csrc/camera_tracks.hpp"

using namespace plv;

static int fails = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++fails;                      \
      printf("FAILED %s: ", #cond); \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
    }                               \
  } while (0)

// (the library's plv_cpi_noise stands behind cpi_attach's noise branch; here: what it was asked)
static std::vector<double> noise_asked;
extern "C" int plv_cpi_noise(const plv_state_view *, const plv_cpi_table *, int n_q, const double *t_q, double *Q, int *clone_index, uint8_t *ok) {
  noise_asked.assign(t_q, t_q + n_q);
  for (int q = 0; q < n_q; ++q) {
    for (int j = 0; j < 36; ++j) Q[36 * (size_t)q + j] = t_q[q];
    clone_index[q] = q, ok[q] = 1;
  }
  return PLV_OK;
}

struct Table {
  std::vector<double> t, clone_t, dt, R, alpha, v;
  plv_cpi_table c{};
  // clones at 10, 11, 12, 13, 14 (the first one gone from the window), records at +0, +0.25, +0.5, +0.75
  Table() {
    for (int i = 0; i < 5; ++i)
      for (int k = 0; k < 4; ++k) {
        t.push_back(10.0 + i + 0.25 * k), clone_t.push_back(10.0 + i), dt.push_back(0.25 * k);
        for (int j = 0; j < 9; ++j) R.push_back(j % 4 == 0 ? 1.0 : 0.0);
        for (int j = 0; j < 3; ++j) alpha.push_back(0.0), v.push_back(0.0);
      }
    c.n = (int)t.size(), c.t = t.data(), c.clone_t = clone_t.data(), c.dt = dt.data(), c.R_I0toIk = R.data(), c.alpha = alpha.data(), c.v = v.data();
  }
};

template <class TrackT> TrackT make_track(uint64_t id, const std::vector<double> &times) {
  constexpr int W = TrackT::W;
  TrackT tr;
  for (double t : times) {
    tr.t.push_back(t);
    for (int w = 0; w < W; ++w) tr.uv.push_back((float)(t + id + 0.1 * w)), tr.uvn.push_back((float)(-t - 0.1 * w));
  }
  return tr;
}

template <class TrackT> void run(const char *kind, const plv_state_view &st, const Table &tab, bool noise) {
  constexpr int W = TrackT::W;
  const double dt = 0.125;  // camera time offset: the query is time + dt
  // stamps whose time + dt is: a stored record (11.25), between records (11.375), between two clones' records (11.875), beyond the
  // table (14.875), a record of the gone clone (10.75), a stored clone record (12.0)
  const double REC = 11.125, MID = 11.25, TWO = 11.75, LATE = 14.75, GONE = 10.625, CLONE = 11.875;
  std::vector<PoolCand<TrackT>> pool;
  pool.push_back({7, make_track<TrackT>(7, {REC, MID, CLONE})});               // every view served
  pool.push_back({3, make_track<TrackT>(3, {GONE, REC, TWO, MID, LATE})});     // three of five go back
  pool.push_back({9, make_track<TrackT>(9, {TWO, LATE})});                     // nothing left
  pool.push_back({4, make_track<TrackT>(4, {CLONE, MID})});
  const std::vector<PoolCand<TrackT>> before = pool;
  TrackMap<TrackT> unused;
  CpiPoses out;
  noise_asked.clear();
  const int rc = cpi_attach(&st, &tab.c, noise, dt, pool, unused, out);
  CHECK(rc == PLV_OK && out.on && out.noise == noise, "%s: cpi_attach returned %d", kind, rc);
  // the distinct served times, in first-seen order
  const std::vector<double> want = {REC + dt, MID + dt, CLONE + dt};
  CHECK(out.times == want, "%s: %zu distinct times", kind, out.times.size());
  size_t o = 0;
  for (size_t f = 0; f < pool.size(); ++f) {
    const TrackT &was = before[f].tr, &now = pool[f].tr;
    const auto un = unused.find(pool[f].id);
    size_t k = 0, u = 0;
    for (size_t i = 0; i < was.t.size(); ++i) {
      const bool served = cpi_servable(st, tab.c, was.t[i] + dt).ok;
      CHECK(served == (was.t[i] == REC || was.t[i] == MID || was.t[i] == CLONE), "%s: time %.3f served %d", kind, was.t[i], (int)served);
      const TrackT *dst = served ? &now : (un == unused.end() ? nullptr : &un->second);
      size_t &at = served ? k : u;
      CHECK(dst && at < dst->t.size() && dst->t[at] == was.t[i], "%s: view %zu of track %d is not where it belongs", kind, i, (int)pool[f].id);
      if (dst && at < dst->t.size())
        for (int w = 0; w < W; ++w) CHECK(dst->uv[W * at + w] == was.uv[W * i + w] && dst->uvn[W * at + w] == was.uvn[W * i + w], "%s: image point moved", kind);
      if (served) {
        CHECK(o < out.pose_of.size() && out.pose_of[o] >= 0 && out.pose_of[o] < (int)out.times.size() && out.times[(size_t)out.pose_of[o]] == was.t[i] + dt,
              "%s: observation %zu carries the index of another time", kind, o);
        ++o;
      }
      ++at;
    }
    CHECK(k == now.t.size() && now.uv.size() == W * k && now.uvn.size() == W * k, "%s: track %d keeps %zu views, %zu expected", kind, (int)pool[f].id, now.t.size(), k);
    CHECK((un == unused.end() ? 0 : un->second.t.size()) == u, "%s: track %d returns %zu views", kind, (int)pool[f].id, u);
  }
  CHECK(o == out.pose_of.size(), "%s: %zu indices for %zu kept observations", kind, out.pose_of.size(), o);
  CHECK(pool[2].tr.t.empty() && unused.count(9) == 1 && unused.count(7) == 0 && unused.count(4) == 0, "%s: who returned what", kind);
  if (noise) {
    CHECK(noise_asked == want && out.Qt.size() == 36 * want.size() && out.Ct.size() == want.size() && out.Qt[36] == want[1] && out.Ct[2] == 2, "%s: covariances per distinct time", kind);
    const CpiStage s = out.stage(&tab.c);
    CHECK(s.n_times == 3 && s.Q == out.Qt.data() && s.clone == out.Ct.data() && s.pose_of == out.pose_of.data(), "%s: stage", kind);
  } else {
    CHECK(noise_asked.empty() && out.Qt.empty() && out.stage(&tab.c).Q == nullptr, "%s: no covariances asked for", kind);
  }
}

int main() {
  Table tab;
  const double clone_time[4] = {11.0, 12.0, 13.0, 14.0};
  plv_state_view st{};
  st.n_clones = 4, st.clone_time = clone_time, st.dt_exp = 0.01;
  // ---- the rule itself, time by time
  struct { double t; bool ok; int e, i0, i1, clone; } q[] = {
      {11.25, true, 5, -1, -1, 0},     // stored record of clone 11
      {12.0, true, 8, -1, -1, 1},      // a clone's own record
      {11.375, true, -1, 5, 6, 0},     // between two records of clone 11
      {11.875, false, -1, -1, -1, -1}, // between the last record of clone 11 and the first of clone 12
      {9.5, false, -1, -1, -1, -1},    // before the first record
      {14.875, false, -1, -1, -1, -1}, // beyond the last
      {14.75, true, 19, -1, -1, 3},    // the last record
      {10.75, false, -1, -1, -1, -1},  // a record of the clone that left the window
      {10.6, false, -1, -1, -1, -1},   // between two records of that clone
  };
  for (const auto &c : q) {
    const CpiHit h = cpi_servable(st, tab.c, c.t);
    CHECK(h.ok == c.ok, "cpi_servable(%.3f) = %d", c.t, (int)h.ok);
    if (c.ok) CHECK(h.e == c.e && h.i0 == c.i0 && h.i1 == c.i1 && h.clone == c.clone, "cpi_servable(%.3f): e %d, i0 %d, i1 %d, clone %d", c.t, h.e, h.i0, h.i1, h.clone);
  }
  plv_cpi_table empty{};
  CHECK(!cpi_servable(st, empty, 11.0).ok, "an empty table serves nothing");
  // ---- tables plv_cpi_poses refuses
  Table bad;
  bad.t[3] = bad.t[2];
  std::vector<PoolCand<Track>> p1;
  p1.push_back({1, make_track<Track>(1, {11.0, 11.25})});
  TrackMap<Track> u1;
  CpiPoses o1;
  CHECK(cpi_attach(&st, &bad.c, false, 0.0, p1, u1, o1) == PLV_E_BADARG && p1[0].tr.t.size() == 2 && u1.empty(), "a table that is not ascending is refused, the pool untouched");
  CHECK(cpi_attach(&st, &tab.c, true, 0.0, p1, u1, o1) == PLV_E_BADARG && p1[0].tr.t.size() == 2, "covariances asked of a table without them");
  for (int noise = 0; noise < 2; ++noise) {
    Table tq;
    std::vector<double> Q(36 * tq.t.size(), 1.0);
    if (noise) tq.c.Q = Q.data();
    run<Track>(noise ? "points + covariances" : "points", st, tq, noise != 0);
    run<LineTrack>(noise ? "lines + covariances" : "lines", st, tq, noise != 0);
  }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok: the table's misses leave the pool, the served views keep their times' indices\n");
  return 0;
}
