// track_db_check.cpp — the database accessors of pl-viwo_amd/csrc/camera_tracks.hpp (export_sorted_ids, export_tracks, erase_ids,
// cleanup_measurements) under AddressSanitizer + UBSan, on hand-made point and line databases and a two-camera feature map.  Every
// result is compared with a plain restatement written here (the loops the three entry-point families spelled out before); output
// arrays are exactly as long as the capacity given and start out filled with a sentinel, so a write too many or too far shows.
#include <cstdio>
#include <map>

#include "../../pl-viwo_amd/csrc/camera_tracks.hpp"

using namespace plv;

static int fails = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      if (fails++ < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                           \
  } while (0)

struct Pair {  // the stereo tracker's feature: one track per camera
  Track cam[2];
};

template <class TrackT> TrackT make_track(uint64_t id, int m) {
  TrackT tr;
  for (int i = 0; i < m; ++i) {
    tr.t.push_back(0.1 * (double)id + i);
    for (int k = 0; k < TrackT::W; ++k) tr.uv.push_back((float)(id * 100 + i * 10 + k)), tr.uvn.push_back((float)(id * 100 + i * 10 + k) * 0.25f);
  }
  return tr;
}

// ---- restatements
template <class Map> std::vector<uint64_t> ids_restated(const Map &db) {
  std::map<uint64_t, int> ordered;
  for (const auto &kv : db) ordered[kv.first] = 0;
  std::vector<uint64_t> out;
  for (const auto &kv : ordered) out.push_back(kv.first);
  return out;
}
struct Out {  // one export's arrays, exactly as long as their capacities
  std::vector<int> ptr, D, pts_ptr, pt_ids;
  std::vector<double> t;
  std::vector<float> uv, uvn;
  int rc = -12345;
  Out(int n, int W, int cap_obs, int cap_pts)
      : ptr(n + 1, -7), D(n, -7), pts_ptr(n + 1, -7), pt_ids(cap_pts, -7), t(cap_obs, -7.0), uv((size_t)W * cap_obs, -7.f), uvn((size_t)W * cap_obs, -7.f) {}
  bool operator==(const Out &o) const {
    return ptr == o.ptr && D == o.D && pts_ptr == o.pts_ptr && pt_ids == o.pt_ids && t == o.t && uv == o.uv && uvn == o.uvn && rc == o.rc;
  }
};
// element by element, as the point export was written; lines: with the direction class and the point-id CSR as the line export had them
template <class TrackT, class Find>
void export_restated(const std::vector<uint64_t> &ids, Find find, int W, bool wt, bool wuv, bool wuvn, int cap_obs, bool line, bool wD, bool wpp,
                     bool wpi, int cap_pts, Out &o) {
  int at = 0, npt = 0;
  o.ptr[0] = 0;
  if (line && wpp) o.pts_ptr[0] = 0;
  for (size_t f = 0; f < ids.size(); ++f) {
    const TrackT *tr = find(ids[f]);
    if (tr) {
      const int m = (int)tr->t.size();
      if (at + m > cap_obs) {
        o.rc = PLV_E_CAPACITY;
        return;
      }
      for (int i = 0; i < m; ++i) {
        if (wt) o.t[at + i] = tr->t[i];
        for (int k = 0; k < W; ++k) {
          if (wuv) o.uv[(size_t)W * (at + i) + k] = tr->uv[(size_t)W * i + k];
          if (wuvn) o.uvn[(size_t)W * (at + i) + k] = tr->uvn[(size_t)W * i + k];
        }
      }
      at += m;
    }
    if constexpr (std::is_same<TrackT, LineTrack>::value) {
      if (line) {
        if (tr) {
          if (wD) o.D[f] = tr->D;
          if (wpp) {
            if (npt + (int)tr->points.size() > cap_pts) {
              o.rc = PLV_E_CAPACITY;
              return;
            }
            for (size_t i = 0; i < tr->points.size(); ++i)
              if (wpi) o.pt_ids[npt + i] = tr->points[i];
            npt += (int)tr->points.size();
          }
        } else if (wD) {
          o.D[f] = 0;
        }
      }
    }
    o.ptr[f + 1] = at;
    if (line && wpp) o.pts_ptr[f + 1] = npt;
  }
  o.rc = PLV_OK;
}

static int n_exports = 0;
template <class TrackT, class Find> void check_exports(const std::vector<uint64_t> &ids, Find find, bool line) {
  constexpr int W = TrackT::W;
  int need_obs = 0, need_pts = 0;
  for (uint64_t id : ids)
    if (const TrackT *tr = find(id)) {
      need_obs += (int)tr->t.size();
      if constexpr (std::is_same<TrackT, LineTrack>::value) need_pts += (int)tr->points.size();
    }
  const int n = (int)ids.size();
  for (int cap_obs : {need_obs, need_obs - 1, need_obs + 3})
    for (int cap_pts : line ? std::vector<int>{need_pts, need_pts - 1} : std::vector<int>{0})
      for (int absent = -1; absent < (line ? 6 : 3); ++absent) {  // which nullable output is absent: t, uv, uvn, D, pts_ptr, pt_ids
        if (cap_obs < 0 || cap_pts < 0) continue;
        const bool wt = absent != 0, wuv = absent != 1, wuvn = absent != 2, wD = line && absent != 3, wpp = line && absent != 4, wpi = line && absent != 5;
        Out want(n, W, cap_obs, cap_pts), got(n, W, cap_obs, cap_pts);
        export_restated<TrackT>(ids, find, W, wt, wuv, wuvn, cap_obs, line, wD, wpp, wpi, cap_pts, want);
        double *t = wt ? got.t.data() : nullptr;
        float *uv = wuv ? got.uv.data() : nullptr, *uvn = wuvn ? got.uvn.data() : nullptr;
        if (!line) {
          got.rc = export_tracks(ids.data(), n, find, got.ptr.data(), t, uv, uvn, cap_obs);
        } else if constexpr (std::is_same<TrackT, LineTrack>::value) {
          // the extras of plv_line_db_export_tracks, around the shared core
          int *D = wD ? got.D.data() : nullptr, *pts_ptr = wpp ? got.pts_ptr.data() : nullptr, *pt_ids = wpi ? got.pt_ids.data() : nullptr;
          int npt = 0;
          if (pts_ptr) pts_ptr[0] = 0;
          auto extras = [&](int i, const LineTrack *tr) {
            if (D) D[i] = tr ? tr->D : 0;
            if (tr && pts_ptr) {
              if (npt + (int)tr->points.size() > cap_pts) return (int)PLV_E_CAPACITY;
              if (pt_ids) std::copy(tr->points.begin(), tr->points.end(), pt_ids + npt);
              npt += (int)tr->points.size();
            }
            if (pts_ptr) pts_ptr[i + 1] = npt;
            return (int)PLV_OK;
          };
          got.rc = export_tracks(ids.data(), n, find, got.ptr.data(), t, uv, uvn, cap_obs, extras);
        }
        CHECK(got == want);
        CHECK(want.rc == ((cap_obs < need_obs || (line && wpp && cap_pts < need_pts)) ? PLV_E_CAPACITY : PLV_OK));
        ++n_exports;
      }
}

int main() {
  // ---- a point database, a line database and a stereo database with the same ids (not in order; tracks of 0 .. 4 observations)
  TrackMap<Track> pts;
  TrackMap<LineTrack> lines;
  std::unordered_map<uint64_t, Pair> pairs;
  const uint64_t have[] = {42, 7, 1000003, 8, 3, 19, (uint64_t)1 << 40};
  int k = 0;
  for (uint64_t id : have) {
    pts[id] = make_track<Track>(id, k % 5);
    lines[id] = make_track<LineTrack>(id, (k + 2) % 5);
    lines[id].D = 1 + k % 3;
    for (int i = 0; i < (k * 2) % 5; ++i) lines[id].points.push_back((int)id % 50 + i);
    pairs[id].cam[0] = make_track<Track>(id, (k + 1) % 4);
    pairs[id].cam[1] = make_track<Track>(id + 1, (k + 3) % 4);
    ++k;
  }
  // ---- sorted ids: exactly enough room, one short (nothing written, the count set), no array
  {
    const std::vector<uint64_t> want = ids_restated(pairs);
    CHECK(want.size() == 7 && want.front() == 3 && want.back() == ((uint64_t)1 << 40));
    std::vector<uint64_t> got(want.size(), 99);
    int n = -1;
    CHECK(export_sorted_ids(pairs, got.data(), (int)got.size(), &n) == PLV_OK && n == 7 && got == want);
    CHECK(export_sorted_ids(lines, got.data(), (int)got.size(), &n) == PLV_OK && got == ids_restated(lines));
    std::vector<uint64_t> small(want.size() - 1, 99);
    n = -1;
    CHECK(export_sorted_ids(pts, small.data(), (int)small.size(), &n) == PLV_E_CAPACITY && n == 7 && small == std::vector<uint64_t>(6, 99));
    n = -1;
    CHECK(export_sorted_ids(pts, nullptr, 7, &n) == PLV_OK && n == 7);
    TrackMap<Track> none;
    CHECK(export_sorted_ids(none, nullptr, 0, &n) == PLV_OK && n == 0);
  }
  // ---- CSR export: present and missing ids, one id twice, none at all
  const std::vector<uint64_t> ask = {8, 5, 42, 42, 1000003, 0, (uint64_t)1 << 40, 3, 7, 19, 77};
  for (const std::vector<uint64_t> &ids : {ask, std::vector<uint64_t>{}, std::vector<uint64_t>{5, 77}}) {
    check_exports<Track>(ids, track_in(pts), false);
    check_exports<LineTrack>(ids, track_in(lines), false);
    check_exports<LineTrack>(ids, track_in(lines), true);
    for (int cam = 0; cam < 2; ++cam)
      check_exports<Track>(ids, [&pairs, cam](uint64_t id) -> const Track * {
        const auto it = pairs.find(id);
        return it == pairs.end() ? nullptr : &it->second.cam[cam];
      }, false);
  }
  // ---- erase: absent ids change nothing, present ones go, twice is once
  {
    TrackMap<LineTrack> db = lines;
    const uint64_t absent[] = {5, 77, 0};
    erase_ids(db, absent, 3);
    CHECK(ids_restated(db) == ids_restated(lines));
    erase_ids(db, absent, 0);
    erase_ids(db, (const uint64_t *)nullptr, 0);
    const uint64_t some[] = {42, 5, 42, 3};
    erase_ids(db, some, 4);
    CHECK(db.size() == 5 && db.find(42) == db.end() && db.find(3) == db.end() && db.find(7) != db.end());
  }
  // ---- cleanup_measurements: a restatement per track (observations with t < t0 go), features with nothing left erased
  auto kept_restated = [](const Track &tr, double t0) {
    Track o;
    for (size_t i = 0; i < tr.t.size(); ++i)
      if (!(tr.t[i] < t0)) {
        o.t.push_back(tr.t[i]);
        o.uv.insert(o.uv.end(), {tr.uv[2 * i], tr.uv[2 * i + 1]});
        o.uvn.insert(o.uvn.end(), {tr.uvn[2 * i], tr.uvn[2 * i + 1]});
      }
    return o;
  };
  auto same = [](const Track &a, const Track &b) { return a.t == b.t && a.uv == b.uv && a.uvn == b.uvn; };
  for (double t0 : {-1.0, 1.0, 2.5, 1e9}) {
    TrackMap<Track> db = pts;
    cleanup_measurements(db, t0);
    size_t left = 0;
    for (const auto &kv : pts) {
      const Track w = kept_restated(kv.second, t0);
      const auto it = db.find(kv.first);
      CHECK(w.t.empty() ? it == db.end() : (it != db.end() && same(it->second, w)));
      left += !w.t.empty();
    }
    CHECK(db.size() == left);
  }
  {
    // two cameras: a feature one camera of which empties stays (with that camera empty), one both cameras of which empty goes
    std::unordered_map<uint64_t, Pair> db;
    db[1].cam[0] = make_track<Track>(0, 2);   // times 0, 1
    db[1].cam[1] = make_track<Track>(0, 4);   // times 0 .. 3
    db[2].cam[0] = make_track<Track>(0, 2);
    db[2].cam[1] = make_track<Track>(0, 1);
    db[3].cam[1] = make_track<Track>(0, 3);   // (camera 0 never saw it)
    const std::unordered_map<uint64_t, Pair> before = db;
    auto drop = [](Pair &f, double t_) { return drop_before(f.cam[0], t_) + drop_before(f.cam[1], t_); };
    cleanup_measurements(db, 2.0, drop);
    CHECK(db.size() == 2 && db.find(2) == db.end());
    for (const auto &kv : before) {
      const Track w0 = kept_restated(kv.second.cam[0], 2.0), w1 = kept_restated(kv.second.cam[1], 2.0);
      const auto it = db.find(kv.first);
      if (w0.t.empty() && w1.t.empty())
        CHECK(it == db.end());
      else
        CHECK(it != db.end() && same(it->second.cam[0], w0) && same(it->second.cam[1], w1));
    }
    CHECK(db[1].cam[0].t.empty() && db[1].cam[1].t.size() == 2 && db[3].cam[1].t.size() == 1);
    cleanup_measurements(db, 10.0, drop);
    CHECK(db.empty());
  }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok: database accessors, %d exports\n", n_exports);
  return 0;
}
