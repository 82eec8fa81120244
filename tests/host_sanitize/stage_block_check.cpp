// The block packer of the Jacobian stagers (pl-viwo_amd/csrc/stage_block.hpp) on its own, for AddressSanitizer + UBSan: a point
// batch and a line batch, laid out array by array as jacobian_api.hip lays them out, with every optional array present and with every
// optional array absent, packed into a heap block of exactly the size the packer reports.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../pl-viwo_amd/csrc/stage_block.hpp"

using plv::StageBlock;

static int fails = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++fails;                           \
      printf("FAILED %s: ", #cond);      \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
    }                                    \
  } while (0)

struct Batch {
  StageBlock B;
  struct Rec {
    const char *name;
    size_t off, bytes, room;             // copied bytes, bytes kept (copied + spare), both before padding
    std::vector<unsigned char> want;     // what must read back
    std::function<void *()> host;
    std::function<const void *()> dev;
    bool filled_by_caller;
  };
  std::vector<Rec> recs;
  std::vector<std::vector<unsigned char>> sources;  // (kept alive until copy_all)
  unsigned seed = 1;

  // W values of T per element, as the stagers add them; src_less: room only, written through host() after copy_all
  template <size_t W, class T> StageBlock::Slot<T> put(const char *name, size_t count, bool present, size_t spare = 0, bool src_less = false) {
    if (!present) {
      StageBlock::Slot<T> none;
      CHECK(!none && B.host(none) == nullptr && B.dev(none) == nullptr, "%s: an absent array must give null", name);
      return none;
    }
    const size_t bytes = W * count * sizeof(T);
    std::vector<unsigned char> data(bytes);
    for (auto &b : data) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
    sources.push_back(data);
    const size_t before = B.total();
    StageBlock::Slot<T> s = src_less ? B.room<T, W>(count) : B.add<W>((const T *)sources.back().data(), count, spare);
    CHECK((bool)s, "%s: no slot", name);
    CHECK(B.offset(s) == before, "%s: offset %zu, the block held %zu bytes", name, B.offset(s), before);
    CHECK(B.total() - before == StageBlock::padded(bytes + spare * sizeof(T)), "%s: grew by %zu", name, B.total() - before);
    StageBlock *pB = &B;
    recs.push_back({name, B.offset(s), bytes, bytes + spare * sizeof(T), data, [pB, s] { return (void *)pB->host(s); },
                    [pB, s] { return (const void *)pB->dev(s); }, src_less});
    return s;
  }

  void pack_and_check(const char *what) {
    CHECK(!B.overflowed(), "%s: capacity", what);
    size_t sum = 0;
    for (const Rec &r : recs) sum += StageBlock::padded(r.room);
    CHECK(sum == B.total(), "%s: padded sizes add up to %zu, total() is %zu", what, sum, B.total());
    unsigned char *h = (unsigned char *)malloc(B.total());  // exactly the reported size: one byte more written is a report
    const char *d = (const char *)(uintptr_t)0x7000000000;   // (never dereferenced)
    B.copy_all(h, d);
    CHECK(B.dev_base() == d, "%s: device base", what);
    size_t end = 0;
    for (const Rec &r : recs) {
      unsigned char *hp = (unsigned char *)r.host();
      CHECK(hp == h + r.off, "%s %s: host address", what, r.name);
      CHECK((const char *)r.dev() == d + r.off, "%s %s: device address", what, r.name);
      CHECK(r.off % 16 == 0, "%s %s: offset %zu is not a multiple of 16", what, r.name, r.off);
      CHECK(r.off >= end, "%s %s: overlaps the array in front (starts at %zu, that one ends at %zu)", what, r.name, r.off, end);
      end = r.off + r.room;
      CHECK(end <= B.total(), "%s %s: ends at %zu past the block (%zu)", what, r.name, end, B.total());
      if (r.filled_by_caller)
        for (size_t i = 0; i < r.bytes; ++i) hp[i] = r.want[i];
    }
    for (const Rec &r : recs) {  // (after every write: a later array that ran into an earlier one shows here)
      const unsigned char *hp = (const unsigned char *)r.host();
      size_t bad = 0;
      for (size_t i = 0; i < r.bytes; ++i) bad += hp[i] != r.want[i];
      CHECK(bad == 0, "%s %s: %zu of %zu bytes differ", what, r.name, bad, r.bytes);
    }
    free(h);
  }
};

// the order of stage_inputs (jacobian_api.hip); opt: res_R / res_p, the riders, res_Q / res_clone, the speculative arrays
static void point_batch(bool opt, size_t N, size_t F, size_t nobs, size_t k) {
  Batch b;
  b.put<1, double>("clone_time", N, true), b.put<9, double>("clone_R", N, true), b.put<3, double>("clone_p", N, true);
  b.put<9, double>("clone_R_fej", N, true), b.put<3, double>("clone_p_fej", N, true), b.put<1, int>("clone_col", N, true, 0, true);
  b.put<1, int>("obs_ptr", F + 1, true);
  const size_t in_front = b.B.total();
  const auto of = b.put<1, int>("obs_feat", nobs, true, 0, true);
  CHECK(b.B.offset(of) == in_front, "obs_feat sits at %zu, the arrays in front take %zu", b.B.offset(of), in_front);
  b.put<1, double>("obs_time", nobs, true), b.put<2, float>("obs_uv", nobs, true);
  b.put<3, double>("p_FinG", F, true), b.put<3, double>("p_FinG_fej", F, true);
  b.put<9, double>("res_R", nobs, opt), b.put<3, double>("res_p", nobs, opt);
  b.put<1, int>("cols", k, true);
  b.put<2, float>("uvn", nobs, opt), b.put<1, uint8_t>("flags", F, opt);
  b.put<36, double>("res_Q", nobs, opt), b.put<1, int>("res_clone", nobs, opt);
  b.put<1, int>("spec_li", F, opt), b.put<1, uint8_t>("spec_meta", F, opt), b.put<1, uint8_t>("spec_prevalid", F, opt);
  b.put<1, int>("obs_end", F, opt);
  b.pack_and_check(opt ? "points, every optional array" : "points, no optional array");
}

// the order of stage_line_inputs; opt: seg_uvn .. has_pt, res_*, the flags, the second state's poses, the chained launch's arrays
static void line_batch(bool opt, size_t N, size_t L, size_t nobs, size_t k, size_t n_anc) {
  Batch b;
  b.put<1, double>("clone_time", N, true), b.put<9, double>("clone_R", N, true), b.put<3, double>("clone_p", N, true);
  b.put<9, double>("clone_R_fej", N, true), b.put<3, double>("clone_p_fej", N, true), b.put<1, int>("clone_col", N, true, 0, true);
  b.put<1, int>("obs_ptr", L + 1, true), b.put<1, double>("obs_time", nobs, true), b.put<4, float>("seg_uv", nobs, true);
  b.put<4, float>("seg_uvn", nobs, opt), b.put<6, double>("line_FinG", L, opt), b.put<1, int>("D", L, opt);
  b.put<3, double>("anchor_pt", L, opt), b.put<1, uint8_t>("has_pt", L, opt);
  b.put<9, double>("res_R", nobs, opt), b.put<3, double>("res_p", nobs, opt);
  b.put<36, double>("res_Q", nobs, opt), b.put<1, int>("res_clone", nobs, opt);
  b.put<1, int>("cols", k, true);
  b.put<1, uint8_t>("flags", L, opt);
  b.put<9, double>("tri clone_R", N, opt), b.put<3, double>("tri clone_p", N, opt);
  b.put<4, double>("chain_q", N, opt), b.put<1, int>("chain_id", N + 3, opt), b.put<1, int>("anc_ptr", L + 1, opt);
  b.put<1, int>("anc_f", n_anc, opt, 1), b.put<1, uint8_t>("anc_has_old", n_anc, opt, 4), b.put<3, double>("anc_old", n_anc, opt, 1);
  b.pack_and_check(opt ? "lines, every optional array" : "lines, no optional array");
}

int main() {
  for (int opt = 0; opt < 2; ++opt) {
    point_batch(opt, 11, 37, 401, 98);   // odd counts: every array needs padding
    point_batch(opt, 4, 1, 1, 0);        // the smallest batch, an empty column map (plv_triangulate)
    line_batch(opt, 11, 23, 187, 91, 5);
    line_batch(opt, 4, 1, 1, 0, 0);      // no anchor candidates: the spare values keep the three arrays apart
  }
  {  // more arrays than the block has room for: refused, nothing written out of bounds
    StageBlock B;
    const int v[4] = {1, 2, 3, 4};
    for (int i = 0; i < StageBlock::kMax; ++i) CHECK((bool)B.add(v, 4), "array %d of %d", i, StageBlock::kMax);
    const size_t total = B.total();
    CHECK(!B.overflowed() && total == 16 * (size_t)StageBlock::kMax, "a full block");
    CHECK(!B.add(v, 4) && B.overflowed() && B.total() == total, "one array too many");
  }
  if (fails) return 1;
  printf("ok: stage blocks packed\n");
  return 0;
}
