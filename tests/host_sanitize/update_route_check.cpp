// The device-free part of the update launch (pl-viwo_amd/csrc/update_route.hpp) on its own, for AddressSanitizer + UBSan: the result
// block's layout against the offset arithmetic it replaced, written through its views into a heap block of exactly the allocated
// size; and the route plan against the conditions plv_msckf_update_resident_launch spelled out before the plan existed (restated
// here as they stood there, not derived from the header), over every combination of the inputs they read.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../pl-viwo_amd/csrc/update_route.hpp"

using namespace plv;

static int fails = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++fails <= 40) {               \
        printf("FAILED %s: ", #cond);    \
        printf(__VA_ARGS__);             \
        printf("\n");                    \
      }                                  \
    }                                    \
  } while (0)

static void layout(int n, int F) {
  const ResultBlock b(n, F);
  const size_t un = (size_t)n, uF = (size_t)F;
  const size_t rows_off = (un * 8 + 16 + uF + 7) & ~(size_t)7, rb = rows_off + uF * 4;
  CHECK(b.dx() == 0 && b.status() == un * 8 && b.head_bytes() == un * 8 + 16 && b.accepted() == un * 8 + 16, "n %d F %d: head", n, F);
  CHECK(b.acc_rows() == rows_off && b.bytes() == rb && b.alloc_bytes() == rb + 16, "n %d F %d: tail", n, F);
  CHECK(b.mirror_bytes() == ((rb + 3) & ~(size_t)3) && b.head_mirror_bytes() == ((un * 8 + 16 + 3) & ~(size_t)3), "n %d F %d: mirrored sizes", n, F);
  CHECK(b.dx() % 8 == 0 && b.status() % 4 == 0 && b.acc_rows() % 4 == 0, "n %d F %d: alignment", n, F);
  // dx | status | accepted | acc_rows, in this order and apart; what is mirrored lies inside the allocation
  CHECK(b.dx() + un * 8 <= b.status() && b.status() + 16 <= b.accepted() && b.accepted() + uF <= b.acc_rows() && b.acc_rows() + uF * 4 <= b.bytes(),
        "n %d F %d: regions overlap", n, F);
  CHECK(b.mirror_bytes() <= b.alloc_bytes() && b.head_mirror_bytes() <= b.alloc_bytes(), "n %d F %d: mirror past the allocation", n, F);

  char *h = (char *)malloc(b.alloc_bytes());  // exactly the allocated size: one byte more written is a report
  memset(h, 0xee, b.alloc_bytes());
  CHECK((char *)b.dx(h) == h && (char *)b.status(h) == h + b.status() && (char *)b.accepted(h) == h + b.accepted() && (char *)b.acc_rows(h) == h + b.acc_rows(),
        "n %d F %d: views", n, F);
  for (int i = 0; i < n; ++i) b.dx(h)[i] = 1000.0 + i;
  for (int i = 0; i < 4; ++i) b.status(h)[i] = -7 - i;
  for (int f = 0; f < F; ++f) b.accepted(h)[f] = (unsigned char)(f * 37 + 1);
  for (int f = 0; f < F; ++f) b.acc_rows(h)[f] = 100000 + f;
  const char *c = h;  // (after every write: a region that ran into another shows here; read through the const views)
  int bad = 0;
  for (int i = 0; i < n; ++i) bad += b.dx(c)[i] != 1000.0 + i;
  for (int i = 0; i < 4; ++i) bad += b.status(c)[i] != -7 - i;
  for (int f = 0; f < F; ++f) bad += b.accepted(c)[f] != (unsigned char)(f * 37 + 1);
  for (int f = 0; f < F; ++f) bad += b.acc_rows(c)[f] != 100000 + f;
  CHECK(bad == 0, "n %d F %d: %d values did not read back", n, F, bad);
  memset(h, 0, b.mirror_bytes());       // ekf_commit_kernel's mirror of the whole block
  memset(h, 0, b.head_mirror_bytes());  // ... and of its head
  free(h);
}

static bool fits(int r) { return r <= 192; }  // dense_kernels.hip: ekf_fast_fits

static long plans() {
  long combos = 0;
  const int ks[3] = {98, 192, 193};
  const int maccs_fixed[4] = {0, 1, 192, 193};
  for (int ik = 0; ik < 3; ++ik) {
    const int k = ks[ik];
    const int mtots[5] = {k - 1, k, k + 1, 192, 193};
    for (int im = 0; im < 5; ++im)
      for (int mp_max = 1; mp_max <= 11; ++mp_max) {
        const int Mtot = mtots[im];
        if (Mtot % mp_max) continue;
        const int F = Mtot / mp_max;
        for (int bits = 0; bits < 256; ++bits) {
          const int compress_mode = bits & 1;
          const bool graph_mode = bits & 2, projected = bits & 4, gathers_valid = bits & 8, prefetched = bits & 16, probe_asked = bits & 32;
          const bool FORCE_FACTOR_FORM = bits & 64, TSQR_TREE = bits & 128;
          UpdateShape s;
          s.F = F, s.fdim = 3, s.k = k, s.ld = mp_max + 3, s.mp_max = mp_max;
          s.compress_mode = compress_mode, s.graph_mode = graph_mode;
          s.projected = projected, s.gathers_valid = gathers_valid, s.prefetched = prefetched, s.probing = probe_asked;
          s.force_factor_form = FORCE_FACTOR_FORM, s.tsqr_tree = TSQR_TREE;
          s.ekf_fast_rows = 192;
          const UpdatePlan p = plan_update(s);
          ++combos;

          // ---- the launch's conditions as they stood
          const int nc = k + 1;
          const bool whiten = Mtot > k && k <= 192 && compress_mode == 0 && !graph_mode;
          const bool probing = probe_asked && !graph_mode;
          const bool start_before = whiten && !prefetched && !probing;
          const int stack_accepted_only = (Mtot > k && k <= 192 && whiten) ? 1 : 0;
          const bool skip = (Mtot > k ? k <= 192 : fits(Mtot));
          size_t tmp_elems = (size_t)std::max(Mtot / (2 * nc) + 2, 16) * nc * nc;
          {
            const size_t nt = (size_t)(nc + 15) / 16, ntri = nt * (nt + 1) / 2;
            tmp_elems = std::max(tmp_elems, (size_t)((Mtot + 63) / 64) * ntri * 256 + (size_t)nc * nc);
          }
          ProjectStep proj = PROJECT_NONE;
          if (!projected) proj = PROJECT_NULLSPACE_AND_GATHERS;
          else if (!gathers_valid) proj = PROJECT_GATHERS_ONLY;

          CHECK(s.Mtot() == Mtot && s.nc() == nc, "shape");
          CHECK(p.whiten == whiten && whitened_route(compress_mode, graph_mode, Mtot, k) == whiten, "whiten: k %d Mtot %d bits %d", k, Mtot, bits);
          CHECK(p.probing == probing && p.prior_before_gate == start_before, "prior before the gate: k %d Mtot %d bits %d", k, Mtot, bits);
          CHECK(p.project == proj, "projection step: bits %d", bits);
          CHECK((int)p.stack_accepted_only == stack_accepted_only, "stack_accepted_only: k %d Mtot %d bits %d", k, Mtot, bits);
          CHECK(p.skip_word == skip, "skip word: k %d Mtot %d bits %d", k, Mtot, bits);
          CHECK(p.tmp_elems == tmp_elems, "tmp_elems: k %d Mtot %d: %zu, was %zu", k, Mtot, p.tmp_elems, tmp_elems);

          // ---- the probe's branch
          for (int ia = 0; ia < 6; ++ia)
            for (int any = 0; any < 2; ++any) {
              const int m_acc = ia < 4 ? maccs_fixed[ia] : ia == 4 ? k : k + 1;
              const TailPlan t = plan_tail(p, any != 0, m_acc);
              ++combos;
              TailKind kind;
              bool prior_now = false;
              if (!any) kind = TAIL_ENDED_AT_GATE;
              else if (whiten && m_acc > 0 && m_acc <= k && fits(m_acc) && !FORCE_FACTOR_FORM) kind = TAIL_DIRECT;
              else {
                kind = TAIL_CHAIN;
                if (whiten && !prefetched) prior_now = true;
              }
              CHECK(t.kind == kind && t.start_prior_now == prior_now, "tail: k %d Mtot %d bits %d any %d m_acc %d", k, Mtot, bits, any, m_acc);
            }

          // ---- the chain
          const bool d_acc_rows = true;  // (the launch always has the rows' array)
          ChainTail tail;
          EkfStep ekf;
          int r, route = 0;
          if (whiten) {
            tail = CHAIN_WHITENED, ekf = EKF_IN_TAIL, r = k, route = 4;
          } else {
            if (Mtot > k) {
              if (projected && d_acc_rows && !TSQR_TREE) tail = CHAIN_HOUSEHOLDER_GATHERED;
              else tail = CHAIN_HOUSEHOLDER;
              r = k;
              route = 2;
            } else {
              tail = CHAIN_STACK_AS_IS;
              r = Mtot;
            }
            ekf = fits(r) ? EKF_FAST : EKF_THEN_COPY;
          }
          const ChainPlan c = plan_chain(p);
          CHECK(c.tail == tail && c.ekf == ekf && c.r == r && (int)c.route == route, "chain: k %d Mtot %d bits %d", k, Mtot, bits);
        }
      }
  }
  return combos;
}

int main() {
  const int ns[7] = {1, 15, 16, 17, 113, 143, 210}, Fs[7] = {0, 1, 7, 8, 9, 70, 250};
  for (int n : ns)
    for (int F : Fs) layout(n, F);
  CHECK(ROUTE_DIRECT == 0 && ROUTE_HOUSEHOLDER == 2 && ROUTE_WHITENED == 4 && ROUTE_WHITENED_REDONE == 5, "route values");
  CHECK(STATUS_NEG_DIAG == 1 && STATUS_S_NOT_PD == 2 && STATUS_WITHHELD == 8 && STATUS_SPEC_OVER_CAP == 16, "status bits");
  for (int flag = 1; flag < 32; ++flag) {  // the three-way text of both error sites
    const char *was = (flag & 16) ? "speculative batch over the selection cap (run again by the caller)" : (flag & 2) ? "S not positive definite" : "negative covariance diagonal";
    CHECK(strcmp(ekf_rejection_text(flag), was) == 0, "rejection text of %d", flag);
  }
  const long combos = plans();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok: update routes, %ld combinations\n", combos);
  return 0;
}
