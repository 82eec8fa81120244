// update_route.hpp — the device-free part of the camera update's launch (plv_api.hip: plv_msckf_update_resident_launch / _wait): the
// layout of the result block, the names of routes and status bits, and the route plan as pure functions of the update's shape.
// Plain C++17, no HIP header: tests/host_sanitize/update_route_check.cpp holds all of it to the conditions it replaced.
#pragma once
#include <algorithm>
#include <cstddef>

namespace plv {

// [dx: n doubles][4 status words][accepted: F bytes][pad to 8][acc_rows: F ints] — on the device (update_state.hpp: result /
// result_l) and mirrored to pinned memory.  Status word 0 is the EKF step's flag (UpdateStatusBit), words 1 and 2 count the gate's
// accepted entries (alternating, AccWords), word 3 is spare.
struct ResultBlock {
  int n, F;
  ResultBlock(int n_, int F_) : n(n_), F(F_) {}
  size_t dx() const { return 0; }
  size_t status() const { return (size_t)n * 8; }
  size_t head_bytes() const { return status() + 16; }  // dx + status words: all an update without a gate of its own reads back
  size_t accepted() const { return head_bytes(); }
  size_t acc_rows() const { return (accepted() + (size_t)F + 7) & ~(size_t)7; }
  size_t bytes() const { return acc_rows() + (size_t)F * 4; }  // what is mirrored to pinned memory
  // ekf_commit_kernel mirrors whole words
  size_t mirror_bytes() const { return (bytes() + 3) & ~(size_t)3; }
  size_t head_mirror_bytes() const { return (head_bytes() + 3) & ~(size_t)3; }
  size_t alloc_bytes() const { return bytes() + 16; }

  double *dx(void *b) const { return (double *)((char *)b + dx()); }
  int *status(void *b) const { return (int *)((char *)b + status()); }
  unsigned char *accepted(void *b) const { return (unsigned char *)b + accepted(); }
  int *acc_rows(void *b) const { return (int *)((char *)b + acc_rows()); }
  const double *dx(const void *b) const { return (const double *)((const char *)b + dx()); }
  const int *status(const void *b) const { return (const int *)((const char *)b + status()); }
  const unsigned char *accepted(const void *b) const { return (const unsigned char *)b + accepted(); }
  const int *acc_rows(const void *b) const { return (const int *)((const char *)b + acc_rows()); }
};

// plv_ctx_update_state::last_route, reported by plv_update_compression_mode and counted in plv_route_counts.  The values are part of
// that interface and fixed; 1 and 3 (the Gram + Cholesky compression and its Householder re-run) are retired.  plv_route_counts[6]
// counts the re-runs (ROUTE_WHITENED_REDONE) next to a chained line launch and [7] is the speculation counter: neither is a route.
enum UpdateRoute : int {
  ROUTE_DIRECT = 0,           // no compression: the stack as it is, the gathered accepted rows behind the probe, or nothing to do
  ROUTE_HOUSEHOLDER = 2,      // [R z] by Householder reflections (TSQR), then EKFUpdate
  ROUTE_WHITENED = 4,         // information matrix + factor of the prior block (DESIGN.md "Whitened update")
  ROUTE_WHITENED_REDONE = 5,  // the whitened update came back rejected / withheld and was run again through Householder (RedoW)
};

// status word 0 of the result block, as the kernels of the EKF step set it
enum UpdateStatusBit : int {
  STATUS_NEG_DIAG = 1,       // a diagonal entry of the posterior covariance would be negative
  STATUS_S_NOT_PD = 2,       // S (or B of the whitened form) is not positive definite
  STATUS_WITHHELD = 8,       // the factor form withheld the update (lambda beyond PLV_WHITEN_LAMBDA_MAX): left to the Householder re-run
  STATUS_SPEC_OVER_CAP = 16  // not a rejection: a speculative batch the selection loop's cap would have cut (run again by the caller)
};
inline const char *ekf_rejection_text(int flag) {
  return (flag & STATUS_SPEC_OVER_CAP) ? "speculative batch over the selection cap (run again by the caller)"
         : (flag & STATUS_S_NOT_PD)    ? "S not positive definite"
                                       : "negative covariance diagonal";
}

// columns the whitened route holds (gram_direct_kernel, the blocked factorisation of the prior block)
static const int WHITEN_MAX_COLS = 192;

// Whitened route (compression mode 0, DESIGN.md "Whitened update"): more stacked rows than columns, within its capacity, and not
// under graph replay (its side stream and its host-side re-run do not replay)
inline bool whitened_route(int compress_mode, bool graph_mode, int Mtot, int k) {
  return Mtot > k && k <= WHITEN_MAX_COLS && compress_mode == 0 && !graph_mode;
}

struct UpdateShape {  // everything the route decision reads
  int F = 0, fdim = 0, k = 0, ld = 0, mp_max = 0;
  int compress_mode = 0;
  bool graph_mode = false;
  bool projected = false;      // the batch arrives null-space projected
  bool gathers_valid = false;  // ... and the covariance gathers that rode on its launch still stand
  bool prefetched = false;     // the prior factor is already running on the side stream (plv_prior_prefetch)
  bool probing = false;        // the caller asked for the gate probe (it does not run under graph replay)
  bool force_factor_form = false, tsqr_tree = false;  // PLV_KNOB_FORCE_FACTOR_FORM, PLV_KNOB_TSQR_TREE
  int ekf_fast_rows = 0;       // the most rows ekf_fast_fits() takes (dense_kernels.hip)
  int Mtot() const { return F * mp_max; }
  int nc() const { return k + 1; }
};

enum ProjectStep { PROJECT_NULLSPACE_AND_GATHERS, PROJECT_GATHERS_ONLY, PROJECT_NONE };

struct UpdatePlan {
  UpdateShape s;
  bool whiten = false;
  bool probing = false;            // the host reads the gate's verdicts before it enqueues the tail
  bool prior_before_gate = false;  // a probed update starts the factor only once it knows that it takes the whitened route
  ProjectStep project = PROJECT_NONE;
  // with more rows than columns the stack goes to gram_direct_kernel, which walks the accepted entries only (not on the routes that
  // may hand the whole stack to the Householder compression)
  bool stack_accepted_only = false;
  // only the blocked-Cholesky route honours the skip word in all of its kernels, so the Householder / LDS-resident fallbacks (more
  // than 192 columns, more rows than ekf_fast takes) run unconditionally
  bool skip_word = false;
  size_t tmp_elems = 0;  // scratch of the compression: the larger of the TSQR tree's levels and the Gram path's partial tiles
};

inline UpdatePlan plan_update(const UpdateShape &s) {
  UpdatePlan p;
  p.s = s;
  const int Mtot = s.Mtot(), nc = s.nc();
  p.whiten = whitened_route(s.compress_mode, s.graph_mode, Mtot, s.k);
  p.probing = s.probing && !s.graph_mode;
  p.prior_before_gate = p.whiten && !s.prefetched && !p.probing;
  p.project = !s.projected ? PROJECT_NULLSPACE_AND_GATHERS : !s.gathers_valid ? PROJECT_GATHERS_ONLY : PROJECT_NONE;
  p.stack_accepted_only = p.whiten;
  p.skip_word = Mtot > s.k ? s.k <= WHITEN_MAX_COLS : Mtot <= s.ekf_fast_rows;
  p.tmp_elems = (size_t)std::max(Mtot / (2 * nc) + 2, 16) * nc * nc;  // TSQR tree levels
  // Gram path: per-chunk partial tiles (64-row chunks, upper 16x16 tiles) + the reduced matrix
  const size_t nt = (size_t)(nc + 15) / 16, ntri = nt * (nt + 1) / 2;
  p.tmp_elems = std::max(p.tmp_elems, (size_t)((Mtot + 63) / 64) * ntri * 256 + (size_t)nc * nc);
  return p;
}

// What a probed update does once the host holds the gate's verdicts
enum TailKind {
  TAIL_ENDED_AT_GATE,  // nothing accepted: dx = 0, no further launch
  TAIL_DIRECT,         // no more accepted rows than columns: the reference does not compress (StateHelper.cpp:604-606); the gathered
                       // rows go through EKFUpdate as they are
  TAIL_CHAIN           // the unprobed update's chain (plan_chain)
};
struct TailPlan {
  TailKind kind;
  bool start_prior_now;  // (TAIL_CHAIN) the whitened route's prior factor was held back for the verdicts
};
inline TailPlan plan_tail(const UpdatePlan &p, bool any_accepted, int m_acc) {
  if (!any_accepted) return {TAIL_ENDED_AT_GATE, false};
  if (p.whiten && m_acc > 0 && m_acc <= p.s.k && m_acc <= p.s.ekf_fast_rows && !p.s.force_factor_form) return {TAIL_DIRECT, false};
  return {TAIL_CHAIN, p.whiten && !p.s.prefetched};
}

enum ChainTail {
  CHAIN_WHITENED,              // gram_information + ekf_whitened: carries its own EKF step
  CHAIN_HOUSEHOLDER_GATHERED,  // the accepted rows gathered first, their count left on the device
  CHAIN_HOUSEHOLDER,           // TSQR on the stack as it is
  CHAIN_STACK_AS_IS            // no more rows than columns: nothing to compress
};
enum EkfStep { EKF_IN_TAIL, EKF_FAST, EKF_THEN_COPY };
struct ChainPlan {
  ChainTail tail;
  EkfStep ekf;
  int r;  // rows the EKF step sees
  UpdateRoute route;
};
inline ChainPlan plan_chain(const UpdatePlan &p) {
  const UpdateShape &s = p.s;
  if (p.whiten) return {CHAIN_WHITENED, EKF_IN_TAIL, s.k, ROUTE_WHITENED};
  ChainPlan c;
  if (s.Mtot() > s.k) {
    c.tail = s.projected && !s.tsqr_tree ? CHAIN_HOUSEHOLDER_GATHERED : CHAIN_HOUSEHOLDER;
    c.r = s.k;
    c.route = ROUTE_HOUSEHOLDER;
  } else {
    c.tail = CHAIN_STACK_AS_IS;
    c.r = s.Mtot();
    c.route = ROUTE_DIRECT;
  }
  c.ekf = c.r <= s.ekf_fast_rows ? EKF_FAST : EKF_THEN_COPY;  // (ekf_fast's last kernel mirrors the result block: no copy command)
  return c;
}

}  // namespace plv
