// update_state.hpp — per-ctx state of the update side shared by plv_api.hip and jacobian_api.hip.
#pragma once
#include <chrono>
#include <vector>

#include "gate_stage.hpp"
#include "plv_ctx.hpp"
#include "plv_internal.hpp"
#include "update_kernels.hpp"
#include "update_route.hpp"

namespace plv {
// What the caller of one update launch (update_resident_launch) hands it beyond the staged batch, and what the launch reports back: a
// local of the caller.  probe: the one-submission line update — the launch waits for the gate, reads its verdicts from pinned memory and
// enqueues compression + EKF only when something was accepted; probe_src .. probe_stride_b: the second block the gate's workgroups copy
// (update_kernels.hpp); probe_hook runs right before that wait.
struct UpdateRiders {
  EkfRiders ekf;  // the chain's share (the skip word is the launch's own choice)
  bool probe = false;
  const void *probe_src = nullptr;
  void *probe_dst = nullptr;
  int probe_stride_a = 0, probe_off_b = 0, probe_stride_b = 0;
  void (*probe_hook)(void *) = nullptr;
  void *probe_hook_arg = nullptr;
  // out: ekf_commit_kernel took the second mirror (else the caller enqueues a copy command) / the applied word; the update ended at the gate
  bool mirror2_taken = false, applied_used = false, ended_at_gate = false;
};
}  // namespace plv

struct plv_ctx_update_state {
  plv::DevBuf q95;
  plv::DevBuf result;   // plv::ResultBlock (update_route.hpp)
  plv::DevBuf covck;    // covariance checkpoint
  int covck_n = 0;      // dimension of the checkpointed covariance (a rollback restores it together with the data)
  plv::DevBuf bHf, bHx, bres, brows, bcols, bwork;  // staged feature batch ([Hf|Hx|res] in bHf) + working copy
  plv::DevBuf bcols_l;                               // the line batch's column map (same reason as plv_ctx::d_stack_l)
  plv::DevBuf &bcols_of(int fdim) { return fdim == 6 ? bcols_l : bcols; }
  int bF = 0, bfdim = 0, bk = 0, bld = 0, bmaxrows = 0;
  bool b_on_device_rows = false;  // rows[] produced on the device (plv_build_jacobians_resident)
  bool b_single_use = false;      // batch is rebuilt every frame: consume it in place, no working copy
  bool b_projected = false;       // the batch is already null-space projected (jacobian_nullspace_kernel)
  unsigned long long b_gather_token = 0;  // plv_ctx::gather_stamp right after the gathers that rode on the batch's launch (0: none)
  plv::GateStage b_gate{};        // on: the batch's Jacobian launch ended with this gate (plv_update_gate_prepare); the update launch starts behind it
  std::vector<int> brows_host;
  // measurement compression (plv_update_compression_mode): 0 = whitened update (information matrix + factor of the prior block; no
  // factor of the measurements), 1 = Householder TSQR on the stacked rows; anything else is refused
  int compress_mode = 0;
  int last_route = 0;       // of the last update: plv::UpdateRoute (update_route.hpp)
  int last_ambiguous = 0;   // always 0 (no route is left that counts unresolved pivots); still reported by plv_update_compression_mode
  // Status block of a LINE update (round 4): the chained line launch reads the point update's dx from `result` while its own gate
  // writes verdicts — and a larger line batch may make its block grow — so the two measurement kinds keep separate blocks, each with
  // its own pair of alternating accepted-entry counters.
  plv::DevBuf result_l;
  struct AccWords {
    int word = 2;             // word of the status block the fused gate's next update counts its accepted entries in (1 or 2, alternating)
    const void *z_ptr = nullptr;  // (z_ptr, z_n, z_word): the counter word known to be zero on the stream — the gate of the update before
    int z_n = 0, z_word = 0;      // zeroed it; anything else (first use, the block moved or grew, cov_n changed, a launch declined the gate) is zeroed by a memset
  } acc[2];
  plv::DevBuf &result_of(int fdim) { return fdim == 6 ? result_l : result; }
  AccWords &acc_of(int fdim) { return acc[fdim == 6 ? 1 : 0]; }
  int acc_word_used = 1;   // the word the last launched update's chain read as its skip word (1: chi2_gate_kernel's)
  // A whitened update that comes back rejected (negative diagonal of P', B not positive definite) is not final: its formulas are
  // not the reference's and lose digits elsewhere (dense_kernels.hip "whitened update": eps x how much better than the prior the
  // measurements know a direction — large for the first update after an initialisation).  The stacked rows are still on the device
  // and the update is run again through a Householder compression and the EKF step on R (ROUTE_WHITENED_REDONE) before the verdict is reported.
  struct RedoW {
    bool armed = false;
    int Mtot = 0, k = 0, n = 0, F = 0, mp_max = 0, fdim = 3;
    size_t tmp_elems = 0, rb = 0;
    double *d_dx = nullptr;
    int *d_flag = nullptr, *d_acc_rows = nullptr;
  } redo_w;
  int pending_F = 0;  // features of a launched, not yet collected plv_msckf_update_resident_launch
  bool pending_at_gate = false;  // ... which ended at the gate (UpdateRiders::probe): already synchronised, its result block is complete
  unsigned long long done_stamp = 0;  // plv_ctx::gather_stamp when done_ev was recorded
  hipEvent_t done_ev = nullptr;  // behind the update's last command: the wait does not cover what the caller enqueues after the launch
  // optional hipGraph replay of the update launch sequence (plv_update_graph_mode): key = every pointer / size / scalar a
  // kernel argument is made of; first sight of a key runs eagerly (sizes every buffer), the second captures, later ones replay
  struct GraphKey {
    const void *P, *Hf, *rows, *cols, *result, *hpin;
    const void *m2_src, *m2_dst, *skip;  // the second mirror block of ekf_commit_kernel and the skip word are kernel arguments too
    size_t m2_bytes;
    int F, fdim, k, ld, n, mp_max;
    double s2, cm, rg;
    unsigned long long epoch;
    bool operator==(const GraphKey &o) const {
      return P == o.P && Hf == o.Hf && rows == o.rows && cols == o.cols && result == o.result && hpin == o.hpin &&
             m2_src == o.m2_src && m2_dst == o.m2_dst && skip == o.skip && m2_bytes == o.m2_bytes && F == o.F &&
             fdim == o.fdim && k == o.k && ld == o.ld && n == o.n && mp_max == o.mp_max && s2 == o.s2 && cm == o.cm && rg == o.rg &&
             epoch == o.epoch;
    }
  };
  bool graph_mode = false, gseen = false;
  GraphKey gkey_seen{}, gkey{};
  hipGraphExec_t gexec = nullptr;
  int graph_replays = 0, graph_captures = 0;
  // Staging of a Jacobian batch, one set per measurement kind: packed inputs (device + pinned; the pinned block's upload is not
  // followed by a host sync) and the triangulation results of the one-submission updates.  The line launch of a frame is staged and
  // enqueued while the point update is still running and being collected (plv_camera_try_update's chained line launch), so nothing
  // of the two halves may share a buffer the host writes or reads.
  struct Staging {
    plv::DevBuf jin, tri;
    plv::DevBuf cpi;  // plv::CpiStage: cpi_pose_kernel's poses of the batch's distinct observation times ([n][9], [n][3]; a second set for the lines' triangulation state; ok)
    plv::PinBuf h_jin, h_tri;
    void release() { jin.release(), tri.release(), cpi.release(), h_jin.release(), h_tri.release(); }
  } stg[2];
  Staging &staging_of(int fdim) { return stg[fdim == 6 ? 1 : 0]; }
  plv::DevBuf eval;
  // the landmark passes (slam_pass.hip): what a pass stages once (clone times and first estimates, every landmark's observations and
  // column map), what it stages per landmark (the clone poses and the landmark as they are now), the landmark's system and its result
  struct SlamPass {
    plv::DevBuf stat, dyn, sys, res;
    plv::PinBuf h_stat, h_dyn, h_res;
    void release() { stat.release(), dyn.release(), sys.release(), res.release(), h_stat.release(), h_dyn.release(), h_res.release(); }
  } slam;
  size_t lt_o_lines = 0;  // plv_lines_update_fused_submit -> _finish: where the triangulated lines sit in tri_l, how many
  int lt_L = 0;
  int pending_fdim = 3;  // measurement size of the launched, not yet collected update (selects the pinned result block)
  // where the last fused point launch left its triangulation results on the device (the chained line launch reads its anchors there)
  const double *pt_tri_p = nullptr;
  const unsigned char *pt_tri_ok = nullptr;
  int pt_tri_F = 0;
  plv::DevBuf chain_words;      // home of applied_word [0] and of the speculative batch's save word [1]
  // the covariance as the last speculative point batch found it (ekf_commit_kernel, plv::CovSave), valid when the save word holds
  // spec_save_seq; spec_save_seq = 0: no batch is waiting to be used or undone
  plv::DevBuf spec_save;
  unsigned spec_save_seq = 0, spec_save_count = 0;
  int spec_save_n = 0;
  int *applied_word = nullptr;  // device word ekf_commit_kernel sets to 1 when the point update changed the state (0: dx is not to be applied)
  bool applied_armed = false;   // ... and the last point launch ended in that kernel with the word as its argument
  hipStream_t spec_stream = nullptr;  // upload of a speculative batch (stage_inputs)
  hipEvent_t spec_ev = nullptr;
  // a submitted point update between plv_points_update_submit and plv_points_update_collect
  struct PointJob {
    bool pending = false, mirrored = false, chain_events = false, spec = false;
    int rc = 0, F = 0, max_sel = 0;
    size_t o_p = 0, o_member = 0, o_words = 0;
    plv::CovSave save;  // a speculative batch: what its launch's commit was handed, and a re-run inside the wait is handed again
    std::chrono::steady_clock::time_point t_entry;
  } point_job;
};
