// line_map_kernels.hip — the line map: 3-D end points of triangulated lines (DESIGN.md "The line map").
//
// The reference publishes LineFeature::EndPoints (ROSPublisher.cpp:220-241) but never computes them (LineHelper.cpp:476-493 is
// commented out), so the definition is the library's own: every view's two end-point rays are brought to their closest approach
// with the Pluecker line, which gives the view's extent [lo, hi] along the line's direction; the line's segment is the lower median
// of the lows and of the highs over its (newest 64) views.
//
//   line_segments_kernel   one wave per line, four lines per workgroup, one lane per observation, fp64.  The observation pose is
//                          obs_pose() of the triangulation (obs_pose.hpp); the medians come from a 64-lane bitonic sort on
//                          cross-lane moves (wave_ops.hpp).  No LDS, no scratch.  A handful of lines with a dozen views each: the
//                          launch is latency-sized (one wave's serial depth: a pose, 21 compare-exchange steps), not bandwidth.
#include "line_map_kernels.hpp"

#include "obs_pose.hpp"
#include "wave_ops.hpp"

namespace plv {

#define LSEG_WAVES 4
#define LSEG_INF __longlong_as_double(0x7ff0000000000000LL)

// index of the n-th set bit of m (n < popcount(m))
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int n) {
  for (int i = 0; i < n; ++i) m &= m - 1ull;
  return __ffsll((long long)m) - 1;
}

__global__ void __launch_bounds__(64 * LSEG_WAVES) line_segments_kernel(JacParams P, double *__restrict__ seg /*[L][8]*/, int *__restrict__ views /*[L]*/,
                                                                         unsigned char *__restrict__ ok_g /*[L]*/) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * LSEG_WAVES + (threadIdx.x >> 6);
  if (l >= P.n_feat) return;  // (wave-uniform)
  const int o0 = P.obs_ptr[l], o1 = P.obs_ptr[l + 1];
  // ---- the line: direction, its nearest point to the origin
  const V3 n = ldV(P.line_FinG + 6 * l), v = ldV(P.line_FinG + 6 * l + 3);
  const double vv = dot3(v, v);
  bool line_ok = vv > 0.0 && vv < LSEG_INF;
#pragma unroll
  for (int i = 0; i < 3; ++i) line_ok = line_ok && fabs(n[i]) < LSEG_INF && fabs(v[i]) < LSEG_INF;  // (false for NaN as well)
  const V3 vh = vsc(v, 1.0 / sqrt(vv));
  const V3 p0 = vsc(cross3(v, n), 1.0 / vv);
  // ---- lane j takes the j-th of the newest 64 usable observations (usable: its time has bounding clones; the track is in time order)
  int usable = 0;
  for (int ob = o0; ob < o1; ob += 64) {
    const int o = ob + lane;
    usable += __popcll(__ballot(o < o1 && bounding_start(P, P.obs_time[o] + P.cam_dt) >= 0));
  }
  const int skip = max(usable - 64, 0);
  int mine = -1, seen = 0;
  for (int ob = o0; ob < o1; ob += 64) {
    const int o = ob + lane;
    const unsigned long long m = __ballot(o < o1 && bounding_start(P, P.obs_time[o] + P.cam_dt) >= 0);
    const int cnt = __popcll(m), want = skip + lane - seen;  // (rank of this lane's observation among the chunk's usable ones)
    if (line_ok && want >= 0 && want < cnt) mine = ob + nth_set_bit(m, want);
    seen += cnt;
  }
  // ---- the view's extent along the line
  double lo = LSEG_INF, hi = LSEG_INF;
  bool counted = false;
  if (mine >= 0) {
    M3 R_GtoC;
    V3 c;
    if (obs_pose(P, mine, R_GtoC, c)) {
      const float *u = P.seg_uvn + 4 * (size_t)mine;
      const V3 w = vsub(c, p0);
      const double d = dot3(vh, w);
      const M3 Rt = tp(R_GtoC);
      double s[2];
      bool kept = true;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const V3 e{{(double)u[2 * j], (double)u[2 * j + 1], 1.0}};
        const V3 r = mv(Rt, e);
        const double b = dot3(vh, r), q = dot3(r, r), g = dot3(r, w), den = q - b * b;
        s[j] = (q * d - b * g) / den;
        const double t = (b * d - g) / den;
        kept = kept && !(den < 1e-6 * q) && t > 0.0 && fabs(s[j]) < LSEG_INF;
      }
      if (kept) {
        counted = true;
        lo = s[0] < s[1] ? s[0] : s[1];
        hi = s[0] < s[1] ? s[1] : s[0];
      }
    }
  }
  // ---- lower medians over the counted views: ascending sort over the lanes, the others carry +inf
  const int k = __popcll(__ballot(counted));
  wave_sort2_f64(lo, hi, lane);
  const int at = k > 0 ? (k - 1) / 2 : 0;
  const double lo_m = __hiloint2double(__shfl(__double2hiint(lo), at, 64), __shfl(__double2loint(lo), at, 64));
  const double hi_m = __hiloint2double(__shfl(__double2hiint(hi), at, 64), __shfl(__double2loint(hi), at, 64));
  if (lane < 8) {  // (the component by selects: an index that varies by lane would put the vectors into scratch)
    const int c3 = lane < 3 ? lane : lane - 3;
    const double pc = c3 == 0 ? p0[0] : c3 == 1 ? p0[1] : p0[2], vc = c3 == 0 ? vh[0] : c3 == 1 ? vh[1] : vh[2];
    double out = 0.0;
    if (k > 0) out = lane < 3 ? pc + lo_m * vc : lane < 6 ? pc + hi_m * vc : lane == 6 ? lo_m : hi_m;
    seg[8 * (size_t)l + lane] = out;
  }
  if (lane == 0) {
    views[l] = k;
    ok_g[l] = k > 0;
  }
}

int launch_line_segments(plv_ctx *ctx, const JacParams &P, double *d_seg, int *d_views, unsigned char *d_ok) {
  ProfScope ps(ctx->prof, "line_segments_kernel", ctx->stream);
  hipLaunchKernelGGL(line_segments_kernel, dim3((P.n_feat + LSEG_WAVES - 1) / LSEG_WAVES), dim3(64 * LSEG_WAVES), 0, ctx->stream, P, d_seg, d_views, d_ok);
  PLV_HIP_CHECK(hipGetLastError());
  return PLV_OK;
}

}  // namespace plv
