// line_map_kernels.hpp — launcher of the line map's kernel (line_map_kernels.hip).
#pragma once
#include "jacobian_kernels.hpp"

namespace plv {

// The 3-D end points of every line of P (P.line_FinG, P.obs_ptr / obs_time / seg_uvn, the state's clones): DESIGN.md "The line map".
// Device outputs: seg [L][8] = P1 (3), P2 (3), lo*, hi*; n_views [L]; ok [L].  Stream-ordered on ctx->stream.
int launch_line_segments(plv_ctx *ctx, const JacParams &P, double *d_seg, int *d_views, unsigned char *d_ok);

}  // namespace plv
