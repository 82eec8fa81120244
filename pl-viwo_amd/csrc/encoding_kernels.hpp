// encoding_kernels.hpp — launcher of encoding_kernels.hip: a camera image in its sensor encoding (PLV_ENC_*) to the 8-bit grey
// image the front end tracks.
#pragma once
#include "plv_ctx.hpp"

namespace plv {

// bytes per pixel of a PLV_ENC_* value (0: not an encoding)
int encoding_bpp(int encoding);
// `src`: packed rows (w * bpp bytes each), 16-byte aligned, in HBM or — src_pinned — in a page-locked host block the kernel reads
// where it lies; d_dst: w * h grey bytes in HBM, 16-byte aligned.  Enqueued on the ctx stream.
int launch_grey_from_encoded(plv_ctx *ctx, const uint8_t *src, bool src_pinned, uint8_t *d_dst, int w, int h, int encoding);

}  // namespace plv
