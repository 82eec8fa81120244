// encoding_kernels.hip — gfx950 kernel that turns a camera image in its sensor encoding into the grey image the front end tracks.
//
//   grey_from_encoded_kernel   cv_bridge::toCvShare(msg, MONO8)   REF call site: PL-VIWO/src/core/ROSHelper.cpp:151-173
//                              (cv::cvtColor COLOR_Bayer*2GRAY / COLOR_BGR2GRAY / COLOR_RGB2GRAY and their 4-byte forms)
//
// Arithmetic contract (DESIGN.md "Image encodings"): integers only, the weights R 4899, G 9617, B 1868 over 2^14 —
//   colour  Y = (R wR + G wG + B wB + 2^13) >> 14
//   Bayer   site of colour c in {R, B}, o the other:  (diag4 w[o] + cross4 wG + 4 centre w[c] + 2^15) >> 16
//           site G:  ((left + right) w[colour of left] + (up + down) w[colour of up] + 2 centre wG + 2^14) >> 15
//           rows 0 / H-1 copy rows 1 / H-2, then columns 0 / W-1 copy columns 1 / W-2: every pixel is the interior value of the
//           site its coordinates clamp to ([1, H-2] x [1, W-2])
// which for RGGB is pl-viwo_amd/kaist.py bayer_rg_to_grey bit for bit.  OpenCV's behaviour as recalled, not a pinned oracle.
//
// One kernel family, by encoding class: every lane produces 16 grey pixels and stores them as one 16-byte vector; the source is read
// as 16-byte vectors only (a strip of Bayer rows with its halo rows and the 3- / 4-byte pixels of a chunk go through LDS, so that a
// byte of a source in page-locked host memory crosses PCIe once, halo rows excepted).  Rows are packed (the host side copies a strided image
// into a packed block); an image whose width is no multiple of 16 takes the byte path of the same code.
#include <cstring>

#include "encoding_kernels.hpp"

namespace plv {

namespace {

enum { CLS_COPY = 0, CLS_BAYER = 1, CLS_C3 = 2, CLS_C4 = 3 };
enum { W_R = 4899, W_G = 9617, W_B = 1868 };

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// PINNED: the source is the page-locked host block — every byte is wanted once, the loads leave the caches alone
template <bool PINNED>
__device__ __forceinline__ u32x4 ld16(const uint8_t *p) {
  const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
  if (PINNED) return __builtin_nontemporal_load(q);
  return *q;
}
template <bool PINNED>
__device__ __forceinline__ unsigned ld1(const uint8_t *p) {
  if (PINNED) return __builtin_nontemporal_load(p);
  return *p;
}
__device__ __forceinline__ unsigned byte_of(const u32x4 &q, int i) { return (q[i >> 2] >> ((i & 3) * 8)) & 255u; }

// ------------------------------------------------------------------------------------------ Bayer
// A workgroup of 1024 lanes takes a strip of `rows` output rows over the whole width (1280 x 8: one vector in and one group of 16
// pixels out per lane, so the strip costs one round trip to the source and one pass of arithmetic): the strip's source rows and the row above and
// below it come into LDS as consecutive 16-byte vectors (a row has no halo columns: the border columns are clamped sites), then every
// lane produces groups of 16 pixels of one row.  Whole rows, because a tile's halo columns would each cost a request of their own to
// a source in host memory — as many requests as the tile's body; the halo rows are 2 / rows of the bytes read (rows = 8: a quarter).
// LDS row: [0, 16) unused, [16, 16 + W) the image row, then up to 31 bytes of padding.
constexpr int BAYER_ROWS = 8, BAYER_THREADS = 1024, BAYER_LDS_MAX = 48 * 1024;
__host__ __device__ inline int bayer_pitch(int W) { return ((W + 15) & ~15) + 32; }

// rb: the site is R or B (w_c its weight, w_o the other's); else G with w_c the weight of its left / right neighbours
__device__ __forceinline__ unsigned bayer_site(bool rb, int w_c, int w_o, int c, int horz, int vert, int diag) {
  const int a = rb ? diag : horz, b = rb ? horz + vert : vert;
  const int wa = rb ? w_o : 2 * w_c, wb = rb ? (int)W_G : 2 * w_o, wc = rb ? 4 * w_c : 4 * (int)W_G;
  return (unsigned)((a * wa + b * wb + c * wc + 32768) >> 16);  // (the G form doubled: same quotient)
}

// arg: bits 0-1 the phase (bit 1 = row parity, bit 0 = column parity of the R sites: RGGB 0, GRBG 1, GBRG 2, BGGR 3), bits 8.. the
// strip's rows
template <bool PINNED>
__device__ __forceinline__ void bayer_body(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int W, int H, int arg) {
  extern __shared__ __attribute__((aligned(16))) uint8_t strip[];
  const int tid = threadIdx.x;
  const int phase = arg & 3, rows = arg >> 8;
  const int pitch = bayer_pitch(W);
  const int y0 = blockIdx.x * rows;
  const int yb = min(max(y0, 1), H - 2) - 1;  // image row of LDS row 0: the strip's clamped sites need rows yb .. yb + rows + 1 at most
  const bool vec = (W & 15) == 0;              // rows start on 16-byte boundaries
  if (vec) {
    const int vpr = W >> 4, nv = (rows + 2) * vpr;
#pragma unroll 4
    for (int i = tid; i < nv; i += BAYER_THREADS) {
      const int r = i / vpr, v = i - r * vpr;
      const int yy = min(yb + r, H - 1);
      *reinterpret_cast<u32x4 *>(strip + r * pitch + 16 + v * 16) = ld16<PINNED>(src + (size_t)yy * W + v * 16);
    }
  } else {
    for (int i = tid; i < (rows + 2) * W; i += BAYER_THREADS) {
      const int r = i / W, c = i - r * W;
      const int yy = min(yb + r, H - 1);
      strip[r * pitch + 16 + c] = (uint8_t)ld1<PINNED>(src + (size_t)yy * W + c);
    }
  }
  __syncthreads();

  const int ry = (phase >> 1) & 1, rx = phase & 1;
  const int gpr = (W + 15) >> 4;  // groups of 16 pixels per row
  for (int g = tid; g < rows * gpr; g += BAYER_THREADS) {
    const int ly = g / gpr, xs = (g - ly * gpr) * 16, y = y0 + ly;
    if (y >= H) break;
    const int cy = min(max(y, 1), H - 2);
    const int dy = (cy ^ ry) & 1;  // 0: a row of R sites, 1: a row of B sites
    const int w_c = dy ? (int)W_B : (int)W_R, w_o = dy ? (int)W_R : (int)W_B;
    const uint8_t *row = strip + (cy - yb) * pitch + 16 + xs;  // the lane's 16 sites, centre row
    unsigned o[4] = {0u, 0u, 0u, 0u};
    if (xs >= 1 && xs + 15 <= W - 2) {  // all 16 sites interior columns: three rows of 18 bytes, one 16-byte LDS read each
      int a[3][18];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint8_t *rk = row + (k - 1) * pitch;
        const u32x4 q = *reinterpret_cast<const u32x4 *>(rk);
        a[k][0] = rk[-1];
        a[k][17] = rk[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[k][j + 1] = (int)byte_of(q, j);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool rb = (((j ^ rx) & 1) == dy);  // (xs is even)
        const unsigned v = bayer_site(rb, w_c, w_o, a[1][j + 1], a[1][j] + a[1][j + 2], a[0][j + 1] + a[2][j + 1],
                                      a[0][j] + a[0][j + 2] + a[2][j] + a[2][j + 2]);
        o[j >> 2] |= v << ((j & 3) * 8);
      }
    } else {  // the first and the last group of a row: site by site, columns clamped
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int cx = min(max(xs + j, 1), W - 2);
        const uint8_t *p = row + (cx - xs);
        const uint8_t *pm = p - pitch, *pp = p + pitch;
        const bool rb = (((cx ^ rx) & 1) == dy);
        const unsigned v = bayer_site(rb, w_c, w_o, p[0], p[-1] + p[1], pm[0] + pp[0], pm[-1] + pm[1] + pp[-1] + pp[1]);
        o[j >> 2] |= v << ((j & 3) * 8);
      }
    }
    uint8_t *d = dst + (size_t)y * W + xs;
    if (vec) {  // (the whole group is inside)
      u32x4 q;
      q[0] = o[0], q[1] = o[1], q[2] = o[2], q[3] = o[3];
      *reinterpret_cast<u32x4 *>(d) = q;
    } else {
      const int nvalid = min(16, W - xs);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < nvalid) d[j] = (uint8_t)(o[j >> 2] >> ((j & 3) * 8));
    }
  }
}

// ------------------------------------------------------------------------------------------ 3- and 4-byte colour
// A workgroup of 256 lanes takes a chunk of 4096 pixels (the image is one packed run of pixels): the chunk's bytes come in as
// consecutive 16-byte vectors, lane after lane, into LDS; every lane then reads the 48 / 64 bytes of its own 16 pixels from there.
template <int BPP, bool PINNED>
__device__ __forceinline__ void colour_body(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int npix, int r_first) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[4096 * BPP];
  const int tid = threadIdx.x;
  const size_t nbytes = (size_t)npix * BPP, base = (size_t)blockIdx.x * 4096 * BPP;
#pragma unroll
  for (int k = 0; k < BPP; ++k) {
    const int vi = tid + k * 256;
    const size_t off = base + (size_t)vi * 16;
    if (off + 16 <= nbytes) {
      *reinterpret_cast<u32x4 *>(stage + vi * 16) = ld16<PINNED>(src + off);
    } else if (off < nbytes) {  // the image's last, partial vector
      const int n = (int)(nbytes - off);
      for (int b = 0; b < n; ++b) stage[vi * 16 + b] = (uint8_t)ld1<PINNED>(src + off + b);
    }
  }
  __syncthreads();
  const int p0 = blockIdx.x * 4096 + tid * 16;
  if (p0 >= npix) return;
  u32x4 in[BPP];
#pragma unroll
  for (int k = 0; k < BPP; ++k) in[k] = *reinterpret_cast<const u32x4 *>(stage + tid * 16 * BPP + k * 16);
  unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int b = j * BPP;
    const unsigned c0 = byte_of(in[b >> 4], b & 15), g = byte_of(in[(b + 1) >> 4], (b + 1) & 15), c2 = byte_of(in[(b + 2) >> 4], (b + 2) & 15);
    const unsigned r = r_first ? c0 : c2, bl = r_first ? c2 : c0;
    const unsigned v = (r * (unsigned)W_R + g * (unsigned)W_G + bl * (unsigned)W_B + 8192u) >> 14;
    o[j >> 2] |= v << ((j & 3) * 8);
  }
  uint8_t *d = dst + p0;
  if (p0 + 16 <= npix) {
    u32x4 q;
    q[0] = o[0], q[1] = o[1], q[2] = o[2], q[3] = o[3];
    *reinterpret_cast<u32x4 *>(d) = q;
  } else {
    const int nvalid = npix - p0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < nvalid) d[j] = (uint8_t)(o[j >> 2] >> ((j & 3) * 8));
  }
}

// ------------------------------------------------------------------------------------------ mono8
template <bool PINNED>
__device__ __forceinline__ void copy_body(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int npix) {
  const int nvec = npix >> 4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += gridDim.x * blockDim.x)
    reinterpret_cast<u32x4 *>(dst)[i] = ld16<PINNED>(src + (size_t)i * 16);
  if (blockIdx.x == 0)
    for (int i = (nvec << 4) + threadIdx.x; i < npix; i += blockDim.x) dst[i] = (uint8_t)ld1<PINNED>(src + i);
}

// arg: the Bayer phase (two bits) and the strip's rows / whether the first byte of a colour pixel is R
template <int CLS, bool PINNED>
__global__ void __launch_bounds__(CLS == CLS_BAYER ? BAYER_THREADS : 256) grey_from_encoded_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int W, int H, int arg) {
  if constexpr (CLS == CLS_BAYER)
    bayer_body<PINNED>(src, dst, W, H, arg);
  else if constexpr (CLS == CLS_C3)
    colour_body<3, PINNED>(src, dst, W * H, arg);
  else if constexpr (CLS == CLS_C4)
    colour_body<4, PINNED>(src, dst, W * H, arg);
  else
    copy_body<PINNED>(src, dst, W * H);
}

template <int CLS>
void launch_class(hipStream_t stream, dim3 grid, dim3 block, size_t lds, bool pinned, const uint8_t *src, uint8_t *dst, int w, int h, int arg) {
  if (pinned)
    hipLaunchKernelGGL((grey_from_encoded_kernel<CLS, true>), grid, block, lds, stream, src, dst, w, h, arg);
  else
    hipLaunchKernelGGL((grey_from_encoded_kernel<CLS, false>), grid, block, lds, stream, src, dst, w, h, arg);
}

const char *const kNames[] = {"mono8", "bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8", "bgr8", "rgb8", "bgra8", "rgba8"};

}  // namespace

int encoding_bpp(int encoding) {
  switch (encoding) {
    case PLV_ENC_MONO8:
    case PLV_ENC_BAYER_RGGB8:
    case PLV_ENC_BAYER_BGGR8:
    case PLV_ENC_BAYER_GBRG8:
    case PLV_ENC_BAYER_GRBG8:
      return 1;
    case PLV_ENC_BGR8:
    case PLV_ENC_RGB8:
      return 3;
    case PLV_ENC_BGRA8:
    case PLV_ENC_RGBA8:
      return 4;
    default:
      return 0;
  }
}

int launch_grey_from_encoded(plv_ctx *ctx, const uint8_t *src, bool src_pinned, uint8_t *d_dst, int w, int h, int encoding) {
  const int bpp = encoding_bpp(encoding);
  const bool bayer = encoding >= PLV_ENC_BAYER_RGGB8 && encoding <= PLV_ENC_BAYER_GRBG8;
  if (!src || !d_dst || bpp == 0 || w < 1 || h < 1 || (bayer && (w < 3 || h < 3)) || (long long)w * h * bpp > 0x7fffffffLL) {
    set_last_error("grey_from_encoded: encoding %d, image %d x %d (a Bayer mosaic is 3 x 3 at least)", encoding, w, h);
    return PLV_E_BADARG;
  }
  if (((uintptr_t)src | (uintptr_t)d_dst) & 15) {
    set_last_error("grey_from_encoded: source and destination must lie on 16-byte boundaries");
    return PLV_E_BADARG;
  }
  const int npix = w * h;
  int rows = BAYER_ROWS;  // (a strip of a very wide mosaic has fewer rows: LDS)
  while (bayer && rows > 1 && (rows + 2) * bayer_pitch(w) > BAYER_LDS_MAX) rows >>= 1;
  if (bayer && (rows + 2) * bayer_pitch(w) > BAYER_LDS_MAX) {
    set_last_error("grey_from_encoded: a Bayer mosaic %d pixels wide does not fit the kernel's row strips", w);
    return PLV_E_BADARG;
  }
  ProfScope ps(ctx->prof, "grey_from_encoded_kernel", ctx->stream);
  if (bayer) {
    // the R sites' (row, column) parity: RGGB (0, 0), BGGR (1, 1), GBRG (1, 0), GRBG (0, 1)
    const int phase = encoding == PLV_ENC_BAYER_RGGB8 ? 0 : encoding == PLV_ENC_BAYER_BGGR8 ? 3 : encoding == PLV_ENC_BAYER_GBRG8 ? 2 : 1;
    launch_class<CLS_BAYER>(ctx->stream, dim3((h + rows - 1) / rows), dim3(BAYER_THREADS), (size_t)(rows + 2) * bayer_pitch(w), src_pinned, src, d_dst,
                            w, h, phase | (rows << 8));
  } else if (bpp == 1) {
    const int blocks = std::min(1024, std::max(1, ((npix >> 4) + 255) / 256));
    launch_class<CLS_COPY>(ctx->stream, dim3(blocks), dim3(256), 0, src_pinned, src, d_dst, w, h, 0);
  } else {
    const int r_first = (encoding == PLV_ENC_RGB8 || encoding == PLV_ENC_RGBA8) ? 1 : 0;
    const dim3 grid((npix + 4095) / 4096);
    if (bpp == 3)
      launch_class<CLS_C3>(ctx->stream, grid, dim3(256), 0, src_pinned, src, d_dst, w, h, r_first);
    else
      launch_class<CLS_C4>(ctx->stream, grid, dim3(256), 0, src_pinned, src, d_dst, w, h, r_first);
  }
  PLV_HIP_CHECK(hipGetLastError());
  return PLV_OK;
}

}  // namespace plv

extern "C" {

int plv_encoding_from_name(const char *name) {
  if (!name) return -1;
  for (int i = 0; i < (int)(sizeof(plv::kNames) / sizeof(plv::kNames[0])); ++i)
    if (!strcmp(name, plv::kNames[i])) return i;
  return -1;
}

int plv_encoding_bytes_per_pixel(int encoding) { return plv::encoding_bpp(encoding); }

}  // extern "C"
