// front_layout_check.cpp — pl-viwo_amd/csrc/match_block.hpp on its own (plain g++, no HIP header on the include path), under
// AddressSanitizer + UBSan: the temporal matching's block against the offset arithmetic it replaced, every field written and read
// back through the views in a heap block of exactly total() bytes, and pack_rows on sources that end at the last row's last byte.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pl-viwo_amd/csrc/match_block.hpp"

using plv::MatchBlock;

static int fails = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      if (fails++ < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                           \
  } while (0)

static void layout(size_t n) {
  const MatchBlock b(n);
  // the literals of the four functions that addressed the block before
  CHECK(b.o_pts0() == 0 && b.o_pts1() == n * 8 && b.o_n0() == n * 16 && b.o_n1() == n * 24 && b.o_iters() == n * 32);
  CHECK(b.o_mask() == n * 36 && b.o_status() == n * 37 && b.total() == n * 38);
  CHECK(b.mirror_bytes() == n * 36 - n * 8);  // launch_ransac's mir_bytes
  CHECK(b.result_bytes() == n * 37 - n * 8);  // the copy command where no kernel mirrored
  // documented order, each region exactly as long as its field, nothing overlaps and nothing is left over
  const size_t off[8] = {b.o_pts0(), b.o_pts1(), b.o_n0(), b.o_n1(), b.o_iters(), b.o_mask(), b.o_status(), b.total()};
  const size_t len[7] = {8, 8, 8, 8, 4, 1, 1};
  for (int i = 0; i < 7; ++i) CHECK(off[i] + n * len[i] == off[i + 1]);
  CHECK(b.o_pts1() + b.mirror_bytes() == b.o_mask() && b.o_pts1() + b.result_bytes() == b.o_status());
}

static void views(size_t n) {
  char *mem = (char *)malloc(n * 38 ? n * 38 : 1);  // exactly total(): a write past any field is the sanitizer's
  const MatchBlock v(n, mem);
  CHECK((char *)v.pts0() == mem && (char *)v.pts1() == mem + n * 8 && (char *)v.n0() == mem + n * 16 && (char *)v.n1() == mem + n * 24);
  CHECK((char *)v.iters() == mem + n * 32 && (char *)v.mask() == mem + n * 36 && (char *)v.status() == mem + n * 37);
  float *f[4] = {v.pts0(), v.pts1(), v.n0(), v.n1()};
  for (int k = 0; k < 4; ++k)
    for (size_t i = 0; i < 2 * n; ++i) f[k][i] = (float)(1000 * k) + (float)i * 0.5f;
  for (size_t i = 0; i < n; ++i) v.iters()[i] = (int)(7 * i + 3), v.mask()[i] = (uint8_t)(i * 5 + 1), v.status()[i] = (uint8_t)(i * 3 + 2);
  for (int k = 0; k < 4; ++k)
    for (size_t i = 0; i < 2 * n; ++i) CHECK(f[k][i] == (float)(1000 * k) + (float)i * 0.5f);
  for (size_t i = 0; i < n; ++i)
    CHECK(v.iters()[i] == (int)(7 * i + 3) && v.mask()[i] == (uint8_t)(i * 5 + 1) && v.status()[i] == (uint8_t)(i * 3 + 2));
  free(mem);
}

static int pack_cases = 0;
static void pack(int bpp, int pad, int w, int h) {
  const size_t row = (size_t)w * bpp, stride = row + pad;
  const size_t src_len = stride * (h - 1) + row;  // ends at the last row's last byte: the last stride's padding is not there
  uint8_t *src = (uint8_t *)malloc(src_len), *dst = (uint8_t *)malloc(row * h);
  for (size_t i = 0; i < src_len; ++i) src[i] = (uint8_t)(i * 131 + 17);
  plv::pack_rows(dst, src, stride, row, h);
  for (int y = 0; y < h; ++y)
    for (size_t x = 0; x < row; ++x) CHECK(dst[(size_t)y * row + x] == src[(size_t)y * stride + x]);
  free(src), free(dst);
  ++pack_cases;
}

int main() {
  for (size_t n = 0; n <= 4096; ++n) layout(n);
  for (size_t n : {(size_t)4097, (size_t)65535, (size_t)65536, (size_t)100003, (size_t)1 << 19, ((size_t)1 << 20) - 1, (size_t)1 << 20}) layout(n);
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)9, (size_t)10, (size_t)11, (size_t)63, (size_t)64, (size_t)65, (size_t)257, (size_t)4096}) views(n);
  for (int bpp = 1; bpp <= 4; ++bpp)
    for (int pad : {0, 5})
      for (int h : {1, 7}) pack(bpp, pad, 13, h);
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok: matching block and pack_rows, %d row copies\n", pack_cases);
  return 0;
}
