// so3_check — pl-viwo_amd/csrc/so3.hpp compiled as plain C++ (no HIP headers) and held to recorded bits.
//   so3_check <tests/golden/so3_bits.json>
// The fixture is a JSON list with one record per line: {"fn": name, "in": [hex doubles], "out": [hex doubles]}; the outputs were
// recorded from the copies of these functions the library had before the header existed.  Every record must be reproduced bit for
// bit (any NaN equals any NaN, +0 and -0 differ).  Then, with inputs made here: exp_so3 / log_so3 invert each other on their general
// (trigonometric) branch, and exp_and_Jl equals exp_so3 and Jl_so3 bit for bit everywhere.
// For every jpl_left_update record a line "jpl <13 hex doubles>" (q, R) goes to stdout: the test compares the library's
// plv_jpl_left_update with it.  Build with -ffp-contract=off, like the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../pl-viwo_amd/csrc/so3.hpp"

using namespace plv;

static bool same_bits(double a, double b) {
  if (std::isnan(a) && std::isnan(b)) return true;
  uint64_t x, y;
  memcpy(&x, &a, 8), memcpy(&y, &b, 8);
  return x == y;
}

// the hex doubles between the '[' that follows `key` and its ']'
static std::vector<double> list_of(const std::string &line, const char *key) {
  std::vector<double> v;
  size_t p = line.find(key);
  if (p == std::string::npos) return v;
  p = line.find('[', p);
  const size_t end = line.find(']', p);
  while (true) {
    const size_t a = line.find('"', p);
    if (a == std::string::npos || a > end) break;
    const size_t b = line.find('"', a + 1);
    v.push_back(strtod(line.substr(a + 1, b - a - 1).c_str(), nullptr));
    p = b + 1;
  }
  return v;
}

static int bad = 0;
static void expect(const std::string &what, const double *got, const std::vector<double> &want, int line_no) {
  for (size_t i = 0; i < want.size(); ++i)
    if (!same_bits(got[i], want[i])) {
      if (bad < 20) printf("line %d %s entry %zu: got %a want %a\n", line_no, what.c_str(), i, got[i], want[i]);
      ++bad;
      return;
    }
}
static void expect_same(const char *what, const M3 &a, const M3 &b, const V3 &w) {
  for (int i = 0; i < 9; ++i)
    if (!same_bits(a.m[i], b.m[i])) {
      if (bad < 20) printf("%s differs at entry %d for w = (%a, %a, %a)\n", what, i, w[0], w[1], w[2]);
      ++bad;
      return;
    }
}
static void exp_and_Jl_is_its_two_halves(const V3 &w) {
  M3 R, Jm;
  exp_and_Jl(w, R, Jm);
  expect_same("exp_and_Jl / exp_so3", R, exp_so3(w), w);
  expect_same("exp_and_Jl / Jl_so3", Jm, Jl_so3(w), w);
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line;
  int line_no = 0, n_rec = 0;
  while (std::getline(f, line)) {
    ++line_no;
    const size_t p = line.find("\"fn\": \"");
    if (p == std::string::npos) continue;
    const std::string fn = line.substr(p + 7, line.find('"', p + 7) - p - 7);
    const std::vector<double> in = list_of(line, "\"in\""), want = list_of(line, "\"out\"");
    const double *x = in.data();
    ++n_rec;
    if (fn == "quat_2_Rot" && in.size() == 4 && want.size() == 9) {
      expect(fn, quat_2_Rot(ldQ(x)).m, want, line_no);
    } else if (fn == "rot_2_quat" && in.size() == 9 && want.size() == 4) {
      expect(fn, rot_2_quat(ldM(x)).q, want, line_no);
    } else if (fn == "quat_multiply" && in.size() == 8 && want.size() == 4) {
      expect(fn, quat_multiply(ldQ(x), ldQ(x + 4)).q, want, line_no);
    } else if (fn == "quatnorm" && in.size() == 4 && want.size() == 4) {
      expect(fn, quatnorm(ldQ(x)).q, want, line_no);
    } else if (fn == "omega_times" && in.size() == 7 && want.size() == 4) {
      expect(fn, omega_times(ldV(x), ldQ(x + 3)).q, want, line_no);
    } else if (fn == "jpl_left_update" && in.size() == 7 && want.size() == 13) {
      double out[13], R_only[9];
      jpl_left_update(x, x + 4, out, out + 4);
      expect(fn, out, want, line_no);
      jpl_left_update(x, x + 4, nullptr, R_only);  // (the call a kernel makes)
      expect(fn + " (R alone)", R_only, std::vector<double>(want.begin() + 4, want.end()), line_no);
      printf("jpl");
      for (double v : out) printf(" %a", v);
      printf("\n");
    } else if (fn == "inv3" && in.size() == 9 && want.size() == 9) {
      expect(fn, inv3(ldM(x)).m, want, line_no);
    } else if (fn == "mm" && in.size() == 18 && want.size() == 9) {
      expect(fn, mm(ldM(x), ldM(x + 9)).m, want, line_no);
    } else if (fn == "mv" && in.size() == 12 && want.size() == 3) {
      expect(fn, mv(ldM(x), ldV(x + 9)).v, want, line_no);
    } else if (fn == "exp_so3" && in.size() == 3 && want.size() == 9) {  // (the fixture holds the branches without sin / cos only)
      expect(fn, exp_so3(ldV(x)).m, want, line_no);
      exp_and_Jl_is_its_two_halves(ldV(x));
    } else if (fn == "Jl_so3" && in.size() == 3 && want.size() == 9) {
      expect(fn, Jl_so3(ldV(x)).m, want, line_no);
      exp_and_Jl_is_its_two_halves(ldV(x));
    } else if (fn == "log_so3" && in.size() == 9 && want.size() == 3) {
      expect(fn, log_so3(ldM(x)).v, want, line_no);
    } else {
      printf("line %d: unknown record %s (%zu in, %zu out)\n", line_no, fn.c_str(), in.size(), want.size());
      ++bad;
    }
  }
  if (n_rec < 100) {
    printf("only %d records\n", n_rec);
    return 1;
  }
  // ---- general branch: angles in [0.01, 2.5] rad, away from both ends, where acos and the division by sin(theta) are well conditioned
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto uni = [&]() {  // (0, 1), a 64-bit LCG's top bits
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return ((s >> 11) + 0.5) / 9007199254740992.0;
  };
  double worst_w = 0, worst_R = 0;
  const int n_gen = 400;
  for (int i = 0; i < n_gen; ++i) {
    V3 a{{2 * uni() - 1, 2 * uni() - 1, 2 * uni() - 1}};
    if (vnorm(a) < 0.1) a = V3{{0, 0, 1}};
    const V3 w = vsc(a, (0.01 + 2.49 * uni()) / vnorm(a));
    const M3 R = exp_so3(w);
    const V3 w2 = log_so3(R);
    const M3 R2 = exp_so3(w2);
    for (int k = 0; k < 3; ++k) worst_w = fmax(worst_w, fabs(w2[k] - w[k]));
    for (int k = 0; k < 9; ++k) worst_R = fmax(worst_R, fabs(R2.m[k] - R.m[k]));
    exp_and_Jl_is_its_two_halves(w);
  }
  printf("general branch, %d cases: max |log(exp(w)) - w| = %.3g, max |exp(log(R)) - R| = %.3g\n", n_gen, worst_w, worst_R);
  if (!(worst_w <= 1e-12) || !(worst_R <= 1e-12)) ++bad;
  // ---- exp_and_Jl at the angles where the branches change, and next to pi
  const double PI = 3.14159265358979323846;
  for (double th : {0.0, 1e-8, 0.99e-7, 1e-7, 1.01e-7, 0.99e-6, 1e-6, 1.01e-6, 1e-3, 1.0, PI - 1e-9, PI, 4.0})
    for (const V3 &a : {V3{{1, 0, 0}}, V3{{0, -1, 0}}, V3{{0, 0, 1}}, V3{{0.6, 0, -0.8}}, V3{{-0.2, 0.3, 0.9327379053088815}}}) exp_and_Jl_is_its_two_halves(vsc(a, th));
  if (bad) {
    printf("%d checks failed\n", bad);
    return 1;
  }
  printf("ok: %d records reproduced bit for bit\n", n_rec);
  return 0;
}
