// asin_forms_host_check.cpp — rt_asin (include/rt_pixelmode.h) against a frozen copy of its earlier text, which called
// rt_asin_poly in both arms of `ax < 0.5`: bit patterns must be equal on every input.  Host only, stand-alone;
// tests/test_asin_forms.py builds it with the sanitizers and runs it.  From the repository root:
//   g++ -std=c++17 -O2 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/asin_forms_host_check.cpp -o asin_forms_host_check && ./asin_forms_host_check
// With an argument it writes the 4,096 doubles of its edge and stream inputs to that file (the device comparison of the
// test reads them), followed by rt_asin of each.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "rt_pixelmode.h"

namespace {

// the earlier rt_asin, word for word
double asin_two_arms(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17,
               pio4_hi = 7.85398163397448278999e-01;
  double ax = x < 0.0 ? -x : x;
  if (!(ax <= 1.0)) return rt_u2d(0x7ff8000000000000ull); /* NaN, also for NaN input */
  if (ax == 1.0) return x * pio2_hi + x * pio2_lo;
  if (ax < 0.5) {
    if (ax < 7.450580596923828125e-09) return x; /* 2^-27 */
    return x + x * rt_asin_poly(x * x);
  }
  double w = 1.0 - ax;
  double t = w * 0.5;
  double r = rt_asin_poly(t);
  double s = rt_sqrt_d(t);
  double res;
  if (ax >= 0.975) {
    res = pio2_hi - (2.0 * (s + s * r) - pio2_lo);
  } else {
    double sh = rt_u2d(rt_d2u(s) & 0xffffffff00000000ull);
    double c = (t - sh * sh) / (s + sh);
    double p = 2.0 * s * r - (pio2_lo - 2.0 * c);
    double q = pio4_hi - 2.0 * sh;
    res = pio4_hi - (p - q);
  }
  return x < 0.0 ? -res : res;
}

unsigned long long mismatches = 0, checked = 0;
void check(double x) {
  const uint64_t a = rt_d2u(rt_asin(x)), b = rt_d2u(asin_two_arms(x));
  ++checked;
  if (a != b) {
    if (mismatches < 10) fprintf(stderr, "x = %a (%016llx): %016llx, earlier form %016llx\n", x, (unsigned long long)rt_d2u(x), (unsigned long long)a, (unsigned long long)b);
    ++mismatches;
  }
}
void around(double v, std::vector<double>* keep) {  // v, its 8 neighbours on either side, and their negatives
  const uint64_t u = rt_d2u(v);
  for (int d = -8; d <= 8; ++d) {
    if (d < 0 && u < (uint64_t)-d) continue;
    const double x = rt_u2d(u + (uint64_t)(int64_t)d);
    check(x), check(-x);
    keep->push_back(x), keep->push_back(-x);
  }
}

// minstd_rand0 and libstdc++'s generate_canonical<double>, as the integrator draws (rt_device.h Rng)
struct Engine {
  uint32_t s;
  uint32_t next() {
    uint64_t p = (uint64_t)s * 16807ull;
    uint32_t x = (uint32_t)(p & 0x7fffffffull) + (uint32_t)(p >> 31);
    if (x >= 0x7fffffffu) x -= 0x7fffffffu;
    return s = x;
  }
  double canonD() {
    const double R = 2147483646.0, R2 = 2147483646.0 * 2147483646.0;
    double sum = (double)(next() - 1u);
    sum += (double)(next() - 1u) * R;
    double r = sum / R2;
    return r >= 1.0 ? 0.99999999999999988898 : r;
  }
};

}  // namespace

int main(int argc, char** argv) {
  std::vector<double> keep;
  const double inf = std::numeric_limits<double>::infinity();
  for (const double v : {0.0, 4.9406564584124654e-324 /* the least denormal */, 2.2250738585072009e-308 /* the largest */,
                         2.2250738585072014e-308, 1e-300, 7.450580596923828125e-09 /* 2^-27 */, 0.5, 0.975, 1.0, 1.5, 2.0, 1e300})
    around(v, &keep);
  for (const double v : {inf, -inf, std::numeric_limits<double>::quiet_NaN(), -std::numeric_limits<double>::quiet_NaN(),
                         rt_u2d(0x7ff0000000000001ull), rt_u2d(0xfff8000000000123ull)}) {
    check(v);
    keep.push_back(v);
  }
  // 10^7 seeded doubles in [-1, 1] (splitmix64; 53 bits each)
  uint64_t z = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 10000000; ++i) {
    z += 0x9e3779b97f4a7c15ull;
    const double x = (double)(rt_mix64(z) >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    check(x);
    if (i < 1024) keep.push_back(x);
  }
  // the hemisphere sample's own argument, canonD() * hi, over 10^6 consecutive engine states
  const double hi = (double)(2 * 1.57079637f) / 3.14159265358979323846;
  Engine e{1u};
  for (int i = 0; i < 1000000; ++i) {
    Engine g{e.s};
    const double x = g.canonD() * hi;
    check(x);
    if (i < 1024) keep.push_back(x);
    e.next();
  }
  printf("%llu values, %llu mismatches\n", checked, mismatches);
  if (argc > 1) {
    keep.resize(4096, 0.25);
    std::vector<double> out(keep.size());
    for (size_t i = 0; i < keep.size(); ++i) out[i] = rt_asin(keep[i]);
    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(keep.data(), 8, keep.size(), f) != keep.size() || fwrite(out.data(), 8, out.size(), f) != out.size() || fclose(f)) {
      fprintf(stderr, "cannot write %s\n", argv[1]);
      return 2;
    }
  }
  return mismatches ? 1 : 0;
}
