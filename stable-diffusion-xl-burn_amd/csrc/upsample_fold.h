// Nearest-2x upsample followed by a padded 3x3 convolution, folded into the weights.  Source H x W, output 2H x 2W, weight w[ky][kx], pad 1.
// Output pixel (2i + a, 2j + b) has phase (a, b): its 3x3 window on the upsampled image reads only 2x2 distinct SOURCE pixels, so each phase is
// a 2x2-tap convolution on the source:
//     W_ab[dy][dx] = sum_{ky in R_a(dy)} sum_{kx in R_b(dx)} w[ky][kx],     R_0(0) = {0}, R_0(1) = {1, 2}, R_1(0) = {0, 1}, R_1(1) = {2}
// and tap (dy, dx) reads source pixel (i + dy - 1 + a, j + dx - 1 + b); a pixel outside the source is the padding of the upsampled image, borders
// included.  4/9 of the products of the gather form (IgemmParams::up).  The sums are taken in fp32 in ONE order, ky major, kx minor, starting from
// the first term -- the packing (f16 rounding, or the (hi, lo) split) comes after.
// Plain C++ shared by the device kernel (elementwise.hip), the host entry sdxl_debug_upsample_fold and the stand-alone sanitizer test.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define SDXL_HD __host__ __device__
#else
#define SDXL_HD
#endif

namespace sdxl {

// first tap and number of taps of R_a(d)
SDXL_HD inline int fold_first(int a, int d) { return a == 0 ? (d == 0 ? 0 : 1) : (d == 0 ? 0 : 2); }
SDXL_HD inline int fold_count(int a, int d) { return (a == 0) == (d == 0) ? 1 : 2; }

// W_ab[dy][dx] of one (cout, cin) pair; w9 = its nine taps [ky][kx]
SDXL_HD inline float fold_tap(const float* w9, int a, int b, int dy, int dx) {
  const int y0 = fold_first(a, dy), ny = fold_count(a, dy), x0 = fold_first(b, dx), nx = fold_count(b, dx);
  float acc = w9[y0 * 3 + x0];
  for (int ky = y0; ky < y0 + ny; ++ky)
    for (int kx = x0; kx < x0 + nx; ++kx)
      if (ky != y0 || kx != x0) acc = acc + w9[ky * 3 + kx];
  return acc;
}

// element e of the folded tensor [phase = 2a + b][Cout][Cin][dy][dx] (four canonical 2x2 convolution weights) from w [Cout][Cin][3][3]
SDXL_HD inline float fold_element(const float* w, size_t pairs, size_t e) {
  const size_t ph = e / (pairs * 4), r = e - ph * pairs * 4, pair = r >> 2;
  const int tap = (int)(r & 3);
  return fold_tap(w + pair * 9, (int)(ph >> 1), (int)(ph & 1), tap >> 1, tap & 1);
}

// host form: out [4][Cout][Cin][2][2]
inline void fold_upsample_weights(const float* w, float* out, size_t cout, size_t cin) {
  const size_t pairs = cout * cin;
  for (size_t e = 0; e < 16 * pairs; ++e) out[e] = fold_element(w, pairs, e);
}

}  // namespace sdxl
