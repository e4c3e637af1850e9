// Antialias tap tables of the down_up filter as a device blob (built by lowpass_v2.hip's build_tables_kernel into a buffer
// the caller owns, read by the kernels of lowpass_v2.hip and lowpass_v3.hip).  Blob layout per table: xmin[n_out] | xsize[n_out] | w[n_out][taps] (ints / floats, 4 bytes each).
// Also the two small functions every low-pass file needs: the tap count of a resample and the reflected index of the blur.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace alg {

// taps of one antialiased-bilinear output: the triangle filter's support is max(scale, 1) on either side
__host__ __device__ inline int aa_taps(int in_size, int out_size) {
  float scale = (float)in_size / (float)out_size;
  float support = scale >= 1.0f ? scale : 1.0f;
  return (int)ceilf(support) * 2 + 1;
}

// index i of a reflect-padded axis of n elements (the edge element is not repeated)
__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

namespace v2 {

// ---- tap tables: blob layout per table = xmin[n_out] | xsize[n_out] | w[n_out][taps] (ints / floats, 4 bytes each) --------
struct Tab {
  int off;   // word offset of the table inside the blob
  int n_out, taps;
  __host__ __device__ int words() const { return n_out * (2 + taps); }
};

struct Tabs {
  Tab dw, dh, uw, uh;
  int words;
};

inline Tabs layout(int H, int W, int h1, int w1) {
  Tabs t;
  int o = 0;
  auto mk = [&](int n_out, int in_size) {
    Tab x;
    x.off = o, x.n_out = n_out, x.taps = aa_taps(in_size, n_out);
    o += x.words();
    return x;
  };
  t.dw = mk(w1, W), t.dh = mk(h1, H), t.uw = mk(W, w1), t.uh = mk(H, h1);
  t.words = (o + 3) & ~3;
  return t;
}

}  // namespace v2
}  // namespace alg
