// The pixel core of the loss kernels: every loss kernel's index split and softmax arithmetic, written once.  loss.hip (libemrt_hip.so) and
// loss_ext/loss_ext.hip (libemrt_hip_loss.so) both compile this text, as the draw kernels share philox.hpp: "pair == two singles",
// "unit weights == plain" and "Dice weight 0 == the Mix loss" hold to the last bit because there is one copy of the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

namespace emrt {

__device__ __forceinline__ void pixel_of(long long idx, long long total, long long HW, long long& n, long long& p) {
  n = total <= 0xffffffffll ? (long long)((unsigned)idx / (unsigned)HW) : idx / HW;      // (32-bit division when it can be)
  p = idx - n * HW;
}

struct PixelStats {
  float mx, den;      // max logit over the classes, sum of exp(logit - max)
};
__device__ __forceinline__ PixelStats pixel_stats(const float* __restrict__ lp, int C, long long HW) {
  PixelStats s;
  s.mx = -3.0e38f;
  for (int c = 0; c < C; ++c) s.mx = fmaxf(s.mx, lp[c * HW]);
  s.den = 0.f;
  for (int c = 0; c < C; ++c) s.den += __expf(lp[c * HW] - s.mx);
  return s;
}
// the pixel's CE; pr = softmax probability of its own class (a label outside [0, C) that is not ignore_index picks logit 0, as it always did)
__device__ __forceinline__ float pixel_ce(const float* __restrict__ lp, int C, long long HW, long long lab, const PixelStats& s, float& pr) {
  const float picked = (lab >= 0 && lab < C) ? lp[lab * HW] : 0.f;
  pr = __expf(picked - s.mx) / s.den;
  // (mx - picked first: it is small and exact for logits of any common offset, where logf(den) + mx rounded at the offset's magnitude -- 3e-5 at 1000)
  return logf(s.den) + (s.mx - picked);
}
__device__ __forceinline__ float pixel_ce(const float* __restrict__ lp, int C, long long HW, long long lab) {
  float pr;
  return pixel_ce(lp, C, HW, lab, pixel_stats(lp, C, HW), pr);
}
// softmax_c of the pixel; inv = 1 / s.den
__device__ __forceinline__ float pixel_softmax(const float* __restrict__ lp, int c, long long HW, const PixelStats& s, float inv) {
  return __expf(lp[c * HW] - s.mx) * inv;
}
// dp[c] = g * (softmax_c - onehot_c)
__device__ __forceinline__ void pixel_grad_store(const float* __restrict__ lp, float* __restrict__ dp, int C, long long HW, long long lab, float g) {
  const PixelStats s = pixel_stats(lp, C, HW);
  const float inv = 1.f / s.den;
  for (int c = 0; c < C; ++c) dp[c * HW] = g * (pixel_softmax(lp, c, HW, s, inv) - (c == lab ? 1.f : 0.f));
}
__device__ __forceinline__ void pixel_zero_store(float* __restrict__ dp, int C, long long HW) {
  for (int c = 0; c < C; ++c) dp[c * HW] = 0.f;
}

// the class weight of a pixel's label: compiled out (1) when CW is false; a label outside [0, C) has weight 0
template <bool CW>
__device__ __forceinline__ float class_weight_of(const float* __restrict__ cw, long long lab, int C) {
  return CW ? ((lab >= 0 && lab < C) ? cw[lab] : 0.f) : 1.f;
}

// grid of a streaming launch: one thread per pixel, capped
inline int stream_grid(long long npix, int cap) {
  long long g = (npix + 255) / 256;
  return (int)(g > cap ? cap : g < 1 ? 1 : g);
}

inline bool shape_ok(int N, int C, int H, int W) { return N >= 1 && C >= 1 && H >= 1 && W >= 1 && (long long)N * H * W < (1ll << 31); }
#define SHAPE_MSG "N, C, H, W >= 1 and N * H * W < 2^31"

}  // namespace emrt
