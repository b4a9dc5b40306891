// libemrt_hip_mstta.so: multi-scale test-time augmentation around the model call of whole-scene inference: scale as one more
// axis of tta_ext's window-level augmentation.  The public interface, the resampling rule and the contract are described in
// include/emrt_hip_mstta.h.  A library of its own because the ABIs of the other five headers are pinned; EMRT_REQUIRE / check_launch are
// ../common.hpp's, the normalisation is ../scene_norm.hpp's.  What this library has in common with tta_ext/tta_ext.hip is
// ../window_variants.hpp's: the variant codes with their validation and decoding, the tiles of a launch's bounding box and the tile
// constants.  The kernels are this file's own; the write-out loop of the crop and the softmax of the accumulation are the same text as in that
// file, and a change to either is made in both.
//
// Two kernels:
//   crop:       a block owns a 32 x 32 tile of one window.  It works out the taps and weights of the tile's rows and columns once (64 threads),
//               blends the footprint's bytes and normalises each pixel once into the three fp32 planes in LDS, rows padded to 33 words, then
//               writes the tile into each of the G variants exactly as tta_crop_windows_kernel does: lanes along the variant's x, so the
//               stores stay contiguous for every code.  A pixel's taps are read (through the cache) once per window, not once per variant.
//   accumulate: a block owns a 16 x 16 tile of the scene inside the bounding box of the launch's footprints, a thread one native pixel.  Per
//               covering footprint (in the order given) it works out the pixel's four taps in the window once; per variant (in the order
//               given) the taps are mapped through the variant -- nothing is copied -- the C logits are blended and their softmax is added
//               to the pixel's sums.  C <= 8 keeps logits and sums in registers; a larger C makes three passes over chunks of eight classes
//               and adds to `final` in place.  The direct form for every code: a transposing variant is read where it lies.  One thread
//               owns a pixel: no atomics, the same bits in every run.
#include "../common.hpp"
#include "../scene_norm.hpp"
#include "../window_variants.hpp"
#include "../../../include/emrt_hip_mstta.h"

thread_local char emrt::g_err[512] = {0};      // this library's own message (EMRT_REQUIRE / check_launch write it): emrt_mst_last_error

namespace emrt {
namespace {

// n footprints of fh x fw native pixels at (y0, x0), each resampled to / from a window of ch x cw
struct MstArgs {
  int n, C, H, W, fh, fw, ch, cw;
  int y0[EMRT_MST_MAX_IMAGES], x0[EMRT_MST_MAX_IMAGES];
};

// -> null, or why the call is refused (codes: HOST int[G]; origins_yx: HOST int[n][2])
const char* fill_args(MstArgs& a, VariantCodes& k, const int* origins_yx, int n, const int* codes, int G, int C, int H, int W, int fh, int fw, int ch,
                      int cw) {
  if (const char* why = check_variant_counts(G, n)) return why;
  if (H < 1 || W < 1) return "H and W must be positive";
  const int e = EMRT_MST_MAX_EDGE, r = EMRT_MST_MAX_RATIO;
  if (fh < 1 || fh > e || fw < 1 || fw > e || ch < 1 || ch > e || cw < 1 || cw > e) return "fh, fw, ch, cw must be 1..2048";
  if (fh > r * ch || ch > r * fh || fw > r * cw || cw > r * fw) return "a footprint and its window differ by more than 4 times";
  if (const char* why = fill_variant_codes(k, codes, G, ch, cw)) return why;
  a.n = n; a.C = C; a.H = H; a.W = W; a.fh = fh; a.fw = fw; a.ch = ch; a.cw = cw;
  for (int j = 0; j < EMRT_MST_MAX_IMAGES; ++j) a.y0[j] = a.x0[j] = 0;
  for (int j = 0; j < n; ++j) {
    a.y0[j] = origins_yx[2 * j];
    a.x0[j] = origins_yx[2 * j + 1];
    if (a.y0[j] < 0 || a.x0[j] < 0 || a.y0[j] > H - fh || a.x0[j] > W - fw) return "a footprint reaches outside the scene";
  }
  return nullptr;
}

// The resampling rule of the header: output index i of n_out reads source samples i0 and i1 of n_src with weight w on i1.  Every integer is
// below 2^24 (sizes <= 2048), so w is one fp32 rounding; n_src == n_out gives i0 = i, w = 0.
__device__ __forceinline__ void mst_tap(int i, int n_out, int n_src, int& i0, int& i1, float& w) {
  const int num = (2 * i + 1) * n_src - n_out, den = 2 * n_out;
  w = 0.f;
  if (num <= 0) {
    i0 = 0;
  } else {
    i0 = num / den;
    if (i0 >= n_src - 1) i0 = n_src - 1;
    else w = (float)(num - i0 * den) / (float)den;
  }
  i1 = min(i0 + 1, n_src - 1);
}

__device__ __forceinline__ float mst_blend(float a, float b, float c, float d, float wx, float wy) {
  const float top = a + wx * (b - a), bot = c + wx * (d - c);
  return top + wy * (bot - top);
}

// ---- crop ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mst_crop_windows_kernel(const unsigned char* __restrict__ scene, float* __restrict__ batch, MstArgs a, VariantCodes k,
                                                               SceneNorm nm) {
  __shared__ float s[3 * CPLANE];
  __shared__ int t0[2 * CT], t1[2 * CT];      // taps of the tile's rows [0, CT) and columns [CT, 2 CT), in the footprint
  __shared__ float tw_[2 * CT];               // ... and their weights
  const int tiles_x = (a.cw + CT - 1) / CT;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, j = blockIdx.y;
  const int tx0 = tx * CT, ty0 = ty * CT;
  const int tw = min(CT, a.cw - tx0), th = min(CT, a.ch - ty0);
  if (threadIdx.x < 2 * CT) {
    const bool col = threadIdx.x >= CT;
    const int l = threadIdx.x - (col ? CT : 0);
    if (l < (col ? tw : th)) {
      int i0, i1;
      float w;
      if (col) mst_tap(tx0 + l, a.cw, a.fw, i0, i1, w);
      else mst_tap(ty0 + l, a.ch, a.fh, i0, i1, w);
      t0[threadIdx.x] = i0; t1[threadIdx.x] = i1; tw_[threadIdx.x] = w;
    }
  }
  __syncthreads();
  const unsigned char* sp = scene + ((long long)a.y0[j] * a.W + a.x0[j]) * 3;      // the footprint's first byte
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int r = i / tw, px = i - r * tw;
    const unsigned char* r0 = sp + (long long)t0[r] * a.W * 3;
    const unsigned char* r1 = sp + (long long)t1[r] * a.W * 3;
    const int c0 = t0[CT + px] * 3, c1 = t1[CT + px] * 3;
    const float wy = tw_[r], wx = tw_[CT + px];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = mst_blend((float)r0[c0 + c], (float)r0[c1 + c], (float)r1[c0 + c], (float)r1[c1 + c], wx, wy);
      s[c * CPLANE + r * CROW + px] = normalise_f32(v, nm.mean[c], nm.stdinv[c]);
    }
  }
  __syncthreads();
  const long long plane = (long long)a.ch * a.cw;
  for (int g = 0; g < k.G; ++g) {
    const Variant m = decode_variant(k.code[g]);
    const bool t = m.t, fv = m.fv, fh = m.fh;
    float* vb = batch + (long long)(j * k.G + g) * 3 * plane;
    for (int i = threadIdx.x; i < th * tw; i += 256) {
      int r, px;      // the lanes run along the variant's x: the tile's columns, or its rows when the variant is transposed
      if (t) { px = i / th; r = i - px * th; }
      else { r = i / tw; px = i - r * tw; }
      const int sy = ty0 + r, sx = tx0 + px;
      const int fy = fv ? a.ch - 1 - sy : sy, fx = fh ? a.cw - 1 - sx : sx;      // where the pixel lies after the reversals ...
      const long long off = t ? (long long)fx * a.cw + fy : (long long)fy * a.cw + fx;      // ... and after the transposition (ch == cw)
#pragma unroll
      for (int c = 0; c < 3; ++c) vb[c * plane + off] = s[c * CPLANE + r * CROW + px];
    }
  }
}

// ---- accumulate ----------------------------------------------------------------------------------------------------------------------------
template <bool SMALL>
__global__ __launch_bounds__(256) void mst_window_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ final,
                                                                    float* __restrict__ count, MstArgs a, VariantCodes k, BoxTiles tl) {
  const int by = blockIdx.x / tl.nx, bx = blockIdx.x - by * tl.nx;
  const int tx0 = tl.x0 + bx * AT, ty0 = tl.y0 + by * AT;
  const int x = tx0 + (threadIdx.x & (AT - 1)), y = ty0 + threadIdx.x / AT;          // the pixel this thread owns
  const bool inside = x < a.W && y < a.H;
  const long long HW = (long long)a.H * a.W, plane = (long long)a.ch * a.cw;
  float* fp = final + (long long)y * a.W + x;
  float acc[ACH];
  if constexpr (SMALL) {
#pragma unroll
    for (int c = 0; c < ACH; ++c) acc[c] = (inside && c < a.C) ? fp[c * HW] : 0.f;
  }
  float hits = 0.f;
  for (int j = 0; j < a.n; ++j) {
    const int wy0 = a.y0[j], wx0 = a.x0[j];
    if (ty0 + AT <= wy0 || ty0 >= wy0 + a.fh || tx0 + AT <= wx0 || tx0 >= wx0 + a.fw) continue;      // (the same for the whole block)
    const int yy = y - wy0, xx = x - wx0;
    if (!(inside && (unsigned)yy < (unsigned)a.fh && (unsigned)xx < (unsigned)a.fw)) continue;      // no barrier below: a thread may leave
    hits += (float)k.G;
    int cy0, cy1, cx0, cx1;      // the pixel's taps in the ch x cw window
    float wy, wx;
    mst_tap(yy, a.fh, a.ch, cy0, cy1, wy);
    mst_tap(xx, a.fw, a.cw, cx0, cx1, wx);
    for (int g = 0; g < k.G; ++g) {
      const Variant m = decode_variant(k.code[g]);
      const bool t = m.t, fv = m.fv, fh = m.fh;
      const float* lp = logits + (long long)(j * k.G + g) * a.C * plane;
      // the inverse of the variant: window pixel (cy, cx) is the variant's (my, mx), or (mx, my) when it is transposed (ch == cw)
      const int my0 = fv ? a.ch - 1 - cy0 : cy0, my1 = fv ? a.ch - 1 - cy1 : cy1;
      const int mx0 = fh ? a.cw - 1 - cx0 : cx0, mx1 = fh ? a.cw - 1 - cx1 : cx1;
      const int o00 = t ? mx0 * a.cw + my0 : my0 * a.cw + mx0, o01 = t ? mx1 * a.cw + my0 : my0 * a.cw + mx1;
      const int o10 = t ? mx0 * a.cw + my1 : my1 * a.cw + mx0, o11 = t ? mx1 * a.cw + my1 : my1 * a.cw + mx1;
      // the blended logits of classes c0 .. c0 + 7 of the owned pixel
      auto load = [&](int c0, float (&v)[ACH]) {
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
          const float* cp = lp + (c0 + i) * plane;
          v[i] = c0 + i < a.C ? mst_blend(cp[o00], cp[o01], cp[o10], cp[o11], wx, wy) : 0.f;
        }
      };
      float v[ACH];
      if constexpr (SMALL) {
        load(0, v);
        float mx = v[0], den = 0.f;
#pragma unroll
        for (int c = 1; c < ACH; ++c)
          if (c < a.C) mx = fmaxf(mx, v[c]);
#pragma unroll
        for (int c = 0; c < ACH; ++c)
          if (c < a.C) { v[c] = expf(v[c] - mx); den += v[c]; }
        const float inv = 1.f / den;
#pragma unroll
        for (int c = 0; c < ACH; ++c)
          if (c < a.C) acc[c] += v[c] * inv;
      } else {
        float mx = 0.f, den = 0.f;
        for (int c0 = 0; c0 < a.C; c0 += ACH) {
          load(c0, v);
#pragma unroll
          for (int i = 0; i < ACH; ++i)
            if (c0 + i < a.C) mx = (c0 + i == 0) ? v[0] : fmaxf(mx, v[i]);
        }
        for (int c0 = 0; c0 < a.C; c0 += ACH) {
          load(c0, v);
#pragma unroll
          for (int i = 0; i < ACH; ++i)
            if (c0 + i < a.C) den += expf(v[i] - mx);
        }
        const float inv = 1.f / den;
        for (int c0 = 0; c0 < a.C; c0 += ACH) {
          load(c0, v);
#pragma unroll
          for (int i = 0; i < ACH; ++i)
            if (c0 + i < a.C) fp[(c0 + i) * HW] += expf(v[i] - mx) * inv;
        }
      }
    }
  }
  if (hits > 0.f) {
    if constexpr (SMALL) {
#pragma unroll
      for (int c = 0; c < ACH; ++c)
        if (c < a.C) fp[c * HW] = acc[c];
    }
    count[(long long)y * a.W + x] += hits;
  }
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" const char* emrt_mst_last_error(void) { return g_err; }

extern "C" int emrt_mst_version(void) { return 1; }

extern "C" int emrt_mst_crop_windows_u8(const unsigned char* scene, float* batch, const int* origins_yx /*host, [n][2]*/, int n, const int* codes /*host, [G]*/,
                                        int G, int H, int W, int fh, int fw, int ch, int cw, double mean0, double mean1, double mean2, double stdinv0,
                                        double stdinv1, double stdinv2, void* stream) {
  EMRT_REQUIRE(scene && batch && origins_yx && codes, "null pointer");
  MstArgs a;
  VariantCodes k;
  const char* why = fill_args(a, k, origins_yx, n, codes, G, 3, H, W, fh, fw, ch, cw);
  EMRT_REQUIRE(!why, why);
  const SceneNorm nm = {{mean0, mean1, mean2}, {stdinv0, stdinv1, stdinv2}};
  const int tiles = ((cw + CT - 1) / CT) * ((ch + CT - 1) / CT);      // at most 64 x 64
  hipLaunchKernelGGL(mst_crop_windows_kernel, dim3((unsigned)tiles, n), dim3(256), 0, (hipStream_t)stream, scene, batch, a, k, nm);
  return check_launch("emrt_mst_crop_windows_u8");
}

extern "C" int emrt_mst_window_accumulate(const float* logits, float* final, float* count, const int* origins_yx /*host, [n][2]*/, int n,
                                          const int* codes /*host, [G]*/, int G, int C, int H, int W, int fh, int fw, int ch, int cw, void* stream) {
  EMRT_REQUIRE(logits && final && count && origins_yx && codes, "null pointer");
  EMRT_REQUIRE(C >= 1 && C <= EMRT_MST_MAX_CLASSES, "C must be 1..256");
  MstArgs a;
  VariantCodes k;
  const char* why = fill_args(a, k, origins_yx, n, codes, G, C, H, W, fh, fw, ch, cw);
  EMRT_REQUIRE(!why, why);
  // the tiles of the footprints' bounding box: the rest of the scene is not touched by this launch
  BoxTiles tl;
  const long long tiles = fill_box_tiles(tl, a.y0, a.x0, n, fh, fw);
  EMRT_REQUIRE(tiles < (1ll << 31), "the footprints span too many tiles");
  if (C <= ACH)
    hipLaunchKernelGGL(mst_window_accumulate_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, logits, final, count, a, k, tl);
  else
    hipLaunchKernelGGL(mst_window_accumulate_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, logits, final, count, a, k, tl);
  return check_launch("emrt_mst_window_accumulate");
}
