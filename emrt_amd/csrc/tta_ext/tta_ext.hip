// libemrt_hip_tta.so: flip and rotation test-time augmentation around the model call of whole-scene inference.  The public
// interface, the variant codes and the contract are described in include/emrt_hip_tta.h.  A library of its own because the ABIs of the other four
// headers are pinned; WindowArgs / fill_windows / EMRT_REQUIRE are ../common.hpp's, the normalisation is ../scene_norm.hpp's (scene.hip's text).
// What this library has in common with mstta_ext/mstta_ext.hip is ../window_variants.hpp's: the variant codes with their validation and decoding,
// the tiles of a launch's bounding box and the tile constants.  The kernels are this file's own; the write-out loop of the crop and the softmax
// of the accumulation are the same text as in that file, and a change to either is made in both.
//
// Two kernels:
//   crop:       a block owns a 32 x 32 tile of one window.  It reads the tile's bytes row by row (each row one contiguous run of at most 96 bytes),
//               normalises them once and keeps the three fp32 planes in LDS, rows padded to 33 words; then it writes the tile into each of the G
//               variants.  For a transposing code the lanes run along the tile's ROWS -- the variant's x -- so the stores stay contiguous and
//               the LDS reads, 33 words apart, fall on different banks.  A scene byte leaves HBM once per window, not G times.
//   accumulate: a block owns a 16 x 16 tile of the scene, a thread one pixel.  Per covering window (in the order given) and per variant (in the
//               order given) it takes the pixel's C logits at the place the inverse transform points to, and adds their softmax to the pixel's
//               sums.  A non-transposing code reads the variant's rows directly (reversed where flipped); a transposing one is staged through
//               LDS, eight classes at a time, by a second thread mapping whose lanes run along the scene's y, the variant's x.  C <= 8 (the
//               shipped datasets) keeps logits and sums in registers and reads every logit once; a larger C makes the three passes of
//               softmax_nchw_acc_kernel (spatial.hip) over chunks of eight classes and adds to `final` in place.  Either way the terms are
//               added to the value `final` held one after the other by the one thread that owns the pixel: no atomics, the same bits in every run.
#include "../common.hpp"
#include "../scene_norm.hpp"
#include "../window_variants.hpp"
#include "../../../include/emrt_hip_tta.h"

thread_local char emrt::g_err[512] = {0};      // this library's own message (EMRT_REQUIRE / check_launch write it): emrt_tta_last_error

namespace emrt {
namespace {

// -> null, or why the codes (HOST int[G]) are refused for n windows of ch x cw
const char* fill_codes(VariantCodes& k, const int* codes, int G, int n, int ch, int cw) {
  const char* why = check_variant_counts(G, n);
  return why ? why : fill_variant_codes(k, codes, G, ch, cw);
}

// ---- crop ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tta_crop_windows_kernel(const unsigned char* __restrict__ scene, float* __restrict__ batch, WindowArgs a, VariantCodes k,
                                                               SceneNorm nm) {
  __shared__ float s[3 * CPLANE];
  const int tiles_x = (a.cw + CT - 1) / CT;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, j = blockIdx.y;
  const int tx0 = tx * CT, ty0 = ty * CT;
  const int tw = min(CT, a.cw - tx0), th = min(CT, a.ch - ty0);
  const int rowb = tw * 3;
  const unsigned char* sp = scene + ((long long)(a.y0[j] + ty0) * a.W + a.x0[j] + tx0) * 3;
  for (int i = threadIdx.x; i < th * rowb; i += 256) {
    const int r = i / rowb, b = i - r * rowb, px = b / 3, c = b - 3 * px;
    const double mean = c == 0 ? nm.mean[0] : (c == 1 ? nm.mean[1] : nm.mean[2]);
    const double stdinv = c == 0 ? nm.stdinv[0] : (c == 1 ? nm.stdinv[1] : nm.stdinv[2]);
    s[c * CPLANE + r * CROW + px] = normalise_u8(sp[(long long)r * a.W * 3 + b], mean, stdinv);
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
constexpr int AROW = AT + 1;                 // words per row of the LDS stage of a transposing code

template <bool SMALL>
__global__ __launch_bounds__(256) void tta_window_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ final,
                                                                    float* __restrict__ count, WindowArgs a, VariantCodes k, BoxTiles tl) {
  __shared__ float s[ACH * AT * AROW];
  const int by = blockIdx.x / tl.nx, bx = blockIdx.x - by * tl.nx;
  const int tx0 = tl.x0 + bx * AT, ty0 = tl.y0 + by * AT;
  const int lx = threadIdx.x & (AT - 1), ly = threadIdx.x / AT;
  const int x = tx0 + lx, y = ty0 + ly;          // the pixel this thread owns
  const int x2 = tx0 + ly, y2 = ty0 + lx;        // the pixel it fetches for a transposing code: lanes along y
  const bool inside = x < a.W && y < a.H, inside2 = x2 < a.W && y2 < a.H;
  const long long HW = (long long)a.H * a.W, plane = (long long)a.ch * a.cw;
  float* fp = final + (long long)y * a.W + x;
  float acc[ACH];
  if constexpr (SMALL) {
#pragma unroll
    for (int c = 0; c < ACH; ++c) acc[c] = (inside && c < a.C) ? fp[c * HW] : 0.f;
  }
  float hits = 0.f;
  for (int j = 0; j < a.n; ++j) {
    const int wy = a.y0[j], wx = a.x0[j];
    if (ty0 + AT <= wy || ty0 >= wy + a.ch || tx0 + AT <= wx || tx0 >= wx + a.cw) continue;      // (the same for the whole block)
    const int yy = y - wy, xx = x - wx, yy2 = y2 - wy, xx2 = x2 - wx;
    const bool cov = inside && (unsigned)yy < (unsigned)a.ch && (unsigned)xx < (unsigned)a.cw;
    const bool cov2 = inside2 && (unsigned)yy2 < (unsigned)a.ch && (unsigned)xx2 < (unsigned)a.cw;
    if (cov) hits += (float)k.G;
    for (int g = 0; g < k.G; ++g) {
      const int code = k.code[g];      // (decoded in place: through decode_variant() this kernel's registers are allocated differently)
      const bool t = (code & 4) != 0, fv = (code & 2) != 0, fh = (code & 1) != 0;
      const float* lp = logits + (long long)(j * k.G + g) * a.C * plane;
      // the inverse of the variant: window pixel (yy, xx) is the variant's (fy, fx), or (fx, fy) when it is transposed
      const long long off = (long long)(fv ? a.ch - 1 - yy : yy) * a.cw + (fh ? a.cw - 1 - xx : xx);
      const long long off2 = (long long)(fh ? a.cw - 1 - xx2 : xx2) * a.cw + (fv ? a.ch - 1 - yy2 : yy2);
      // the logits of classes c0 .. c0 + 7 of the owned pixel (called by every thread of the block: a transposing code goes through LDS)
      auto load = [&](int c0, float (&v)[ACH]) {
        if (t) {
          __syncthreads();      // the chunk before this one has been read
#pragma unroll
          for (int i = 0; i < ACH; ++i)
            if (cov2 && c0 + i < a.C) s[(i * AT + lx) * AROW + ly] = lp[(c0 + i) * plane + off2];
          __syncthreads();
#pragma unroll
          for (int i = 0; i < ACH; ++i) v[i] = s[(i * AT + ly) * AROW + lx];
        } else {
#pragma unroll
          for (int i = 0; i < ACH; ++i) v[i] = (cov && c0 + i < a.C) ? lp[(c0 + i) * plane + off] : 0.f;
        }
      };
      float v[ACH];
      if constexpr (SMALL) {
        load(0, v);
        if (cov) {
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
        }
      } else {
        float mx = 0.f, den = 0.f;
        for (int c0 = 0; c0 < a.C; c0 += ACH) {
          load(c0, v);
          if (cov) {
#pragma unroll
            for (int i = 0; i < ACH; ++i)
              if (c0 + i < a.C) mx = (c0 + i == 0) ? v[0] : fmaxf(mx, v[i]);
          }
        }
        for (int c0 = 0; c0 < a.C; c0 += ACH) {
          load(c0, v);
          if (cov) {
#pragma unroll
            for (int i = 0; i < ACH; ++i)
              if (c0 + i < a.C) den += expf(v[i] - mx);
          }
        }
        const float inv = 1.f / den;
        for (int c0 = 0; c0 < a.C; c0 += ACH) {
          load(c0, v);
          if (cov) {
#pragma unroll
            for (int i = 0; i < ACH; ++i)
              if (c0 + i < a.C) fp[(c0 + i) * HW] += expf(v[i] - mx) * inv;
          }
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

extern "C" const char* emrt_tta_last_error(void) { return g_err; }

extern "C" int emrt_tta_version(void) { return 1; }

extern "C" int emrt_tta_crop_windows_u8(const unsigned char* scene, float* batch, const int* origins_yx /*host, [n][2]*/, int n, const int* codes /*host, [G]*/,
                                        int G, int H, int W, int ch, int cw, double mean0, double mean1, double mean2, double stdinv0, double stdinv1,
                                        double stdinv2, void* stream) {
  EMRT_REQUIRE(scene && batch && origins_yx && codes, "null pointer");
  EMRT_REQUIRE(H >= 1 && W >= 1 && ch >= 1 && cw >= 1, "H, W, ch, cw must be positive");
  VariantCodes k;
  const char* why = fill_codes(k, codes, G, n, ch, cw);
  EMRT_REQUIRE(!why, why);
  WindowArgs a;
  EMRT_REQUIRE(fill_windows(a, origins_yx, n, 3, H, W, ch, cw) == 0, "1..64 windows inside the image");
  const SceneNorm nm = {{mean0, mean1, mean2}, {stdinv0, stdinv1, stdinv2}};
  const long long tiles = (long long)((cw + CT - 1) / CT) * ((ch + CT - 1) / CT);
  EMRT_REQUIRE(tiles < (1ll << 31), "the window is too large");
  hipLaunchKernelGGL(tta_crop_windows_kernel, dim3((unsigned)tiles, n), dim3(256), 0, (hipStream_t)stream, scene, batch, a, k, nm);
  return check_launch("emrt_tta_crop_windows_u8");
}

extern "C" int emrt_tta_window_accumulate(const float* logits, float* final, float* count, const int* origins_yx /*host, [n][2]*/, int n,
                                          const int* codes /*host, [G]*/, int G, int C, int H, int W, int ch, int cw, void* stream) {
  EMRT_REQUIRE(logits && final && count && origins_yx && codes, "null pointer");
  EMRT_REQUIRE(C >= 1 && C <= EMRT_TTA_MAX_CLASSES, "C must be 1..256");
  EMRT_REQUIRE(H >= 1 && W >= 1 && ch >= 1 && cw >= 1, "H, W, ch, cw must be positive");
  VariantCodes k;
  const char* why = fill_codes(k, codes, G, n, ch, cw);
  EMRT_REQUIRE(!why, why);
  WindowArgs a;
  EMRT_REQUIRE(fill_windows(a, origins_yx, n, C, H, W, ch, cw) == 0, "1..64 windows inside the image");
  // the tiles of the windows' bounding box: the rest of the scene is not touched by this launch
  BoxTiles tl;
  const long long tiles = fill_box_tiles(tl, a.y0, a.x0, n, ch, cw);
  EMRT_REQUIRE(tiles < (1ll << 31), "the windows span too many tiles");
  if (C <= ACH)
    hipLaunchKernelGGL(tta_window_accumulate_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, logits, final, count, a, k, tl);
  else
    hipLaunchKernelGGL(tta_window_accumulate_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, logits, final, count, a, k, tl);
  return check_launch("emrt_tta_window_accumulate");
}
