// What the two window-level test-time-augmentation libraries share, written once: tta_ext/tta_ext.hip (flips and rotations) and
// mstta_ext/mstta_ext.hip (scale as one more axis) compile this text.  Here are the variant codes, their validation and decoding,
// the tile constants of the two kernels, and the tiles of a launch's bounding box.  The kernels' bodies stay with each library -- how the LDS
// tile is filled (scene_norm.hpp's normalise_u8 of bytes, or normalise_f32 of a four-tap blend) and written out, how a pixel's logits are
// fetched and their softmax added -- as do its argument records, entry points and message.  (The write-out loop and the softmax are the same
// text in both files: as __forceinline__ templates over a caller's load() they compile to other registers and other timings than in place.)
#pragma once
#include <hip/hip_runtime.h>
#include "scene_norm.hpp"      // fills the CT x CT tile that the crop kernels hold in LDS
#include "../../include/emrt_hip_tta.h"
#include "../../include/emrt_hip_mstta.h"

namespace emrt {

static_assert(EMRT_TTA_MAX_VARIANTS == EMRT_MST_MAX_VARIANTS && EMRT_TTA_MAX_IMAGES == EMRT_MST_MAX_IMAGES &&
                  EMRT_TTA_MAX_CLASSES == EMRT_MST_MAX_CLASSES,
              "one record and one set of messages serve both headers' limits");

// ---- variant codes: bit 2 transposes, bit 1 reverses the rows, bit 0 the columns (include/emrt_hip_tta.h) --------------------------------------
struct VariantCodes {
  int G;
  int code[EMRT_TTA_MAX_VARIANTS];
};

// -> null, or why G variants of n windows are refused (checked before a library's own size checks ...)
inline const char* check_variant_counts(int G, int n) {
  if (G < 1 || G > EMRT_TTA_MAX_VARIANTS) return "G must be 1..8";
  if (n < 1 || (long long)n * G > EMRT_TTA_MAX_IMAGES) return "n >= 1 and n * G <= 64";
  return nullptr;
}

// (... and this after them) -> null, or why the codes (HOST int[G], G as checked above) are refused for windows of ch x cw
inline const char* fill_variant_codes(VariantCodes& k, const int* codes, int G, int ch, int cw) {
  k.G = G;
  for (int g = 0; g < EMRT_TTA_MAX_VARIANTS; ++g) k.code[g] = 0;
  for (int g = 0; g < G; ++g) {
    if (codes[g] < 0 || codes[g] > 7) return "codes must be 0..7";
    for (int h = 0; h < g; ++h)
      if (codes[h] == codes[g]) return "a code is repeated";
    if ((codes[g] & 4) && ch != cw) return "a transposing code (4..7) needs ch == cw";
    k.code[g] = codes[g];
  }
  return nullptr;
}

struct Variant {
  bool t, fv, fh;      // transposed, rows reversed, columns reversed
};
__device__ __forceinline__ Variant decode_variant(int code) { return {(code & 4) != 0, (code & 2) != 0, (code & 1) != 0}; }

// ---- crop ----------------------------------------------------------------------------------------------------------------------------------
constexpr int CT = 32;                       // tile edge
constexpr int CROW = CT + 1;                 // words per LDS row: a column walk (33 words apart) touches every bank once
constexpr int CPLANE = CT * CROW + 11;       // words per channel plane; + 11 spreads the three channels of a pixel, stored by neighbouring lanes

// ---- accumulate ----------------------------------------------------------------------------------------------------------------------------
constexpr int AT = 16;                       // tile edge: 256 pixels, one per thread
constexpr int ACH = 8;                       // classes per chunk

struct BoxTiles {
  int x0, y0, nx;                            // the tiles of one launch: origin (a multiple of AT) and tiles per row of the bounding box
};

// -> the number of AT x AT tiles that cover the bounding box of n rectangles of eh x ew at (y0[j], x0[j]) (HOST): a launch touches no other
inline long long fill_box_tiles(BoxTiles& tl, const int* y0, const int* x0, int n, int eh, int ew) {
  int x_lo = x0[0], x_hi = x0[0], y_lo = y0[0], y_hi = y0[0];
  for (int j = 1; j < n; ++j) {
    x_lo = x0[j] < x_lo ? x0[j] : x_lo; x_hi = x0[j] > x_hi ? x0[j] : x_hi;
    y_lo = y0[j] < y_lo ? y0[j] : y_lo; y_hi = y0[j] > y_hi ? y0[j] : y_hi;
  }
  tl.x0 = x_lo / AT * AT;
  tl.y0 = y_lo / AT * AT;
  tl.nx = (x_hi + ew - tl.x0 + AT - 1) / AT;
  return (long long)tl.nx * ((y_hi + eh - tl.y0 + AT - 1) / AT);
}

}  // namespace emrt
