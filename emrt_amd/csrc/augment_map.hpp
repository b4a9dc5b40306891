// The per-pixel geometry of the training augmentation, ONE text for both shared libraries: libemrt_hip.so (augment.hip: emrt_augment_tiles,
// emrt_scene_sample) and libemrt_hip_augment.so (augment_ext/augment_ext.hip: the same chain with a vertical flip and colour distortion).
// It covers the coordinates, the bilinear blend, the nearest label and the padding; what follows the map (distortion, normalisation, the
// stores) belongs to the kernel that calls it.  The arithmetic is the numpy chain's, operation for operation:
//   coordinates (float64): sy = max((y + 0.5) * (H / h) - 0.5, 0); y0 = min((long)sy, H - 1); y1 = min(y0 + 1, H - 1); wy = (float)(sy - y0)
//   blend (float32):       top = a00 * (1 - wx) + a01 * wx; bot = a10 * (1 - wx) + a11 * wx; v = top * (1 - wy) + bot * wy
//   label (nearest):       ly = min((long)(y * (H / h)), H - 1)
// A size-equal resize needs no shortcut: H / h == 1 gives sy == y, wy == 0 and v == a00 exactly.
// FMA contraction is off wherever this text is compiled: a fused multiply-add rounds once where numpy rounds twice.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

namespace emrt {

constexpr int AUG_FLIP_H = 1;          // bits of AugView::flip: columns mirrored after the crop
constexpr int AUG_FLIP_V = 2;          // ... rows mirrored after the crop

// One sample's source and decisions as the per-pixel map reads them: img / lab point at the sample's first pixel, `pitch` is the distance
// between two rows in PIXELS (the sample's own W for a packed tile, the scene's W for a window of a scene).
struct AugView {
  const unsigned char* img;
  const unsigned char* lab;
  long long pitch;
  double ry, rx;
  int H, W, h, w, off_y, off_x, flip;
};

// Output pixel (oy, ox) of an OH x OW crop: v = the 3 channels before normalisation, lab = the source's label byte (label_pad outside the resized
// image; read only when want_label).
__device__ __forceinline__ void augment_map(const AugView& s, int OH, int OW, const float (&pad)[3], int label_pad, bool want_label, int oy, int ox,
                                            float (&v)[3], int& lab) {
  const int y = ((s.flip & AUG_FLIP_V) ? OH - 1 - oy : oy) + s.off_y;      // row / column in the padded, resized image
  const int x = ((s.flip & AUG_FLIP_H) ? OW - 1 - ox : ox) + s.off_x;      // the flips follow the crop
  lab = label_pad;
  if (y < s.h && x < s.w) {
    double sy = ((double)y + 0.5) * s.ry - 0.5;
    double sx = ((double)x + 0.5) * s.rx - 0.5;
    sy = sy < 0.0 ? 0.0 : sy;
    sx = sx < 0.0 ? 0.0 : sx;
    const long long y0 = min((long long)sy, (long long)s.H - 1), y1 = min(y0 + 1, (long long)s.H - 1);
    const long long x0 = min((long long)sx, (long long)s.W - 1), x1 = min(x0 + 1, (long long)s.W - 1);
    const float wy = (float)(sy - (double)y0), wx = (float)(sx - (double)x0);
    const unsigned char* r0 = s.img + y0 * s.pitch * 3;
    const unsigned char* r1 = s.img + y1 * s.pitch * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = (float)r0[x0 * 3 + c] * (1.0f - wx) + (float)r0[x1 * 3 + c] * wx;
      const float bot = (float)r1[x0 * 3 + c] * (1.0f - wx) + (float)r1[x1 * 3 + c] * wx;
      v[c] = top * (1.0f - wy) + bot * wy;
    }
    if (want_label) {
      const long long ly = min((long long)((double)y * s.ry), (long long)s.H - 1);
      const long long lx = min((long long)((double)x * s.rx), (long long)s.W - 1);
      lab = s.lab[ly * s.pitch + lx];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = pad[c];
  }
}

}  // namespace emrt
