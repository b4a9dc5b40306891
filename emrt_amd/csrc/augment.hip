// Training augmentation of decoded uint8 tiles: the Potsdam / Vaihingen chain ResizeStepScaling -> RandomPaddingCrop ->
// RandomHorizontalFlip -> Normalize, and LoveDA's Normalize alone (emrt_amd/src/transforms, get_transforms), as ONE launch per batch.
// The host draws every random decision (DevicePlan.plan) and passes them as per-sample descriptors; this file only runs the map.
//
// One thread = one output pixel of one sample: the 3 normalised fp32 channels of out[b][c][oy][ox] and the int64 label.  The arithmetic is
// the numpy chain's, operation for operation, so the result is bit-identical to the CPU transforms:
//   coordinates (float64): sy = max((y + 0.5) * (H / h) - 0.5, 0); y0 = min((long)sy, H - 1); y1 = min(y0 + 1, H - 1); wy = (float)(sy - y0)
//   blend (float32):       top = a00 * (1 - wx) + a01 * wx; bot = a10 * (1 - wx) + a11 * wx; v = top * (1 - wy) + bot * wy
//   label (nearest):       ly = min((long)(y * (H / h)), H - 1)
//   normalise (float64):   (float)(((double)v - mean) * stdinv)
// A size-equal resize needs no shortcut: H / h == 1 gives sy == y, wy == 0 and v == a00 exactly.
// FMA contraction is off for the whole file: a fused multiply-add rounds once where numpy rounds twice.
#pragma clang fp contract(off)
#include "common.hpp"

namespace emrt {
namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_CHUNK = 16;          // samples per launch: descriptors travel in the kernel arguments (AugArgs < 2 KiB)
constexpr int AUG_MAX_SIDE = 1 << 15;  // any source / resized side; keeps every byte count far from overflow

struct AugSample {
  long long img_off, lab_off;          // byte offsets into src
  double ry, rx;                       // H / h, W / w (computed on the host, as Python does)
  int H, W, h, w, off_y, off_x, flip, pad_;
};

struct AugArgs {
  const unsigned char* src;
  float* out;
  long long* labels;                   // nullable
  long long out_bs;
  double mean[3], stdinv[3];
  float pad[3];
  int label_pad;
  int OH, OW, b0;
  unsigned char lut[256];
  AugSample s[AUG_CHUNK];
};

__global__ __launch_bounds__(AUG_THREADS) void emrt_augment_kernel(AugArgs a) {
  const int npix = a.OH * a.OW;
  const int p = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (p >= npix) return;
  const AugSample& s = a.s[blockIdx.y];
  const int oy = p / a.OW, ox = p - oy * a.OW;
  const int y = oy + s.off_y;                                  // row / column in the padded, resized image
  const int x = (s.flip ? a.OW - 1 - ox : ox) + s.off_x;       // the flip follows the crop
  const long long b = a.b0 + blockIdx.y;
  float v[3];
  int lab = a.label_pad;
  if (y < s.h && x < s.w) {
    double sy = ((double)y + 0.5) * s.ry - 0.5;
    double sx = ((double)x + 0.5) * s.rx - 0.5;
    sy = sy < 0.0 ? 0.0 : sy;
    sx = sx < 0.0 ? 0.0 : sx;
    const long long y0 = min((long long)sy, (long long)s.H - 1), y1 = min(y0 + 1, (long long)s.H - 1);
    const long long x0 = min((long long)sx, (long long)s.W - 1), x1 = min(x0 + 1, (long long)s.W - 1);
    const float wy = (float)(sy - (double)y0), wx = (float)(sx - (double)x0);
    const unsigned char* img = a.src + s.img_off;
    const unsigned char* r0 = img + y0 * s.W * 3;
    const unsigned char* r1 = img + y1 * s.W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = (float)r0[x0 * 3 + c] * (1.0f - wx) + (float)r0[x1 * 3 + c] * wx;
      const float bot = (float)r1[x0 * 3 + c] * (1.0f - wx) + (float)r1[x1 * 3 + c] * wx;
      v[c] = top * (1.0f - wy) + bot * wy;
    }
    if (a.labels) {
      const long long ly = min((long long)((double)y * s.ry), (long long)s.H - 1);
      const long long lx = min((long long)((double)x * s.rx), (long long)s.W - 1);
      lab = a.src[s.lab_off + ly * s.W + lx];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = a.pad[c];
  }
  float* o = a.out + b * a.out_bs + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long long)c * npix] = (float)(((double)v[c] - a.mean[c]) * a.stdinv[c]);
  if (a.labels) a.labels[b * npix + p] = a.lut[lab];
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" int emrt_augment_tiles(const void* src, size_t src_bytes, const EmrtAugDesc* descs, int B, int OH, int OW, const double* mean,
                                  const double* stdinv, const float* img_pad, int label_pad, const unsigned char* label_lut, float* out,
                                  long long out_bs, long long* labels, void* stream) {
  EMRT_REQUIRE(src && descs && out && mean && stdinv && img_pad, "null pointer");
  EMRT_REQUIRE(B > 0 && OH > 0 && OW > 0 && OH <= AUG_MAX_SIDE && OW <= AUG_MAX_SIDE, "B, OH and OW must be positive (OH, OW <= 32768)");
  EMRT_REQUIRE((long long)OH * OW < (1ll << 31) / 4, "crop too large");
  EMRT_REQUIRE(out_bs >= 3ll * OH * OW, "out_bs smaller than one [3][OH][OW] image");
  EMRT_REQUIRE(label_pad >= 0 && label_pad <= 255, "label_pad must be 0..255");
  const long long nbytes = (long long)src_bytes;
  EMRT_REQUIRE(nbytes >= 0, "src_bytes too large");
  // every descriptor is checked before the first launch: a bad one is an error, never an out-of-range read
  const char* fn = __func__;
  for (int i = 0; i < B; ++i) {
    const EmrtAugDesc& d = descs[i];
    auto bad = [&](const char* what) {
      char msg[160];
      snprintf(msg, sizeof(msg), "descriptor %d: %s", i, what);
      return fail(fn, msg);
    };
    if (!(d.H > 0 && d.W > 0 && d.h > 0 && d.w > 0)) return bad("sizes must be positive");
    if (d.H > AUG_MAX_SIDE || d.W > AUG_MAX_SIDE || d.h > AUG_MAX_SIDE || d.w > AUG_MAX_SIDE) return bad("side longer than 32768");
    if (d.off_y < 0 || d.off_x < 0 || (long long)d.off_y + OH > (d.h > OH ? d.h : OH) || (long long)d.off_x + OW > (d.w > OW ? d.w : OW))
      return bad("crop outside the padded image");
    if (d.flip != 0 && d.flip != 1) return bad("flip must be 0 or 1");
    const long long hw = (long long)d.H * d.W;
    if (d.img_off < 0 || d.img_off > nbytes - 3 * hw) return bad("image outside the staged buffer");
    if (labels && (d.lab_off < 0 || d.lab_off > nbytes - hw)) return bad("label map outside the staged buffer");
  }
  AugArgs a{};
  a.src = (const unsigned char*)src;
  a.out = out;
  a.labels = labels;
  a.out_bs = out_bs;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean[c];
    a.stdinv[c] = stdinv[c];
    a.pad[c] = img_pad[c];
  }
  a.label_pad = label_pad;
  a.OH = OH;
  a.OW = OW;
  for (int i = 0; i < 256; ++i) a.lut[i] = label_lut ? label_lut[i] : (unsigned char)i;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)((OH * OW + AUG_THREADS - 1) / AUG_THREADS);
  for (int b0 = 0; b0 < B; b0 += AUG_CHUNK) {
    const int nb = B - b0 < AUG_CHUNK ? B - b0 : AUG_CHUNK;
    a.b0 = b0;
    for (int j = 0; j < nb; ++j) {
      const EmrtAugDesc& d = descs[b0 + j];
      AugSample& s = a.s[j];
      s.img_off = d.img_off;
      s.lab_off = labels ? d.lab_off : 0;
      s.ry = (double)d.H / (double)d.h;
      s.rx = (double)d.W / (double)d.w;
      s.H = d.H; s.W = d.W; s.h = d.h; s.w = d.w;
      s.off_y = d.off_y; s.off_x = d.off_x; s.flip = d.flip; s.pad_ = 0;
    }
    hipLaunchKernelGGL(emrt_augment_kernel, dim3(gx, (unsigned)nb), dim3(AUG_THREADS), 0, st, a);
    if (int r = check_launch(__func__)) return r;
  }
  return 0;
}
