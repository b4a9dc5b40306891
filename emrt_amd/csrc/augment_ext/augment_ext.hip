// libemrt_hip_augment.so: the training augmentation of ../augment.hip extended by RandomVerticalFlip and RandomDistort (brightness, contrast,
// saturation), for packed tiles (emrt_aug_tiles) and for windows of resident scenes with the decisions drawn on the device (emrt_aug_scene_draw,
// emrt_aug_scene_sample).  The public interface and the arithmetic are described in include/emrt_hip_augment.h; the geometry is the text
// ../augment_map.hpp shares with libemrt_hip.so.  A library of its own because the ABI of emrt_hip.h is frozen.
//
// Two kernels, each written once over a "source" (how a block finds its sample: kernel arguments for tiles, the draw table for scenes):
//   statistics: a thread recomputes its output pixels up to the op before contrast and sums their luminance (at most 32 blocks per sample stride
//               over the crop); wave shuffle, LDS across the four waves, ONE 64-bit atomic add per block into sums[b].  Integer sums: the same
//               result from run to run.
//   apply:      geometry, truncation to uint8, the ops in order (the contrast mean from sums[b]), float64 normalisation, stores.
// FMA contraction is off for the whole file: PIL's blend and numpy round twice where a fused multiply-add rounds once.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../../include/emrt_hip_augment.h"
#include "../augment_map.hpp"
#include "../philox.hpp"

namespace emrt {
namespace {

thread_local char g_aug_err[512] = "";

int fail(const char* fn, const char* msg) {
  snprintf(g_aug_err, sizeof(g_aug_err), "%s: %s", fn, msg);
  return -1;
}
int check_launch(const char* fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_aug_err, sizeof(g_aug_err), "%s: launch failed: %s", fn, hipGetErrorString(e));
    return -2;
  }
  return 0;
}
#define AUG_REQUIRE(cond, msg)                 \
  do {                                         \
    if (!(cond)) return fail(__func__, msg);   \
  } while (0)

constexpr int AUG_THREADS = 256;
constexpr int AUG_CHUNK = 16;          // samples per launch: descriptors travel in the kernel arguments
constexpr int AUG_MAX_SIDE = 1 << 15;  // any source / resized side; keeps every byte count far from overflow
constexpr int AUG_MAX_OPS = 3;
constexpr int AUG_STATS_BLOCKS = 32;   // most blocks per sample of the statistics launch: each ends in ONE atomic on the sample's sum, and adds
                                       // of many blocks to one address queue up behind one another
constexpr int SCENE_MAX_SCALES = 16;
constexpr int DRAW_COLS = EMRT_AUG_DRAW_COLS;
constexpr int DRAW_THREADS = 64;

struct AugOps {
  int n;
  int op[AUG_MAX_OPS];
  float f[AUG_MAX_OPS];
};

// What every sample of a batch shares: the outputs and the constants of the chain.
struct AugCommon {
  float* out;
  long long* labels;                   // nullable
  unsigned long long* sums;            // [B] luminance sums (nullable when no sample can apply contrast)
  long long out_bs;
  double mean[3], stdinv[3];
  float pad[3];
  int label_pad;
  int OH, OW;
  int distort;
  unsigned char lut[256];
};

__device__ __forceinline__ int luminance(const int (&x)[3]) { return (x[0] * 19595 + x[1] * 38470 + x[2] * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) on one channel: float32, the product rounded before the sum.
__device__ __forceinline__ int blend(int d, int x, float f) {
  const float t = (float)d + f * (float)(x - d);
  if (f >= 0.0f && f <= 1.0f) return (int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ void apply_op(int (&x)[3], int op, float f, int mean_l) {
  const int l = luminance(x);
  const int d = op == EMRT_AUG_OP_BRIGHTNESS ? 0 : (op == EMRT_AUG_OP_CONTRAST ? mean_l : l);
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = blend(d, x[c], f);
}

__device__ __forceinline__ void quantise(const float (&v)[3], int (&x)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = min(max((int)v[c], 0), 255);      // astype('uint8') of a value in [0, 256): truncation
}

// The ops of a sample up to (not including) position `upto`, in order; mean_l serves contrast.  Written as three unrolled, predicated steps: with
// constant indices o.op / o.f stay in registers (a loop with a run-time bound made the compiler park them in LDS).
__device__ __forceinline__ void apply_ops(int (&x)[3], const AugOps& o, int upto, int mean_l) {
#pragma unroll
  for (int i = 0; i < AUG_MAX_OPS; ++i)
    if (i < upto) apply_op(x, o.op[i], o.f[i], mean_l);
}

// Position of contrast among the sample's ops, -1 if it is not applied.
__device__ __forceinline__ int contrast_at(const AugOps& o) {
  int k = -1;
#pragma unroll
  for (int i = AUG_MAX_OPS - 1; i >= 0; --i)
    if (i < o.n && o.op[i] == EMRT_AUG_OP_CONTRAST) k = i;
  return k;
}

// ---- the two kernels ----------------------------------------------------------------------------------------------------------------------------
template <class Src>
__global__ __launch_bounds__(AUG_THREADS) void aug_stats_kernel(Src a) {
  __shared__ unsigned red[AUG_THREADS / 64];
  AugView s;
  AugOps o;
  long long b;
  a.sample(blockIdx.y, s, o, b);
  const int k = contrast_at(o);        // block-uniform
  if (k < 0) return;
  const AugCommon& c = a.c;
  const int npix = c.OH * c.OW;
  unsigned l = 0;                      // (fewer than 2^29 pixels over 32 blocks of 256: a thread adds < 2^16 values <= 255, a wave sum stays below 2^30)
  for (int p = blockIdx.x * AUG_THREADS + threadIdx.x; p < npix; p += gridDim.x * AUG_THREADS) {
    const int oy = p / c.OW, ox = p - oy * c.OW;
    float v[3];
    int lab, x[3];
    augment_map(s, c.OH, c.OW, c.pad, c.label_pad, false, oy, ox, v, lab);
    quantise(v, x);
    apply_ops(x, o, k, 0);
    l += (unsigned)luminance(x);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = l;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < AUG_THREADS / 64; ++w) t += red[w];
    atomicAdd(c.sums + b, t);
  }
}

template <class Src>
__global__ __launch_bounds__(AUG_THREADS) void aug_apply_kernel(Src a) {
  const AugCommon& c = a.c;
  const int npix = c.OH * c.OW;
  const int p = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (p >= npix) return;
  AugView s;
  AugOps o;
  long long b;
  a.sample(blockIdx.y, s, o, b);
  const int oy = p / c.OW, ox = p - oy * c.OW;
  float v[3];
  int lab;
  augment_map(s, c.OH, c.OW, c.pad, c.label_pad, c.labels != nullptr, oy, ox, v, lab);
  if (c.distort) {
    int x[3];
    quantise(v, x);
    const int mean_l = contrast_at(o) >= 0 ? (int)((double)c.sums[b] / (double)npix + 0.5) : 0;      // block-uniform
    apply_ops(x, o, o.n, mean_l);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (float)x[k];
  }
  float* dst = c.out + b * c.out_bs + p;
#pragma unroll
  for (int k = 0; k < 3; ++k) dst[(long long)k * npix] = (float)(((double)v[k] - c.mean[k]) * c.stdinv[k]);
  if (c.labels) c.labels[b * npix + p] = c.lut[lab];
}

// ---- packed tiles: the decisions ride in the kernel arguments -----------------------------------------------------------------------------------
struct TileSample {
  long long img_off, lab_off;          // byte offsets into src
  double ry, rx;                       // H / h, W / w (computed on the host, as Python does)
  int H, W, h, w, off_y, off_x, flip, n_ops;
  int op[AUG_MAX_OPS];
  float f[AUG_MAX_OPS];
};

struct TileSrc {
  const unsigned char* src;
  AugCommon c;
  int b0;
  TileSample s[AUG_CHUNK];
  __device__ __forceinline__ void sample(int j, AugView& v, AugOps& o, long long& b) const {
    const TileSample& t = s[j];
    v.img = src + t.img_off;
    v.lab = src + t.lab_off;
    v.pitch = t.W;
    v.ry = t.ry; v.rx = t.rx;
    v.H = t.H; v.W = t.W; v.h = t.h; v.w = t.w;
    v.off_y = t.off_y; v.off_x = t.off_x; v.flip = t.flip;
    o.n = t.n_ops;
#pragma unroll
    for (int i = 0; i < AUG_MAX_OPS; ++i) {
      o.op[i] = t.op[i];
      o.f[i] = t.f[i];
    }
    b = (long long)b0 + j;
  }
};

// ---- windows of resident scenes: the decisions come from the draw table -------------------------------------------------------------------------
struct SceneSrc {
  const unsigned char* bank;
  const EmrtSceneEntry* scenes;        // device
  const int* draws;                    // device, [B][DRAW_COLS]
  AugCommon c;
  int n_scenes, th, tw;
  __device__ __forceinline__ void sample(int j, AugView& v, AugOps& o, long long& b) const {
    const int* d = draws + (long long)j * DRAW_COLS;
    // the table is device memory this kernel did not write: every value is brought into its range, so a stale or foreign table reads wrong
    // pixels, never memory outside the bank (rows written by emrt_aug_scene_draw are inside these ranges already and pass unchanged)
    const EmrtSceneEntry e = scenes[min(max(d[0], 0), n_scenes - 1)];
    const int y0 = min(max(d[1], 0), e.H - th), x0 = min(max(d[2], 0), e.W - tw);
    v.H = th; v.W = tw;
    v.h = min(max(d[4], 1), AUG_MAX_SIDE); v.w = min(max(d[5], 1), AUG_MAX_SIDE);
    v.off_y = min(max(d[6], 0), max(v.h, c.OH) - c.OH);
    v.off_x = min(max(d[7], 0), max(v.w, c.OW) - c.OW);
    v.flip = (d[8] != 0 ? AUG_FLIP_H : 0) | (d[9] != 0 ? AUG_FLIP_V : 0);
    v.ry = (double)th / (double)v.h;   // H / h in float64: correctly rounded here as in Python
    v.rx = (double)tw / (double)v.w;
    v.pitch = e.W;
    v.img = bank + e.img_off + ((long long)y0 * e.W + x0) * 3;
    v.lab = bank + e.lab_off + ((long long)y0 * e.W + x0);
    o.n = c.distort ? min(max(d[11], 0), AUG_MAX_OPS) : 0;
#pragma unroll
    for (int i = 0; i < AUG_MAX_OPS; ++i) {
      o.op[i] = min(max(d[12 + i], 0), 2);
      o.f[i] = fminf(fmaxf(__int_as_float(d[15 + i]), 0.0f), 2.0f);      // (fmaxf of a NaN and 0 is 0)
    }
    b = j;
  }
};

// Philox4x32-10, `below` and `unit`: ../philox.hpp, the text ../augment.hip compiles too.
struct DrawArgs {
  const long long* step;               // device: the step counter
  const EmrtSceneEntry* scenes;        // device
  const long long* cum;                // device, [n_scenes + 1], cum[0] = 0
  int* draws;                          // device, [B][DRAW_COLS]
  double prob, vprob;
  double range[3], op_prob[3];
  unsigned k0, k1, first;              // key words; rank * B
  int n_scenes, B, th, tw, OH, OW, n_scales, distort;
  int scale_hw[SCENE_MAX_SCALES][2];
};

__global__ __launch_bounds__(DRAW_THREADS) void aug_scene_draw_kernel(DrawArgs a) {
  const int b = blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (b >= a.B) return;
  const unsigned long long step = (unsigned long long)a.step[0];
  const unsigned s_lo = (unsigned)step, s_hi = (unsigned)(step >> 32), id = a.first + (unsigned)b;
  const Philox r0 = philox4x32_10(s_lo, s_hi, id, 0u, a.k0, a.k1);
  const Philox r1 = philox4x32_10(s_lo, s_hi, id, 1u, a.k0, a.k1);
  const Philox r2 = philox4x32_10(s_lo, s_hi, id, 2u, a.k0, a.k1);
  const Philox r3 = philox4x32_10(s_lo, s_hi, id, 3u, a.k0, a.k1);
  const Philox r4 = philox4x32_10(s_lo, s_hi, id, 4u, a.k0, a.k1);
  const long long g = (long long)below(r0.v[0], r0.v[1], (unsigned long long)a.cum[a.n_scenes]);
  int lo = 0, hi = a.n_scenes - 1;     // the last scene whose first origin is <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.cum[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const long long rem = g - a.cum[lo];
  const long long nx = (long long)a.scenes[lo].W - a.tw + 1;
  const int k = (int)below(r0.v[2], r0.v[3], (unsigned long long)a.n_scales);
  const int h = a.scale_hw[k][0], w = a.scale_hw[k][1];
  int* d = a.draws + (long long)b * DRAW_COLS;
  d[0] = lo;
  d[1] = (int)(rem / nx);
  d[2] = (int)(rem % nx);
  d[3] = k;
  d[4] = h;
  d[5] = w;
  d[6] = (int)below(r1.v[0], r1.v[1], (unsigned long long)((h > a.OH ? h : a.OH) - a.OH + 1));
  d[7] = (int)below(r1.v[2], r1.v[3], (unsigned long long)((w > a.OW ? w : a.OW) - a.OW + 1));
  d[8] = unit(r2.v[0]) < a.prob ? 1 : 0;
  d[9] = unit(r2.v[1]) < a.vprob ? 1 : 0;
  // the permutation of (brightness, contrast, saturation, hue) with lexicographic rank `perm`: factorial number system, 3! 2! 1!
  const int perm = (int)below(r3.v[0], r3.v[1], 24ull);
  d[10] = perm;
  // (no private arrays with run-time indices: they would live in scratch memory.  `left` holds the ops not yet placed, one per 4 bits)
  unsigned left = 0x3210u;
  int rest = perm, n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = i == 0 ? 6 : (i == 1 ? 2 : 1);
    const int q = i < 3 ? rest / f : 0;
    rest -= q * f;
    const int op = (int)((left >> (4 * q)) & 0xFu);
    left = (left & ((1u << (4 * q)) - 1u)) | ((left >> (4 * q + 4)) << (4 * q));
    if (op < 3 && a.distort) {
      const unsigned wp = op == 0 ? r3.v[2] : (op == 1 ? r4.v[0] : r4.v[2]), wf = op == 0 ? r3.v[3] : (op == 1 ? r4.v[1] : r4.v[3]);
      const double prob = op == 0 ? a.op_prob[0] : (op == 1 ? a.op_prob[1] : a.op_prob[2]);
      const double range = op == 0 ? a.range[0] : (op == 1 ? a.range[1] : a.range[2]);
      if (unit(wp) < prob) {
        const double lower = 1.0 - range, upper = 1.0 + range;
        d[12 + n] = op;
        d[15 + n] = __float_as_int((float)(lower + (upper - lower) * unit(wf)));
        ++n;
      }
    }
  }
  d[11] = n;
  for (int i = n; i < AUG_MAX_OPS; ++i) {
    d[12 + i] = 0;
    d[15 + i] = __float_as_int(1.0f);
  }
}

// ---- host checks --------------------------------------------------------------------------------------------------------------------------------
// The tile fits every scene, every scene lies inside the bank (on the HOST mirror of the scene table).
int check_scenes(const char* fn, const EmrtSceneEntry* scenes, int n_scenes, size_t bank_bytes, int th, int tw) {
  if (!(n_scenes > 0)) return fail(fn, "n_scenes must be positive");
  if (!(th > 0 && tw > 0 && th <= AUG_MAX_SIDE && tw <= AUG_MAX_SIDE)) return fail(fn, "the tile must be positive (th, tw <= 32768)");
  const long long nbytes = (long long)bank_bytes;
  if (nbytes < 0) return fail(fn, "bank_bytes too large");
  char msg[200];
  for (int i = 0; i < n_scenes; ++i) {
    const EmrtSceneEntry& e = scenes[i];
    if (!(e.H > 0 && e.W > 0)) {
      snprintf(msg, sizeof(msg), "scene %d: sizes must be positive, got %dx%d", i, e.H, e.W);
      return fail(fn, msg);
    }
    if (th > e.H || tw > e.W) {
      snprintf(msg, sizeof(msg), "scene %d: the %dx%d tile is larger than the %dx%d scene", i, th, tw, e.H, e.W);
      return fail(fn, msg);
    }
    const long long hw = (long long)e.H * e.W;
    if (e.img_off < 0 || hw > nbytes / 3 || e.img_off > nbytes - 3 * hw || e.lab_off < 0 || e.lab_off > nbytes - hw) {
      snprintf(msg, sizeof(msg), "scene %d: image or label map outside the bank (%lld bytes)", i, nbytes);
      return fail(fn, msg);
    }
  }
  return 0;
}

int fill_common(const char* fn, AugCommon& c, int B, int OH, int OW, int distort, const double* mean, const double* stdinv, const float* img_pad,
                int label_pad, const unsigned char* label_lut, float* out, long long out_bs, long long* labels, void* workspace,
                size_t workspace_bytes, bool need_sums) {
  if (!(OH > 0 && OW > 0 && OH <= AUG_MAX_SIDE && OW <= AUG_MAX_SIDE)) return fail(fn, "B, OH and OW must be positive (OH, OW <= 32768)");
  if (!((long long)OH * OW < (1ll << 31) / 4)) return fail(fn, "crop too large");
  if (!(out_bs >= 3ll * OH * OW)) return fail(fn, "out_bs smaller than one [3][OH][OW] image");
  if (!(label_pad >= 0 && label_pad <= 255)) return fail(fn, "label_pad must be 0..255");
  if (distort)
    for (int k = 0; k < 3; ++k)
      if (!(img_pad[k] >= 0.0f && img_pad[k] < 256.0f)) return fail(fn, "with distortion img_pad must lie in [0, 256)");
  if (need_sums) {
    if (!workspace) return fail(fn, "null pointer (workspace)");
    if (workspace_bytes < (size_t)B * sizeof(unsigned long long)) return fail(fn, "workspace smaller than emrt_aug_workspace_bytes(B)");
    if (((uintptr_t)workspace & 7u) != 0) return fail(fn, "workspace must be 8-byte aligned");
  }
  c.out = out;
  c.labels = labels;
  c.sums = need_sums ? (unsigned long long*)workspace : nullptr;
  c.out_bs = out_bs;
  for (int k = 0; k < 3; ++k) {
    c.mean[k] = mean[k];
    c.stdinv[k] = stdinv[k];
    c.pad[k] = img_pad[k];
  }
  c.label_pad = label_pad;
  c.OH = OH;
  c.OW = OW;
  c.distort = distort ? 1 : 0;
  for (int i = 0; i < 256; ++i) c.lut[i] = label_lut ? label_lut[i] : (unsigned char)i;
  return 0;
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" const char* emrt_aug_last_error(void) { return g_aug_err; }

extern "C" int emrt_aug_version(void) { return 1; }

extern "C" size_t emrt_aug_workspace_bytes(int B) {
  if (B <= 0) {
    fail(__func__, "B must be positive");
    return 0;
  }
  return (size_t)B * sizeof(unsigned long long);
}

extern "C" int emrt_aug_tiles(const void* src, size_t src_bytes, const EmrtAugOpsDesc* descs, int B, int OH, int OW, int distort,
                              const double* mean, const double* stdinv, const float* img_pad, int label_pad, const unsigned char* label_lut,
                              float* out, long long out_bs, long long* labels, void* workspace, size_t workspace_bytes, void* stream) {
  AUG_REQUIRE(src && descs && out && mean && stdinv && img_pad, "null pointer");
  AUG_REQUIRE(B > 0 && OH > 0 && OW > 0 && OH <= AUG_MAX_SIDE && OW <= AUG_MAX_SIDE, "B, OH and OW must be positive (OH, OW <= 32768)");
  const long long nbytes = (long long)src_bytes;
  AUG_REQUIRE(nbytes >= 0, "src_bytes too large");
  // every descriptor is checked before the first launch: a bad one is an error, never an out-of-range read
  const char* fn = __func__;
  bool any_contrast = false;
  for (int i = 0; i < B; ++i) {
    const EmrtAugOpsDesc& d = descs[i];
    auto bad = [&](const char* what) {
      char msg[160];
      snprintf(msg, sizeof(msg), "descriptor %d: %s", i, what);
      return fail(fn, msg);
    };
    if (!(d.H > 0 && d.W > 0 && d.h > 0 && d.w > 0)) return bad("sizes must be positive");
    if (d.H > AUG_MAX_SIDE || d.W > AUG_MAX_SIDE || d.h > AUG_MAX_SIDE || d.w > AUG_MAX_SIDE) return bad("side longer than 32768");
    if (d.off_y < 0 || d.off_x < 0 || (long long)d.off_y + OH > (d.h > OH ? d.h : OH) || (long long)d.off_x + OW > (d.w > OW ? d.w : OW))
      return bad("crop outside the padded image");
    if (d.flip < 0 || d.flip > (EMRT_AUG_FLIP_H | EMRT_AUG_FLIP_V)) return bad("flip must be a mask of EMRT_AUG_FLIP_H | EMRT_AUG_FLIP_V");
    const long long hw = (long long)d.H * d.W;
    if (d.img_off < 0 || d.img_off > nbytes - 3 * hw) return bad("image outside the staged buffer");
    if (labels && (d.lab_off < 0 || d.lab_off > nbytes - hw)) return bad("label map outside the staged buffer");
    if (d.n_ops < 0 || d.n_ops > AUG_MAX_OPS) return bad("n_ops must be 0..3");
    if (d.n_ops > 0 && !distort) return bad("colour ops need distort != 0");
    unsigned seen = 0;
    for (int k = 0; k < d.n_ops; ++k) {
      if (d.op[k] < 0 || d.op[k] > EMRT_AUG_OP_SATURATION) return bad("op code must be 0 (brightness), 1 (contrast) or 2 (saturation)");
      if (seen & (1u << d.op[k])) return bad("an op appears twice");
      seen |= 1u << d.op[k];
      if (!(d.factor[k] >= 0.0f && d.factor[k] <= FLT_MAX)) return bad("factors must be finite and >= 0");
      if (d.op[k] == EMRT_AUG_OP_CONTRAST) any_contrast = true;
    }
  }
  TileSrc a{};
  if (int r = fill_common(fn, a.c, B, OH, OW, distort, mean, stdinv, img_pad, label_pad, label_lut, out, out_bs, labels, workspace,
                          workspace_bytes, any_contrast))
    return r;
  a.src = (const unsigned char*)src;
  hipStream_t st = (hipStream_t)stream;
  if (any_contrast) {
    (void)hipMemsetAsync(workspace, 0, (size_t)B * sizeof(unsigned long long), st);
    if (int r = check_launch(fn)) return r;
  }
  const unsigned gx = (unsigned)((OH * OW + AUG_THREADS - 1) / AUG_THREADS);
  for (int b0 = 0; b0 < B; b0 += AUG_CHUNK) {
    const int nb = B - b0 < AUG_CHUNK ? B - b0 : AUG_CHUNK;
    a.b0 = b0;
    bool contrast = false;
    for (int j = 0; j < nb; ++j) {
      const EmrtAugOpsDesc& d = descs[b0 + j];
      TileSample& s = a.s[j];
      s.img_off = d.img_off;
      s.lab_off = labels ? d.lab_off : 0;
      s.ry = (double)d.H / (double)d.h;
      s.rx = (double)d.W / (double)d.w;
      s.H = d.H; s.W = d.W; s.h = d.h; s.w = d.w;
      s.off_y = d.off_y; s.off_x = d.off_x; s.flip = d.flip; s.n_ops = d.n_ops;
      for (int k = 0; k < AUG_MAX_OPS; ++k) {
        s.op[k] = k < d.n_ops ? d.op[k] : 0;
        s.f[k] = k < d.n_ops ? d.factor[k] : 1.0f;
        if (k < d.n_ops && d.op[k] == EMRT_AUG_OP_CONTRAST) contrast = true;
      }
    }
    if (contrast) {
      hipLaunchKernelGGL(aug_stats_kernel<TileSrc>, dim3(gx < AUG_STATS_BLOCKS ? gx : AUG_STATS_BLOCKS, (unsigned)nb), dim3(AUG_THREADS), 0, st, a);
      if (int r = check_launch(fn)) return r;
    }
    hipLaunchKernelGGL(aug_apply_kernel<TileSrc>, dim3(gx, (unsigned)nb), dim3(AUG_THREADS), 0, st, a);
    if (int r = check_launch(fn)) return r;
  }
  return 0;
}

extern "C" int emrt_aug_scene_draw(const long long* step_counter, const EmrtSceneEntry* scenes, const long long* cum_origins,
                                   const EmrtSceneEntry* scenes_host, const long long* cum_origins_host, int n_scenes, size_t bank_bytes,
                                   long long key, int rank, int B, int th, int tw, int OH, int OW, double flip_prob, double vflip_prob, int distort,
                                   const double* ranges, const double* probs, const int* scale_hw, int n_scales, int* draws, void* stream) {
  AUG_REQUIRE(step_counter && scenes && cum_origins && scenes_host && cum_origins_host && scale_hw && draws && ranges && probs, "null pointer");
  AUG_REQUIRE(B > 0 && OH > 0 && OW > 0 && OH <= AUG_MAX_SIDE && OW <= AUG_MAX_SIDE, "B, OH and OW must be positive (OH, OW <= 32768)");
  AUG_REQUIRE(n_scales >= 1 && n_scales <= SCENE_MAX_SCALES, "1 to 16 scale entries");
  AUG_REQUIRE(rank >= 0 && ((long long)rank + 1) * B <= (1ll << 32), "rank * B + b must fit the 32-bit counter word");
  AUG_REQUIRE(flip_prob >= 0.0 && flip_prob <= 1.0, "the flip probability must be in [0, 1]");      // (false for NaN)
  AUG_REQUIRE(vflip_prob >= 0.0 && vflip_prob <= 1.0, "the vertical flip probability must be in [0, 1]");
  DrawArgs a{};
  for (int k = 0; k < 3; ++k) {
    AUG_REQUIRE(probs[k] >= 0.0 && probs[k] <= 1.0, "every op probability must be in [0, 1]");
    AUG_REQUIRE(ranges[k] >= 0.0 && ranges[k] <= 1.0, "every op range must be in [0, 1] (range < 0 or a negative factor)");
    a.range[k] = ranges[k];
    a.op_prob[k] = probs[k];
  }
  if (int r = check_scenes(__func__, scenes_host, n_scenes, bank_bytes, th, tw)) return r;
  AUG_REQUIRE(cum_origins_host[0] == 0, "the cumulative origin table must start at 0");
  for (int i = 0; i < n_scenes; ++i) {
    char msg[200];
    if (cum_origins_host[i + 1] <= cum_origins_host[i]) {
      snprintf(msg, sizeof(msg), "the cumulative origin table is not increasing at scene %d", i);
      return fail(__func__, msg);
    }
    const long long want = ((long long)scenes_host[i].H - th + 1) * ((long long)scenes_host[i].W - tw + 1);
    if (cum_origins_host[i + 1] - cum_origins_host[i] != want) {
      snprintf(msg, sizeof(msg), "scene %d: the cumulative origin table holds %lld origins, the scene and tile sizes give %lld", i,
               cum_origins_host[i + 1] - cum_origins_host[i], want);
      return fail(__func__, msg);
    }
  }
  for (int k = 0; k < n_scales; ++k) {
    const int h = scale_hw[2 * k], w = scale_hw[2 * k + 1];
    if (!(h > 0 && w > 0 && h <= AUG_MAX_SIDE && w <= AUG_MAX_SIDE)) {
      char msg[160];
      snprintf(msg, sizeof(msg), "scale entry %d: sizes must be 1..32768, got %dx%d", k, h, w);
      return fail(__func__, msg);
    }
    a.scale_hw[k][0] = h;
    a.scale_hw[k][1] = w;
  }
  a.step = step_counter;
  a.scenes = scenes;
  a.cum = cum_origins;
  a.draws = draws;
  a.prob = flip_prob;
  a.vprob = vflip_prob;
  a.k0 = (unsigned)((unsigned long long)key & 0xFFFFFFFFull);
  a.k1 = (unsigned)((unsigned long long)key >> 32);
  a.first = (unsigned)((long long)rank * B);
  a.n_scenes = n_scenes; a.B = B; a.th = th; a.tw = tw; a.OH = OH; a.OW = OW; a.n_scales = n_scales; a.distort = distort ? 1 : 0;
  hipLaunchKernelGGL(aug_scene_draw_kernel, dim3((unsigned)((B + DRAW_THREADS - 1) / DRAW_THREADS)), dim3(DRAW_THREADS), 0, (hipStream_t)stream, a);
  return check_launch(__func__);
}

extern "C" int emrt_aug_scene_sample(const unsigned char* bank, size_t bank_bytes, const EmrtSceneEntry* scenes, const EmrtSceneEntry* scenes_host,
                                     int n_scenes, const int* draws, int B, int th, int tw, int OH, int OW, int distort, const double* mean,
                                     const double* stdinv, const float* img_pad, int label_pad, const unsigned char* label_lut, float* out,
                                     long long out_bs, long long* labels, void* workspace, size_t workspace_bytes, void* stream) {
  AUG_REQUIRE(bank && scenes && scenes_host && draws && out && mean && stdinv && img_pad, "null pointer");
  AUG_REQUIRE(B > 0 && B <= 65535, "B must be 1..65535");
  SceneSrc a{};
  if (int r = fill_common(__func__, a.c, B, OH, OW, distort, mean, stdinv, img_pad, label_pad, label_lut, out, out_bs, labels, workspace,
                          workspace_bytes, distort != 0))
    return r;
  if (int r = check_scenes(__func__, scenes_host, n_scenes, bank_bytes, th, tw)) return r;
  a.bank = bank;
  a.scenes = scenes;
  a.draws = draws;
  a.n_scenes = n_scenes; a.th = th; a.tw = tw;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)((OH * OW + AUG_THREADS - 1) / AUG_THREADS);
  if (distort) {
    (void)hipMemsetAsync(workspace, 0, (size_t)B * sizeof(unsigned long long), st);
    if (int r = check_launch(__func__)) return r;
    hipLaunchKernelGGL(aug_stats_kernel<SceneSrc>, dim3(gx < AUG_STATS_BLOCKS ? gx : AUG_STATS_BLOCKS, (unsigned)B), dim3(AUG_THREADS), 0, st, a);
    if (int r = check_launch(__func__)) return r;
  }
  hipLaunchKernelGGL(aug_apply_kernel<SceneSrc>, dim3(gx, (unsigned)B), dim3(AUG_THREADS), 0, st, a);
  return check_launch(__func__);
}
