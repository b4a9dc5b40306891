// Training augmentation of decoded uint8 tiles: the Potsdam / Vaihingen chain ResizeStepScaling -> RandomPaddingCrop ->
// RandomHorizontalFlip -> Normalize, and LoveDA's Normalize alone (emrt_amd/src/transforms, get_transforms), as ONE launch per batch.
// emrt_augment_tiles: the host draws every random decision (DevicePlan.plan) and passes them as per-sample descriptors.  emrt_scene_draw /
// emrt_scene_sample (second half of the file): the decisions are drawn on the device and the sources are windows of whole scenes.  One map serves both.
//
// One thread = one output pixel of one sample: the 3 normalised fp32 channels of out[b][c][oy][ox] and the int64 label.  The arithmetic is
// the numpy chain's, operation for operation, so the result is bit-identical to the CPU transforms: the geometry (coordinates, bilinear blend,
// nearest label, padding) is augment_map.hpp, the text libemrt_hip_augment.so compiles too, and then
//   normalise (float64):   (float)(((double)v - mean) * stdinv)
// FMA contraction is off for the whole file: a fused multiply-add rounds once where numpy rounds twice.
#pragma clang fp contract(off)
#include "common.hpp"
#include "augment_map.hpp"
#include "philox.hpp"

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

// What every sample of a batch shares: the outputs and the constants of the chain.
struct AugCommon {
  float* out;
  long long* labels;                   // nullable
  long long out_bs;
  double mean[3], stdinv[3];
  float pad[3];
  int label_pad;
  int OH, OW;
  unsigned char lut[256];
};

struct AugArgs {
  const unsigned char* src;
  AugCommon c;
  int b0;
  AugSample s[AUG_CHUNK];
};

// Output pixel p of sample b: the shared map (augment_map.hpp), then the normalisation and the stores.  Both kernels below are this function
// under two ways of finding `s`.
__device__ __forceinline__ void augment_pixel(const AugCommon& a, const AugView& s, long long b, int p) {
  const int npix = a.OH * a.OW;
  const int oy = p / a.OW, ox = p - oy * a.OW;
  float v[3];
  int lab;
  augment_map(s, a.OH, a.OW, a.pad, a.label_pad, a.labels != nullptr, oy, ox, v, lab);
  float* o = a.out + b * a.out_bs + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long long)c * npix] = (float)(((double)v[c] - a.mean[c]) * a.stdinv[c]);
  if (a.labels) a.labels[b * npix + p] = a.lut[lab];
}

__global__ __launch_bounds__(AUG_THREADS) void emrt_augment_kernel(AugArgs a) {
  const int p = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (p >= a.c.OH * a.c.OW) return;
  const AugSample& s = a.s[blockIdx.y];
  AugView v;
  v.img = a.src + s.img_off;
  v.lab = a.src + s.lab_off;
  v.pitch = s.W;
  v.ry = s.ry; v.rx = s.rx;
  v.H = s.H; v.W = s.W; v.h = s.h; v.w = s.w;
  v.off_y = s.off_y; v.off_x = s.off_x; v.flip = s.flip;
  augment_pixel(a.c, v, (long long)a.b0 + blockIdx.y, p);
}

// ---- tiles cut out of whole scenes that live in device memory (emrt_scene_draw, emrt_scene_sample) ---------------------------------------------
// The random decisions are drawn ON THE DEVICE from the step counter, so a replayed hipGraph cuts a new batch every time and the host does
// nothing per step.  Philox4x32-10, its key and counter and the integer draw `below` are philox.hpp, shared with the other two libraries:
//   block 0, words 0-1: tile origin among all origins of all scenes -> scene by binary search in the cumulative table, y0 = rem / nx, x0 = rem % nx
//   block 0, words 2-3: scale index
//   block 1, words 0-1: off_y below max(h, OH) - OH + 1;  words 2-3: off_x below max(w, OW) - OW + 1
//   block 2, word 0:    flip = (double)word * 2^-32 < prob
constexpr int SCENE_MAX_SCALES = 16;
constexpr int DRAW_COLS = 10;          // scene, y0, x0, scale_index, h, w, off_y, off_x, flip, 0
constexpr int DRAW_THREADS = 64;

struct DrawArgs {
  const long long* step;               // device: the step counter
  const EmrtSceneEntry* scenes;        // device
  const long long* cum;                // device, [n_scenes + 1], cum[0] = 0
  int* draws;                          // device, [B][DRAW_COLS]
  double prob;
  unsigned k0, k1, first;              // key words; rank * B
  int n_scenes, B, th, tw, OH, OW, n_scales;
  int scale_hw[SCENE_MAX_SCALES][2];
};

__global__ __launch_bounds__(DRAW_THREADS) void emrt_scene_draw_kernel(DrawArgs a) {
  const int b = blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (b >= a.B) return;
  const unsigned long long step = (unsigned long long)a.step[0];
  const unsigned s_lo = (unsigned)step, s_hi = (unsigned)(step >> 32), id = a.first + (unsigned)b;
  const Philox r0 = philox4x32_10(s_lo, s_hi, id, 0u, a.k0, a.k1);
  const Philox r1 = philox4x32_10(s_lo, s_hi, id, 1u, a.k0, a.k1);
  const Philox r2 = philox4x32_10(s_lo, s_hi, id, 2u, a.k0, a.k1);
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
  d[8] = (double)r2.v[0] * (1.0 / 4294967296.0) < a.prob ? 1 : 0;
  d[9] = 0;
}

struct SampleArgs {
  const unsigned char* bank;
  const EmrtSceneEntry* scenes;        // device
  const int* draws;                    // device, [B][DRAW_COLS]
  AugCommon c;
  int n_scenes, th, tw;
};

__global__ __launch_bounds__(AUG_THREADS) void emrt_scene_sample_kernel(SampleArgs a) {
  const int p = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (p >= a.c.OH * a.c.OW) return;
  const int* d = a.draws + (long long)blockIdx.y * DRAW_COLS;
  // the table is device memory this kernel did not write: every value is brought into its range, so a stale or foreign table reads wrong pixels,
  // never memory outside the bank (rows written by emrt_scene_draw are inside these ranges already and pass unchanged)
  const EmrtSceneEntry e = a.scenes[min(max(d[0], 0), a.n_scenes - 1)];
  const int y0 = min(max(d[1], 0), e.H - a.th), x0 = min(max(d[2], 0), e.W - a.tw);
  AugView v;
  v.H = a.th; v.W = a.tw;
  v.h = min(max(d[4], 1), AUG_MAX_SIDE); v.w = min(max(d[5], 1), AUG_MAX_SIDE);
  v.off_y = min(max(d[6], 0), max(v.h, a.c.OH) - a.c.OH);
  v.off_x = min(max(d[7], 0), max(v.w, a.c.OW) - a.c.OW);
  v.flip = d[8] != 0;
  v.ry = (double)a.th / (double)v.h;   // H / h in float64: correctly rounded here as in Python
  v.rx = (double)a.tw / (double)v.w;
  v.pitch = e.W;
  v.img = a.bank + e.img_off + ((long long)y0 * e.W + x0) * 3;
  v.lab = a.bank + e.lab_off + ((long long)y0 * e.W + x0);
  augment_pixel(a.c, v, blockIdx.y, p);
}

// The checks both scene entry points share, on the HOST mirror of the scene table: the tile fits every scene, every scene lies inside the bank.
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

int fill_common(const char* fn, AugCommon& c, int OH, int OW, const double* mean, const double* stdinv, const float* img_pad, int label_pad,
                const unsigned char* label_lut, float* out, long long out_bs, long long* labels) {
  if (!(OH > 0 && OW > 0 && OH <= AUG_MAX_SIDE && OW <= AUG_MAX_SIDE)) return fail(fn, "B, OH and OW must be positive (OH, OW <= 32768)");
  if (!((long long)OH * OW < (1ll << 31) / 4)) return fail(fn, "crop too large");
  if (!(out_bs >= 3ll * OH * OW)) return fail(fn, "out_bs smaller than one [3][OH][OW] image");
  if (!(label_pad >= 0 && label_pad <= 255)) return fail(fn, "label_pad must be 0..255");
  c.out = out;
  c.labels = labels;
  c.out_bs = out_bs;
  for (int k = 0; k < 3; ++k) {
    c.mean[k] = mean[k];
    c.stdinv[k] = stdinv[k];
    c.pad[k] = img_pad[k];
  }
  c.label_pad = label_pad;
  c.OH = OH;
  c.OW = OW;
  for (int i = 0; i < 256; ++i) c.lut[i] = label_lut ? label_lut[i] : (unsigned char)i;
  return 0;
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" int emrt_augment_tiles(const void* src, size_t src_bytes, const EmrtAugDesc* descs, int B, int OH, int OW, const double* mean,
                                  const double* stdinv, const float* img_pad, int label_pad, const unsigned char* label_lut, float* out,
                                  long long out_bs, long long* labels, void* stream) {
  EMRT_REQUIRE(src && descs && out && mean && stdinv && img_pad, "null pointer");
  EMRT_REQUIRE(B > 0, "B, OH and OW must be positive (OH, OW <= 32768)");
  AugArgs a{};
  if (int r = fill_common(__func__, a.c, OH, OW, mean, stdinv, img_pad, label_pad, label_lut, out, out_bs, labels)) return r;
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
  a.src = (const unsigned char*)src;
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

extern "C" int emrt_scene_draw(const long long* step_counter, const EmrtSceneEntry* scenes, const long long* cum_origins,
                               const EmrtSceneEntry* scenes_host, const long long* cum_origins_host, int n_scenes, size_t bank_bytes, long long key,
                               int rank, int B, int th, int tw, int OH, int OW, double flip_prob, const int* scale_hw /*host, [n_scales][2]*/,
                               int n_scales, int* draws, void* stream) {
  EMRT_REQUIRE(step_counter && scenes && cum_origins && scenes_host && cum_origins_host && scale_hw && draws, "null pointer");
  EMRT_REQUIRE(B > 0 && OH > 0 && OW > 0 && OH <= AUG_MAX_SIDE && OW <= AUG_MAX_SIDE, "B, OH and OW must be positive (OH, OW <= 32768)");
  EMRT_REQUIRE(n_scales >= 1 && n_scales <= SCENE_MAX_SCALES, "1 to 16 scale entries");
  EMRT_REQUIRE(rank >= 0 && ((long long)rank + 1) * B <= (1ll << 32), "rank * B + b must fit the 32-bit counter word");
  EMRT_REQUIRE(flip_prob >= 0.0 && flip_prob <= 1.0, "the flip probability must be in [0, 1]");      // (false for NaN)
  if (int r = check_scenes(__func__, scenes_host, n_scenes, bank_bytes, th, tw)) return r;
  EMRT_REQUIRE(cum_origins_host[0] == 0, "the cumulative origin table must start at 0");
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
  DrawArgs a{};
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
  a.k0 = (unsigned)((unsigned long long)key & 0xFFFFFFFFull);
  a.k1 = (unsigned)((unsigned long long)key >> 32);
  a.first = (unsigned)((long long)rank * B);
  a.n_scenes = n_scenes; a.B = B; a.th = th; a.tw = tw; a.OH = OH; a.OW = OW; a.n_scales = n_scales;
  hipLaunchKernelGGL(emrt_scene_draw_kernel, dim3((unsigned)((B + DRAW_THREADS - 1) / DRAW_THREADS)), dim3(DRAW_THREADS), 0, (hipStream_t)stream, a);
  return check_launch(__func__);
}

extern "C" int emrt_scene_sample(const unsigned char* bank, size_t bank_bytes, const EmrtSceneEntry* scenes, const EmrtSceneEntry* scenes_host,
                                 int n_scenes, const int* draws, int B, int th, int tw, int OH, int OW, const double* mean, const double* stdinv,
                                 const float* img_pad, int label_pad, const unsigned char* label_lut, float* out, long long out_bs,
                                 long long* labels, void* stream) {
  EMRT_REQUIRE(bank && scenes && scenes_host && draws && out && mean && stdinv && img_pad, "null pointer");
  EMRT_REQUIRE(B > 0 && B <= 65535, "B must be 1..65535");
  SampleArgs a{};
  if (int r = fill_common(__func__, a.c, OH, OW, mean, stdinv, img_pad, label_pad, label_lut, out, out_bs, labels)) return r;
  if (int r = check_scenes(__func__, scenes_host, n_scenes, bank_bytes, th, tw)) return r;
  a.bank = bank;
  a.scenes = scenes;
  a.draws = draws;
  a.n_scenes = n_scenes; a.th = th; a.tw = tw;
  const unsigned gx = (unsigned)((OH * OW + AUG_THREADS - 1) / AUG_THREADS);
  hipLaunchKernelGGL(emrt_scene_sample_kernel, dim3(gx, (unsigned)B), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
  return check_launch(__func__);
}
