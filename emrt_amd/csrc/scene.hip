// Whole-scene prediction for gfx950: the two ends of `python -m emrt_amd.predict` around the model.
//
//  * emrt_scene_crop_windows_u8: windows of a uint8 HWC scene -> normalised fp32 NCHW batch.  The value is transforms.Normalize's own
//    arithmetic, (float)(((double)u8 - mean[c]) * stdinv[c]): float64 math, one rounding -- the bits the CPU transform makes.
//  * emrt_scene_finish: the accumulated sums (and hit counts) of the sliding window -> class index, colour, overlay and per-class areas in
//    ONE pass: what emrt_window_normalise + emrt_argmax_nchw + a per-class colouring loop on the host did in three.  Reads the C + 1 fp32
//    planes once, writes 1 + 3 (+ 3) bytes per pixel.
//
// Both are pure streaming: four consecutive pixels of a row per lane (16-byte loads from the fp32 planes, the byte outputs packed into whole
// dwords), a grid-stride loop over a capped grid; a one-pixel-per-thread form covers ragged widths and unaligned pointers.
#include "common.hpp"
#include "scene_norm.hpp"      // SceneNorm, normalise_u8

using namespace emrt;

namespace {

constexpr int SC_MAX_CLASSES = 256;
constexpr int SC_MAX_BLOCKS = 2048;          // 8 blocks of 256 threads per CU; the rest of the work is grid-strided

inline int scene_grid(long long items) {
  long long g = (items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > SC_MAX_BLOCKS ? SC_MAX_BLOCKS : g));
}

// VEC = 4: one thread makes four consecutive x of one window row for the three channels (cw % 4 == 0, batch 16-byte aligned); VEC = 1: one x.
// The scene bytes of a window row start anywhere, so they are read as bytes (a wave reads one contiguous run of 768 of them).
template <int VEC>
__global__ __launch_bounds__(256) void scene_crop_windows_kernel(const unsigned char* __restrict__ scene, float* __restrict__ batch, WindowArgs a,
                                                                 SceneNorm nm) {
  const int cwv = a.cw / VEC;
  const long long total = (long long)a.n * a.ch * cwv;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    int xq, y;
    long long jj;
    unravel3(idx, cwv, a.ch, total <= 0xffffffffll, xq, y, jj);
    const int j = (int)jj, x = xq * VEC;
    const unsigned char* sp = scene + ((long long)(a.y0[j] + y) * a.W + a.x0[j] + x) * 3;
    float* bp = batch + (((long long)j * 3) * a.ch + y) * a.cw + x;
    const long long plane = (long long)a.ch * a.cw;
    if constexpr (VEC == 4) {
      unsigned b[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) b[i] = sp[i];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(bp + c * plane) = make_float4(normalise_u8(b[c], nm.mean[c], nm.stdinv[c]), normalise_u8(b[3 + c], nm.mean[c], nm.stdinv[c]),
                                                                 normalise_u8(b[6 + c], nm.mean[c], nm.stdinv[c]), normalise_u8(b[9 + c], nm.mean[c], nm.stdinv[c]));
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) bp[c * plane] = normalise_u8(sp[c], nm.mean[c], nm.stdinv[c]);
    }
  }
}

struct ScenePalette {
  unsigned rgb[SC_MAX_CLASSES];          // r | g << 8 | b << 16
};

// argmax_nchw_kernel's rule (spatial.hip): the first maximum wins, a NaN counts as the maximum, a NaN in class 0 stays
__device__ __forceinline__ void argmax_step(float v, int c, float& best, int& bi) {
  if (best == best && (v > best || v != v)) { best = v; bi = c; }
}

__device__ __forceinline__ unsigned blend_rgb(unsigned col, unsigned src, float alpha, float beta) {
  unsigned out = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v = alpha * (float)((col >> (8 * k)) & 255u) + beta * (float)((src >> (8 * k)) & 255u) + 0.5f;      // in [0.5, 255.5]: truncation is floor
    out |= (unsigned)v << (8 * k);
  }
  return out;
}

// four 24-bit pixels <-> the three dwords they occupy in an HWC byte row
__device__ __forceinline__ void pack_rgb4(const unsigned (&p)[4], unsigned (&w)[3]) {
  w[0] = p[0] | (p[1] << 24);
  w[1] = (p[1] >> 8) | (p[2] << 16);
  w[2] = (p[2] >> 16) | (p[3] << 8);
}
__device__ __forceinline__ void unpack_rgb4(const unsigned (&w)[3], unsigned (&p)[4]) {
  p[0] = w[0] & 0xffffffu;
  p[1] = (w[0] >> 24) | ((w[1] & 0xffffu) << 8);
  p[2] = (w[1] >> 16) | ((w[2] & 0xffu) << 16);
  p[3] = w[2] >> 8;
}

struct Rgb4 {
  unsigned w[3];
};

// One item = VEC consecutive pixels of the flat [N * H * W] pixel index (VEC = 4: W % 4 == 0, so an item never leaves its row and every plane
// offset is a multiple of 16 bytes).  values [N][C][HW], count [N][HW] or null, scene / color / overlay [N][HW][3] bytes, index [N][HW] bytes.
template <int VEC>
__global__ __launch_bounds__(256) void scene_finish_kernel(const float* __restrict__ values, const float* __restrict__ count, ScenePalette pal,
                                                           const unsigned char* __restrict__ scene, float alpha, unsigned char* __restrict__ index,
                                                           unsigned char* __restrict__ color, unsigned char* __restrict__ overlay,
                                                           long long* __restrict__ areas, int C, unsigned HW, unsigned items) {
  __shared__ unsigned s_pal[SC_MAX_CLASSES];
  __shared__ unsigned s_hist[SC_MAX_CLASSES];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    s_pal[c] = pal.rgb[c];
    s_hist[c] = 0u;
  }
  __syncthreads();
  const float beta = 1.f - alpha;
  for (unsigned it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
    const unsigned p = it * VEC, n = p / HW, r = p - n * HW;          // (N * H * W < 2^31: 32-bit arithmetic throughout)
    const float* vp = values + (long long)n * C * HW + r;
    float cnt[VEC], best[VEC];
    int bi[VEC];
    if constexpr (VEC == 4) {
      if (count) {
        const float4 k = *reinterpret_cast<const float4*>(count + p);
        cnt[0] = k.x; cnt[1] = k.y; cnt[2] = k.z; cnt[3] = k.w;
      }
    } else {
      if (count) cnt[0] = count[p];
    }
    for (int c = 0; c < C; ++c) {
      float v[VEC];
      if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(vp + (long long)c * HW);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        v[0] = vp[(long long)c * HW];
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        if (count) v[i] = v[i] / cnt[i];          // window_normalise_kernel's division: an uncovered pixel is 0 / 0 = NaN, class 0
        if (c == 0) { best[i] = v[i]; bi[i] = 0; }
        else argmax_step(v[i], c, best[i], bi[i]);
      }
    }
    unsigned col[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) col[i] = s_pal[bi[i]];
    if constexpr (VEC == 4) {
      const unsigned packed = (unsigned)bi[0] | ((unsigned)bi[1] << 8) | ((unsigned)bi[2] << 16) | ((unsigned)bi[3] << 24);
      *reinterpret_cast<unsigned*>(index + p) = packed;
      if (color) {
        Rgb4 o;
        pack_rgb4(col, o.w);
        *reinterpret_cast<Rgb4*>(color + (long long)p * 3) = o;
      }
      if (overlay) {
        const Rgb4 s = *reinterpret_cast<const Rgb4*>(scene + (long long)p * 3);
        unsigned src[4], mix[4];
        unpack_rgb4(s.w, src);
#pragma unroll
        for (int i = 0; i < 4; ++i) mix[i] = blend_rgb(col[i], src[i], alpha, beta);
        Rgb4 o;
        pack_rgb4(mix, o.w);
        *reinterpret_cast<Rgb4*>(overlay + (long long)p * 3) = o;
      }
      if (areas) {
        // maps are mostly large one-class regions: when every active lane holds the same four classes, one lane adds for the wave
        // instead of 64 lanes queueing on one LDS word
        const unsigned long long active = __ballot(1);
        const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)packed);
        if (__ballot(packed == first) == active) {
          if ((int)__lane_id() == __ffsll((long long)active) - 1) {
            const unsigned lanes = (unsigned)__popcll(active);
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(&s_hist[(first >> (8 * i)) & 255u], lanes);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) atomicAdd(&s_hist[bi[i]], 1u);
        }
      }
    } else {
      index[p] = (unsigned char)bi[0];
      if (color) {
        unsigned char* cp = color + (long long)p * 3;
        cp[0] = (unsigned char)(col[0] & 255u); cp[1] = (unsigned char)((col[0] >> 8) & 255u); cp[2] = (unsigned char)(col[0] >> 16);
      }
      if (overlay) {
        const unsigned char* sp = scene + (long long)p * 3;
        const unsigned mix = blend_rgb(col[0], (unsigned)sp[0] | ((unsigned)sp[1] << 8) | ((unsigned)sp[2] << 16), alpha, beta);
        unsigned char* op = overlay + (long long)p * 3;
        op[0] = (unsigned char)(mix & 255u); op[1] = (unsigned char)((mix >> 8) & 255u); op[2] = (unsigned char)(mix >> 16);
      }
      if (areas) atomicAdd(&s_hist[bi[0]], 1u);
    }
  }
  if (areas) {          // integer sums: the same areas whatever the order the blocks arrive in
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x)
      if (s_hist[c]) atomicAdd(reinterpret_cast<unsigned long long*>(areas + c), (unsigned long long)s_hist[c]);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

extern "C" int emrt_scene_crop_windows_u8(const unsigned char* scene, float* batch, const int* origins_yx /*host, [n][2]*/, int n, int H, int W, int ch,
                                          int cw, double mean0, double mean1, double mean2, double stdinv0, double stdinv1, double stdinv2,
                                          void* stream) {
  EMRT_REQUIRE(scene && batch && origins_yx, "null pointer");
  EMRT_REQUIRE(H >= 1 && W >= 1 && ch >= 1 && cw >= 1, "H, W, ch, cw must be positive");
  WindowArgs a;
  EMRT_REQUIRE(fill_windows(a, origins_yx, n, 3, H, W, ch, cw) == 0, "1..64 windows inside the image");
  const SceneNorm nm = {{mean0, mean1, mean2}, {stdinv0, stdinv1, stdinv2}};
  if (cw % 4 == 0 && aligned(batch, 16))
    hipLaunchKernelGGL(scene_crop_windows_kernel<4>, dim3(scene_grid((long long)n * ch * (cw / 4))), dim3(256), 0, (hipStream_t)stream, scene, batch, a, nm);
  else
    hipLaunchKernelGGL(scene_crop_windows_kernel<1>, dim3(scene_grid((long long)n * ch * cw)), dim3(256), 0, (hipStream_t)stream, scene, batch, a, nm);
  return check_launch("emrt_scene_crop_windows_u8");
}

extern "C" int emrt_scene_finish(const float* values, const float* count, const unsigned char* palette /*host, [C][3]*/, const unsigned char* scene,
                                 float alpha, unsigned char* index, unsigned char* color, unsigned char* overlay, long long* areas, int N, int C, int H,
                                 int W, void* stream) {
  EMRT_REQUIRE(C >= 1 && C <= SC_MAX_CLASSES, "C must be 1..256");
  EMRT_REQUIRE(values && index && palette, "null pointer");
  EMRT_REQUIRE(!overlay || scene, "overlay needs scene");
  EMRT_REQUIRE(alpha >= 0.f && alpha <= 1.f, "alpha must be in [0, 1]");
  EMRT_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H, W must be positive");
  const long long npix = (long long)N * H * W;
  EMRT_REQUIRE(npix < (1ll << 31), "N * H * W must be below 2^31");
  ScenePalette pal;
  for (int c = 0; c < C; ++c) pal.rgb[c] = (unsigned)palette[3 * c] | ((unsigned)palette[3 * c + 1] << 8) | ((unsigned)palette[3 * c + 2] << 16);
  for (int c = C; c < SC_MAX_CLASSES; ++c) pal.rgb[c] = 0u;
  const unsigned HW = (unsigned)((long long)H * W);
  const bool v4 = W % 4 == 0 && aligned(values, 16) && (!count || aligned(count, 16)) && aligned(index, 4) && (!color || aligned(color, 4)) &&
                  (!overlay || (aligned(overlay, 4) && aligned(scene, 4)));
  if (v4)
    hipLaunchKernelGGL(scene_finish_kernel<4>, dim3(scene_grid(npix / 4)), dim3(256), 0, (hipStream_t)stream, values, count, pal, scene, alpha, index, color,
                       overlay, areas, C, HW, (unsigned)(npix / 4));
  else
    hipLaunchKernelGGL(scene_finish_kernel<1>, dim3(scene_grid(npix)), dim3(256), 0, (hipStream_t)stream, values, count, pal, scene, alpha, index, color,
                       overlay, areas, C, HW, (unsigned)npix);
  return check_launch("emrt_scene_finish");
}
