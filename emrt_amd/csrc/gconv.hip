// Grouped 3x3 convolution (pad 1, stride 1 / 2) on NHWC maps: the cardinality-64 middle layer of the ResNeXt bottleneck
// (backbones/resnext.py, BottleneckBlock.conv1: 64 groups of 4 / 8 / 16 / 32 channels).  Direct convolution on the VALU: at these
// group widths the layer does 9 * Cg multiply-adds per loaded activation (36 .. 288), far below the bf16 MFMA ridge, so it is bound by
// bytes and launch latency, not by the matrix cores.
//
// Weights are [OC][3][3][Cg] (ParamStore's layout of a [OC, Cg, 3, 3] parameter); OC = groups * Og, Og = OC / groups.
//   forward : one thread = 4 output channels (one group) x GC_PPT consecutive output pixels; the group's Cg input channels are read in
//             16-byte (or 8-byte) vectors per tap, the weights from the L1 / L2 (the same few KiB for every block of a channel slice)
//   dgrad   : the same form over INPUT pixels and input channels: dx = sum over taps and the group's Og output channels of dy * w
//   wgrad   : one thread = (oc, tap, 8 input channels); the pixel reduction is cut into slices over gridDim.y, fp32 atomics into dW
// The forward output and dx are written without atomics: bit-identical run to run.
#include "common.hpp"

namespace emrt {
namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_PPT = 4;        // output (forward) / input (dgrad) pixels per thread

struct GconvArgs {
  const void* x;          // forward: input map;  dgrad: dy
  const void* w;          // [OC][3][3][Cg]
  void* y;                // forward: output;     dgrad: dx
  const float* bias;      // forward only (nullable)
  const float* scale;     // forward only (nullable): eval-mode folded BatchNorm
  double* stats;          // forward only (nullable): fp64 [8][2 * OC]
  int N, H, W, C, ldin;   // dims of x (dgrad: of dy, C = OC)
  long long in_bs;
  int OH, OW, OC, ldout;  // dims of y (dgrad: of dx, OC = C of the layer)
  long long out_bs;
  int stride, relu, accumulate;
  int Cg, Og;             // input / output channels per group of the LAYER
  int QB, PS;             // channel quads per block, pixel slots per block
  long long ntiles;
  int ldres;              // dgrad: dx's own stride (accumulate reads it)
};

template <class T, int CH>
__device__ __forceinline__ void load_ch(const T* p, float (&o)[CH]) {
  if constexpr (CH == 8) Vec8<T>::load(p, o);
  else Vec4<T>::load(p, o);
}

template <class T, int CG>
__global__ __launch_bounds__(GC_THREADS) void gconv_fwd_kernel(GconvArgs a) {
  constexpr int CH = CG >= 8 ? 8 : 4;
  __shared__ float red[2 * GC_THREADS * 4];
  const int t = threadIdx.x;
  const int q = t % a.QB, ps = t / a.QB;
  const int quad = blockIdx.y * a.QB + q;
  const bool active = ps < a.PS && quad * 4 < a.OC;
  const int oc0 = active ? quad * 4 : 0;
  const int cin0 = (oc0 / a.Og) * CG;
  const T* __restrict__ x = (const T*)a.x;
  const T* __restrict__ w = (const T*)a.w + (long long)oc0 * 9 * CG;
  const int M = a.N * a.OH * a.OW;
  float ss[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
  float osc[4], osh[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    osc[o] = a.scale ? a.scale[oc0 + o] : 1.f;
    osh[o] = a.bias ? a.bias[oc0 + o] : 0.f;
  }
  for (long long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    if (!active) continue;
    const int m0 = (int)(tile * (a.PS * GC_PPT)) + ps * GC_PPT;
    int iy0[GC_PPT], ix0[GC_PPT];
    long long xb[GC_PPT];
#pragma unroll
    for (int p = 0; p < GC_PPT; ++p) {
      const int m = m0 + p;
      if (m < M) {
        const int ox = m % a.OW, r = m / a.OW, oy = r % a.OH, n = r / a.OH;
        iy0[p] = oy * a.stride - 1; ix0[p] = ox * a.stride - 1;
        xb[p] = (long long)n * a.in_bs + cin0;
      } else {
        iy0[p] = -1000; ix0[p] = -1000; xb[p] = 0;
      }
    }
    float acc[4][GC_PPT];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int p = 0; p < GC_PPT; ++p) acc[o][p] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      long long off[GC_PPT];
#pragma unroll
      for (int p = 0; p < GC_PPT; ++p) {
        const int iy = iy0[p] + ky, ix = ix0[p] + kx;
        off[p] = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? xb[p] + ((long long)iy * a.W + ix) * a.ldin : -1;
      }
#pragma unroll 1
      for (int c0 = 0; c0 < CG; c0 += CH) {      // (one pass at Cg 4 / 8; unrolled, Cg 32 held 256 VGPRs: one wave per SIMD)
        float wv[4][CH];
#pragma unroll
        for (int o = 0; o < 4; ++o) load_ch<T, CH>(w + (o * 9 + tap) * CG + c0, wv[o]);
#pragma unroll
        for (int p = 0; p < GC_PPT; ++p) {
          float xv[CH];
          if (off[p] >= 0) {
            load_ch<T, CH>(x + off[p] + c0, xv);
          } else {
#pragma unroll
            for (int e = 0; e < CH; ++e) xv[e] = 0.f;
          }
#pragma unroll
          for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int e = 0; e < CH; ++e) acc[o][p] = fmaf(xv[e], wv[o][e], acc[o][p]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < GC_PPT; ++p) {
      const int m = m0 + p;
      if (m >= M) continue;
      const int ox = m % a.OW, r = m / a.OW, oy = r % a.OH, n = r / a.OH;
      float v[4];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        float s = fmaf(acc[o][p], osc[o], osh[o]);
        if (a.relu) s = fmaxf(s, 0.f);
        v[o] = to_f32(from_f32<T>(s));       // statistics of what the next kernel will read
        ss[o] += v[o];
        sq[o] = fmaf(v[o], v[o], sq[o]);
      }
      Vec4<T>::store((T*)a.y + (long long)n * a.out_bs + ((long long)oy * a.OW + ox) * a.ldout + oc0, v);
    }
  }
  if (a.stats) {
    // per-block column sums through LDS, then one fp64 atomic per channel and statistic into replica (block & 7)
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      red[t * 4 + o] = active ? ss[o] : 0.f;
      red[(GC_THREADS + t) * 4 + o] = active ? sq[o] : 0.f;
    }
    __syncthreads();
    const int cols = 4 * a.QB;
    for (int e = t; e < 2 * cols; e += GC_THREADS) {
      const int which = e / cols, col = e - which * cols;
      float s = 0.f;
      for (int k = 0; k < a.PS; ++k) s += red[(which * GC_THREADS + k * a.QB + col / 4) * 4 + (col & 3)];
      const int oc = blockIdx.y * a.QB * 4 + col;
      if (oc < a.OC) atomicAdd(a.stats + (long long)(blockIdx.x & 7) * 2 * a.OC + (long long)which * a.OC + oc, (double)s);
    }
  }
}

// dx[n, iy, ix, ci] (+)= sum_{tap, o < Og} dy[n, oy, ox, g * Og + o] * w[g * Og + o][tap][ci - g * Cg],  iy = oy * stride - 1 + ky
template <class T>
__global__ __launch_bounds__(GC_THREADS) void gconv_dgrad_kernel(GconvArgs a) {
  const int t = threadIdx.x;
  const int q = t % a.QB, ps = t / a.QB;
  const int quad = blockIdx.y * a.QB + q;
  const bool active = ps < a.PS && quad * 4 < a.OC;       // (OC = the layer's input channels here)
  if (!active) return;
  const int ci0 = quad * 4, g = ci0 / a.Cg, cl0 = ci0 - g * a.Cg;
  const int ocg0 = g * a.Og;
  const T* __restrict__ dy = (const T*)a.x;
  const T* __restrict__ w = (const T*)a.w + (long long)ocg0 * 9 * a.Cg + cl0;
  const int M = a.N * a.OH * a.OW;              // input pixels of the layer (= dx pixels)
  const int s = a.stride;
  for (long long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int m0 = (int)(tile * (a.PS * GC_PPT)) + ps * GC_PPT;
    int iy[GC_PPT], ix[GC_PPT];
    long long db[GC_PPT];
#pragma unroll
    for (int p = 0; p < GC_PPT; ++p) {
      const int m = m0 + p;
      if (m < M) {
        ix[p] = m % a.OW; const int r = m / a.OW; iy[p] = r % a.OH; const int n = r / a.OH;
        db[p] = (long long)n * a.in_bs + ocg0;
      } else {
        iy[p] = -100000; ix[p] = -100000; db[p] = 0;
      }
    }
    float acc[4][GC_PPT];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int p = 0; p < GC_PPT; ++p) acc[c][p] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      long long off[GC_PPT];
#pragma unroll
      for (int p = 0; p < GC_PPT; ++p) {
        const int ny = iy[p] + 1 - ky, nx = ix[p] + 1 - kx;
        const int oy = ny / s, ox = nx / s;
        off[p] = (ny >= 0 && nx >= 0 && oy * s == ny && ox * s == nx && oy < a.H && ox < a.W) ? db[p] + ((long long)oy * a.W + ox) * a.ldin : -1;
      }
#pragma unroll 1
      for (int o0 = 0; o0 < a.Og; o0 += 4) {
        float wv[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) Vec4<T>::load(w + ((long long)(o0 + j) * 9 + tap) * a.Cg, wv[j]);
#pragma unroll
        for (int p = 0; p < GC_PPT; ++p) {
          if (off[p] < 0) continue;
          float dv[4];
          Vec4<T>::load(dy + off[p] + o0, dv);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c][p] = fmaf(dv[j], wv[j][c], acc[c][p]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < GC_PPT; ++p) {
      const int m = m0 + p;
      if (m >= M) continue;
      const int n = m / (a.OH * a.OW);
      T* dst = (T*)a.y + (long long)n * a.out_bs + ((long long)iy[p] * a.OW + ix[p]) * a.ldout + ci0;
      float v[4] = {acc[0][p], acc[1][p], acc[2][p], acc[3][p]};
      if (a.accumulate) {
        float old[4];
        Vec4<T>::load(dst, old);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += old[c];
      }
      Vec4<T>::store(dst, v);
    }
  }
}

struct GwgradArgs {
  const void* x; const void* dy; float* dw; float* dbias;
  int N, H, W, C, ldx; long long x_bs;
  int OH, OW, OC, lddy; long long dy_bs;
  int stride, Cg, Og;
  int rows_per_slice;
};

// dW[oc][tap][cc * CH .. +CH) += sum over the slice's output pixels of dy[., oc] * x[tap position of ., g * Cg + cc * CH ..]
template <class T, int CG>
__global__ __launch_bounds__(GC_THREADS) void gconv_wgrad_kernel(GwgradArgs a) {
  constexpr int CH = CG >= 8 ? 8 : 4, NCC = CG / CH;
  const long long e = (long long)blockIdx.x * GC_THREADS + threadIdx.x;
  if (e >= (long long)a.OC * 9 * NCC) return;
  const int cc = (int)(e % NCC);
  const int r9 = (int)(e / NCC);
  const int tap = r9 % 9, oc = r9 / 9;
  const int ky = tap / 3, kx = tap - 3 * ky;
  const int cin = (oc / a.Og) * CG + cc * CH;
  const T* __restrict__ x = (const T*)a.x;
  const T* __restrict__ dy = (const T*)a.dy;
  const int M = a.N * a.OH * a.OW;
  const int r0 = blockIdx.y * a.rows_per_slice;
  const int r1 = min(M, r0 + a.rows_per_slice);
  float acc[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) acc[i] = 0.f;
  float db = 0.f;
  constexpr int U = 4;
  for (int m = r0; m < r1; m += U) {
    float dv[U], xv[U][CH];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int mm = m + u;
      dv[u] = 0.f;
#pragma unroll
      for (int i = 0; i < CH; ++i) xv[u][i] = 0.f;
      if (mm < r1) {
        const int ox = mm % a.OW, rr = mm / a.OW, oy = rr % a.OH, n = rr / a.OH;
        dv[u] = to_f32(dy[(long long)n * a.dy_bs + ((long long)oy * a.OW + ox) * a.lddy + oc]);
        const int iy = oy * a.stride - 1 + ky, ix = ox * a.stride - 1 + kx;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) load_ch<T, CH>(x + (long long)n * a.x_bs + ((long long)iy * a.W + ix) * a.ldx + cin, xv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      db += dv[u];
#pragma unroll
      for (int i = 0; i < CH; ++i) acc[i] = fmaf(dv[u], xv[u][i], acc[i]);
    }
  }
  if (a.dw) {
    float* d = a.dw + ((long long)oc * 9 + tap) * CG + cc * CH;
#pragma unroll
    for (int i = 0; i < CH; ++i) atomicAdd(d + i, acc[i]);
  }
  if (a.dbias && tap == 0 && cc == 0) atomicAdd(a.dbias + oc, db);
}

int check_common(const char* fn, int N, int H, int W, int C, int OH, int OW, int OC, int stride, int groups) {
  if (!(N > 0 && H > 0 && W > 0 && C > 0 && OC > 0 && groups > 0)) return fail(fn, "bad dims");
  if (stride != 1 && stride != 2) return fail(fn, "stride must be 1 or 2");
  if (C % groups || OC % groups) return fail(fn, "C and OC must be multiples of groups");
  const int Cg = C / groups, Og = OC / groups;
  if (Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32) return fail(fn, "channels per group must be 4, 8, 16 or 32");
  if (Og % 4) return fail(fn, "output channels per group must be a multiple of 4");
  if (OH != (H + 2 - 3) / stride + 1 || OW != (W + 2 - 3) / stride + 1) return fail(fn, "output size mismatch (3x3, pad 1)");
  if ((long long)N * H * W + 512 >= (1ll << 31)) return fail(fn, "more than 2^31 pixels");
  return 0;
}

inline bool al16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

void pick_block(int quads, int& QB, int& PS) {
  QB = quads < 64 ? quads : 64;
  PS = GC_THREADS / QB;
}

template <class T>
int launch_fwd(GconvArgs a, hipStream_t st) {
  const int quads = a.OC / 4;
  pick_block(quads, a.QB, a.PS);
  const int nslices = (quads + a.QB - 1) / a.QB;
  const long long M = (long long)a.N * a.OH * a.OW;
  a.ntiles = (M + a.PS * GC_PPT - 1) / (a.PS * GC_PPT);
  // with statistics, every block ends with 2 * 4 * QB fp64 atomics: at most 2048 blocks, grid-striding over the pixel tiles
  const long long cap = a.stats ? (2048 + nslices - 1) / nslices : 4096;
  const unsigned gx = (unsigned)(a.ntiles < cap ? a.ntiles : cap);
  const dim3 grid(gx, (unsigned)nslices);
  switch (a.Cg) {
    case 4: hipLaunchKernelGGL((gconv_fwd_kernel<T, 4>), grid, dim3(GC_THREADS), 0, st, a); break;
    case 8: hipLaunchKernelGGL((gconv_fwd_kernel<T, 8>), grid, dim3(GC_THREADS), 0, st, a); break;
    case 16: hipLaunchKernelGGL((gconv_fwd_kernel<T, 16>), grid, dim3(GC_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL((gconv_fwd_kernel<T, 32>), grid, dim3(GC_THREADS), 0, st, a); break;
  }
  return check_launch("emrt_gconv2d");
}

template <class T>
int launch_dgrad(GconvArgs a, hipStream_t st) {
  const int quads = a.OC / 4;          // input-channel quads of the layer
  pick_block(quads, a.QB, a.PS);
  const int nslices = (quads + a.QB - 1) / a.QB;
  const long long M = (long long)a.N * a.OH * a.OW;
  a.ntiles = (M + a.PS * GC_PPT - 1) / (a.PS * GC_PPT);
  const unsigned gx = (unsigned)(a.ntiles < 4096 ? a.ntiles : 4096);
  hipLaunchKernelGGL((gconv_dgrad_kernel<T>), dim3(gx, (unsigned)nslices), dim3(GC_THREADS), 0, st, a);
  return check_launch("emrt_gconv2d_bwd");
}

template <class T>
int launch_wgrad(GwgradArgs a, hipStream_t st) {
  const int CH = a.Cg >= 8 ? 8 : 4;
  const long long threads = (long long)a.OC * 9 * (a.Cg / CH);
  const int M = a.N * a.OH * a.OW;
  // slices of the pixel reduction: about 1M threads in all, at least 32 pixels per slice (at 128K threads a slice of stage 1 was 585 pixels long
  // and the launch took 339 us, latency-bound; the extra fp32 atomics into dW cost far less)
  long long S = 1048576 / threads;
  if (S > M / 32) S = M / 32;
  if (S < 1) S = 1;
  a.rows_per_slice = (int)((M + S - 1) / S);
  S = (M + a.rows_per_slice - 1) / a.rows_per_slice;
  const dim3 grid((unsigned)((threads + GC_THREADS - 1) / GC_THREADS), (unsigned)S);
  switch (a.Cg) {
    case 4: hipLaunchKernelGGL((gconv_wgrad_kernel<T, 4>), grid, dim3(GC_THREADS), 0, st, a); break;
    case 8: hipLaunchKernelGGL((gconv_wgrad_kernel<T, 8>), grid, dim3(GC_THREADS), 0, st, a); break;
    case 16: hipLaunchKernelGGL((gconv_wgrad_kernel<T, 16>), grid, dim3(GC_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL((gconv_wgrad_kernel<T, 32>), grid, dim3(GC_THREADS), 0, st, a); break;
  }
  return check_launch("emrt_gconv2d_bwd");
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" int emrt_gconv2d(const void* in, const void* w, void* out, const float* bias, int N, int H, int W, int C, int ldin, long long in_bs,
                            int OH, int OW, int OC, int ldout, long long out_bs, int stride, int groups, int relu, double* bn_stats,
                            const float* out_scale, int dtype, void* stream) {
  EMRT_REQUIRE(in && w && out, "null pointer");
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(dtype != EMRT_F16 || !bn_stats, "fp16 (dtype 2) is inference-only: no BatchNorm statistics");
  if (int r = check_common(__func__, N, H, W, C, OH, OW, OC, stride, groups)) return r;
  EMRT_REQUIRE(ldin >= C && ldout >= OC && in_bs >= (long long)H * W * ldin && out_bs >= (long long)OH * OW * ldout, "strides smaller than the map");
  EMRT_REQUIRE(ldin % 8 == 0 && in_bs % 8 == 0 && ldout % 4 == 0 && out_bs % 4 == 0, "ldin / in_bs must be multiples of 8, ldout / out_bs of 4");
  EMRT_REQUIRE(al16(in) && al16(w) && ((uintptr_t)out) % (dtype == EMRT_F32 ? 16 : 8) == 0, "operands must be 16-byte aligned (out: one 4-channel vector)");
  GconvArgs a;
  a.x = in; a.w = w; a.y = out; a.bias = bias; a.scale = out_scale; a.stats = bn_stats;
  a.N = N; a.H = H; a.W = W; a.C = C; a.ldin = ldin; a.in_bs = in_bs;
  a.OH = OH; a.OW = OW; a.OC = OC; a.ldout = ldout; a.out_bs = out_bs;
  a.stride = stride; a.relu = relu; a.accumulate = 0; a.Cg = C / groups; a.Og = OC / groups; a.ldres = 0;
  hipStream_t st = (hipStream_t)stream;
  return with_fwd_dtype("emrt_gconv2d", dtype, [&](auto t) { return launch_fwd<decltype(t)>(a, st); });
}

extern "C" int emrt_gconv2d_bwd(const void* x, const void* dy, const void* w, void* dx, int lddx, long long dx_bs, int accumulate, float* dw, float* dbias,
                                int N, int H, int W, int C, int ldx, long long x_bs, int OH, int OW, int OC, int lddy, long long dy_bs, int stride,
                                int groups, int dtype, void* stream) {
  EMRT_REQUIRE_TRAIN_DTYPE(dtype);
  EMRT_REQUIRE(dy && (dx || dw || dbias), "null pointer");
  if (int r = check_common(__func__, N, H, W, C, OH, OW, OC, stride, groups)) return r;
  EMRT_REQUIRE(lddy >= OC && dy_bs >= (long long)OH * OW * lddy && lddy % 4 == 0 && dy_bs % 4 == 0, "lddy / dy_bs: multiples of 4, at least the map");
  EMRT_REQUIRE(((uintptr_t)dy) % 16 == 0, "dy must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    EMRT_REQUIRE(w && lddx >= C && dx_bs >= (long long)H * W * lddx && lddx % 4 == 0 && dx_bs % 4 == 0, "lddx / dx_bs: multiples of 4, at least the map");
    EMRT_REQUIRE(al16(w) && ((uintptr_t)dx) % (dtype == EMRT_F32 ? 16 : 8) == 0, "w must be 16-byte aligned, dx one 4-channel vector");
    GconvArgs a;
    a.x = dy; a.w = w; a.y = dx; a.bias = nullptr; a.scale = nullptr; a.stats = nullptr;
    a.N = N; a.H = OH; a.W = OW; a.C = OC; a.ldin = lddy; a.in_bs = dy_bs;
    a.OH = H; a.OW = W; a.OC = C; a.ldout = lddx; a.out_bs = dx_bs;
    a.stride = stride; a.relu = 0; a.accumulate = accumulate; a.Cg = C / groups; a.Og = OC / groups; a.ldres = 0;
    const int r = with_train_dtype("emrt_gconv2d_bwd", dtype, [&](auto t) { return launch_dgrad<decltype(t)>(a, st); });
    if (r) return r;
  }
  if (dw || dbias) {
    EMRT_REQUIRE(x && ldx >= C && x_bs >= (long long)H * W * ldx && ldx % 8 == 0 && x_bs % 8 == 0 && al16(x), "x: 16-byte aligned, ldx / x_bs multiples of 8");
    GwgradArgs b;
    b.x = x; b.dy = dy; b.dw = dw; b.dbias = dbias;
    b.N = N; b.H = H; b.W = W; b.C = C; b.ldx = ldx; b.x_bs = x_bs;
    b.OH = OH; b.OW = OW; b.OC = OC; b.lddy = lddy; b.dy_bs = dy_bs;
    b.stride = stride; b.Cg = C / groups; b.Og = OC / groups; b.rows_per_slice = 0;
    return with_train_dtype("emrt_gconv2d_bwd", dtype, [&](auto t) { return launch_wgrad<decltype(t)>(b, st); });
  }
  return 0;
}
