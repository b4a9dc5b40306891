// libemrt_hip_loss.so: cross entropy + Dice, one pass over the logits forward and one backward.  The public interface, the
// contract and the closed-form gradient are described in include/emrt_hip_loss.h; the pixel arithmetic is ../loss_pixel.hpp, the text the
// kernels of ../loss.hip compile, and the reductions are block_sum_256 / block_tree_sum_f64 of ../common.hpp.  A library of its own because
// the ABIs of the other three headers are pinned.
//
// Three kernels, the head (1 or 2) as the second grid dimension of the two streaming ones, so a pair is the single form's code and bits:
//   forward:  grid-stride over the pixels, at most LX_MAX_BLOCKS blocks per head.  Per thread the CE sums of wce_fwd_kernel (same grid rule,
//             same order, block_sum_256) and, for a chunk of eight classes held in registers, I_c and P_c; the integer T_c is counted per wave
//             by ballot.  The block's sums go into the workspace.  C <= 8 is one pass; a larger C makes one pass per chunk (the logits are read
//             again).
//   finalize: one block.  The blocks' partial sums are added in float64 (the CE sums by block_tree_sum_f64, the class sums a wave per row); result,
//             coef and the pair's total are written.
//   backward: grid-stride, every logit read and every gradient written once; coef rides in LDS.
// No floating-point atomics anywhere.
#include "../common.hpp"
#include "../loss_pixel.hpp"
#include "../../../include/emrt_hip_loss.h"

namespace emrt {
namespace {

thread_local char g_lx_err[512] = "";

int lx_fail(const char* fn, const char* msg) {
  snprintf(g_lx_err, sizeof(g_lx_err), "%s: %s", fn, msg);
  return -1;
}
int lx_check_launch(const char* fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_lx_err, sizeof(g_lx_err), "%s: launch failed: %s", fn, hipGetErrorString(e));
    return -2;
  }
  return 0;
}
#define LX_REQUIRE(cond, msg)                     \
  do {                                            \
    if (!(cond)) return lx_fail(__func__, msg);   \
  } while (0)

constexpr int LX_MAX_BLOCKS = 1024;      // blocks per head of the forward: the partials' workspace (the CE kernels' cap: the same grid rule)
constexpr int LX_BWD_BLOCKS = 4096;
constexpr int LX_CHUNK = 8;              // classes whose sums a thread keeps in registers
constexpr int LX_HEAD = 3;               // a block's partials start with {sum w CE, sum w, non-ignored count} ...
constexpr int LX_PER_CHUNK = 3 * LX_CHUNK;      // ... then per chunk {I[8], P[8], T[8]}
constexpr int LX_ROW_GROUP = 3;          // finalize: class rows whose loads a wave has in flight together

inline int lx_chunks(int C) { return (C + LX_CHUNK - 1) / LX_CHUNK; }
inline int lx_stride(int C) { return LX_HEAD + lx_chunks(C) * LX_PER_CHUNK; }      // floats per block

struct DiceHeads {
  const float* logits[2];
  float* result[2];       // float[8] per head
  float* coef[2];         // float[2 C] per head
  float* dlogits[2];      // backward only
  const float* up[2];     // backward only: upstream scalars or null
  float w[2];             // head weights (total / backward)
};

// Workspace of one head, stride(C) * LX_MAX_BLOCKS floats: first {sum w[y] CE, sum w[y], count} per block (block-major, as the CE kernels keep
// theirs), then per chunk of eight classes the rows I[8], P[8], T[8], each LX_MAX_BLOCKS long (sum-major: the finalize reads them coalesced).
__device__ __forceinline__ float* lx_class_rows(float* head_ws, int chunk) {
  return head_ws + (size_t)LX_HEAD * LX_MAX_BLOCKS + (size_t)chunk * LX_PER_CHUNK * LX_MAX_BLOCKS;
}

// The wave's sums of 16 per-thread values in 17 cross-lane exchanges, where 16 wave_sum calls take 96: at offset 32 a lane keeps one half of the
// values and hands the other half to its partner, at 16 a quarter, ... until every lane holds one value's sum over the 16 lanes that share its
// two low bits; offsets 2 and 1 finish it.  -> in lane L the sum of value L >> 2 over the wave.  One fixed order: the same bits in every run.
// (With 2 pixels per thread at 8 x 256 x 256 the forward is this reduction as much as the pass: with 27 wave_sum calls it took 26.6 us, with this 15.5.)
template <int HALF, int O>
__device__ __forceinline__ void wave_halve(float (&v)[2 * LX_CHUNK], int lane) {
  const bool up = (lane & O) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float keep = up ? v[i + HALF] : v[i], send = up ? v[i] : v[i + HALF];
    v[i] = keep + __shfl_xor(send, O, 64);
  }
}
__device__ __forceinline__ float wave_sum_16(float (&v)[2 * LX_CHUNK]) {
  const int lane = threadIdx.x & 63;
  wave_halve<8, 32>(v, lane);
  wave_halve<4, 16>(v, lane);
  wave_halve<2, 8>(v, lane);
  wave_halve<1, 4>(v, lane);
  float s = v[0];
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  return s;
}

// (__launch_bounds__(256, 8): eight waves per SIMD, i.e. at most 64 VGPRs, so that the pair's 2 x 1024 blocks are resident at once, 8 per CU)
template <bool CW>
__global__ __launch_bounds__(256, 8) void dice_fwd_kernel(DiceHeads hd, const long long* __restrict__ labels, const float* __restrict__ cw, int N, int C,
                                                          long long HW, int ignore_index, float* __restrict__ partial_all, int stride) {
  __shared__ float red[2 * LX_CHUNK * 4];
  __shared__ int redT[LX_CHUNK * 4];
  const int h = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* __restrict__ logits = hd.logits[h];
  float* __restrict__ head_ws = partial_all + (size_t)h * LX_MAX_BLOCKS * stride;
  const long long total = (long long)N * HW;
  for (int c0 = 0, chunk = 0; c0 < C; c0 += LX_CHUNK, ++chunk) {
    float acc[LX_HEAD] = {0.f, 0.f, 0.f};
    float IP[2 * LX_CHUNK];      // I[8], then P[8]
    int T[LX_CHUNK];             // the WAVE's counts: one ballot and population count per class and pixel
#pragma unroll
    for (int j = 0; j < LX_CHUNK; ++j) { IP[j] = 0.f; IP[LX_CHUNK + j] = 0.f; T[j] = 0; }
    // (the pixels of wce_fwd_kernel's grid-stride loop in its order, with a trip count that is the same in every lane of the block: all 64 lanes
    // of a wave take part in every ballot, so T is the same in all of them)
    for (long long base = (long long)blockIdx.x * blockDim.x; base < total; base += (long long)gridDim.x * blockDim.x) {
      const long long idx = base + threadIdx.x;
      const long long lab = idx < total ? labels[idx] : (long long)ignore_index;
#pragma unroll
      for (int j = 0; j < LX_CHUNK; ++j) {
        if (c0 + j < C) T[j] += __popcll(__ballot(lab != ignore_index && lab == c0 + j));
      }
      if (lab == ignore_index) continue;
      long long n, p;
      pixel_of(idx, total, HW, n, p);
      const float* lp = logits + n * C * HW + p;
      const PixelStats s = pixel_stats(lp, C, HW);
      if (c0 == 0) {      // the CE sums, as wce_fwd_kernel forms them
        float pr;
        const float ce = pixel_ce(lp, C, HW, lab, s, pr);
        const float w = class_weight_of<CW>(cw, lab, C);
        acc[0] += CW ? w * ce : ce;
        acc[1] += w;
        acc[2] += 1.f;
      }
      const float inv = 1.f / s.den;
#pragma unroll
      for (int j = 0; j < LX_CHUNK; ++j) {
        const int c = c0 + j;
        if (c < C) {      // (wave-uniform)
          const float pc = pixel_softmax(lp, c, HW, s, inv);
          IP[LX_CHUNK + j] += pc;
          if (lab == c) IP[j] += pc;
        }
      }
    }
    if (c0 == 0) {
      block_sum_256<LX_HEAD>(acc, red, head_ws + (size_t)blockIdx.x * LX_HEAD);
      __syncthreads();
    }
    const float s16 = wave_sum_16(IP);
    if ((lane & 3) == 0) red[wv * 2 * LX_CHUNK + (lane >> 2)] = s16;
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < LX_CHUNK; ++j) redT[wv * LX_CHUNK + j] = T[j];
    }
    __syncthreads();
    float* rows = lx_class_rows(head_ws, chunk);
    if (threadIdx.x < 2 * LX_CHUNK) {      // the four waves in order 0..3, as block_sum_256 adds them
      float a = 0.f;
      for (int w = 0; w < 4; ++w) a += red[w * 2 * LX_CHUNK + threadIdx.x];
      rows[(size_t)threadIdx.x * LX_MAX_BLOCKS + blockIdx.x] = a;
    } else if (threadIdx.x < LX_PER_CHUNK) {      // (a block counts fewer than 2^21 + 1 pixels: exact as a float)
      const int j = threadIdx.x - 2 * LX_CHUNK;
      rows[(size_t)threadIdx.x * LX_MAX_BLOCKS + blockIdx.x] = (float)(redT[j] + redT[LX_CHUNK + j] + redT[2 * LX_CHUNK + j] + redT[3 * LX_CHUNK + j]);
    }
    __syncthreads();
  }
}

// one block; per head: result = {L, CE, Dice, sum w, count, 0, 0, 0}, coef = {a_c, b_c}; total[0] = sum of w_h * L_h (null: not wanted).
//  * the CE sums of all heads go through ONE block_tree_sum_f64, which adds each of its columns in the same order whatever their number: the
//    bits of wce_finalize_kernel's sums.
//  * the class rows need no particular order, only a fixed one: a wave owns a row (I_c, P_c or T_c of one head, LX_MAX_BLOCKS floats, read
//    coalesced), its lanes add their 16 entries in float64 and a butterfly of six exchanges adds the lanes.
template <int NH>
__global__ __launch_bounds__(256) void dice_finalize_kernel(DiceHeads hd, const float* __restrict__ partial_all, int stride, int nblk, int C, float ce_weight,
                                                            float dice_weight, float smooth, float* __restrict__ total) {
  __shared__ double r[NH * LX_HEAD][256];
  __shared__ double row_sum[NH][LX_PER_CHUNK];
  __shared__ double dice_of[NH][EMRT_LX_MAX_CLASSES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double a[NH * LX_HEAD];
#pragma unroll
  for (int k = 0; k < NH * LX_HEAD; ++k) a[k] = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
#pragma unroll
      for (int k = 0; k < LX_HEAD; ++k) a[h * LX_HEAD + k] += partial_all[(size_t)h * LX_MAX_BLOCKS * stride + (size_t)i * LX_HEAD + k];
    }
  }
  block_tree_sum_f64<NH * LX_HEAD>(a, r);
  for (int c0 = 0, chunk = 0; c0 < C; c0 += LX_CHUNK, ++chunk) {
    // wave wv owns the rows q = wv + 4 rr; a lane takes every 64th entry of a row.  The loads of LX_ROW_GROUP rows are issued together and none is
    // conditional (past nblk the index is clamped and the value dropped): the partials were written by other XCDs a moment ago, a load of them
    // takes about 0.3 us, and behind a per-load `i < nblk ? row[i] : 0` the 16 loads of a row waited for one another (60 us for the launch).
    constexpr int PER_LANE = LX_MAX_BLOCKS / 64, ROWS = NH * LX_PER_CHUNK / 4;
    static_assert(ROWS % LX_ROW_GROUP == 0, "the rows of a wave come in whole groups");
    for (int r0 = 0; r0 < ROWS; r0 += LX_ROW_GROUP) {
      float x[LX_ROW_GROUP][PER_LANE];
#pragma unroll
      for (int g = 0; g < LX_ROW_GROUP; ++g) {
        const int q = wv + 4 * (r0 + g), h = q / LX_PER_CHUNK, k = q - h * LX_PER_CHUNK;
        const float* row = lx_class_rows((float*)partial_all + (size_t)h * LX_MAX_BLOCKS * stride, chunk) + (size_t)k * LX_MAX_BLOCKS;
#pragma unroll
        for (int u = 0; u < PER_LANE; ++u) {
          const int i = u * 64 + lane;
          x[g][u] = row[i < nblk ? i : 0];
        }
      }
#pragma unroll
      for (int g = 0; g < LX_ROW_GROUP; ++g) {
        const int q = wv + 4 * (r0 + g), h = q / LX_PER_CHUNK, k = q - h * LX_PER_CHUNK;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < PER_LANE; ++u) s += (double)(u * 64 + lane < nblk ? x[g][u] : 0.f);      // (entries from nblk on were never written)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) row_sum[h][k] = s;
      }
    }
    __syncthreads();
    if (threadIdx.x < NH * LX_CHUNK) {      // class c of head h from its I, P, T: dice_c and the backward's coefficients
      const int h = threadIdx.x / LX_CHUNK, j = threadIdx.x - h * LX_CHUNK, c = c0 + j;
      if (c < C) {
        const double s = (double)smooth, dw = (double)dice_weight, U = row_sum[h][LX_CHUNK + j] + row_sum[h][2 * LX_CHUNK + j] + s;
        const double num = 2.0 * row_sum[h][j] + s;
        const bool live = U > 0.0;      // U = 0 (only with s = 0, no pixel of the class and no probability mass): dice 1, no gradient
        float* coef = hd.coef[h];
        dice_of[h][c] = live ? num / U : 1.0;
        coef[c] = live ? (float)(-2.0 * dw / ((double)C * U)) : 0.f;
        coef[C + c] = live ? (float)(dw * num / ((double)C * U * U)) : 0.f;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int h = 0; h < NH; ++h) {
      const double ce_sum = r[h * LX_HEAD][0], sum_w = r[h * LX_HEAD + 1][0], count = r[h * LX_HEAD + 2][0];
      double dsum = 0.0;
      for (int c = 0; c < C; ++c) dsum += dice_of[h][c];
      // Paddle's cross_entropy divides by count + (count == 0): every pixel ignored (or of weight 0) gives CE 0, not 0 / 0 (wce_finalize_kernel)
      const double den = sum_w > 0.0 ? sum_w : 1.0;
      const float ce = (float)(ce_sum / den), dice = (float)(1.0 - dsum / (double)C);
      float* result = hd.result[h];
      result[0] = (float)((double)ce_weight * (double)ce + (double)dice_weight * (double)dice);      // (weights 1 and 0: the bits of ce)
      result[1] = ce;
      result[2] = dice;
      result[3] = (float)sum_w;
      result[4] = (float)count;
      result[5] = 0.f; result[6] = 0.f; result[7] = 0.f;
      t += hd.w[h] * result[0];
    }
    if (total) total[0] = t;
  }
}

// dlogits_k = w_h * up_h * ( ce_weight * w[y] / sum w * (p_k - [y = k]) + p_k * (g_k - sum_c p_c g_c) ),  g_c = a_c [y = c] + b_c; ignored: zeros
template <bool CW>
__global__ __launch_bounds__(256) void dice_bwd_kernel(DiceHeads hd, const long long* __restrict__ labels, const float* __restrict__ cw, int N, int C,
                                                       long long HW, int ignore_index, float ce_weight) {
  __shared__ float sa[EMRT_LX_MAX_CLASSES], sb[EMRT_LX_MAX_CLASSES];
  const int h = blockIdx.y;
  const float* __restrict__ logits = hd.logits[h];
  float* __restrict__ dlogits = hd.dlogits[h];
  const float* __restrict__ res = hd.result[h];
  for (int c = threadIdx.x; c < C; c += 256) { sa[c] = hd.coef[h][c]; sb[c] = hd.coef[h][C + c]; }
  __syncthreads();
  const long long total = (long long)N * HW;
  const float den_w = res[3] > 0.f ? res[3] : 1.f;
  const float gd = hd.w[h] * (hd.up[h] ? hd.up[h][0] : 1.f);
  const float gce = gd * ce_weight / den_w;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long lab = labels[idx];
    long long n, p;
    pixel_of(idx, total, HW, n, p);
    const float* lp = logits + n * C * HW + p;
    float* dp = dlogits + n * C * HW + p;
    if (lab == ignore_index) {
      pixel_zero_store(dp, C, HW);
      continue;
    }
    const float w = class_weight_of<CW>(cw, lab, C);
    const float gw = CW ? gce * w : gce;
    const PixelStats s = pixel_stats(lp, C, HW);
    const float inv = 1.f / s.den;
    float pg = 0.f;      // sum_c p_c g_c
    for (int c = 0; c < C; ++c) pg += pixel_softmax(lp, c, HW, s, inv) * (sb[c] + (c == lab ? sa[c] : 0.f));
    for (int c = 0; c < C; ++c) {
      const float pc = pixel_softmax(lp, c, HW, s, inv);
      const float g = sb[c] + (c == lab ? sa[c] : 0.f);
      dp[c * HW] = gw * (pc - (c == lab ? 1.f : 0.f)) + gd * (pc * (g - pg));
    }
  }
}

inline bool weight_ok(float v) { return v >= 0.f; }      // (false for NaN)

int dice_forward(const char* fn, int NH, const DiceHeads& hd, const long long* labels, const float* cw, int N, int C, int H, int W, int ignore_index,
                 float ce_weight, float dice_weight, float smooth, float* total, void* workspace, void* stream) {
  const int grid = stream_grid((long long)N * H * W, LX_MAX_BLOCKS), stride = lx_stride(C);
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid, NH), dim3(256), 0, st, hd, labels, cw, N, C, (long long)H * W, ignore_index, (float*)workspace, stride);
  };
  if (cw) launch(dice_fwd_kernel<true>);
  else launch(dice_fwd_kernel<false>);
  auto finalize = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(256), 0, st, hd, (const float*)workspace, stride, grid, C, ce_weight, dice_weight, smooth, total);
  };
  if (NH == 2) finalize(dice_finalize_kernel<2>);
  else finalize(dice_finalize_kernel<1>);
  return lx_check_launch(fn);
}

int dice_backward(const char* fn, int NH, const DiceHeads& hd, const long long* labels, const float* cw, int N, int C, int H, int W, int ignore_index,
                  float ce_weight, void* stream) {
  const int grid = stream_grid((long long)N * H * W, LX_BWD_BLOCKS);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid, NH), dim3(256), 0, (hipStream_t)stream, hd, labels, cw, N, C, (long long)H * W, ignore_index, ce_weight);
  };
  if (cw) launch(dice_bwd_kernel<true>);
  else launch(dice_bwd_kernel<false>);
  return lx_check_launch(fn);
}

#define LX_CLASSES_MSG "C must be 1..64 (EMRT_LX_MAX_CLASSES)"
#define LX_REQUIRE_SHAPE(N, C, H, W)                                              \
  LX_REQUIRE((C) >= 1 && (C) <= EMRT_LX_MAX_CLASSES, LX_CLASSES_MSG);             \
  LX_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG)
#define LX_REQUIRE_WEIGHTS(ce_weight, dice_weight, smooth)                                                               \
  LX_REQUIRE(weight_ok(ce_weight) && weight_ok(dice_weight), "ce_weight and dice_weight must be >= 0 and not NaN");      \
  LX_REQUIRE(ce_weight > 0.f || dice_weight > 0.f, "ce_weight and dice_weight are both 0");                              \
  LX_REQUIRE(weight_ok(smooth), "smooth must be >= 0 and not NaN")

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" const char* emrt_lx_last_error(void) { return g_lx_err; }

extern "C" int emrt_lx_version(void) { return 1; }

extern "C" size_t emrt_lx_dice_ce_workspace_bytes(int C, int heads) {
  if (C < 1 || C > EMRT_LX_MAX_CLASSES || heads < 1 || heads > 2) return 0;
  return (size_t)heads * LX_MAX_BLOCKS * lx_stride(C) * sizeof(float);
}

extern "C" int emrt_lx_dice_ce_fwd(const float* logits, const long long* labels, const float* class_weight, int N, int C, int H, int W, int ignore_index,
                                   float ce_weight, float dice_weight, float smooth, float* result, float* coef, void* workspace, void* stream) {
  LX_REQUIRE(logits && labels && result && coef && workspace, "null pointer");
  LX_REQUIRE_SHAPE(N, C, H, W);
  LX_REQUIRE_WEIGHTS(ce_weight, dice_weight, smooth);
  return dice_forward(__func__, 1, DiceHeads{{logits}, {result}, {coef}, {}, {}, {1.f}}, labels, class_weight, N, C, H, W, ignore_index, ce_weight,
                      dice_weight, smooth, nullptr, workspace, stream);
}

extern "C" int emrt_lx_dice_ce_bwd(const float* logits, const long long* labels, const float* class_weight, const float* result, const float* coef,
                                   const float* upstream, float weight, float ce_weight, int N, int C, int H, int W, int ignore_index, float* dlogits,
                                   void* stream) {
  LX_REQUIRE(logits && labels && result && coef && dlogits, "null pointer");
  LX_REQUIRE_SHAPE(N, C, H, W);
  LX_REQUIRE(weight_ok(ce_weight), "ce_weight must be >= 0 and not NaN");
  return dice_backward(__func__, 1, DiceHeads{{logits}, {(float*)result}, {(float*)coef}, {dlogits}, {upstream}, {weight}}, labels, class_weight, N, C, H, W,
                       ignore_index, ce_weight, stream);
}

extern "C" int emrt_lx_dice_ce_pair_fwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, int N, int C, int H,
                                        int W, int ignore_index, float wa, float wb, float ce_weight, float dice_weight, float smooth, float* res_a,
                                        float* res_b, float* coef_a, float* coef_b, float* total, void* workspace, void* stream) {
  LX_REQUIRE(logits_a && logits_b && labels && res_a && res_b && coef_a && coef_b && total && workspace, "null pointer");
  LX_REQUIRE_SHAPE(N, C, H, W);
  LX_REQUIRE_WEIGHTS(ce_weight, dice_weight, smooth);
  return dice_forward(__func__, 2, DiceHeads{{logits_a, logits_b}, {res_a, res_b}, {coef_a, coef_b}, {}, {}, {wa, wb}}, labels, class_weight, N, C, H, W,
                      ignore_index, ce_weight, dice_weight, smooth, total, workspace, stream);
}

extern "C" int emrt_lx_dice_ce_pair_bwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, const float* res_a,
                                        const float* res_b, const float* coef_a, const float* coef_b, const float* up_a, const float* up_b, float wa,
                                        float wb, float ce_weight, int N, int C, int H, int W, int ignore_index, float* dlogits_a, float* dlogits_b,
                                        void* stream) {
  LX_REQUIRE(logits_a && logits_b && labels && res_a && res_b && coef_a && coef_b && dlogits_a && dlogits_b, "null pointer");
  LX_REQUIRE_SHAPE(N, C, H, W);
  LX_REQUIRE(weight_ok(ce_weight), "ce_weight must be >= 0 and not NaN");
  return dice_backward(__func__, 2, DiceHeads{{logits_a, logits_b}, {(float*)res_a, (float*)res_b}, {(float*)coef_a, (float*)coef_b}, {dlogits_a, dlogits_b},
                                              {up_a, up_b}, {wa, wb}},
                       labels, class_weight, N, C, H, W, ignore_index, ce_weight, stream);
}
