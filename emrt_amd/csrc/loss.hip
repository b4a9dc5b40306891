// The loss kernels for gfx950: softmax cross entropy, its class-weighted form and hard-pixel mining, all HBM-bound streaming
// passes over fp32 NCHW logits.  ONE copy of the per-pixel arithmetic (pixel_stats / pixel_ce / pixel_grad_store / pixel_zero_store) serves every
// kernel here, so "pair == two singles", "unit weights == plain" and "OHEM pair == singles" hold to the last bit by construction.
//
//  * softmax cross entropy with ignore_index (reference: losses/mix_softmax_cross_entropy_loss.py:27-35 -> paddle
//    nn.CrossEntropyLoss(ignore_index=255, axis=1)): the class-weighted family below with the weight compiled out.
//  * OhemCrossEntropyLoss (reference: losses/ohem_cross_entropy_loss.py:41-79).  The reference finds its threshold with an argsort over every
//    pixel and a device-to-host read in the middle of the loss; here the min_kept-th smallest probability is found by an exact radix select
//    (11 + 11 + 10 bits, most significant digit first) over the fp32 bit patterns, entirely on the device: a captured step stays one graph.
//    Only integer atomics take part in the selection, so the threshold -- and with it the mask, the loss and the gradient -- is the same bits
//    in every run.
//  * nn.CrossEntropyLoss(weight=w, ignore_index) (reference: losses/cross_entropy_loss.py:30-35; the form MixSoftmaxCrossEntropyLoss is built
//    on): loss = sum w[y] CE / sum w[y] over the non-ignored pixels, one head or the two heads of the Mix loss in one pass.
#include <cfloat>
#include "common.hpp"
#include "loss_pixel.hpp"

using namespace emrt;

namespace {

constexpr int OH_BINS = 2048;              // bins of one digit's histogram (the last digit uses 1024 of them)
constexpr int OH_STATE = 16;               // words of selection state behind the three histograms
constexpr int OH_MAX_BLOCKS = 1024;
constexpr int OH_HIST_BLOCKS = 128;        // most blocks per head of the digit-histogram launches
constexpr unsigned OH_IGNORED = 0xffffffffu;      // stored "probability" of an ignored pixel: a NaN pattern no computed value has; p < t is false for it

// state words
enum { ST_PREFIX = 0, ST_RANK = 1, ST_DONE = 2, ST_VALID = 3 };

// NH = 1 head, or the main and the auxiliary head on the same labels: blockIdx.y is the head, so two heads cost the launches of one
template <int NH>
struct OhemHeads {
  const float* logits[NH];
  float* prob[NH];         // stored p, [npix] per head (the caller's: it lives until the backward)
  float* result[NH];       // float[8] per head
  float* dlogits[NH];      // backward only
  const float* up[NH];     // backward only: upstream scalars or null
  float w[NH];             // head weights (total / backward)
};

// workspace layout for NH heads: NH x (3 histograms + state) in one piece (one memset), NH x loss partials, NH x per-pixel CE
struct OhemWs {
  unsigned* hist;       // [NH][3 * OH_BINS + OH_STATE]
  float* partial;       // [NH][OH_MAX_BLOCKS][2]
  float* ce;            // [NH][npix]
};
constexpr int OH_SEL_WORDS = 3 * OH_BINS + OH_STATE;
inline size_t ohem_bytes(long long npix, int heads) { return (size_t)heads * ((size_t)OH_SEL_WORDS * 4 + (size_t)OH_MAX_BLOCKS * 2 * 4 + (size_t)npix * 4); }
inline OhemWs ohem_ws(void* workspace, int heads) {
  OhemWs w;
  w.hist = (unsigned*)workspace;
  w.partial = (float*)(w.hist + (size_t)heads * OH_SEL_WORDS);
  w.ce = w.partial + (size_t)heads * OH_MAX_BLOCKS * 2;
  return w;
}

// (the pixel core -- pixel_of, pixel_stats, pixel_ce, pixel_grad_store, pixel_zero_store, class_weight_of -- is loss_pixel.hpp)

// the block's LDS histogram -> the global bins: one integer atomic per non-empty bin
__device__ __forceinline__ void flush_bins(const unsigned* lh, unsigned* __restrict__ gh, int nbins) {
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += blockDim.x) {
    const unsigned v = lh[i];
    if (v) atomicAdd(gh + i, v);
  }
}

// pass over the logits: p = softmax probability of the pixel's own class and its CE, both stored;
// histogram of the keys' first digit over the non-ignored pixels (its total is num_valid)
template <int NH>
__global__ __launch_bounds__(256) void ohem_prob_kernel(OhemHeads<NH> hd, const long long* __restrict__ labels, int N, int C, long long HW, int ignore_index,
                                                        OhemWs ws) {
  __shared__ unsigned lh[OH_BINS];
  const int h = blockIdx.y;
  const float* __restrict__ logits = hd.logits[h];
  float* __restrict__ prob = hd.prob[h];
  const long long total = (long long)N * HW;
  float* __restrict__ ce = ws.ce + h * total;
  for (int i = threadIdx.x; i < OH_BINS; i += 256) lh[i] = 0u;
  __syncthreads();
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long lab = labels[idx];
    if (lab == ignore_index) {
      prob[idx] = __uint_as_float(OH_IGNORED);
      ce[idx] = 0.f;
      continue;
    }
    long long n, p;
    pixel_of(idx, total, HW, n, p);
    const float* lp = logits + n * C * HW + p;
    float pr;
    const float v = pixel_ce(lp, C, HW, lab, pixel_stats(lp, C, HW), pr);
    prob[idx] = pr;
    ce[idx] = v;
    atomicAdd(&lh[__float_as_uint(pr) >> 21], 1u);
  }
  flush_bins(lh, ws.hist + h * OH_SEL_WORDS, OH_BINS);
}

// digits 1 and 2: histogram of the next digit over the keys that carry the prefix found so far
template <int NH, int PASS>
__global__ __launch_bounds__(256) void ohem_hist_kernel(OhemHeads<NH> hd, long long total, OhemWs ws) {
  constexpr int NB = PASS == 1 ? OH_BINS : OH_BINS / 2;
  __shared__ unsigned lh[NB];
  const int h = blockIdx.y;
  unsigned* hist_all = ws.hist + h * OH_SEL_WORDS;
  const unsigned* state = hist_all + 3 * OH_BINS;
  if (state[ST_DONE]) return;                 // the threshold is already decided (keep-all or min_kept == 0): nothing to select
  const unsigned prefix = state[ST_PREFIX];
  const float* __restrict__ prob = hd.prob[h];
  for (int i = threadIdx.x; i < NB; i += 256) lh[i] = 0u;
  __syncthreads();
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const unsigned key = __float_as_uint(prob[idx]);
    if (PASS == 1) {
      if ((key >> 21) == (prefix >> 21)) atomicAdd(&lh[(key >> 10) & 2047u], 1u);
    } else {
      if ((key >> 10) == (prefix >> 10)) atomicAdd(&lh[key & 1023u], 1u);
    }
  }
  flush_bins(lh, hist_all + PASS * OH_BINS, NB);
}

// one block per head: scan the bins of digit PASS, find the bin that holds the wanted rank, extend the prefix.  PASS 0 also applies the branches that
// need no selection; PASS 2 turns the full key into the threshold.  result[2] = threshold (+inf: every non-ignored pixel is kept).
template <int NH, int PASS>
__global__ __launch_bounds__(256) void ohem_scan_kernel(OhemHeads<NH> hd, OhemWs ws, long long min_kept, float thresh) {
  constexpr int NB = PASS == 2 ? OH_BINS / 2 : OH_BINS, PER = NB / 256, SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
  __shared__ unsigned sc[256];
  const int hh = blockIdx.x;
  unsigned* hist_all = ws.hist + hh * OH_SEL_WORDS;
  unsigned* state = hist_all + 3 * OH_BINS;
  float* result = hd.result[hh];
  if (PASS > 0 && state[ST_DONE]) return;
  const unsigned prefix = PASS == 0 ? 0u : state[ST_PREFIX];
  unsigned rank = PASS == 0 ? 0u : state[ST_RANK];
  const unsigned* h = hist_all + PASS * OH_BINS + threadIdx.x * PER;
  unsigned loc[PER], s = 0u;
#pragma unroll
  for (int i = 0; i < PER; ++i) { loc[i] = h[i]; s += loc[i]; }
  sc[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {          // inclusive scan of the 256 per-thread sums
    const unsigned add = (int)threadIdx.x >= o ? sc[threadIdx.x - o] : 0u;
    __syncthreads();
    sc[threadIdx.x] += add;
    __syncthreads();
  }
  if (PASS == 0) {
    const unsigned num_valid = sc[255];
    const bool keep_all = num_valid == 0u || min_kept >= (long long)num_valid, no_rank = min_kept <= 0;
    if (keep_all || no_rank) {
      if (threadIdx.x == 0) {
        state[ST_VALID] = num_valid;
        state[ST_DONE] = 1u;
        result[2] = keep_all ? __uint_as_float(0x7f800000u) : thresh;
      }
      return;
    }
    rank = (unsigned)min_kept;
    if (threadIdx.x == 0) state[ST_VALID] = num_valid;
  }
  unsigned before = sc[threadIdx.x] - s;        // keys in the bins below this thread's
  if (rank > before && rank <= before + s) {    // exactly one thread: the ranks 1..total are covered once
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (rank > before && rank <= before + loc[i]) {
        const unsigned key = prefix | ((unsigned)(threadIdx.x * PER + i) << SHIFT);
        if (PASS == 2) {
          const float kth = __uint_as_float(key);
          result[2] = kth > thresh ? kth : thresh;
        } else {
          state[ST_PREFIX] = key;
          state[ST_RANK] = rank - before;
        }
      }
      before += loc[i];
    }
  }
}

// kept = p < threshold on the STORED values (an ignored pixel's stored pattern compares false)
template <int NH>
__global__ __launch_bounds__(256) void ohem_sum_kernel(OhemHeads<NH> hd, long long total, OhemWs ws) {
  __shared__ float red[2 * 4];
  const int h = blockIdx.y;
  const float* __restrict__ prob = hd.prob[h];
  const float* __restrict__ ce = ws.ce + h * total;
  float* partial = ws.partial + h * OH_MAX_BLOCKS * 2;
  const float thr = hd.result[h][2];
  float acc[2] = {0.f, 0.f};      // loss, kept count
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    if (prob[idx] < thr) { acc[0] += ce[idx]; acc[1] += 1.f; }
  }
  block_sum_256<2>(acc, red, partial + blockIdx.x * 2);
}

// one block; per head: result = {loss, kept count, threshold (written by the scan), non-ignored count, 1 / (kept + 1e-5 npix) or 0 when nothing is
// kept}; total[0] = sum of w_h * loss_h (null: not wanted)
template <int NH>
__global__ __launch_bounds__(256) void ohem_finalize_kernel(OhemHeads<NH> hd, OhemWs ws, int nblk, double npix, float* __restrict__ total) {
  __shared__ double r[2][256];
  float t = 0.f;
  for (int h = 0; h < NH; ++h) {
    const float* partial = ws.partial + h * OH_MAX_BLOCKS * 2;
    double a[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += 256) { a[0] += partial[i * 2]; a[1] += partial[i * 2 + 1]; }
    block_tree_sum_f64<2>(a, r);
    if (threadIdx.x == 0) {
      // mean(loss * mask) / (mean(mask) + 1e-5) of the reference, numerator and denominator times npix (npix counts the ignored pixels too)
      const double den = r[1][0] + 1e-5 * npix;
      float* result = hd.result[h];
      result[0] = (float)(r[0][0] / den);
      result[1] = (float)r[1][0];
      result[3] = (float)ws.hist[h * OH_SEL_WORDS + 3 * OH_BINS + ST_VALID];
      result[4] = r[1][0] > 0.0 ? (float)(1.0 / den) : 0.f;
      t += hd.w[h] * result[0];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && total) total[0] = t;
}

// dlogits = weight * upstream * (softmax - onehot) / (kept + 1e-5 npix) on the kept pixels (membership from the stored p, as the forward), 0 elsewhere
template <int NH>
__global__ __launch_bounds__(256) void ohem_bwd_kernel(OhemHeads<NH> hd, const long long* __restrict__ labels, int N, int C, long long HW, int ignore_index) {
  const int h = blockIdx.y;
  const float* __restrict__ logits = hd.logits[h];
  const float* __restrict__ prob = hd.prob[h];
  float* __restrict__ dlogits = hd.dlogits[h];
  const long long total = (long long)N * HW;
  const float thr = hd.result[h][2];
  const float g = hd.w[h] * (hd.up[h] ? hd.up[h][0] : 1.f) * hd.result[h][4];
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long lab = labels[idx];
    long long n, p;
    pixel_of(idx, total, HW, n, p);
    const float* lp = logits + n * C * HW + p;
    float* dp = dlogits + n * C * HW + p;
    if (lab == ignore_index || !(prob[idx] < thr)) pixel_zero_store(dp, C, HW);
    else pixel_grad_store(lp, dp, C, HW, lab, g);
  }
}

// ------------------------------------------------------------------------------------------------
// cross entropy, NH = 1 head or the 2 heads of the Mix loss (mix_softmax_cross_entropy_loss.py:29-35,44-51: CE(main) + 0.4 CE(aux) on the SAME
// labels, read once).  CW = true: class-weighted, cw[C] on the device; CW = false: the plain CE -- no weight load, no multiply: what
// emrt_softmax_ce_* runs, and emrt_wce_* with class_weight == NULL.
// ------------------------------------------------------------------------------------------------
// The kernels take the heads as plain __restrict__ pointer and scalar arguments (head b unused when NH = 1), as the plain CE kernels always
// did: handed over as a by-value record the plain forward measured 0.6 us slower at 8 x 6 x 256 x 256.
// partial[block] = {sum w[y] CE of head a, (of head b,) sum w[y]}
template <int NH, bool CW>
__global__ __launch_bounds__(256) void wce_fwd_kernel(const float* __restrict__ la, const float* __restrict__ lb, const long long* __restrict__ labels,
                                                      const float* __restrict__ cw, int N, int C, long long HW, int ignore_index,
                                                      float* __restrict__ partial) {
  __shared__ float red[(NH + 1) * 4];
  const long long total = (long long)N * HW;
  float acc[NH + 1];
#pragma unroll
  for (int h = 0; h <= NH; ++h) acc[h] = 0.f;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long lab = labels[idx];
    if (lab == ignore_index) continue;
    long long n, p;
    pixel_of(idx, total, HW, n, p);
    const float w = class_weight_of<CW>(cw, lab, C);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const float ce = pixel_ce((h ? lb : la) + n * C * HW + p, C, HW, lab);
      acc[h] += CW ? w * ce : ce;
    }
    acc[NH] += w;
  }
  block_sum_256<NH + 1>(acc, red, partial + blockIdx.x * (NH + 1));
}

// result of head h = {sum w CE / sum w, sum w} (plain: {mean loss over the non-ignored pixels, their count}); two heads: total[0] = wa * loss_a +
// wb * loss_b
template <int NH>
__global__ __launch_bounds__(256) void wce_finalize_kernel(const float* __restrict__ partial, int nblk, float wa, float wb, float* __restrict__ res_a,
                                                           float* __restrict__ res_b, float* __restrict__ total) {
  __shared__ double r[NH + 1][256];
  double a[NH + 1];
#pragma unroll
  for (int h = 0; h <= NH; ++h) a[h] = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
    for (int h = 0; h <= NH; ++h) a[h] += partial[i * (NH + 1) + h];
  }
  block_tree_sum_f64<NH + 1>(a, r);
  if (threadIdx.x == 0) {
    // Paddle's cross_entropy divides by count + (count == 0): every pixel ignored (or of weight 0) gives loss 0, not 0 / 0
    const double den = r[NH][0] > 0.0 ? r[NH][0] : 1.0;
    res_a[0] = (float)(r[0][0] / den); res_a[1] = (float)r[NH][0];
    if (NH == 2) {
      res_b[0] = (float)(r[NH - 1][0] / den); res_b[1] = (float)r[NH][0];
      // two products and one add in the compiled kernel (no fused multiply-add), for the plain and the weighted pair alike; the weighted pair used
      // to start the sum from 0.f, which differs only in the sign of a zero total under negative head weights
      total[0] = wa * res_a[0] + wb * res_b[0];
    }
  }
}

// dlogits_h = w_h * up_h * w[y] * (softmax - onehot) / sum w[y]     (up_h: device scalar or null == 1; all ignored: zero gradient)
template <int NH, bool CW>
__global__ __launch_bounds__(256) void wce_bwd_kernel(const float* __restrict__ la, const float* __restrict__ lb, const long long* __restrict__ labels,
                                                      const float* __restrict__ cw, const float* __restrict__ res, const float* __restrict__ up_a,
                                                      const float* __restrict__ up_b, float wa, float wb, int N, int C, long long HW, int ignore_index,
                                                      float* __restrict__ da, float* __restrict__ db) {
  const long long total = (long long)N * HW;
  const float den_w = res[1] > 0.f ? res[1] : 1.f, inv_den = 1.f / den_w;
  // (both forms multiply by the reciprocal, so a head of the pair carries the single call's bits; the single form used to divide, which differed
  // from the pair in the last bit wherever the denominator is no power of two)
  const float ga = wa * (up_a ? up_a[0] : 1.f) * inv_den;
  const float gb = NH == 1 ? 0.f : wb * (up_b ? up_b[0] : 1.f) * inv_den;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long lab = labels[idx];
    long long n, p;
    pixel_of(idx, total, HW, n, p);
    const float w = lab == ignore_index ? 0.f : class_weight_of<CW>(cw, lab, C);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const float* lp = (h ? lb : la) + n * C * HW + p;
      float* dp = (h ? db : da) + n * C * HW + p;
      const float g = h ? gb : ga;
      if (lab == ignore_index) pixel_zero_store(dp, C, HW);
      else pixel_grad_store(lp, dp, C, HW, lab, CW ? g * w : g);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side.  Grids: one thread per pixel, capped (1024 blocks forward -- the partials' workspace --, 4096 backward, 128 for the digit histograms).
// ------------------------------------------------------------------------------------------------
// the one filler of the OHEM head record: every array is per head, in head order
template <int NH>
OhemHeads<NH> ohem_heads(const float* const (&logits)[NH], const float* const (&prob)[NH], const float* const (&result)[NH], float* const (&dlogits)[NH],
                         const float* const (&up)[NH], const float (&w)[NH]) {
  OhemHeads<NH> hd;
  for (int h = 0; h < NH; ++h) {
    hd.logits[h] = logits[h]; hd.prob[h] = (float*)prob[h]; hd.result[h] = (float*)result[h]; hd.dlogits[h] = dlogits[h]; hd.up[h] = up[h]; hd.w[h] = w[h];
  }
  return hd;
}

// the heads of a CE call on the host, a = [0], b = [1] (null / 0 when NH = 1)
struct WceHeads {
  const float* logits[2];
  float* out[2];          // forward: result[2] per head; backward: dlogits
  const float* up[2];
  float w[2];
};

// forward of the CE family: the streaming launch + the one-block finalize; cw == nullptr takes the plain kernels
template <int NH>
int wce_forward(const char* fn, const WceHeads& hd, const long long* labels, const float* cw, int N, int C, int H, int W, int ignore_index, float* total,
                void* workspace, void* stream) {
  const int grid = stream_grid((long long)N * H * W, 1024);
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, hd.logits[0], hd.logits[1], labels, cw, N, C, (long long)H * W, ignore_index, (float*)workspace);
  };
  if (cw) launch(wce_fwd_kernel<NH, true>);
  else launch(wce_fwd_kernel<NH, false>);
  hipLaunchKernelGGL(wce_finalize_kernel<NH>, dim3(1), dim3(256), 0, st, (const float*)workspace, grid, hd.w[0], hd.w[1], hd.out[0], hd.out[1], total);
  return check_launch(fn);
}
template <int NH>
int wce_backward(const char* fn, const WceHeads& hd, const long long* labels, const float* cw, const float* res, int N, int C, int H, int W,
                 int ignore_index, void* stream) {
  const int grid = stream_grid((long long)N * H * W, 4096);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, hd.logits[0], hd.logits[1], labels, cw, res, hd.up[0], hd.up[1], hd.w[0], hd.w[1],
                       N, C, (long long)H * W, ignore_index, hd.out[0], hd.out[1]);
  };
  if (cw) launch(wce_bwd_kernel<NH, true>);
  else launch(wce_bwd_kernel<NH, false>);
  return check_launch(fn);
}

template <int NH>
int ohem_forward(const char* fn, const OhemHeads<NH>& hd, const long long* labels, int N, int C, int H, int W, int ignore_index, float thresh,
                 long long min_kept, float* total, void* workspace, void* stream) {
  const long long npix = (long long)N * H * W, HW = (long long)H * W;
  const OhemWs w = ohem_ws(workspace, NH);
  hipStream_t st = (hipStream_t)stream;
  const int grid = stream_grid(npix, OH_MAX_BLOCKS);
  // the digit histograms read 4 bytes per pixel and end with one global atomic per non-empty bin and block: the second digit fills most of its 2048
  // bins, so at 1024 blocks the flush (up to 4 M atomics for two heads) was most of the kernel: 18.9 us -> 10.9 us (rocprofv3 average over 8 x 256^2 and 4 x 512^2)
  const int hgrid = stream_grid(npix, OH_HIST_BLOCKS);
  if (hipMemsetAsync(w.hist, 0, (size_t)NH * OH_SEL_WORDS * 4, st) != hipSuccess) return check_launch(fn);
  hipLaunchKernelGGL(ohem_prob_kernel<NH>, dim3(grid, NH), dim3(256), 0, st, hd, labels, N, C, HW, ignore_index, w);
  hipLaunchKernelGGL((ohem_scan_kernel<NH, 0>), dim3(NH), dim3(256), 0, st, hd, w, min_kept, thresh);
  hipLaunchKernelGGL((ohem_hist_kernel<NH, 1>), dim3(hgrid, NH), dim3(256), 0, st, hd, npix, w);
  hipLaunchKernelGGL((ohem_scan_kernel<NH, 1>), dim3(NH), dim3(256), 0, st, hd, w, min_kept, thresh);
  hipLaunchKernelGGL((ohem_hist_kernel<NH, 2>), dim3(hgrid, NH), dim3(256), 0, st, hd, npix, w);
  hipLaunchKernelGGL((ohem_scan_kernel<NH, 2>), dim3(NH), dim3(256), 0, st, hd, w, min_kept, thresh);
  hipLaunchKernelGGL(ohem_sum_kernel<NH>, dim3(grid, NH), dim3(256), 0, st, hd, npix, w);
  hipLaunchKernelGGL(ohem_finalize_kernel<NH>, dim3(1), dim3(256), 0, st, hd, w, grid, (double)npix, total);
  return check_launch(fn);
}

template <int NH>
int ohem_backward(const char* fn, const OhemHeads<NH>& hd, const long long* labels, int N, int C, int H, int W, int ignore_index, void* stream) {
  hipLaunchKernelGGL(ohem_bwd_kernel<NH>, dim3(stream_grid((long long)N * H * W, 4096), NH), dim3(256), 0, (hipStream_t)stream, hd, labels, N, C,
                     (long long)H * W, ignore_index);
  return check_launch(fn);
}

}  // namespace

// workspace of one OHEM forward over `heads` (1 or 2) heads of npix = N * H * W pixels: per head three digit histograms, the selection state, the
// loss partials and the per-pixel CE values (the stored probabilities are the caller's `prob`: they live until the backward)
extern "C" size_t emrt_ohem_workspace_bytes(long long npix, int heads) {
  if (npix < 1 || heads < 1 || heads > 2) return 0;
  return ohem_bytes(npix, heads);
}

extern "C" int emrt_ohem_ce_fwd(const float* logits, const long long* labels, int N, int C, int H, int W, int ignore_index, float thresh,
                                long long min_kept, float* prob, float* result, void* workspace, void* stream) {
  EMRT_REQUIRE(logits && labels && prob && result && workspace, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  EMRT_REQUIRE(min_kept >= 0, "min_kept >= 0");
  EMRT_REQUIRE(thresh == thresh, "thresh is NaN");
  return ohem_forward<1>(__func__, ohem_heads<1>({logits}, {prob}, {result}, {nullptr}, {nullptr}, {1.f}), labels, N, C, H, W, ignore_index, thresh, min_kept,
                         nullptr, workspace, stream);
}

extern "C" int emrt_ohem_ce_bwd(const float* logits, const long long* labels, const float* prob, const float* result, const float* upstream,
                                float weight, int N, int C, int H, int W, int ignore_index, float* dlogits, void* stream) {
  EMRT_REQUIRE(logits && labels && prob && result && dlogits, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  return ohem_backward<1>(__func__, ohem_heads<1>({logits}, {prob}, {result}, {dlogits}, {upstream}, {weight}), labels, N, C, H, W, ignore_index, stream);
}

extern "C" int emrt_ohem_ce_pair_fwd(const float* logits_a, const float* logits_b, const long long* labels, int N, int C, int H, int W, int ignore_index,
                                     float thresh, long long min_kept, float wa, float wb, float* prob_a, float* prob_b, float* res_a, float* res_b,
                                     float* total, void* workspace, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && prob_a && prob_b && res_a && res_b && total && workspace, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  EMRT_REQUIRE(min_kept >= 0, "min_kept >= 0");
  EMRT_REQUIRE(thresh == thresh, "thresh is NaN");
  return ohem_forward<2>(__func__, ohem_heads<2>({logits_a, logits_b}, {prob_a, prob_b}, {res_a, res_b}, {nullptr, nullptr}, {nullptr, nullptr}, {wa, wb}),
                         labels, N, C, H, W, ignore_index, thresh, min_kept, total, workspace, stream);
}

extern "C" int emrt_ohem_ce_pair_bwd(const float* logits_a, const float* logits_b, const long long* labels, const float* prob_a, const float* prob_b,
                                     const float* res_a, const float* res_b, const float* up_a, const float* up_b, float wa, float wb, int N, int C,
                                     int H, int W, int ignore_index, float* dlogits_a, float* dlogits_b, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && prob_a && prob_b && res_a && res_b && dlogits_a && dlogits_b, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  return ohem_backward<2>(__func__, ohem_heads<2>({logits_a, logits_b}, {prob_a, prob_b}, {res_a, res_b}, {dlogits_a, dlogits_b}, {up_a, up_b}, {wa, wb}),
                          labels, N, C, H, W, ignore_index, stream);
}

// ---- plain CE: the family with the weight compiled out (no shape refusal: these entry points never had one).  workspace: emrt_ce_workspace_bytes()
extern "C" size_t emrt_ce_workspace_bytes(void) { return 1024 * 3 * sizeof(float); }

// result[2] (device): {mean loss, non-ignored count}
extern "C" int emrt_softmax_ce_fwd(const float* logits, const long long* labels, int N, int C, int H, int W, int ignore_index,
                                   float* result, void* workspace, void* stream) {
  EMRT_REQUIRE(logits && labels && result && workspace, "null pointer");
  return wce_forward<1>(__func__, WceHeads{{logits}, {result}, {}, {1.f}}, labels, nullptr, N, C, H, W, ignore_index, nullptr, workspace, stream);
}

// dlogits = weight * upstream * (softmax - onehot) / count     (upstream: device scalar or null == 1)
extern "C" int emrt_softmax_ce_bwd(const float* logits, const long long* labels, const float* result, const float* upstream,
                                   float weight, int N, int C, int H, int W, int ignore_index, float* dlogits, void* stream) {
  EMRT_REQUIRE(logits && labels && result && dlogits, "null pointer");
  return wce_backward<1>(__func__, WceHeads{{logits}, {dlogits}, {upstream}, {weight}}, labels, nullptr, result, N, C, H, W, ignore_index, stream);
}

// both heads at once: res_a / res_b (device float[2] each: {mean loss, non-ignored count}), total[0] = wa * loss_a + wb * loss_b
extern "C" int emrt_softmax_ce_pair_fwd(const float* logits_a, const float* logits_b, const long long* labels, int N, int C, int H, int W,
                                        int ignore_index, float wa, float wb, float* res_a, float* res_b, float* total, void* workspace, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && res_a && res_b && total && workspace, "null pointer");
  return wce_forward<2>(__func__, WceHeads{{logits_a, logits_b}, {res_a, res_b}, {}, {wa, wb}}, labels, nullptr, N, C, H, W, ignore_index,
                        total, workspace, stream);
}

// d logits_a = wa * up_a * (softmax - onehot) / count, d logits_b likewise (up_*: device scalars or NULL == 1); res_a from the forward
extern "C" int emrt_softmax_ce_pair_bwd(const float* logits_a, const float* logits_b, const long long* labels, const float* res_a, const float* up_a,
                                        const float* up_b, float wa, float wb, int N, int C, int H, int W, int ignore_index, float* dlogits_a,
                                        float* dlogits_b, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && res_a && dlogits_a && dlogits_b, "null pointer");
  return wce_backward<2>(__func__, WceHeads{{logits_a, logits_b}, {dlogits_a, dlogits_b}, {up_a, up_b}, {wa, wb}}, labels, nullptr, res_a, N, C, H, W,
                         ignore_index, stream);
}

// ---- class-weighted CE: class_weight == NULL is the plain CE above, kernel for kernel
extern "C" int emrt_wce_fwd(const float* logits, const long long* labels, const float* class_weight, int N, int C, int H, int W, int ignore_index,
                            float* result, void* workspace, void* stream) {
  EMRT_REQUIRE(logits && labels && result && workspace, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  return wce_forward<1>(__func__, WceHeads{{logits}, {result}, {}, {1.f}}, labels, class_weight, N, C, H, W, ignore_index, nullptr, workspace, stream);
}

extern "C" int emrt_wce_bwd(const float* logits, const long long* labels, const float* class_weight, const float* result, const float* upstream,
                            float weight, int N, int C, int H, int W, int ignore_index, float* dlogits, void* stream) {
  EMRT_REQUIRE(logits && labels && result && dlogits, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  return wce_backward<1>(__func__, WceHeads{{logits}, {dlogits}, {upstream}, {weight}}, labels, class_weight, result, N, C, H, W, ignore_index, stream);
}

extern "C" int emrt_wce_pair_fwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, int N, int C, int H,
                                 int W, int ignore_index, float wa, float wb, float* res_a, float* res_b, float* total, void* workspace, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && res_a && res_b && total && workspace, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  return wce_forward<2>(__func__, WceHeads{{logits_a, logits_b}, {res_a, res_b}, {}, {wa, wb}}, labels, class_weight, N, C, H, W,
                        ignore_index, total, workspace, stream);
}

extern "C" int emrt_wce_pair_bwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, const float* res_a,
                                 const float* up_a, const float* up_b, float wa, float wb, int N, int C, int H, int W, int ignore_index,
                                 float* dlogits_a, float* dlogits_b, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && res_a && dlogits_a && dlogits_b, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), SHAPE_MSG);
  return wce_backward<2>(__func__, WceHeads{{logits_a, logits_b}, {dlogits_a, dlogits_b}, {up_a, up_b}, {wa, wb}}, labels, class_weight, res_a, N, C, H, W,
                         ignore_index, stream);
}
