// Hard-pixel mining and class-weighted cross entropy for gfx950.
//
//  * OhemCrossEntropyLoss (reference: losses/ohem_cross_entropy_loss.py:41-79).  The reference finds its threshold with an argsort over every
//    pixel and a device-to-host read in the middle of the loss; here the min_kept-th smallest probability is found by an exact radix select
//    (11 + 11 + 10 bits, most significant digit first) over the fp32 bit patterns, entirely on the device: a captured step stays one graph.
//    Only integer atomics take part in the selection, so the threshold -- and with it the mask, the loss and the gradient -- is the same bits
//    in every run.
//  * nn.CrossEntropyLoss(weight=w, ignore_index) (reference: losses/cross_entropy_loss.py:30-35; the form MixSoftmaxCrossEntropyLoss is built
//    on): loss = sum w[y] CE / sum w[y] over the non-ignored pixels, one head or the two heads of the Mix loss in one pass.
#include <cfloat>
#include "common.hpp"

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

__device__ __forceinline__ void pixel_of(long long idx, long long total, long long HW, long long& n, long long& p) {
  n = total <= 0xffffffffll ? (long long)((unsigned)idx / (unsigned)HW) : idx / HW;      // (32-bit division when it can be)
  p = idx - n * HW;
}

// the block's LDS histogram -> the global bins: one integer atomic per non-empty bin
__device__ __forceinline__ void flush_bins(const unsigned* lh, unsigned* __restrict__ gh, int nbins) {
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += blockDim.x) {
    const unsigned v = lh[i];
    if (v) atomicAdd(gh + i, v);
  }
}

// pass over the logits: p = softmax probability of the pixel's own class (the arithmetic of loss_optim.hip's ce_pixel) and its CE, both stored;
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
    float mx = -3.0e38f;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lp[c * HW]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += __expf(lp[c * HW] - mx);
    const float picked = (lab >= 0 && lab < C) ? lp[lab * HW] : 0.f;
    const float pr = __expf(picked - mx) / den;
    prob[idx] = pr;
    ce[idx] = logf(den) + mx - picked;
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
  float ls = 0.f, cnt = 0.f;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    if (prob[idx] < thr) { ls += ce[idx]; cnt += 1.f; }
  }
  ls = wave_sum(ls);
  cnt = wave_sum(cnt);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[wv * 2] = ls; red[wv * 2 + 1] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < 4; ++w) { a += red[w * 2]; b += red[w * 2 + 1]; }
    partial[blockIdx.x * 2] = a;
    partial[blockIdx.x * 2 + 1] = b;
  }
}

// one block; per head: result = {loss, kept count, threshold (written by the scan), non-ignored count, 1 / (kept + 1e-5 npix) or 0 when nothing is
// kept}; total[0] = sum of w_h * loss_h (null: not wanted)
template <int NH>
__global__ __launch_bounds__(256) void ohem_finalize_kernel(OhemHeads<NH> hd, OhemWs ws, int nblk, double npix, float* __restrict__ total) {
  __shared__ double ra[256], rb[256];
  float t = 0.f;
  for (int h = 0; h < NH; ++h) {
    const float* partial = ws.partial + h * OH_MAX_BLOCKS * 2;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) { a += partial[i * 2]; b += partial[i * 2 + 1]; }
    ra[threadIdx.x] = a;
    rb[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) { ra[threadIdx.x] += ra[threadIdx.x + o]; rb[threadIdx.x] += rb[threadIdx.x + o]; }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      // mean(loss * mask) / (mean(mask) + 1e-5) of the reference, numerator and denominator times npix (npix counts the ignored pixels too)
      const double den = rb[0] + 1e-5 * npix;
      float* result = hd.result[h];
      result[0] = (float)(ra[0] / den);
      result[1] = (float)rb[0];
      result[3] = (float)ws.hist[h * OH_SEL_WORDS + 3 * OH_BINS + ST_VALID];
      result[4] = rb[0] > 0.0 ? (float)(1.0 / den) : 0.f;
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
    if (lab == ignore_index || !(prob[idx] < thr)) {
      for (int c = 0; c < C; ++c) dp[c * HW] = 0.f;
      continue;
    }
    float mx = -3.0e38f;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lp[c * HW]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += __expf(lp[c * HW] - mx);
    const float inv = 1.f / den;
    for (int c = 0; c < C; ++c) dp[c * HW] = g * (__expf(lp[c * HW] - mx) * inv - (c == lab ? 1.f : 0.f));
  }
}

// ------------------------------------------------------------------------------------------------
// class-weighted cross entropy, NH = 1 head or the 2 heads of the Mix loss
// ------------------------------------------------------------------------------------------------
template <int NH>
struct WceHeads {
  const float* logits[NH];
  float* out[NH];          // forward: result[2] per head; backward: dlogits
  const float* up[NH];
  float w[NH];
};

__device__ __forceinline__ float class_weight_of(const float* __restrict__ cw, long long lab, int C) {
  return cw ? ((lab >= 0 && lab < C) ? cw[lab] : 0.f) : 1.f;
}

// partial[block] = {sum w[y] CE of head 0, (of head 1,) sum w[y]}
template <int NH>
__global__ __launch_bounds__(256) void wce_fwd_kernel(WceHeads<NH> hd, const long long* __restrict__ labels, const float* __restrict__ cw, int N, int C,
                                                      long long HW, int ignore_index, float* __restrict__ partial) {
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
    const float w = class_weight_of(cw, lab, C);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const float* lp = hd.logits[h] + n * C * HW + p;
      float mx = -3.0e38f;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, lp[c * HW]);
      float den = 0.f;
      for (int c = 0; c < C; ++c) den += __expf(lp[c * HW] - mx);
      const float picked = (lab >= 0 && lab < C) ? lp[lab * HW] : 0.f;
      acc[h] += w * (logf(den) + mx - picked);
    }
    acc[NH] += w;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h <= NH; ++h) {
    const float v = wave_sum(acc[h]);
    if (lane == 0) red[wv * (NH + 1) + h] = v;
  }
  __syncthreads();
  if (threadIdx.x <= NH) {
    float a = 0.f;
    for (int w = 0; w < 4; ++w) a += red[w * (NH + 1) + threadIdx.x];
    partial[blockIdx.x * (NH + 1) + threadIdx.x] = a;
  }
}

// result of head h = {sum w CE / sum w, sum w}; two heads: total[0] = wa * loss_a + wb * loss_b
template <int NH>
__global__ __launch_bounds__(256) void wce_finalize_kernel(const float* __restrict__ partial, int nblk, WceHeads<NH> hd, float* __restrict__ total) {
  __shared__ double r[NH + 1][256];
  double a[NH + 1];
#pragma unroll
  for (int h = 0; h <= NH; ++h) a[h] = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
    for (int h = 0; h <= NH; ++h) a[h] += partial[i * (NH + 1) + h];
  }
#pragma unroll
  for (int h = 0; h <= NH; ++h) r[h][threadIdx.x] = a[h];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int h = 0; h <= NH; ++h) r[h][threadIdx.x] += r[h][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double den = r[NH][0] > 0.0 ? r[NH][0] : 1.0;      // every pixel ignored (or of weight 0): loss 0, not 0 / 0
    float t = 0.f;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      hd.out[h][0] = (float)(r[h][0] / den);
      hd.out[h][1] = (float)r[NH][0];
      t += hd.w[h] * hd.out[h][0];
    }
    if (total) total[0] = t;
  }
}

// dlogits_h = w_h * up_h * w[y] * (softmax - onehot) / sum w[y]
template <int NH>
__global__ __launch_bounds__(256) void wce_bwd_kernel(WceHeads<NH> hd, const long long* __restrict__ labels, const float* __restrict__ cw,
                                                      const float* __restrict__ res, int N, int C, long long HW, int ignore_index) {
  const long long total = (long long)N * HW;
  const float den_w = res[1] > 0.f ? res[1] : 1.f, inv_den = 1.f / den_w;
  float gh[NH];
  // (the quotient / reciprocal forms of emrt_softmax_ce_bwd / _pair_bwd: unit class weights give their bits)
#pragma unroll
  for (int h = 0; h < NH; ++h) gh[h] = NH == 1 ? hd.w[h] * (hd.up[h] ? hd.up[h][0] : 1.f) / den_w : hd.w[h] * (hd.up[h] ? hd.up[h][0] : 1.f) * inv_den;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long lab = labels[idx];
    long long n, p;
    pixel_of(idx, total, HW, n, p);
    const float w = lab == ignore_index ? 0.f : class_weight_of(cw, lab, C);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const float* lp = hd.logits[h] + n * C * HW + p;
      float* dp = hd.out[h] + n * C * HW + p;
      if (lab == ignore_index) {
        for (int c = 0; c < C; ++c) dp[c * HW] = 0.f;
        continue;
      }
      const float g = gh[h] * w;
      float mx = -3.0e38f;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, lp[c * HW]);
      float den = 0.f;
      for (int c = 0; c < C; ++c) den += __expf(lp[c * HW] - mx);
      const float inv = 1.f / den;
      for (int c = 0; c < C; ++c) dp[c * HW] = g * (__expf(lp[c * HW] - mx) * inv - (c == lab ? 1.f : 0.f));
    }
  }
}

inline int stream_grid(long long npix, int cap) {
  long long g = (npix + 255) / 256;
  return (int)(g > cap ? cap : g < 1 ? 1 : g);
}

inline bool shape_ok(int N, int C, int H, int W) { return N >= 1 && C >= 1 && H >= 1 && W >= 1 && (long long)N * H * W < (1ll << 31); }


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
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  EMRT_REQUIRE(min_kept >= 0, "min_kept >= 0");
  EMRT_REQUIRE(thresh == thresh, "thresh is NaN");
  OhemHeads<1> hd = {};
  hd.logits[0] = logits; hd.prob[0] = prob; hd.result[0] = result; hd.w[0] = 1.f;
  return ohem_forward<1>("emrt_ohem_ce_fwd", hd, labels, N, C, H, W, ignore_index, thresh, min_kept, nullptr, workspace, stream);
}

extern "C" int emrt_ohem_ce_bwd(const float* logits, const long long* labels, const float* prob, const float* result, const float* upstream,
                                float weight, int N, int C, int H, int W, int ignore_index, float* dlogits, void* stream) {
  EMRT_REQUIRE(logits && labels && prob && result && dlogits, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  OhemHeads<1> hd = {};
  hd.logits[0] = logits; hd.prob[0] = (float*)prob; hd.result[0] = (float*)result; hd.dlogits[0] = dlogits; hd.up[0] = upstream; hd.w[0] = weight;
  hipLaunchKernelGGL(ohem_bwd_kernel<1>, dim3(stream_grid((long long)N * H * W, 4096)), dim3(256), 0, (hipStream_t)stream, hd, labels, N, C,
                     (long long)H * W, ignore_index);
  return check_launch("emrt_ohem_ce_bwd");
}

extern "C" int emrt_ohem_ce_pair_fwd(const float* logits_a, const float* logits_b, const long long* labels, int N, int C, int H, int W, int ignore_index,
                                     float thresh, long long min_kept, float wa, float wb, float* prob_a, float* prob_b, float* res_a, float* res_b,
                                     float* total, void* workspace, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && prob_a && prob_b && res_a && res_b && total && workspace, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  EMRT_REQUIRE(min_kept >= 0, "min_kept >= 0");
  EMRT_REQUIRE(thresh == thresh, "thresh is NaN");
  OhemHeads<2> hd = {};
  hd.logits[0] = logits_a; hd.prob[0] = prob_a; hd.result[0] = res_a; hd.w[0] = wa;
  hd.logits[1] = logits_b; hd.prob[1] = prob_b; hd.result[1] = res_b; hd.w[1] = wb;
  return ohem_forward<2>("emrt_ohem_ce_pair_fwd", hd, labels, N, C, H, W, ignore_index, thresh, min_kept, total, workspace, stream);
}

extern "C" int emrt_ohem_ce_pair_bwd(const float* logits_a, const float* logits_b, const long long* labels, const float* prob_a, const float* prob_b,
                                     const float* res_a, const float* res_b, const float* up_a, const float* up_b, float wa, float wb, int N, int C,
                                     int H, int W, int ignore_index, float* dlogits_a, float* dlogits_b, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && prob_a && prob_b && res_a && res_b && dlogits_a && dlogits_b, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  OhemHeads<2> hd = {};
  hd.logits[0] = logits_a; hd.prob[0] = (float*)prob_a; hd.result[0] = (float*)res_a; hd.dlogits[0] = dlogits_a; hd.up[0] = up_a; hd.w[0] = wa;
  hd.logits[1] = logits_b; hd.prob[1] = (float*)prob_b; hd.result[1] = (float*)res_b; hd.dlogits[1] = dlogits_b; hd.up[1] = up_b; hd.w[1] = wb;
  hipLaunchKernelGGL(ohem_bwd_kernel<2>, dim3(stream_grid((long long)N * H * W, 4096), 2), dim3(256), 0, (hipStream_t)stream, hd, labels, N, C,
                     (long long)H * W, ignore_index);
  return check_launch("emrt_ohem_ce_pair_bwd");
}

extern "C" int emrt_wce_fwd(const float* logits, const long long* labels, const float* class_weight, int N, int C, int H, int W, int ignore_index,
                            float* result, void* workspace, void* stream) {
  EMRT_REQUIRE(logits && labels && result && workspace, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  const int grid = stream_grid((long long)N * H * W, 1024);
  hipStream_t st = (hipStream_t)stream;
  WceHeads<1> hd;
  hd.logits[0] = logits; hd.out[0] = result; hd.up[0] = nullptr; hd.w[0] = 1.f;
  hipLaunchKernelGGL(wce_fwd_kernel<1>, dim3(grid), dim3(256), 0, st, hd, labels, class_weight, N, C, (long long)H * W, ignore_index, (float*)workspace);
  hipLaunchKernelGGL(wce_finalize_kernel<1>, dim3(1), dim3(256), 0, st, (const float*)workspace, grid, hd, (float*)nullptr);
  return check_launch("emrt_wce_fwd");
}

extern "C" int emrt_wce_bwd(const float* logits, const long long* labels, const float* class_weight, const float* result, const float* upstream,
                            float weight, int N, int C, int H, int W, int ignore_index, float* dlogits, void* stream) {
  EMRT_REQUIRE(logits && labels && result && dlogits, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  WceHeads<1> hd;
  hd.logits[0] = logits; hd.out[0] = dlogits; hd.up[0] = upstream; hd.w[0] = weight;
  hipLaunchKernelGGL(wce_bwd_kernel<1>, dim3(stream_grid((long long)N * H * W, 4096)), dim3(256), 0, (hipStream_t)stream, hd, labels, class_weight, result, N,
                     C, (long long)H * W, ignore_index);
  return check_launch("emrt_wce_bwd");
}

extern "C" int emrt_wce_pair_fwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, int N, int C, int H,
                                 int W, int ignore_index, float wa, float wb, float* res_a, float* res_b, float* total, void* workspace, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && res_a && res_b && total && workspace, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  const int grid = stream_grid((long long)N * H * W, 1024);
  hipStream_t st = (hipStream_t)stream;
  WceHeads<2> hd;
  hd.logits[0] = logits_a; hd.out[0] = res_a; hd.up[0] = nullptr; hd.w[0] = wa;
  hd.logits[1] = logits_b; hd.out[1] = res_b; hd.up[1] = nullptr; hd.w[1] = wb;
  hipLaunchKernelGGL(wce_fwd_kernel<2>, dim3(grid), dim3(256), 0, st, hd, labels, class_weight, N, C, (long long)H * W, ignore_index, (float*)workspace);
  hipLaunchKernelGGL(wce_finalize_kernel<2>, dim3(1), dim3(256), 0, st, (const float*)workspace, grid, hd, total);
  return check_launch("emrt_wce_pair_fwd");
}

extern "C" int emrt_wce_pair_bwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, const float* res_a,
                                 const float* up_a, const float* up_b, float wa, float wb, int N, int C, int H, int W, int ignore_index,
                                 float* dlogits_a, float* dlogits_b, void* stream) {
  EMRT_REQUIRE(logits_a && logits_b && labels && res_a && dlogits_a && dlogits_b, "null pointer");
  EMRT_REQUIRE(shape_ok(N, C, H, W), "N, C, H, W >= 1 and N * H * W < 2^31");
  WceHeads<2> hd;
  hd.logits[0] = logits_a; hd.out[0] = dlogits_a; hd.up[0] = up_a; hd.w[0] = wa;
  hd.logits[1] = logits_b; hd.out[1] = dlogits_b; hd.up[1] = up_b; hd.w[1] = wb;
  hipLaunchKernelGGL(wce_bwd_kernel<2>, dim3(stream_grid((long long)N * H * W, 4096)), dim3(256), 0, (hipStream_t)stream, hd, labels, class_weight, res_a, N,
                     C, (long long)H * W, ignore_index);
  return check_launch("emrt_wce_pair_bwd");
}
