// Optimizer and weight-packing kernels for gfx950 (all HBM-bound streaming kernels; the losses live in loss.hip).
//
//  * ClipGradByGlobalNorm + L2 decay + Momentum, and Adam / AdamW, over ONE flat fp32 parameter buffer
//    (reference: solver/optimizer.py:29-40; the learning rate -- lr_scheduler.py:30-267 -- is evaluated on the device from a step counter so
//    the whole step can live in one hipGraph)
//  * per-step weight packing: fp32 master [OC][taps][C] -> compute-dtype forward copy [OC][taps][C] and transposed
//    dgrad copy [C][taps][OC] (LDS 32x32 tile transpose, one launch for every GEMM weight of the model).
#include <cfloat>
#include <type_traits>
#include "common.hpp"

using namespace emrt;

__global__ void axpby_scalar_kernel(float* out, const float* a, float wa, const float* b, float wb) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = wa * a[0] + (b ? wb * b[0] : 0.f);
}

extern "C" int emrt_scalar_axpby(float* out, const float* a, float wa, const float* b, float wb, void* stream) {
  EMRT_REQUIRE(out && a, "null pointer");
  hipLaunchKernelGGL(axpby_scalar_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out, a, wa, b, wb);
  return check_launch("emrt_scalar_axpby");
}

// ------------------------------------------------------------------------------------------------
// optimizer
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, long long n, float* __restrict__ partial) {
  __shared__ float red[4];
  float s = 0.f;
  const long long n4 = n / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - n4 * 4)) { const float v = g[n4 * 4 + threadIdx.x]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// state[0] = clip scale (clip / max(norm, clip), or 1 when clip <= 0), state[1] = global grad norm
__global__ __launch_bounds__(256) void clip_scale_kernel(const float* __restrict__ partial, int nblk, float clip, float* __restrict__ state) {
  __shared__ double red[1][256];
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < nblk; i += 256) s[0] += partial[i];
  block_tree_sum_f64<1>(s, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0][0]);
    state[1] = norm;
    state[0] = clip > 0.f ? clip / fmaxf(norm, clip) : 1.f;
  }
}

// what every optimizer step carries: the flat buffers, the step counter, the lr-mult ranges, the optional outputs
struct StepArgs {
  float* p; const float* g;
  float* s[2];                   // fp32 state streams, same indexing as p: velocity | moment1, moment2
  long long n;
  const float* state;            // clip scale at [0]
  const long long* step;         // device step counter (0-based index of this step)
  int nranges;
  long long r0[32], r1[32];      // element ranges whose learning rate is multiplied by `range_mult`
  float range_mult;
  float* lr_out;                 // optional: lr used this step
  void* mirror;                  // optional: compute-dtype copy of the parameters, same indexing as p
};

// The streaming skeleton of every optimizer kernel: four elements per thread (16-byte accesses on the 2 + NS fp32 streams), the lr-mult range
// lookup, the scalar tail in block 0.  elem(sel, p, g, s[NS]) -> new p updates the element's state in place; sel = 1 inside an lr-mult range.
// The compute-dtype mirror of the parameters -- the forward GEMM operand, same index as the master copy -- is written here instead of by a
// second pass over the master buffer.
template <class MT, bool NT, int NS, class F>
__device__ __forceinline__ void stream_update(const StepArgs& a, F elem) {
  typedef __attribute__((ext_vector_type(4))) float f32x4;
  MT* mirror = (MT*)a.mirror;
  const long long n4 = a.n / 4;
  for (long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += (long long)gridDim.x * blockDim.x) {
    const long long i = i4 * 4;
    // master copy, state and gradient are touched once per step (1.1 GB at 56 M parameters): non-temporal, so that they do not push the
    // compute-dtype mirror written below -- the next forward's GEMM operand -- out of the last-level cache (knob sgd_nt, default on)
    float p[4], g[4], st[4][NS];
    {
      f32x4 pq, gq, sq[NS];
      if (NT) {
        pq = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.p) + i4);
        gq = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.g) + i4);
#pragma unroll
        for (int k = 0; k < NS; ++k) sq[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.s[k]) + i4);
      } else {
        pq = reinterpret_cast<const f32x4*>(a.p)[i4];
        gq = reinterpret_cast<const f32x4*>(a.g)[i4];
#pragma unroll
        for (int k = 0; k < NS; ++k) sq[k] = reinterpret_cast<const f32x4*>(a.s[k])[i4];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = pq[e]; g[e] = gq[e];
#pragma unroll
        for (int k = 0; k < NS; ++k) st[e][k] = sq[k][e];
      }
    }
    bool any = false;
    for (int r = 0; r < a.nranges; ++r) any |= (i + 3 >= a.r0[r] && i < a.r1[r]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int sel = 0;
      if (any)
        for (int r = 0; r < a.nranges; ++r)
          if (i + e >= a.r0[r] && i + e < a.r1[r]) sel = 1;
      p[e] = elem(sel, p[e], g[e], st[e]);
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const f32x4 q = {st[0][k], st[1][k], st[2][k], st[3][k]};
      if (NT) __builtin_nontemporal_store(q, reinterpret_cast<f32x4*>(a.s[k]) + i4);
      else reinterpret_cast<f32x4*>(a.s[k])[i4] = q;
    }
    if (NT) __builtin_nontemporal_store((f32x4){p[0], p[1], p[2], p[3]}, reinterpret_cast<f32x4*>(a.p) + i4);
    else reinterpret_cast<f32x4*>(a.p)[i4] = (f32x4){p[0], p[1], p[2], p[3]};
    if (mirror) Vec4<MT>::store(mirror + i, p);
  }
  if (blockIdx.x == 0) {
    for (long long i = n4 * 4 + threadIdx.x; i < a.n; i += blockDim.x) {
      int sel = 0;
      for (int r = 0; r < a.nranges; ++r)
        if (i >= a.r0[r] && i < a.r1[r]) sel = 1;
      float st[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) st[k] = a.s[k][i];
      const float pn = elem(sel, a.p[i], a.g[i], st);
#pragma unroll
      for (int k = 0; k < NS; ++k) a.s[k][i] = st[k];
      a.p[i] = pn;
      if (mirror) mirror[i] = from_f32<MT>(pn);
    }
  }
}

// Learning rate of step s (the device step counter = paddle's last_epoch) under an EmrtLrSchedule (include/emrt_hip.h states the four kinds;
// solver/lr_scheduler.py:30-267).  fp32, every step quotient formed in double; the ONE copy every optimizer
// kernel uses (kind 0 is the polynomial emrt_sgd_momentum_step has built in).
__device__ __forceinline__ float lr_at(const EmrtLrSchedule& sc, long long s) {
  const long long T = sc.total_steps, W = sc.warmup_steps;
  if (sc.kind == 0) {
    const long long t = s > T ? T : s;
    const float frac = 1.f - (float)((double)t / (double)T);
    return (sc.base_lr - sc.end_lr) * powf(frac, sc.power) + sc.end_lr;
  }
  if (sc.kind == 1) {
    float lr;
    if (s < W) {
      lr = sc.warmup_lr_init + (sc.base_lr - sc.warmup_lr_init) * (float)((double)s / (double)W);
    } else {
      const float f = 1.f - (float)((double)(s - W) / (double)(T - W));
      if (f < 0.f) return sc.end_lr;            // the reference's pow() turns complex here and it answers lr_min
      lr = sc.warmup_lr_init + (sc.base_lr - sc.warmup_lr_init) * powf(f, sc.power);
    }
    return lr <= sc.end_lr ? sc.end_lr : lr;
  }
  if (sc.kind == 2) {
    if (s < W) return sc.warmup_lr_init + (sc.base_lr - sc.warmup_lr_init) * (float)((double)s / (double)W);
    const long long tc = s % T;
    return sc.end_lr + 0.5f * (sc.base_lr - sc.end_lr) * (1.f + cosf(3.14159265358979323846f * (float)((double)tc / (double)T)));
  }
  if (s <= W) return sc.base_lr * (float)((double)s / (double)W);
  int k = 0;
  for (int i = 0; i < sc.nmilestones; ++i) k += (sc.milestones[i] <= s) ? 1 : 0;
  return sc.base_lr * powf(sc.gamma, (float)k);
}

struct SgdArgs {
  StepArgs c;
  EmrtLrSchedule sched;
  float momentum, weight_decay;
};

// ClipGradByGlobalNorm + L2 decay + Momentum: g' = g * scale + wd * p, v = momentum * v + g', p -= lr * mult * v
template <class MT, bool NT>
__global__ __launch_bounds__(256) void sgd_momentum_sched_kernel(SgdArgs a) {
  const float lr = lr_at(a.sched, a.c.step ? a.c.step[0] : 0);
  if (a.c.lr_out && blockIdx.x == 0 && threadIdx.x == 0) a.c.lr_out[0] = lr;
  const float scale = a.c.state ? a.c.state[0] : 1.f, lr_r = lr * a.c.range_mult, momentum = a.momentum, wd = a.weight_decay;
  stream_update<MT, NT, 1>(a.c, [=](int sel, float p, float g, float (&v)[1]) {
    // explicit fused multiply-adds: the contraction is then the same in every instantiation of this kernel (left to the compiler, the
    // non-temporal and the plain variant differed in the last bit on ~1 % of the elements)
    const float gg = fmaf(wd, p, g * scale);
    v[0] = fmaf(momentum, v[0], gg);
    return fmaf(-(sel ? lr_r : lr), v[0], p);
  });
}

struct AdamArgs {
  StepArgs c;                    // step: this is update number step[0] + 1
  EmrtLrSchedule sched;
  float beta1, beta2, eps, weight_decay;
};

// Adam / AdamW, one streaming pass through stream_update with two state streams.
// What depends on the step alone is formed ONCE PER BLOCK, in double, and handed round through LDS: t = step + 1, the bias terms
// 1 - beta^t (fp32 powf of 0.999^t has lost them at t ~ 1e5), and from them, for lr and for lr * range_mult, the step size
// lr_e * sqrt(1 - beta2^t) / (1 - beta1^t) and the decoupled decay factor 1 - lr_e * wd, plus eps * sqrt(1 - beta2^t): one rounding each.
// The moments go through double as well -- g = grad * scale is exact there and m, v are rounded once --, the rest is fp32 with explicit
// fused multiply-adds and the correctly rounded square root and division: sqrtf and / are that under hipcc's defaults, which the build's flags
// leave alone (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt); HIP's __fsqrt_rn is NOT (it compiles to the bare v_sqrt_f32).
struct AdamConsts {
  float step_size, step_size_r, decay, decay_r, eps_t;      // _r: inside an lr-mult range
};

template <bool DECOUPLED>
__device__ __forceinline__ float adam_element(const AdamConsts& c, const double b1, const double b2, const double scale, const double wd, const int sel,
                                              const float p, const float g, float& m, float& v) {
  double gd = (double)g * scale;
  if (!DECOUPLED) gd = fma(wd, (double)p, gd);
  m = (float)fma(b1, (double)m, (1.0 - b1) * gd);
  v = (float)fma(b2, (double)v, (1.0 - b2) * (gd * gd));
  const float pd = DECOUPLED ? p * (sel ? c.decay_r : c.decay) : p;
  const float q = m / (sqrtf(v) + c.eps_t);       // 0 / (0 + eps_t) = 0: padded stem channels stay exactly zero
  return fmaf(-(sel ? c.step_size_r : c.step_size), q, pd);
}

template <class MT, bool NT, bool DECOUPLED>
__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
  __shared__ AdamConsts cs;
  if (threadIdx.x == 0) {
    const long long s = a.c.step ? a.c.step[0] : 0;
    const float lr = lr_at(a.sched, s);
    if (a.c.lr_out && blockIdx.x == 0) a.c.lr_out[0] = lr;
    const double t = (double)(s + 1);
    const double bc1 = 1.0 - pow((double)a.beta1, t), bc2s = sqrt(1.0 - pow((double)a.beta2, t));
    const double lre = (double)lr, lre_r = (double)lr * (double)a.c.range_mult;
    cs.step_size = (float)(lre * bc2s / bc1);
    cs.step_size_r = (float)(lre_r * bc2s / bc1);
    cs.decay = (float)(1.0 - lre * (double)a.weight_decay);
    cs.decay_r = (float)(1.0 - lre_r * (double)a.weight_decay);
    cs.eps_t = (float)((double)a.eps * bc2s);
  }
  __syncthreads();
  const AdamConsts c = cs;
  const double b1 = (double)a.beta1, b2 = (double)a.beta2, wd = (double)a.weight_decay, scale = a.c.state ? (double)a.c.state[0] : 1.0;
  stream_update<MT, NT, 2>(a.c, [=](int sel, float p, float g, float (&mv)[2]) { return adam_element<DECOUPLED>(c, b1, b2, scale, wd, sel, p, g, mv[0], mv[1]); });
}

__global__ void counter_add_kernel(long long* c, long long d) {
  if (threadIdx.x == 0 && blockIdx.x == 0) c[0] += d;
}

// Per-class areas of a prediction against its labels (reference: src/utils/metrics.py:20-59 calculate_area): intersect / prediction / label pixel counts with
// ignore_index, accumulated into out[3][ncls] (int64).  Per-block LDS histograms, one global atomic per (block, class, kind).
template <class LT>
__global__ __launch_bounds__(256) void seg_areas_kernel(const int* __restrict__ pred, const LT* __restrict__ label, long long n, int ncls, int ignore,
                                                        unsigned long long* __restrict__ out) {
  __shared__ unsigned cnt[3 * 256];
  for (int i = threadIdx.x; i < 3 * ncls; i += blockDim.x) cnt[i] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long l = (long long)label[i];
    if (l == ignore) continue;
    const int p = pred[i];
    const bool pv = p >= 0 && p < ncls, lv = l >= 0 && l < ncls;
    if (pv) atomicAdd(&cnt[ncls + p], 1u);
    if (lv) atomicAdd(&cnt[2 * ncls + (int)l], 1u);
    if (pv && (long long)p == l) atomicAdd(&cnt[p], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * ncls; i += blockDim.x)
    if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

extern "C" int emrt_segmentation_areas(const int* pred, const void* label, int label_is_int64, long long n, int num_classes, int ignore_index,
                                       long long* out, void* stream) {
  EMRT_REQUIRE(pred && label && out, "null pointer");
  EMRT_REQUIRE(num_classes >= 1 && num_classes <= 256 && n >= 0, "1..256 classes");
  EMRT_REQUIRE(label_is_int64 >= 0 && label_is_int64 <= 2, "label_is_int64 selects the label type: 0 = int32, 1 = int64, 2 = uint8");
  if (n == 0) return 0;
  long long grid = (n + 256 * 16 - 1) / (256 * 16);
  if (grid > 1024) grid = 1024;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* o = (unsigned long long*)out;
  // uint8 (the label maps of a scene bank, at any byte offset): one byte per lane, so nothing is assumed about the pointer's alignment
  if (label_is_int64 == 2) hipLaunchKernelGGL((seg_areas_kernel<unsigned char>), dim3((unsigned)grid), dim3(256), 0, st, pred, (const unsigned char*)label, n, num_classes, ignore_index, o);
  else if (label_is_int64 == 1) hipLaunchKernelGGL((seg_areas_kernel<long long>), dim3((unsigned)grid), dim3(256), 0, st, pred, (const long long*)label, n, num_classes, ignore_index, o);
  else hipLaunchKernelGGL((seg_areas_kernel<int>), dim3((unsigned)grid), dim3(256), 0, st, pred, (const int*)label, n, num_classes, ignore_index, o);
  return check_launch("emrt_segmentation_areas");
}

extern "C" size_t emrt_gradnorm_workspace_bytes(void) { return 2048 * sizeof(float); }

extern "C" int emrt_grad_clip_scale(const float* grads, long long n, float clip, float* state /*[2]*/, void* workspace, void* stream) {
  EMRT_REQUIRE(grads && state && workspace, "null pointer");
  EMRT_REQUIRE(((uintptr_t)grads) % 16 == 0, "grads must be 16-byte aligned");
  int grid = (int)((n / 4 + 255) / 256);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(grid), dim3(256), 0, st, grads, n, (float*)workspace);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, grid, clip, state);
  return check_launch("emrt_grad_clip_scale");
}

// host-side refusals of a schedule descriptor (nothing is launched for a bad one); NULL when it is fine
static const char* lr_schedule_problem(const EmrtLrSchedule* sc) {
  if (!sc) return "null schedule";
  if (sc->kind < 0 || sc->kind > 3) return "unknown schedule kind (0 PolynomialDecay, 1 WarmupPolyLR, 2 WarmupCosineLR, 3 WarmupMultiStepLR)";
  if (sc->total_steps < 1) return "total_steps must be positive";
  if (sc->warmup_steps < 0) return "warmup_steps must not be negative";
  if (sc->kind == 1 && sc->total_steps <= sc->warmup_steps) return "WarmupPolyLR needs total_steps > warmup_steps";
  if (sc->kind == 3 && sc->warmup_steps < 1) return "WarmupMultiStepLR needs warmup_steps >= 1";
  if (sc->nmilestones < 0 || sc->nmilestones > 16) return "0..16 milestones";
  for (int i = 1; i < sc->nmilestones; ++i)
    if (sc->milestones[i] <= sc->milestones[i - 1]) return "milestones must be increasing";
  return nullptr;
}

// The refusals every optimizer entry point shares and the fill of the common arguments (nothing is launched for a bad call).  state: the NS fp32
// state streams; ranges: HOST [nranges][2].  NULL when the call is fine, else the reason, which the entry point reports under its own name.
template <int NS>
static const char* fill_step_args(StepArgs& c, float* params, const float* grads, float* const (&state)[NS], long long n, const float* clip_state,
                                  const long long* step, const long long* ranges, int nranges, float range_mult, float* lr_out, void* mirror, int mirror_dtype) {
  uintptr_t bits = (uintptr_t)params | (uintptr_t)grads;
  bool all = params && grads;
  for (int k = 0; k < NS; ++k) { all = all && state[k]; bits |= (uintptr_t)state[k]; }
  if (!all) return "null pointer";
  if (mirror && mirror_dtype != EMRT_BF16 && mirror_dtype != EMRT_F16) return "the parameter mirror is bf16 or fp16";
  if (bits % 16 != 0 || (mirror && (uintptr_t)mirror % 8 != 0)) return "buffers must be 16-byte aligned";
  if (nranges < 0 || nranges > 32 || (nranges != 0 && !ranges)) return "0..32 lr-mult ranges";
  c.p = params; c.g = grads; c.n = n; c.state = clip_state; c.step = step;
  for (int k = 0; k < NS; ++k) c.s[k] = state[k];
  c.nranges = nranges; c.range_mult = range_mult; c.lr_out = lr_out; c.mirror = mirror;
  for (int r = 0; r < nranges; ++r) { c.r0[r] = ranges[2 * r]; c.r1[r] = ranges[2 * r + 1]; }
  return nullptr;
}

// The one launch ladder: sgd_nt knob x mirror dtype (no mirror: the bf16 instantiation, which then never touches it).  launch is a generic lambda
// called with a value of the mirror's element type and an integral_constant for NT.
template <class L>
static int launch_step(const char* fn, long long n, void* mirror, int mirror_dtype, L&& launch) {
  int grid = (int)((n / 4 + 255) / 256);
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  const bool f16 = mirror && mirror_dtype == EMRT_F16;
  if (g_tune.sgd_nt != 0) {
    if (f16) launch(f16_t{}, std::true_type{}, grid);
    else launch(bf16_t{}, std::true_type{}, grid);
  } else {
    if (f16) launch(f16_t{}, std::false_type{}, grid);
    else launch(bf16_t{}, std::false_type{}, grid);
  }
  return check_launch(fn);
}

static int sgd_step(const char* fn, float* params, const float* grads, float* velocity, long long n, const float* clip_state, const long long* step,
                    const EmrtLrSchedule* sched, bool builtin, float momentum, float weight_decay, const long long* ranges, int nranges, float range_mult,
                    float* lr_out, void* mirror, int mirror_dtype, void* stream) {
  SgdArgs a;
  memset(&a, 0, sizeof(a));
  if (const char* why = fill_step_args<1>(a.c, params, grads, {velocity}, n, clip_state, step, ranges, nranges, range_mult, lr_out, mirror, mirror_dtype))
    return emrt::fail(fn, why);
  // builtin: the kind-0 descriptor emrt_sgd_momentum_step made of its own arguments; all that can be wrong with it is decay_steps
  if (const char* why = !builtin ? lr_schedule_problem(sched) : sched->total_steps > 0 ? nullptr : "decay_steps must be positive") return emrt::fail(fn, why);
  a.sched = *sched;
  a.momentum = momentum; a.weight_decay = weight_decay;
  return launch_step(fn, n, mirror, mirror_dtype, [&](auto mt, auto nt, int grid) {
    hipLaunchKernelGGL((sgd_momentum_sched_kernel<decltype(mt), decltype(nt)::value>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  });
}

// the built-in polynomial is the kind-0 schedule: one kernel serves both entry points
extern "C" int emrt_sgd_momentum_step(float* params, const float* grads, float* velocity, long long n, const float* clip_state,
                                      const long long* step, float base_lr, float end_lr, float power, long long decay_steps,
                                      float momentum, float weight_decay, const long long* ranges /*host [nranges][2]*/,
                                      int nranges, float range_mult, float* lr_out, void* mirror, int mirror_dtype, void* stream) {
  EmrtLrSchedule sc;
  memset(&sc, 0, sizeof(sc));
  sc.kind = 0; sc.base_lr = base_lr; sc.end_lr = end_lr; sc.power = power;
  sc.total_steps = decay_steps;
  return sgd_step(__func__, params, grads, velocity, n, clip_state, step, &sc, true, momentum, weight_decay,
                  ranges, nranges, range_mult, lr_out, mirror, mirror_dtype, stream);
}

extern "C" int emrt_sgd_momentum_step_sched(float* params, const float* grads, float* velocity, long long n, const float* clip_state,
                                            const long long* step, const EmrtLrSchedule* sched, float momentum, float weight_decay,
                                            const long long* ranges /*host [nranges][2]*/, int nranges, float range_mult, float* lr_out,
                                            void* mirror, int mirror_dtype, void* stream) {
  return sgd_step(__func__, params, grads, velocity, n, clip_state, step, sched, false, momentum, weight_decay, ranges, nranges,
                  range_mult, lr_out, mirror, mirror_dtype, stream);
}

extern "C" int emrt_adamw_step(float* params, const float* grads, float* moment1, float* moment2, long long n, const float* clip_state,
                               const long long* step, const EmrtLrSchedule* sched, float beta1, float beta2, float eps, float weight_decay,
                               int decoupled, const long long* ranges /*host [nranges][2]*/, int nranges, float range_mult, float* lr_out,
                               void* mirror, int mirror_dtype, void* stream) {
  AdamArgs a;
  memset(&a, 0, sizeof(a));
  if (const char* why = fill_step_args<2>(a.c, params, grads, {moment1, moment2}, n, clip_state, step, ranges, nranges, range_mult, lr_out, mirror, mirror_dtype))
    return emrt::fail(__func__, why);
  EMRT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "0 <= beta < 1");
  EMRT_REQUIRE(eps > 0.f, "eps must be positive");
  // the kernel adds eps * sqrt(1 - beta2^t) in fp32, smallest at t = 1: were that to underflow, an all-zero element (a padded stem channel) would
  // compute 0 / 0 instead of staying zero
  EMRT_REQUIRE((float)((double)eps * sqrt(1.0 - (double)beta2)) >= FLT_MIN, "eps is too small: eps * sqrt(1 - beta2) must be a normal fp32 number");
  EMRT_REQUIRE(decoupled == 0 || decoupled == 1, "decoupled is 0 (Adam) or 1 (AdamW)");
  if (const char* why = lr_schedule_problem(sched)) return emrt::fail(__func__, why);
  a.sched = *sched;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
  return launch_step(__func__, n, mirror, mirror_dtype, [&](auto mt, auto nt, int grid) {
    if (decoupled) hipLaunchKernelGGL((adamw_kernel<decltype(mt), decltype(nt)::value, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((adamw_kernel<decltype(mt), decltype(nt)::value, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  });
}

extern "C" int emrt_counter_add(long long* counter, long long delta, void* stream) {
  EMRT_REQUIRE(counter, "null pointer");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter, delta);
  return check_launch("emrt_counter_add");
}

// ------------------------------------------------------------------------------------------------
// weight packing.  Descriptor table (device, int64 x 8 per entry):
//   {src_off, fwd_off (-1: none), bwd_off (-1: none), OC, taps, C, tile_prefix (first flat tile id), unused}
// One 32x32 (oc x c) tile per block per tap; flat tile id -> descriptor by binary search on tile_prefix.
// ------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ master, T* __restrict__ packed,
                                                           const long long* __restrict__ desc, int ndesc, int bwd_only) {
  __shared__ float tile[32][33];
  const long long tid = blockIdx.x;
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid * 8 + 6] <= tid) lo = mid; else hi = mid - 1;
  }
  const long long* d = desc + lo * 8;
  const long long src = d[0], fo = bwd_only ? -1 : d[1], bo = d[2];
  if (fo < 0 && bo < 0) return;
  // bwd_only: the forward copy (the optimizer's mirror) is current -- transpose from it (half the bytes of the fp32 master)
  const T* mir = (bwd_only && d[1] >= 0) ? packed + d[1] : nullptr;
  const int OC = (int)d[3], taps = (int)d[4], C = (int)d[5];
  const int tc = (C + 31) / 32, toc = (OC + 31) / 32;
  long long local = tid - d[6];
  const int ct = (int)(local % tc); local /= tc;
  const int ot = (int)(local % toc);
  const int tap = (int)(local / toc);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oc = ot * 32 + ty + 8 * r, c = ct * 32 + tx;
    float v = 0.f;
    if (oc < OC && c < C) {
      const long long idx = ((long long)oc * taps + tap) * C + c;
      v = mir ? to_f32(mir[idx]) : master[src + idx];
      if (fo >= 0) packed[fo + idx] = from_f32<T>(v);
    }
    tile[ty + 8 * r][tx] = v;
  }
  if (bo < 0) return;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = ct * 32 + ty + 8 * r, oc = ot * 32 + tx;
    if (oc < OC && c < C) packed[bo + ((long long)c * taps + tap) * OC + oc] = from_f32<T>(tile[tx][ty + 8 * r]);
  }
}

// The per-step form: only the transposed dgrad copies, 64x64 (oc x c) tiles, 16-byte accesses on both sides (the 32x32 kernel above
// writes 2-byte elements in 64-byte runs: 1.8 TB/s).  Source = the compute-dtype forward copy when the descriptor has one (the
// optimizer's mirror, current by construction), else the fp32 master.  desc[7] = first 64x64 tile id of the descriptor.
template <class T>
__global__ __launch_bounds__(256) void pack_bwd64_kernel(const float* __restrict__ master, T* __restrict__ packed,
                                                         const long long* __restrict__ desc, int ndesc) {
  __shared__ float tile[64][65];
  const long long tid = blockIdx.x;
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid * 8 + 7] <= tid) lo = mid; else hi = mid - 1;
  }
  const long long* d = desc + lo * 8;
  const long long src = d[0], fo = d[1], bo = d[2];
  if (bo < 0) return;
  const int OC = (int)d[3], taps = (int)d[4], C = (int)d[5];
  const int tc = (C + 63) / 64, toc = (OC + 63) / 64;
  long long local = tid - d[7];
  const int ct = (int)(local % tc); local /= tc;
  const int ot = (int)(local % toc);
  const int tap = (int)(local / toc);
  if (tap >= taps) return;
  const T* mir = fo >= 0 ? packed + fo : nullptr;
  const int sub = threadIdx.x & 7, rw = threadIdx.x >> 3;      // 8 chunks of 8 elements x 32 rows per pass
  const bool vc = (C % 8) == 0, voc = (OC % 8) == 0;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int ol = rw + 32 * ps, oc = ot * 64 + ol, c0 = ct * 64 + sub * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (oc < OC && c0 < C) {
      const long long idx = ((long long)oc * taps + tap) * C + c0;
      if (vc) {
        if (mir) Vec8<T>::load(mir + idx, v);
        else Vec8<float>::load(master + src + idx, v);
      } else {
        for (int e = 0; e < 8; ++e)
          if (c0 + e < C) v[e] = mir ? to_f32(mir[idx + e]) : master[src + idx + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[ol][sub * 8 + e] = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int cl = rw + 32 * ps, c = ct * 64 + cl, o0 = ot * 64 + sub * 8;
    if (c >= C || o0 >= OC) continue;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[sub * 8 + e][cl];
    T* dst = packed + bo + ((long long)c * taps + tap) * OC + o0;
    if (voc) Vec8<T>::store(dst, v);
    else
      for (int e = 0; e < 8; ++e)
        if (o0 + e < OC) dst[e] = from_f32<T>(v[e]);
  }
}

extern "C" int emrt_pack_weights(const float* master, void* packed, const long long* desc_dev, int ndesc, long long total_tiles,
                                 long long total_tiles64, int bwd_only, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(master && packed && desc_dev, "null pointer");
  EMRT_REQUIRE(ndesc > 0 && total_tiles > 0 && total_tiles < 2147483647LL && total_tiles64 >= 0 && total_tiles64 < 2147483647LL, "bad descriptor table");
  hipStream_t st = (hipStream_t)stream;
  return with_fwd_dtype("emrt_pack_weights", dtype, [&](auto t) {
    using T = decltype(t);
    if (bwd_only && total_tiles64 > 0) {
      hipLaunchKernelGGL((pack_bwd64_kernel<T>), dim3((unsigned)total_tiles64), dim3(256), 0, st, master, (T*)packed, desc_dev, ndesc);
      return check_launch("emrt_pack_weights");
    }
    hipLaunchKernelGGL((pack_weights_kernel<T>), dim3((unsigned)total_tiles), dim3(256), 0, st, master, (T*)packed, desc_dev, ndesc, bwd_only);
    return check_launch("emrt_pack_weights");
  });
}
