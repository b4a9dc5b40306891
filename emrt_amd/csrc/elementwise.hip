// Small streaming kernels: adds (with batch broadcast), gradient accumulation, dropout (+ReLU mask) forward/backward,
// sigmoid, dtype casts, memset.  Reference sites: with_pos_embed (transformer_encoder_decoder.py:154-155,273-274),
// nn.Dropout / nn.Dropout2D (:115,119,122,250,255,261,263; paddle_EMRT.py:208; fcn_head.py:65), F.sigmoid (:466).
#include "common.hpp"
#include <stdlib.h>

using namespace emrt;

thread_local char emrt::g_err[512] = {0};

extern "C" const char* emrt_last_error(void) { return emrt::g_err; }
extern "C" int emrt_abi_version(void) { return 9; }

// ---- tuning knobs: one table, environment read once at load time --------------------------------------------------
namespace {
struct TuneEntry { const char* name; int emrt::Tuning::*field; int def; };
const TuneEntry kTune[] = {
    {"conv_tile", &emrt::Tuning::conv_tile, 0},         {"wgrad_split", &emrt::Tuning::wgrad_split, 0},
    {"thin_cblk", &emrt::Tuning::thin_cblk, 64},        {"thin_blocks", &emrt::Tuning::thin_blocks, 128},
    {"thin_ch", &emrt::Tuning::thin_ch, 8},             {"no_thin_bwd", &emrt::Tuning::no_thin_bwd, 0},
    {"pair_max", &emrt::Tuning::pair_max, 768},         {"msda_fwd_global", &emrt::Tuning::msda_fwd_global, 0},
    {"bn_block_kb", &emrt::Tuning::bn_block_kb, 0},     {"ln_atomic", &emrt::Tuning::ln_atomic, 1},
    {"bn_slice_c", &emrt::Tuning::bn_slice_c, 0},
    {"msda_fwd_chunks", &emrt::Tuning::msda_fwd_chunks, 0}, {"msda_fwd_threads", &emrt::Tuning::msda_fwd_threads, 1024},
    {"msda_fwd_probe", &emrt::Tuning::msda_fwd_probe, 0}, {"wgrad_nst", &emrt::Tuning::wgrad_nst, 2},
    {"igemm64_nst", &emrt::Tuning::igemm64_nst, 3}, {"msda_bwd_global", &emrt::Tuning::msda_bwd_global, 0},
    {"msda_lds_min_pairs", &emrt::Tuning::msda_lds_min_pairs, 2048}, {"msda_bwd_dref_lds", &emrt::Tuning::msda_bwd_dref_lds, 1},
    {"gn_group_blocks", &emrt::Tuning::gn_group_blocks, 0}, {"gn_stat_rows", &emrt::Tuning::gn_stat_rows, 32},
    {"gn_bwd_stat_rows", &emrt::Tuning::gn_bwd_stat_rows, 32}, {"gn_apply_rows", &emrt::Tuning::gn_apply_rows, 8},
    {"msda_scatter_cuts", &emrt::Tuning::msda_scatter_cuts, 0}, {"msda_scatter_qsplit", &emrt::Tuning::msda_scatter_qsplit, 0}, {"msda_band_halo", &emrt::Tuning::msda_band_halo, 0},
    {"igemm8p_probe", &emrt::Tuning::igemm8p_probe, 0}, {"igemm8p_min_blocks", &emrt::Tuning::igemm8p_min_blocks, 160}, {"igemm8p_cmajor", &emrt::Tuning::igemm8p_cmajor, 0},
    {"wgrad8p_min_steps", &emrt::Tuning::wgrad8p_min_steps, 8}, {"wgrad8p_slab", &emrt::Tuning::wgrad8p_slab, 1}, {"wgrad8p_force", &emrt::Tuning::wgrad8p_force, 0}, {"wgrad8p_xcd", &emrt::Tuning::wgrad8p_xcd, 1},
    {"wgrad_no_overwrite", &emrt::Tuning::wgrad_no_overwrite, 0}, {"no_ksplit128", &emrt::Tuning::no_ksplit128, 0}, {"ln_bwd_rows", &emrt::Tuning::ln_bwd_rows, 0}, {"ln_bwd_max_blocks", &emrt::Tuning::ln_bwd_max_blocks, 0}, {"bn_operand_blocks", &emrt::Tuning::bn_operand_blocks, 0}, {"no_s2_dgrad", &emrt::Tuning::no_s2_dgrad, 0}, {"wgroup_blocks", &emrt::Tuning::wgroup_blocks, 1024}, {"wgroup_min_steps", &emrt::Tuning::wgroup_min_steps, 32}, {"wgroup_max", &emrt::Tuning::wgroup_max, 0},
    {"no_bna", &emrt::Tuning::no_bna, 0}, {"memcpy_kernel", &emrt::Tuning::memcpy_kernel, 0}, {"xk", &emrt::Tuning::xk, 0}, {"mha_valu", &emrt::Tuning::mha_valu, 0}, {"mha_bwd_split", &emrt::Tuning::mha_bwd_split, 1}, {"msda_scatter_merge", &emrt::Tuning::msda_scatter_merge, 0},
    {"wgroup8", &emrt::Tuning::wgroup8, 0}, {"wgroup8_blocks", &emrt::Tuning::wgroup8_blocks, 0}, {"wgroup8_min_work", &emrt::Tuning::wgroup8_min_work, 6000},
    {"msda_scatter_mfma", &emrt::Tuning::msda_scatter_mfma, 1}, {"sgd_nt", &emrt::Tuning::sgd_nt, 1}, {"ln_bwd_threads", &emrt::Tuning::ln_bwd_threads, 512}, {"msda_mf_bands", &emrt::Tuning::msda_mf_bands, 0},
};
emrt::Tuning tuning_from_env() {
  emrt::Tuning t;
  for (const TuneEntry& e : kTune) {
    char env[64] = "EMRT_";
    size_t n = strlen(env);
    for (const char* c = e.name; *c && n + 1 < sizeof(env); ++c) env[n++] = (char)((*c >= 'a' && *c <= 'z') ? *c - 32 : *c);
    env[n] = 0;
    // the probe knob switches parts of a kernel OFF (wrong results, timing experiments only): never from the environment of a
    // production process, only through an explicit emrt_set_tuning() call of the experiment script
    const char* v = (strcmp(e.name, "msda_fwd_probe") == 0 || strcmp(e.name, "igemm8p_probe") == 0) ? nullptr : getenv(env);
    t.*(e.field) = v ? atoi(v) : e.def;
  }
  return t;
}
}  // namespace
emrt::Tuning emrt::g_tune = tuning_from_env();
emrt::Scratch emrt::g_scratch = {nullptr, 0, nullptr, nullptr, nullptr};

extern "C" int emrt_set_scratch(void* ptr, size_t bytes, void* stream) {
  EMRT_REQUIRE((ptr != nullptr) == (bytes > 0) && ((uintptr_t)ptr) % 256 == 0, "scratch must be 256-byte aligned device memory (or nullptr, 0)");
  // the SAME region again: only the stream it belongs to changes (host state, legal during a stream capture: the caller moves the region to the
  // capture stream for the duration of a capture and back -- a graph's kernels are ordered among themselves like one stream's).  No memset:
  // the counters are zero between launches by construction.
  if (ptr && ptr == emrt::g_scratch.ptr && emrt::g_scratch.tick && bytes == emrt::g_scratch.bytes + emrt::SCRATCH_TICK_BYTES + emrt::SCRATCH_XK_BYTES) {
    emrt::g_scratch.stream = stream;
    return 0;
  }
  emrt::g_scratch.ptr = ptr;
  emrt::g_scratch.bytes = bytes;
  emrt::g_scratch.stream = stream;
  emrt::g_scratch.tick = nullptr;
  emrt::g_scratch.xk_part = nullptr;
  // a region of more than 16 MiB gives its last 8 MiB + 64 KiB to the cross-block K split: partial tiles, then arrival counters; the counters are
  // zeroed HERE, once, on the registered stream (an enqueued memset, no synchronisation) and every launch leaves them zero again
  if (ptr && bytes >= (16u << 20) + emrt::SCRATCH_XK_BYTES + emrt::SCRATCH_TICK_BYTES && bytes % 256 == 0) {
    emrt::g_scratch.bytes = bytes - emrt::SCRATCH_TICK_BYTES - emrt::SCRATCH_XK_BYTES;
    emrt::g_scratch.xk_part = reinterpret_cast<float*>(static_cast<char*>(ptr) + emrt::g_scratch.bytes);
    emrt::g_scratch.tick = reinterpret_cast<unsigned*>(static_cast<char*>(ptr) + emrt::g_scratch.bytes + emrt::SCRATCH_XK_BYTES);
    if (hipMemsetAsync(emrt::g_scratch.tick, 0, emrt::SCRATCH_TICK_BYTES, (hipStream_t)stream) != hipSuccess) {
      emrt::g_scratch.tick = nullptr;
      return emrt::fail("emrt_set_scratch", "cannot zero the arrival counters");
    }
  }
  return 0;
}

extern "C" int emrt_set_tuning(const char* name, int value) {
  EMRT_REQUIRE(name, "null name");
  for (const TuneEntry& e : kTune)
    if (strcmp(e.name, name) == 0) { emrt::g_tune.*(e.field) = value; return 0; }
  return emrt::fail("emrt_set_tuning", "unknown knob");
}
extern "C" int emrt_get_tuning(const char* name, int* value) {
  EMRT_REQUIRE(name && value, "null pointer");
  for (const TuneEntry& e : kTune)
    if (strcmp(e.name, name) == 0) { *value = emrt::g_tune.*(e.field); return 0; }
  return emrt::fail("emrt_get_tuning", "unknown knob");
}

static inline int ew_grid(long long total) {
  long long g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

// out[i] = a[i] + b[i % period]   (n, period multiples of 4)
template <class T>
__global__ __launch_bounds__(256) void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, long long n4,
                                                  long long period4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float x[4], y[4];
    Vec4<T>::load(a + i * 4, x);
    Vec4<T>::load(b + ((n4 | period4) <= 0xffffffffll ? (long long)((unsigned)i % (unsigned)period4) : i % period4) * 4, y);      // (32-bit division: common.hpp, unravel)
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] += y[e];
    Vec4<T>::store(out + i * 4, x);
  }
}

// out[i] = a[i] + float_row[i % period]  (fp32 broadcast operand, e.g. a parameter row)
template <class T>
__global__ __launch_bounds__(256) void add_f32row_kernel(const T* __restrict__ a, const float* __restrict__ b, T* __restrict__ out,
                                                         long long n4, long long period4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float x[4];
    Vec4<T>::load(a + i * 4, x);
    const float4 y = reinterpret_cast<const float4*>(b)[(n4 | period4) <= 0xffffffffll ? (long long)((unsigned)i % (unsigned)period4) : i % period4];
    x[0] += y.x; x[1] += y.y; x[2] += y.z; x[3] += y.w;
    Vec4<T>::store(out + i * 4, x);
  }
}

// out[r][:] = a[r][:] + rows[level of r][:]: rows [L][C] fp32, level l = token rows [start[l], start[l + 1]) (the encoder's pos = sine + level_embed[l],
// transformer_encoder_decoder.py:447-448: one launch for all levels)
struct LevelStarts { int start[5]; int L; };
template <class T>
__global__ __launch_bounds__(256) void add_f32row_levels_kernel(const T* __restrict__ a, const float* __restrict__ rows, T* __restrict__ out,
                                                                long long n4, int C4, LevelStarts ls) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / C4), c4 = (int)(i - (long long)r * C4);
    int l = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) l += (k < ls.L && r >= ls.start[k]) ? 1 : 0;
    float x[4];
    Vec4<T>::load(a + i * 4, x);
    const float4 y = reinterpret_cast<const float4*>(rows)[(long long)l * C4 + c4];
    x[0] += y.x; x[1] += y.y; x[2] += y.z; x[3] += y.w;
    Vec4<T>::store(out + i * 4, x);
  }
}

// dst[b][r][c] += src[b][r][c]: three-level strided views (batch stride, row stride, unit column stride) -- covers
// dense tensors, token slabs of [B, Lv, C] and channel slices of the concat buffer (gradient accumulation into views)
template <class T>
__global__ __launch_bounds__(256) void acc3d_kernel(T* __restrict__ dst, long long dst_bs, long long dst_rs, const T* __restrict__ src,
                                                    long long src_bs, long long src_rs, long long B, long long rows, long long cols4) {
  const long long total = B * rows * cols4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c4, ri;
    long long b;
    unravel3(i, (int)cols4, (int)rows, total <= 0xffffffffll, c4, ri, b);      // (rows, cols < 2^31: host-checked)
    const long long c = (long long)c4 * 4, r = ri;
    float x[4], y[4];
    Vec4<T>::load(dst + b * dst_bs + r * dst_rs + c, x);
    Vec4<T>::load(src + b * src_bs + r * src_rs + c, y);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] += y[e];
    Vec4<T>::store(dst + b * dst_bs + r * dst_rs + c, x);
  }
}

// out[b][r][c] = a[b][r][c] + b2[b][r][c]
template <class T>
__global__ __launch_bounds__(256) void add3d_kernel(const T* __restrict__ a, long long a_bs, long long a_rs, const T* __restrict__ b2,
                                                    long long b_bs, long long b_rs, T* __restrict__ out, long long o_bs, long long o_rs,
                                                    long long B, long long rows, long long cols4) {
  const long long total = B * rows * cols4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c4, ri;
    long long b;
    unravel3(i, (int)cols4, (int)rows, total <= 0xffffffffll, c4, ri, b);      // (rows, cols < 2^31: host-checked)
    const long long c = (long long)c4 * 4, r = ri;
    float x[4], y[4];
    Vec4<T>::load(a + b * a_bs + r * a_rs + c, x);
    Vec4<T>::load(b2 + b * b_bs + r * b_rs + c, y);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] += y[e];
    Vec4<T>::store(out + b * o_bs + r * o_rs + c, x);
  }
}

// y = dropout(x) (inverted, scale 1/(1-p)).  mode 0: per element; mode 1: per (image, channel) (Dropout2D, NHWC rows of C)
template <class T>
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long long n4, float p,
                                                          const unsigned long long* __restrict__ seed, unsigned salt, int mode,
                                                          long long hw, int C) {
  const unsigned long long sd = seed[0];
  const float ks = 1.f / (1.f - p);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float v[4];
    Vec4<T>::load(x + i * 4, v);
    if (mode == 0) {      // one draw per quad of elements (drop_hash.hpp: drop_quad)
      uint32_t h[2];
      drop_quad(sd, salt, (unsigned long long)i, h);
      const uint32_t thr = drop_thr16(p);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = drop_quad_keep(h, e, thr) ? v[e] * ks : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long idx = i * 4 + e;
        v[e] = uniform01(sd, salt, (unsigned long long)((idx / C / hw) * C + idx % C)) >= p ? v[e] * ks : 0.f;
      }
    }
    Vec4<T>::store(y + i * 4, v);
  }
}

// dx = dy * dropmask/(1-p) * (relu_out > 0)      (either mask optional: p == 0 / relu_out == null)
template <class T>
__global__ __launch_bounds__(256) void mask_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ relu_out, T* __restrict__ dx,
                                                       long long n4, float p, const unsigned long long* __restrict__ seed,
                                                       unsigned salt, int mode, long long hw, int C) {
  const unsigned long long sd = (p > 0.f && seed) ? seed[0] : 0ull;
  const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float g[4];
    Vec4<T>::load(dy + i * 4, g);
    if (p > 0.f && seed && mode == 0) {
      uint32_t h[2];
      drop_quad(sd, salt, (unsigned long long)i, h);
      const uint32_t thr = drop_thr16(p);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = drop_quad_keep(h, e, thr) ? g[e] * ks : 0.f;
    } else if (p > 0.f && seed) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long idx = i * 4 + e;
        g[e] = uniform01(sd, salt, (unsigned long long)((idx / C / hw) * C + idx % C)) >= p ? g[e] * ks : 0.f;
      }
    } else if (p > 0.f) {      // seed == NULL: relu_out is dropout(relu(.)) as emrt_conv2d_drop stored it -- (relu_out > 0) below is BOTH masks, this the scale
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] *= ks;
    }
    if (relu_out) {
      float r[4];
      Vec4<T>::load(relu_out + i * 4, r);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = r[e] > 0.f ? g[e] : 0.f;
    }
    Vec4<T>::store(dx + i * 4, g);
  }
}

__global__ void sigmoid_fwd_kernel(const float* x, float* y, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = 1.f / (1.f + __expf(-x[i]));
}
__global__ void sigmoid_bwd_kernel(const float* y, const float* dy, float* dx, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dx[i] = dy[i] * y[i] * (1.f - y[i]);
}

template <class TI, class TO>
__global__ __launch_bounds__(256) void cast_kernel(const TI* __restrict__ in, TO* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = from_f32<TO>(to_f32(in[i]));
}

extern "C" int emrt_add(const void* a, const void* b, void* out, long long n, long long period, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(a && b && out, "null pointer");
  EMRT_REQUIRE(n % 4 == 0 && period % 4 == 0 && period > 0, "n and period must be multiples of 4");
  hipStream_t st = (hipStream_t)stream;
  return with_fwd_dtype("emrt_add", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((add_kernel<T>), dim3(ew_grid(n / 4)), dim3(256), 0, st, (const T*)a, (const T*)b, (T*)out, n / 4, period / 4);
    return check_launch("emrt_add");
  });
}

extern "C" int emrt_add3d(const void* a, long long a_bs, long long a_rs, const void* b, long long b_bs, long long b_rs, void* out,
                          long long out_bs, long long out_rs, long long B, long long rows, long long cols, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(a && b && out, "null pointer");
  EMRT_REQUIRE(cols % 4 == 0 && a_rs % 4 == 0 && b_rs % 4 == 0 && out_rs % 4 == 0 && a_bs % 4 == 0 && b_bs % 4 == 0 && out_bs % 4 == 0,
               "cols and strides must be multiples of 4");
  EMRT_REQUIRE(B > 0 && rows > 0 && cols > 0 && rows < (1ll << 31) && cols < (1ll << 31), "rows / cols must be in [1, 2^31)");
  hipStream_t st = (hipStream_t)stream;
  const int grid = ew_grid(B * rows * (cols / 4));
  return with_fwd_dtype("emrt_add3d", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((add3d_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)a, a_bs, a_rs, (const T*)b, b_bs, b_rs, (T*)out, out_bs, out_rs, B, rows, cols / 4);
    return check_launch("emrt_add3d");
  });
}

// ---- token concat / split: [B][n_i][C] dense parts <-> dense [B][sum n_i][C] in ONE launch (the pyramid-pooling tokens of
// paddle_EMRT.py:70-78 took a memset and four accumulates each way) ----
#define EMRT_MAX_PARTS 8
struct ConcatArgs {
  void* part[EMRT_MAX_PARTS];
  int n[EMRT_MAX_PARTS], start[EMRT_MAX_PARTS];
  int nparts, B, C4, total;
};
template <class T, int SPLIT>
__global__ __launch_bounds__(256) void concat_tokens_kernel(ConcatArgs a, T* __restrict__ whole) {
  const long long count = (long long)a.B * a.total * a.C4;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < count; idx += (long long)gridDim.x * blockDim.x) {
    int q, row;
    long long bb;
    unravel3(idx, a.C4, a.total, count <= 0xffffffffll, q, row, bb);
    const int b = (int)bb;
    int p = 0;
#pragma unroll
    for (int k = 1; k < EMRT_MAX_PARTS; ++k)
      if (k < a.nparts && row >= a.start[k]) p = k;
    T* pp = (T*)a.part[p] + (((long long)b * a.n[p] + (row - a.start[p])) * a.C4 + q) * 4;
    T* wp = whole + idx * 4;
    float v[4];
    if (SPLIT) { Vec4<T>::load(wp, v); Vec4<T>::store(pp, v); }
    else { Vec4<T>::load(pp, v); Vec4<T>::store(wp, v); }
  }
}
extern "C" int emrt_concat_tokens(void* const* parts, const int* n, int nparts, void* whole, int B, int C, int split, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(parts && n && whole && nparts >= 1 && nparts <= EMRT_MAX_PARTS && C % 4 == 0 && B > 0, "1..8 parts, C a multiple of 4");
  ConcatArgs a;
  memset(&a, 0, sizeof(a));
  int total = 0;
  for (int i = 0; i < nparts; ++i) {
    EMRT_REQUIRE(parts[i] && n[i] > 0, "null / empty part");
    a.part[i] = parts[i]; a.n[i] = n[i]; a.start[i] = total;
    total += n[i];
  }
  a.nparts = nparts; a.B = B; a.C4 = C / 4; a.total = total;
  hipStream_t st = (hipStream_t)stream;
  const int grid = ew_grid((long long)B * total * (C / 4));
  return with_fwd_dtype("emrt_concat_tokens", dtype, [&](auto t) {
    using T = decltype(t);
    if (split) hipLaunchKernelGGL((concat_tokens_kernel<T, 1>), dim3(grid), dim3(256), 0, st, a, (T*)whole);
    else hipLaunchKernelGGL((concat_tokens_kernel<T, 0>), dim3(grid), dim3(256), 0, st, a, (T*)whole);
    return check_launch("emrt_concat_tokens");
  });
}

extern "C" int emrt_acc3d(void* dst, long long dst_bs, long long dst_rs, const void* src, long long src_bs, long long src_rs, long long B,
                          long long rows, long long cols, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(dst && src, "null pointer");
  EMRT_REQUIRE(cols % 4 == 0 && dst_rs % 4 == 0 && src_rs % 4 == 0 && dst_bs % 4 == 0 && src_bs % 4 == 0, "cols and strides must be multiples of 4");
  EMRT_REQUIRE(B > 0 && rows > 0 && cols > 0 && rows < (1ll << 31) && cols < (1ll << 31), "rows / cols must be in [1, 2^31)");
  hipStream_t st = (hipStream_t)stream;
  const int grid = ew_grid(B * rows * (cols / 4));
  return with_fwd_dtype("emrt_acc3d", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((acc3d_kernel<T>), dim3(grid), dim3(256), 0, st, (T*)dst, dst_bs, dst_rs, (const T*)src, src_bs, src_rs, B, rows, cols / 4);
    return check_launch("emrt_acc3d");
  });
}

extern "C" int emrt_add_f32row(const void* a, const float* row, void* out, long long n, long long period, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(a && row && out, "null pointer");
  EMRT_REQUIRE(n % 4 == 0 && period % 4 == 0 && period > 0, "n and period must be multiples of 4");
  hipStream_t st = (hipStream_t)stream;
  return with_fwd_dtype("emrt_add_f32row", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((add_f32row_kernel<T>), dim3(ew_grid(n / 4)), dim3(256), 0, st, (const T*)a, row, (T*)out, n / 4, period / 4);
    return check_launch("emrt_add_f32row");
  });
}

extern "C" int emrt_add_f32row_levels(const void* a, const float* rows, void* out, const int* level_start, int L, int Lv, int C, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(a && rows && out && level_start, "null pointer");
  EMRT_REQUIRE(L >= 1 && L <= 4 && C % 4 == 0 && C > 0 && Lv > 0, "1..4 levels, C a multiple of 4");
  LevelStarts ls;
  for (int l = 0; l < 5; ++l) ls.start[l] = Lv;
  ls.L = L;
  for (int l = 0; l < L; ++l) {
    EMRT_REQUIRE(level_start[l] >= 0 && level_start[l] < Lv && (l == 0 ? level_start[0] == 0 : level_start[l] > level_start[l - 1]), "level_start must start at 0 and increase");
    ls.start[l] = level_start[l];
  }
  const long long n4 = (long long)Lv * C / 4;
  hipStream_t st = (hipStream_t)stream;
  return with_fwd_dtype("emrt_add_f32row_levels", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((add_f32row_levels_kernel<T>), dim3(ew_grid(n4)), dim3(256), 0, st, (const T*)a, rows, (T*)out, n4, C / 4, ls);
    return check_launch("emrt_add_f32row_levels");
  });
}

extern "C" int emrt_dropout_fwd(const void* x, void* y, long long n, float p, const unsigned long long* seed, unsigned salt, int mode,
                                long long hw, int C, int dtype, void* stream) {
  EMRT_REQUIRE_TRAIN_DTYPE(dtype);
  EMRT_REQUIRE(x && y && seed, "null pointer");
  EMRT_REQUIRE(n % 4 == 0 && p >= 0.f && p < 1.f, "n must be a multiple of 4, 0 <= p < 1");
  EMRT_REQUIRE(mode == 0 || (hw > 0 && C > 0), "channel mode needs hw and C");
  hipStream_t st = (hipStream_t)stream;
  return with_train_dtype("emrt_dropout_fwd", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((dropout_fwd_kernel<T>), dim3(ew_grid(n / 4)), dim3(256), 0, st, (const T*)x, (T*)y, n / 4, p, seed, salt, mode, hw, C);
    return check_launch("emrt_dropout_fwd");
  });
}

extern "C" int emrt_mask_bwd(const void* dy, const void* relu_out, void* dx, long long n, float p, const unsigned long long* seed,
                             unsigned salt, int mode, long long hw, int C, int dtype, void* stream) {
  EMRT_REQUIRE_TRAIN_DTYPE(dtype);
  EMRT_REQUIRE(dy && dx, "null pointer");
  EMRT_REQUIRE(n % 4 == 0 && p >= 0.f && p < 1.f, "n must be a multiple of 4, 0 <= p < 1");
  EMRT_REQUIRE(p == 0.f || seed || relu_out, "dropout needs a device seed (or, seed == NULL, the stored output of emrt_conv2d_drop as relu_out)");
  hipStream_t st = (hipStream_t)stream;
  return with_train_dtype("emrt_mask_bwd", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((mask_bwd_kernel<T>), dim3(ew_grid(n / 4)), dim3(256), 0, st, (const T*)dy, (const T*)relu_out, (T*)dx, n / 4, p, seed, salt, mode, hw, C);
    return check_launch("emrt_mask_bwd");
  });
}

extern "C" int emrt_sigmoid_fwd(const float* x, float* y, long long n, void* stream) {
  EMRT_REQUIRE(x && y, "null pointer");
  hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return check_launch("emrt_sigmoid_fwd");
}
extern "C" int emrt_sigmoid_bwd(const float* y, const float* dy, float* dx, long long n, void* stream) {
  EMRT_REQUIRE(y && dy && dx, "null pointer");
  hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, y, dy, dx, n);
  return check_launch("emrt_sigmoid_bwd");
}

// direction 0: f32 -> dtype ; 1: dtype -> f32
extern "C" int emrt_cast(const void* in, void* out, long long n, int direction, int dtype, void* stream) {
  EMRT_REQUIRE_FWD_DTYPE(dtype);
  EMRT_REQUIRE(in && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = ew_grid(n);
  return with_fwd_dtype("emrt_cast", dtype, [&](auto t) {
    using T = decltype(t);
    if (direction == 0) hipLaunchKernelGGL((cast_kernel<float, T>), dim3(grid), dim3(256), 0, st, (const float*)in, (T*)out, n);
    else hipLaunchKernelGGL((cast_kernel<T, float>), dim3(grid), dim3(256), 0, st, (const T*)in, (float*)out, n);
    return check_launch("emrt_cast");
  });
}

extern "C" int emrt_memset(void* ptr, int value, size_t bytes, void* stream) {
  EMRT_REQUIRE(ptr || bytes == 0, "null pointer");
  if (bytes == 0) return 0;
  hipError_t e = hipMemsetAsync(ptr, value, bytes, (hipStream_t)stream);
  if (e != hipSuccess) return emrt::fail("emrt_memset", hipGetErrorString(e));
  return 0;
}

// 16 bytes per lane, grid-stride: the staging copy as an ordinary kernel of the stream (see emrt_memcpy)
__global__ __launch_bounds__(256) void copy16_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

extern "C" int emrt_memcpy(void* dst, const void* src, size_t bytes, void* stream) {
  EMRT_REQUIRE((dst && src) || bytes == 0, "null pointer");
  if (bytes == 0 || dst == src) return 0;
  // Knob memcpy_kernel = 1 (A/B, default 0): the copy as an ordinary kernel of the stream instead of the runtime's hipMemcpyAsync.  The per-dispatch
  // timeline (profiles/r5c_timeline_cfg2.txt) shows ~85 us of idle queue in front of the runtime's copy between two hipGraph launches, but the step
  // time is the same with either form and with no staging copy at all (round 6: 947.6 / 948.0 / 948.2 tiles/s): the gap is the profiler's, not the step's.
  if (g_tune.memcpy_kernel && bytes % 16 == 0 && ((uintptr_t)dst | (uintptr_t)src) % 16 == 0) {
    const size_t n16 = bytes / 16;
    size_t blocks = (n16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)dst, (const uint4*)src, n16);
    return emrt::check_launch("emrt_memcpy");
  }
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return emrt::fail("emrt_memcpy", hipGetErrorString(e));
  return 0;
}

extern "C" int emrt_device_info(int* cu_count, size_t* lds_bytes, char* arch, int arch_len) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return emrt::fail("emrt_device_info", hipGetErrorString(e));
  hipDeviceProp_t p;
  e = hipGetDeviceProperties(&p, dev);
  if (e != hipSuccess) return emrt::fail("emrt_device_info", hipGetErrorString(e));
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (lds_bytes) *lds_bytes = p.sharedMemPerBlock;
  if (arch && arch_len > 0) { strncpy(arch, p.gcnArchName, arch_len - 1); arch[arch_len - 1] = 0; }
  return 0;
}

// HIP-event timing helpers for bench.py: events are recorded on the SAME stream the kernels are launched on.
extern "C" int emrt_event_create(void** ev) {
  hipEvent_t e;
  hipError_t r = hipEventCreate(&e);
  if (r != hipSuccess) return emrt::fail("emrt_event_create", hipGetErrorString(r));
  *ev = (void*)e;
  return 0;
}
extern "C" int emrt_event_record(void* ev, void* stream) {
  hipError_t r = hipEventRecord((hipEvent_t)ev, (hipStream_t)stream);
  if (r != hipSuccess) return emrt::fail("emrt_event_record", hipGetErrorString(r));
  return 0;
}
extern "C" int emrt_event_elapsed_ms(void* start, void* stop, float* ms) {
  hipError_t r = hipEventSynchronize((hipEvent_t)stop);
  if (r == hipSuccess) r = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
  if (r != hipSuccess) return emrt::fail("emrt_event_elapsed_ms", hipGetErrorString(r));
  return 0;
}
extern "C" int emrt_event_destroy(void* ev) {
  return hipEventDestroy((hipEvent_t)ev) == hipSuccess ? 0 : emrt::fail("emrt_event_destroy", "hipEventDestroy failed");
}
