// libemrt_hip_sampler.so: class-aware tile origins for the resident-scene sampler.  The public interface, the index layout and the arithmetic
// of the redraw are described in include/emrt_hip_sampler.h; Philox4x32-10 and the integer draw are ../philox.hpp, the text the two draw
// kernels compile.  A library of its own because the ABIs of the other two headers are pinned.
//
// Two kernels, both one wave (64 lanes) per unit of work and integer-only:
//   row counts: a wave owns one row of one label map.  Lanes load aligned 32-bit words of the row (the up to three bytes before the first and
//               after the last aligned word go one per lane in a pass of their own), map each byte through the lookup table, and for every class
//               one ballot + population count per byte lane gives the row's count; lane c keeps class c's sum.  No atomics, no float.
//   redraw:     a wave owns one sample.  All lanes take the same decisions from Philox blocks 8 and 9; the class's prefix table and the row
//               table are searched 64 entries per load (the launch sits on the step's critical path: dependent loads are its cost);
//               the row is then scanned 256 bytes per pass (four coalesced 64-byte loads in flight), ballot + population count find the chunk
//               and the lane that hold the j-th pixel of the class.  Lane 0 writes columns 0-2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../../include/emrt_hip_sampler.h"
#include "../philox.hpp"

namespace emrt {
namespace {

thread_local char g_smp_err[512] = "";

int fail(const char* fn, const char* msg) {
  snprintf(g_smp_err, sizeof(g_smp_err), "%s: %s", fn, msg);
  return -1;
}
int check_launch(const char* fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_smp_err, sizeof(g_smp_err), "%s: launch failed: %s", fn, hipGetErrorString(e));
    return -2;
  }
  return 0;
}
#define SMP_REQUIRE(cond, msg)                 \
  do {                                         \
    if (!(cond)) return fail(__func__, msg);   \
  } while (0)

constexpr int SMP_WAVE = 64;
constexpr int SMP_COUNT_WAVES = 4;     // rows per block of the counting launch
constexpr int SMP_MAX_SIDE = 1 << 15;  // the tile's sides, as in the draw and sample launches
constexpr int SMP_NOT_A_CLASS = 256;   // what a byte outside the row "maps to": above every class

// The last scene whose first row is <= r: always a valid scene index, whatever the table holds.
__device__ __forceinline__ int scene_of_row(const long long* row_start, int n_scenes, long long r) {
  int lo = 0, hi = n_scenes - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row_start[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct CountArgs {
  const unsigned char* bank;
  const EmrtSceneEntry* scenes;        // device
  const long long* row_start;          // device, [n_scenes + 1]
  int* counts;                         // device, [total_rows][n_classes]
  long long total_rows;
  int n_scenes, n_classes;
  unsigned char lut[256];
};

__global__ __launch_bounds__(SMP_WAVE * SMP_COUNT_WAVES) void smp_row_counts_kernel(CountArgs a) {
  const int lane = threadIdx.x & (SMP_WAVE - 1);
  const long long row = (long long)blockIdx.x * SMP_COUNT_WAVES + (threadIdx.x >> 6);
  if (row >= a.total_rows) return;     // (the whole wave leaves: every ballot below is taken by 64 lanes)
  const int s = scene_of_row(a.row_start, a.n_scenes, row);
  const EmrtSceneEntry e = a.scenes[s];
  const long long y = clampll(row - a.row_start[s], 0, (long long)e.H - 1);
  const unsigned char* p = a.bank + e.lab_off + y * e.W;
  const int W = e.W;
  const int to_word = (int)((4u - (unsigned)((uintptr_t)p & 3u)) & 3u);
  const int head = to_word < W ? to_word : W;
  const int nwords = (W - head) >> 2, tail = W - head - 4 * nwords;
  const unsigned* pw = (const unsigned*)(p + head);
  for (int cbase = 0; cbase < a.n_classes; cbase += SMP_WAVE) {      // (one trip for up to 64 classes; lane l keeps class cbase + l)
    const int cend = cbase + SMP_WAVE < a.n_classes ? cbase + SMP_WAVE : a.n_classes;
    int acc = 0;
    for (int w0 = 0; w0 < nwords; w0 += SMP_WAVE) {
      const int wi = w0 + lane;
      const bool ok = wi < nwords;
      const unsigned v = ok ? pw[wi] : 0u;
      const int m0 = ok ? a.lut[v & 255u] : SMP_NOT_A_CLASS, m1 = ok ? a.lut[(v >> 8) & 255u] : SMP_NOT_A_CLASS;
      const int m2 = ok ? a.lut[(v >> 16) & 255u] : SMP_NOT_A_CLASS, m3 = ok ? a.lut[v >> 24] : SMP_NOT_A_CLASS;
      for (int c = cbase; c < cend; ++c) {
        const int n = __popcll(__ballot(m0 == c)) + __popcll(__ballot(m1 == c)) + __popcll(__ballot(m2 == c)) + __popcll(__ballot(m3 == c));
        if (lane == c - cbase) acc += n;
      }
    }
    {      // the bytes before the first and after the last aligned word: at most three each, one per lane
      int m = SMP_NOT_A_CLASS;
      if (lane < head) m = a.lut[p[lane]];
      else if (lane - head < tail) m = a.lut[p[head + 4 * nwords + (lane - head)]];
      for (int c = cbase; c < cend; ++c) {
        const int n = __popcll(__ballot(m == c));
        if (lane == c - cbase) acc += n;
      }
    }
    if (cbase + lane < cend) a.counts[row * a.n_classes + cbase + lane] = acc;
  }
}

struct RedrawArgs {
  const long long* step;               // device: the step counter
  const unsigned char* bank;
  const EmrtSceneEntry* scenes;        // device
  const long long* row_start;          // device, [n_scenes + 1]
  const long long* cum;                // device, [n_classes][R + 1]
  const unsigned long long* thr;       // device, [n_classes]
  int* draws;                          // device, [B][cols]
  double prob;
  long long R;
  unsigned k0, k1, first;              // key words; rank * B
  int n_scenes, n_classes, last_cls, th, tw, cols;
  unsigned char lut[256];
};

__global__ __launch_bounds__(SMP_WAVE) void smp_class_redraw_kernel(RedrawArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const unsigned long long step = (unsigned long long)a.step[0];
  const unsigned s_lo = (unsigned)step, s_hi = (unsigned)(step >> 32), id = a.first + (unsigned)b;
  const Philox r8 = philox4x32_10(s_lo, s_hi, id, (unsigned)EMRT_SMP_BLOCK_CLASS, a.k0, a.k1);
  if (!(unit(r8.v[0]) < a.prob)) return;      // (every decision below is the same in all 64 lanes: the wave stays whole)
  const Philox r9 = philox4x32_10(s_lo, s_hi, id, (unsigned)EMRT_SMP_BLOCK_OFFSET, a.k0, a.k1);
  int cls = 0;                         // lane l compares threshold c0 + l: one load per 64 classes
  for (int c0 = 0; c0 < a.n_classes; c0 += SMP_WAVE) {
    const int c = c0 + lane;
    cls += __popcll(__ballot(c < a.n_classes && (unsigned long long)r8.v[1] >= a.thr[c]));
  }
  cls = cls < a.last_cls ? cls : a.last_cls;
  const long long* cum = a.cum + (long long)cls * (a.R + 1);
  const long long n_cls = cum[a.R];
  if (n_cls <= 0) return;
  const long long k = (long long)below(r8.v[2], r8.v[3], (unsigned long long)n_cls);
  // The last row of [0, R) whose prefix is <= k, the row that holds pixel k, by a 64-way search: the lanes probe 64 evenly spaced rows of the
  // range at once and the range shrinks to the stretch behind the last probe that is <= k.  Three rounds of one load each for a quarter of a
  // million rows, where a binary search is a chain of 18 dependent loads on the step's critical path.
  long long lo = 0, n = a.R;
  while (n > 1) {
    const long long stride = (n + SMP_WAVE - 1) / SMP_WAVE, i = lo + lane * stride;
    const unsigned long long le = __ballot(i < lo + n && cum[i] <= k);
    const int t = le ? 63 - __clzll((long long)le) : 0;      // (the prefix is monotone: the lanes that are <= k are lanes 0..t)
    const long long end = lo + n;
    lo += t * stride;
    n = end - lo < stride ? end - lo : stride;
  }
  long long j = k - cum[lo];
  if (j < 0) return;                   // (only a foreign table: cum[0] is 0)
  int s = 0;                           // the last scene whose first row is <= lo, 64 scenes per round (row_start[0] is 0)
  for (int s0 = 0; s0 < a.n_scenes; s0 += SMP_WAVE) {
    const int c = s0 + lane;
    const unsigned long long le = __ballot(c < a.n_scenes && a.row_start[c] <= lo);
    if (!le) break;
    s = s0 + 63 - __clzll((long long)le);
  }
  const EmrtSceneEntry e = a.scenes[s];
  const int y = (int)clampll(lo - a.row_start[s], 0, (long long)e.H - 1);
  const unsigned char* p = a.bank + e.lab_off + (long long)y * e.W;
  int x = -1;
  for (int xb = 0; xb < e.W && x < 0; xb += 4 * SMP_WAVE) {
    int m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int xi = xb + q * SMP_WAVE + lane;
      m[q] = xi < e.W ? (int)a.lut[p[xi]] : SMP_NOT_A_CLASS;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool mine = m[q] == cls;
      const unsigned long long mask = __ballot(mine);
      const long long cnt = __popcll(mask);
      if (x < 0) {
        if (j < cnt) {
          const long long before = __popcll(mask & ((1ull << lane) - 1ull));
          const unsigned long long hit = __ballot(mine && before == j);
          x = xb + q * SMP_WAVE + __ffsll(hit) - 1;
        } else {
          j -= cnt;
        }
      }
    }
  }
  if (x < 0) return;                   // the index promised a pixel the row does not hold: the uniform draw stands
  if (lane == 0) {
    const int dy = (int)__umulhi(r9.v[0], (unsigned)a.th), dx = (int)__umulhi(r9.v[1], (unsigned)a.tw);
    int* d = a.draws + (long long)b * a.cols;
    d[0] = s;
    d[1] = min(max(y - dy, 0), e.H - a.th);
    d[2] = min(max(x - dx, 0), e.W - a.tw);
  }
}

// The checks both entry points share, on the HOST mirrors: every scene lies inside the bank and holds the tile; row_start is the running sum
// of the heights.  -> 0, with the number of rows in *R.
int check_tables(const char* fn, const EmrtSceneEntry* scenes, const long long* row_start, int n_scenes, size_t bank_bytes, int th, int tw, long long* R) {
  if (!(n_scenes > 0)) return fail(fn, "n_scenes must be positive");
  if (!(th > 0 && tw > 0 && th <= SMP_MAX_SIDE && tw <= SMP_MAX_SIDE)) return fail(fn, "the tile must be positive (th, tw <= 32768)");
  const long long nbytes = (long long)bank_bytes;
  if (nbytes < 0) return fail(fn, "bank_bytes too large");
  if (row_start[0] != 0) return fail(fn, "the row table must start at 0");
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
    if (row_start[i + 1] - row_start[i] != e.H) {
      snprintf(msg, sizeof(msg), "scene %d: the row table holds %lld rows, the scene has %d", i, row_start[i + 1] - row_start[i], e.H);
      return fail(fn, msg);
    }
  }
  *R = row_start[n_scenes];
  return 0;
}

void fill_lut(unsigned char* lut, const unsigned char* label_lut) {
  for (int i = 0; i < 256; ++i) lut[i] = label_lut ? label_lut[i] : (unsigned char)i;
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" const char* emrt_smp_last_error(void) { return g_smp_err; }

extern "C" int emrt_smp_version(void) { return 1; }

extern "C" int emrt_smp_row_counts(const unsigned char* bank, size_t bank_bytes, const EmrtSceneEntry* scenes, const EmrtSceneEntry* scenes_host,
                                   const long long* row_start, const long long* row_start_host, int n_scenes, const unsigned char* label_lut,
                                   int n_classes, int* counts, long long total_rows, void* stream) {
  SMP_REQUIRE(bank && scenes && scenes_host && row_start && row_start_host && counts, "null pointer");
  SMP_REQUIRE(n_classes >= 1 && n_classes <= EMRT_SMP_MAX_CLASSES, "n_classes must be 1..256");
  long long R = 0;
  if (int r = check_tables(__func__, scenes_host, row_start_host, n_scenes, bank_bytes, 1, 1, &R)) return r;
  SMP_REQUIRE(total_rows == R, "total_rows is not the last entry of the row table");
  SMP_REQUIRE(R <= (1ll << 31) - SMP_COUNT_WAVES, "too many rows");
  CountArgs a{};
  a.bank = bank;
  a.scenes = scenes;
  a.row_start = row_start;
  a.counts = counts;
  a.total_rows = R;
  a.n_scenes = n_scenes;
  a.n_classes = n_classes;
  fill_lut(a.lut, label_lut);
  const unsigned blocks = (unsigned)((R + SMP_COUNT_WAVES - 1) / SMP_COUNT_WAVES);
  hipLaunchKernelGGL(smp_row_counts_kernel, dim3(blocks), dim3(SMP_WAVE * SMP_COUNT_WAVES), 0, (hipStream_t)stream, a);
  return check_launch(__func__);
}

extern "C" int emrt_smp_class_redraw(const long long* step_counter, const unsigned char* bank, size_t bank_bytes, const EmrtSceneEntry* scenes,
                                     const EmrtSceneEntry* scenes_host, const long long* row_start, const long long* row_start_host, int n_scenes,
                                     const long long* class_cum, const unsigned long long* thresholds, const unsigned long long* thresholds_host,
                                     int n_classes, const unsigned char* label_lut, long long key, int rank, int B, int th, int tw, double prob,
                                     int* draws, int draw_cols, void* stream) {
  SMP_REQUIRE(step_counter && bank && scenes && scenes_host && row_start && row_start_host && class_cum && thresholds && thresholds_host && draws,
              "null pointer");
  SMP_REQUIRE(B > 0, "B must be positive");
  SMP_REQUIRE(rank >= 0 && ((long long)rank + 1) * B <= (1ll << 32), "rank * B + b must fit the 32-bit counter word");
  SMP_REQUIRE(n_classes >= 1 && n_classes <= EMRT_SMP_MAX_CLASSES, "n_classes must be 1..256");
  SMP_REQUIRE(prob >= 0.0 && prob <= 1.0, "the class-mode probability must be in [0, 1]");      // (false for NaN)
  SMP_REQUIRE(draw_cols == 10 || draw_cols == 18, "draw_cols must be 10 (emrt_scene_draw) or 18 (emrt_aug_scene_draw)");
  long long R = 0;
  if (int r = check_tables(__func__, scenes_host, row_start_host, n_scenes, bank_bytes, th, tw, &R)) return r;
  int last_cls = -1;
  for (int c = 0; c < n_classes; ++c) {
    SMP_REQUIRE(thresholds_host[c] <= (1ull << 32) && (c == 0 || thresholds_host[c] >= thresholds_host[c - 1]),
                "the class thresholds must be non-decreasing and at most 2^32");
    if (last_cls < 0 && thresholds_host[c] == (1ull << 32)) last_cls = c;
  }
  SMP_REQUIRE(last_cls >= 0, "the last class threshold must be exactly 2^32");
  RedrawArgs a{};
  a.step = step_counter;
  a.bank = bank;
  a.scenes = scenes;
  a.row_start = row_start;
  a.cum = class_cum;
  a.thr = thresholds;
  a.draws = draws;
  a.prob = prob;
  a.R = R;
  a.k0 = (unsigned)((unsigned long long)key & 0xFFFFFFFFull);
  a.k1 = (unsigned)((unsigned long long)key >> 32);
  a.first = (unsigned)((long long)rank * B);
  a.n_scenes = n_scenes; a.n_classes = n_classes; a.last_cls = last_cls; a.th = th; a.tw = tw; a.cols = draw_cols;
  fill_lut(a.lut, label_lut);
  hipLaunchKernelGGL(smp_class_redraw_kernel, dim3((unsigned)B), dim3(SMP_WAVE), 0, (hipStream_t)stream, a);
  return check_launch(__func__);
}
