// libemrt_hip_rot.so: the quarter turn of the training augmentation as an in-place post-pass over a finished batch.  The public interface, the
// orbit decomposition and the draw layout are described in include/emrt_hip_rot.h; Philox4x32-10 and the integer draw are ../philox.hpp, the text
// the draw kernels of the other libraries compile.  A library of its own because the table of the six libraries before it is pinned.
//
// One kernel behind both entry points.  blockIdx = (tile of the fundamental domain, plane 0..3 of the sample: three fp32 image planes and the int64
// label plane, sample of the launch); the sample's turn comes by value (emrt_rot_batch) or from Philox block 5 (emrt_rot_scene_batch).
//
// Tile and block size, from the LDS numbers of the kernel guides (160 KiB per CU; 64 banks of 4 bytes; the bank of a byte address a is (a / 4) % 32
// for ds_read_b32 and every ds_write, (a / 4) % 64 for ds_read_b64; lanes conflict within a 32-lane half):
//   T = 32: a row of a rectangle is 128 bytes of fp32 (256 of int64), whole cache lines once n is a multiple of 64; a block of 256 threads moves
//           8 rows per pass.  Four rectangles of 32 rows x 33 elements are 16.5 KiB for an image plane and 33 KiB for the label plane (the static
//           allocation is the larger one): 4 blocks = 16 waves per CU, 4 per SIMD, fit the 160 KiB.
//   pitch 33 elements: the transposed read walks a column, lane l at element 33 * l.  fp32: word 33 * l, bank (33 * l) % 32 = l, every bank once
//           per half.  int64: words 66 * l and 66 * l + 1, banks (2 * l) % 64 and the next, again all different within a half.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "../../../include/emrt_hip_rot.h"
#include "../philox.hpp"

namespace emrt {
namespace {

thread_local char g_rot_err[512] = "";

int fail(const char* fn, const char* msg) {
  snprintf(g_rot_err, sizeof(g_rot_err), "%s: %s", fn, msg);
  return -1;
}
int check_launch(const char* fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_rot_err, sizeof(g_rot_err), "%s: launch failed: %s", fn, hipGetErrorString(e));
    return -2;
  }
  return 0;
}
#define ROT_REQUIRE(cond, msg)                 \
  do {                                         \
    if (!(cond)) return fail(__func__, msg);   \
  } while (0)

constexpr int ROT_T = 32;                  // tile edge
constexpr int ROT_PITCH = ROT_T + 1;       // elements per LDS row
constexpr int ROT_ROWS = 8;                // rows per pass of the block
constexpr int ROT_THREADS = ROT_T * ROT_ROWS;
constexpr int ROT_RECT = ROT_T * ROT_PITCH;      // elements of one rectangle in LDS

struct RotArgs {
  float* images;                       // device, [B][3][n][n]
  long long* labels;                   // device, [B][n][n], or null
  const long long* step;               // device: the step counter (scene path), or null: the turns below
  int* turns_out;                      // device, [B] (scene path), or null
  double prob;
  unsigned k0, k1, first;              // key words; rank * B
  int n, tiles_x, first_sample;        // the plane's edge; tiles per row of the domain; the launch's first sample
  int turn[EMRT_ROT_CHUNK];            // the launch's turns (tile path)
};

// The four rectangles of a domain tile at (r0, c0) of th x tw, in orbit order: rectangle i is the tile turned i times.  With (a, b) the position
// inside the tile, the same pixel's orbit has the local (row, column)
//   0: (a, b)   1: (tw - 1 - b, a)   2: (th - 1 - a, tw - 1 - b)   3: (b, th - 1 - a)
// in the rectangles at
//   0: (r0, c0)   1: (n - c0 - tw, r0)   2: (n - r0 - th, n - c0 - tw)   3: (c0, n - r0 - th),   of th x tw (even i) or tw x th (odd i).
struct Tile {
  int n, r0, c0, th, tw;
  __device__ __forceinline__ int row0(int i) const { return i == 0 ? r0 : (i == 1 ? n - c0 - tw : (i == 2 ? n - r0 - th : c0)); }
  __device__ __forceinline__ int col0(int i) const { return i == 0 ? c0 : (i == 1 ? r0 : (i == 2 ? n - c0 - tw : n - r0 - th)); }
  __device__ __forceinline__ int rows(int i) const { return (i & 1) ? tw : th; }
  __device__ __forceinline__ int cols(int i) const { return (i & 1) ? th : tw; }
};

template <typename T>
__device__ __forceinline__ void turn_tile(T* plane, const Tile t, int k, T* lds) {
  const int tx = threadIdx.x & (ROT_T - 1), ty = threadIdx.x >> 5;
  const long long n = t.n;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int h = t.rows(i), w = t.cols(i);
    const T* src = plane + (long long)t.row0(i) * n + t.col0(i);
    for (int lr = ty; lr < h; lr += ROT_ROWS)
      if (tx < w) lds[i * ROT_RECT + lr * ROT_PITCH + tx] = src[lr * n + tx];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int h = t.rows(j), w = t.cols(j), i = (j - k) & 3;
    T* dst = plane + (long long)t.row0(j) * n + t.col0(j);
    for (int lr = ty; lr < h; lr += ROT_ROWS) {
      if (tx < w) {
        // the position (a, b) inside the tile of the pixel that lands at (lr, tx) of rectangle j ...
        const int a = j == 0 ? lr : (j == 1 ? tx : (j == 2 ? t.th - 1 - lr : t.th - 1 - tx));
        const int b = j == 0 ? tx : (j == 1 ? t.tw - 1 - lr : (j == 2 ? t.tw - 1 - tx : lr));
        // ... and where rectangle i holds it
        const int sr = i == 0 ? a : (i == 1 ? t.tw - 1 - b : (i == 2 ? t.th - 1 - a : b));
        const int sc = i == 0 ? b : (i == 1 ? a : (i == 2 ? t.tw - 1 - b : t.th - 1 - a));
        dst[lr * n + tx] = lds[i * ROT_RECT + sr * ROT_PITCH + sc];
      }
    }
  }
}

__global__ __launch_bounds__(ROT_THREADS) void rot_turn_kernel(RotArgs a) {
  __shared__ long long lds[4 * ROT_RECT];
  const int b = a.first_sample + (int)blockIdx.z, plane = blockIdx.y;
  int k;
  if (a.step != nullptr) {             // (the same decision in every thread of every block of the sample)
    const unsigned long long step = (unsigned long long)a.step[0];
    const Philox r = philox4x32_10((unsigned)step, (unsigned)(step >> 32), a.first + (unsigned)b, (unsigned)EMRT_ROT_BLOCK, a.k0, a.k1);
    k = unit(r.v[0]) < a.prob ? 1 + (int)below(r.v[1], r.v[2], 3ull) : 0;
    if (a.turns_out != nullptr && blockIdx.x == 0 && plane == 0 && threadIdx.x == 0) a.turns_out[b] = k;
  } else {
    k = a.turn[blockIdx.z] & 3;
  }
  if (k == 0) return;
  const int dom_rows = (a.n + 1) >> 1, dom_cols = a.n >> 1;
  Tile t;
  t.n = a.n;
  t.r0 = ((int)blockIdx.x / a.tiles_x) * ROT_T;
  t.c0 = ((int)blockIdx.x % a.tiles_x) * ROT_T;
  t.th = min(ROT_T, dom_rows - t.r0);
  t.tw = min(ROT_T, dom_cols - t.c0);
  if (t.th <= 0 || t.tw <= 0) return;      // (n = 1: the domain is empty; the whole block leaves)
  const long long hw = (long long)a.n * a.n;
  if (plane < 3)
    turn_tile<float>(a.images + ((long long)b * 3 + plane) * hw, t, k, reinterpret_cast<float*>(lds));
  else
    turn_tile<long long>(a.labels + (long long)b * hw, t, k, lds);
}

// tiles of the fundamental domain of an n x n plane: -> tiles per row, with the launch's count in *tiles (at least 1: the scene path's one block
// per sample that writes turns_out exists for n = 1 too)
int domain_tiles(int n, unsigned* tiles) {
  const int ty = ((n + 1) / 2 + ROT_T - 1) / ROT_T, tx = (n / 2 + ROT_T - 1) / ROT_T;
  *tiles = (unsigned)(ty * tx > 0 ? ty * tx : 1);
  return tx > 0 ? tx : 1;
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" const char* emrt_rot_last_error(void) { return g_rot_err; }

extern "C" int emrt_rot_version(void) { return 1; }

extern "C" int emrt_rot_batch(float* images, long long* labels, const int* turns, int B, int n, void* stream) {
  ROT_REQUIRE(B >= 1, "B must be at least 1");
  ROT_REQUIRE(n >= 1, "n must be at least 1");
  ROT_REQUIRE(n <= EMRT_ROT_MAX_SIDE, "n must be at most 32768");
  ROT_REQUIRE(turns, "null pointer");
  for (int b = 0; b < B; ++b) {
    if (turns[b] < 0 || turns[b] > 3) {
      char msg[120];
      snprintf(msg, sizeof(msg), "turns[%d] is %d: a turn must be 0..3", b, turns[b]);
      return fail(__func__, msg);
    }
  }
  ROT_REQUIRE(images, "null pointer");
  RotArgs a{};
  a.images = images;
  a.labels = labels;
  a.n = n;
  unsigned tiles = 0;
  a.tiles_x = domain_tiles(n, &tiles);
  for (int b0 = 0; b0 < B; b0 += EMRT_ROT_CHUNK) {
    const int nb = B - b0 < EMRT_ROT_CHUNK ? B - b0 : EMRT_ROT_CHUNK;
    bool any = false;
    for (int i = 0; i < EMRT_ROT_CHUNK; ++i) {
      a.turn[i] = i < nb ? turns[b0 + i] : 0;
      any = any || a.turn[i] != 0;
    }
    if (!any) continue;
    a.first_sample = b0;
    hipLaunchKernelGGL(rot_turn_kernel, dim3(tiles, labels ? 4u : 3u, (unsigned)nb), dim3(ROT_THREADS), 0, (hipStream_t)stream, a);
    if (int r = check_launch(__func__)) return r;
  }
  return 0;
}

extern "C" int emrt_rot_scene_batch(const long long* step_counter, long long key, int rank, int B, int n, double prob, float* images,
                                    long long* labels, int* turns_out, void* stream) {
  ROT_REQUIRE(B >= 1 && B <= EMRT_ROT_MAX_BATCH, "B must be 1..65535");
  ROT_REQUIRE(n >= 1, "n must be at least 1");
  ROT_REQUIRE(n <= EMRT_ROT_MAX_SIDE, "n must be at most 32768");
  ROT_REQUIRE(step_counter && images && turns_out, "null pointer");
  ROT_REQUIRE(rank >= 0 && ((long long)rank + 1) * B <= (1ll << 32), "rank * B + b must fit the 32-bit counter word");
  ROT_REQUIRE(prob >= 0.0 && prob <= 1.0, "the rotation probability must be in [0, 1]");      // (false for NaN)
  RotArgs a{};
  a.images = images;
  a.labels = labels;
  a.step = step_counter;
  a.turns_out = turns_out;
  a.prob = prob;
  a.k0 = (unsigned)((unsigned long long)key & 0xFFFFFFFFull);
  a.k1 = (unsigned)((unsigned long long)key >> 32);
  a.first = (unsigned)((long long)rank * B);
  a.n = n;
  unsigned tiles = 0;
  a.tiles_x = domain_tiles(n, &tiles);
  hipLaunchKernelGGL(rot_turn_kernel, dim3(tiles, labels ? 4u : 3u, (unsigned)B), dim3(ROT_THREADS), 0, (hipStream_t)stream, a);
  return check_launch(__func__);
}
