// libemrt_hip_bnd.so: the boundary band of a class map and the eroded / boundary metric counts of a whole-scene evaluation.  The definitions, the
// two-pass decomposition and the layout of the counts are described in include/emrt_hip_bnd.h.  A library of its own because the tables of the
// seven libraries before it are pinned.  Integers only: no floating point in any kernel or on the host side.
//
// Three kernels, one per entry point, 256 threads each.
//   runs:  a tile of 8 rows x 256 columns with r more columns on either side, staged in LDS as int32 whatever the map's type ((256 + 64) * 8 * 4 =
//          10 KiB static).  Lane l loads column x0 - r + l of a row, so a wave reads 256 (int32) or 64 (uint8) contiguous bytes; thread t then owns
//          column t and walks outwards at most r steps per row.  In LDS lane l reads word c + l for a constant c: every bank once per 32-lane half.
//   band:  a tile of 32 rows x 128 columns with r more rows above and below: the map as int32 and the runs as bytes, (32 + 2r) * 128 * 5 bytes of
//          DYNAMIC LDS -- 23.75 KiB at r = 3 (6 blocks = 24 waves per CU in the 160 KiB), 60 KiB at r = 32, inside the 64 KiB a launch may ask
//          for.  The int32 part comes first and is a multiple of 512 bytes, so both parts keep the 16-byte alignment of the base.  A
//          thread owns one column of every second row and looks at most 2r + 1 rows up and down it: lane l at word c + l again, and the run
//          bytes of four neighbouring lanes share a word (one address per word: no conflict).  w(dy) comes by value in the kernel arguments and
//          is indexed by the loop counter, the same for every lane.
//   areas: seg_areas_kernel's scheme (csrc/optim.hip) with six rows: per-block 32-bit counters in LDS, one 64-bit global atomic per non-zero
//          counter and block.  A block counts at most n / gridDim.x + 256 pixels, below 2^32 for every n the grid's cap of 1024 blocks leaves.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "../../../include/emrt_hip_bnd.h"

namespace emrt {
namespace {

thread_local char g_bnd_err[512] = "";

int fail(const char* fn, const char* msg) {
  snprintf(g_bnd_err, sizeof(g_bnd_err), "%s: %s", fn, msg);
  return -1;
}
int check_launch(const char* fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_bnd_err, sizeof(g_bnd_err), "%s: launch failed: %s", fn, hipGetErrorString(e));
    return -2;
  }
  return 0;
}
#define BND_REQUIRE(cond, msg)                 \
  do {                                         \
    if (!(cond)) return fail(__func__, msg);   \
  } while (0)

constexpr int BND_THREADS = 256;
constexpr int BND_R = EMRT_BND_MAX_RADIUS;
constexpr int BND_RUN_W = 256, BND_RUN_H = 8;          // the row pass's tile: one column per thread
constexpr int BND_RUN_PITCH = BND_RUN_W + 2 * BND_R;
constexpr int BND_COL_W = 128, BND_COL_H = 32;         // the column pass's tile: one column per thread, every second row

template <class T>
__global__ __launch_bounds__(BND_THREADS) void bnd_runs_kernel(const T* __restrict__ map, unsigned char* __restrict__ runs, int H, int W, int r) {
  __shared__ int tile[BND_RUN_H * BND_RUN_PITCH];
  const int x0 = (int)blockIdx.x * BND_RUN_W, y0 = (int)blockIdx.y * BND_RUN_H, tx = threadIdx.x;
  const int rows = min(BND_RUN_H, H - y0), span = BND_RUN_W + 2 * r;
  for (int ly = 0; ly < rows; ++ly) {
    const T* src = map + (long long)(y0 + ly) * W;
    for (int i = tx; i < span; i += BND_THREADS) {
      const int gx = x0 - r + i;
      if (gx >= 0 && gx < W) tile[ly * BND_RUN_PITCH + i] = (int)src[gx];
    }
  }
  __syncthreads();
  const int gx = x0 + tx;
  if (gx >= W) return;
  for (int ly = 0; ly < rows; ++ly) {
    const int* row = tile + ly * BND_RUN_PITCH + r + tx;      // row[d] is column gx + d: staged for -r <= d <= r wherever it is inside the image
    const int c = row[0];
    int k = 0;
    while (k < r) {
      const int d = k + 1;
      if (gx - d >= 0 && row[-d] != c) break;
      if (gx + d < W && row[d] != c) break;
      k = d;
    }
    runs[(long long)(y0 + ly) * W + gx] = (unsigned char)k;
  }
}

struct BandArgs {
  const void* map;
  const unsigned char* runs;
  unsigned char* band;
  int H, W, r;
  unsigned char w[2 * BND_R + 1];      // w(dy) at index dy + r
};

template <class T>
__global__ __launch_bounds__(BND_THREADS) void bnd_band_kernel(BandArgs a) {
  extern __shared__ __align__(16) int bnd_lds[];
  const int r = a.r, H = a.H, W = a.W, staged = BND_COL_H + 2 * r;
  int* m = bnd_lds;                                                                        // [staged][BND_COL_W]
  unsigned char* rn = reinterpret_cast<unsigned char*>(bnd_lds + staged * BND_COL_W);      // [staged][BND_COL_W]
  const T* map = static_cast<const T*>(a.map);
  const int x0 = (int)blockIdx.x * BND_COL_W, y0 = (int)blockIdx.y * BND_COL_H;
  const int tx = threadIdx.x & (BND_COL_W - 1), ty = threadIdx.x / BND_COL_W, gx = x0 + tx;
  if (gx < W) {
    for (int lr = ty; lr < staged; lr += BND_THREADS / BND_COL_W) {
      const int gy = y0 - r + lr;
      if (gy >= 0 && gy < H) {
        const long long g = (long long)gy * W + gx;
        m[lr * BND_COL_W + tx] = (int)map[g];
        rn[lr * BND_COL_W + tx] = a.runs[g];
      }
    }
  }
  __syncthreads();
  if (gx >= W) return;
  for (int ly = ty; ly < BND_COL_H; ly += BND_THREADS / BND_COL_W) {
    const int gy = y0 + ly;
    if (gy >= H) break;
    const int c = m[(ly + r) * BND_COL_W + tx];
    int hit = 0;
    for (int dy = -r; dy <= r; ++dy) {
      if (gy + dy < 0 || gy + dy >= H) continue;
      const int idx = (ly + r + dy) * BND_COL_W + tx;      // row gy + dy: staged, as 0 <= ly + r + dy < staged
      if (m[idx] != c || (int)rn[idx] < (int)a.w[dy + r]) {
        hit = 1;
        break;
      }
    }
    a.band[(long long)gy * W + gx] = (unsigned char)hit;
  }
}

__global__ __launch_bounds__(BND_THREADS) void bnd_areas_kernel(const int* __restrict__ pred, const unsigned char* __restrict__ label,
                                                                const unsigned char* __restrict__ band_pred, const unsigned char* __restrict__ band_label,
                                                                long long n, int ncls, int ignore, unsigned long long* __restrict__ out) {
  __shared__ unsigned cnt[6 * 256];
  for (int i = threadIdx.x; i < 6 * ncls; i += blockDim.x) cnt[i] = 0;
  __syncthreads();
  unsigned* er = cnt;                  // eroded: intersect, prediction, label
  unsigned* bd = cnt + 3 * ncls;       // boundary: the same three
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int l = (int)label[i];
    if (l == ignore) continue;
    const int p = pred[i];
    const bool pv = p >= 0 && p < ncls, lv = l < ncls, bl = band_label[i] != 0, bp = band_pred[i] != 0;
    if (!bl) {
      if (pv) atomicAdd(&er[ncls + p], 1u);
      if (lv) atomicAdd(&er[2 * ncls + l], 1u);
      if (pv && p == l) atomicAdd(&er[p], 1u);
    } else {
      if (lv) atomicAdd(&bd[2 * ncls + l], 1u);
      if (bp && pv && p == l) atomicAdd(&bd[p], 1u);
    }
    if (bp && pv) atomicAdd(&bd[ncls + p], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 6 * ncls; i += blockDim.x)
    if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

// the largest w with w * w + dy * dy <= r * r, in integers
int disk_half_width(int r, int dy) {
  int w = 0;
  while ((w + 1) * (w + 1) + dy * dy <= r * r) ++w;
  return w;
}

int check_map(const char* fn, int map_kind, int H, int W, int radius) {
  if (map_kind != 0 && map_kind != 2) return fail(fn, "map_kind selects the map's type: 0 = int32, 2 = uint8");
  if (H < 1 || H > EMRT_BND_MAX_SIDE) return fail(fn, "H must be 1..65536");
  if (W < 1 || W > EMRT_BND_MAX_SIDE) return fail(fn, "W must be 1..65536");
  if (radius < 1 || radius > EMRT_BND_MAX_RADIUS) return fail(fn, "radius must be 1..32");
  return 0;
}

}  // namespace
}  // namespace emrt

using namespace emrt;

extern "C" const char* emrt_bnd_last_error(void) { return g_bnd_err; }

extern "C" int emrt_bnd_version(void) { return 1; }

extern "C" int emrt_bnd_runs(const void* map, int map_kind, int H, int W, int radius, unsigned char* runs, void* stream) {
  BND_REQUIRE(map && runs, "null pointer");
  if (int r = check_map(__func__, map_kind, H, W, radius)) return r;
  const dim3 grid((unsigned)((W + BND_RUN_W - 1) / BND_RUN_W), (unsigned)((H + BND_RUN_H - 1) / BND_RUN_H));
  if (map_kind == 2)
    hipLaunchKernelGGL((bnd_runs_kernel<unsigned char>), grid, dim3(BND_THREADS), 0, (hipStream_t)stream, (const unsigned char*)map, runs, H, W, radius);
  else
    hipLaunchKernelGGL((bnd_runs_kernel<int>), grid, dim3(BND_THREADS), 0, (hipStream_t)stream, (const int*)map, runs, H, W, radius);
  return check_launch(__func__);
}

extern "C" int emrt_bnd_band(const void* map, int map_kind, const unsigned char* runs, int H, int W, int radius, int shape, unsigned char* band,
                             void* stream) {
  BND_REQUIRE(map && runs && band, "null pointer");
  if (int r = check_map(__func__, map_kind, H, W, radius)) return r;
  BND_REQUIRE(shape == EMRT_BND_DISK || shape == EMRT_BND_SQUARE, "shape must be 0 (disk) or 1 (square)");
  BandArgs a{};
  a.map = map;
  a.runs = runs;
  a.band = band;
  a.H = H;
  a.W = W;
  a.r = radius;
  for (int dy = -radius; dy <= radius; ++dy) a.w[dy + radius] = (unsigned char)(shape == EMRT_BND_SQUARE ? radius : disk_half_width(radius, dy < 0 ? -dy : dy));
  const dim3 grid((unsigned)((W + BND_COL_W - 1) / BND_COL_W), (unsigned)((H + BND_COL_H - 1) / BND_COL_H));
  const unsigned lds = (unsigned)((BND_COL_H + 2 * radius) * BND_COL_W * 5);
  if (map_kind == 2)
    hipLaunchKernelGGL((bnd_band_kernel<unsigned char>), grid, dim3(BND_THREADS), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((bnd_band_kernel<int>), grid, dim3(BND_THREADS), lds, (hipStream_t)stream, a);
  return check_launch(__func__);
}

extern "C" int emrt_bnd_areas(const int* pred, const unsigned char* label, const unsigned char* band_pred, const unsigned char* band_label, long long n,
                              int num_classes, int ignore_index, long long* out, void* stream) {
  BND_REQUIRE(pred && label && band_pred && band_label && out, "null pointer");
  BND_REQUIRE(num_classes >= 1 && num_classes <= 256, "num_classes must be 1..256");
  BND_REQUIRE(n >= 0, "n must not be negative");
  if (n == 0) return 0;
  long long grid = (n + BND_THREADS * 16 - 1) / (BND_THREADS * 16);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(bnd_areas_kernel, dim3((unsigned)grid), dim3(BND_THREADS), 0, (hipStream_t)stream, pred, label, band_pred, band_label, n, num_classes,
                     ignore_index, (unsigned long long*)out);
  return check_launch(__func__);
}
