/* emrt_hip_sampler.h -- C-ABI of libemrt_hip_sampler.so: class-aware tile origins for the resident-scene sampler.
 *
 * emrt_scene_draw / emrt_aug_scene_draw cut every tile at a uniformly drawn origin, which reproduces the pixel imbalance of the scenes.  This
 * library adds "rare class sampling": a label index built once (emrt_smp_row_counts), and a launch between the draw and the sample launch
 * (emrt_smp_class_redraw) that moves a share of the windows so that each holds a pixel of a class drawn from a chosen distribution.
 *
 * Why a third library: emrt_hip.h is frozen at ABI 9 and emrt_hip_augment.h has its exact entry list pinned by the test suite.  Neither of
 * those libraries calls this one; a run with DATA.SCENE_SAMPLING.MODE "uniform" never loads it.
 *
 * Conventions, as in emrt_hip.h: plain pointers and sizes; every launch goes to the caller's stream; nothing is allocated and nothing
 * synchronises; every argument is checked on the HOST before anything is launched (the host mirror of the scene table against bank_bytes among
 * them); 0 on success, non-zero on refusal, and emrt_smp_last_error() then gives this library's own thread-local message.  Pointers are device
 * pointers unless marked HOST.
 *
 * The index.  Rows of all label maps are numbered in bank order: global row Ri = row_start[s] + y, row_start[0] = 0, row_start[n_scenes] = R.
 *   counts   int32 [R][n_classes]: pixels of class c in row Ri after label_lut; bytes that map to a value >= n_classes are not counted
 *   cum      int64 [n_classes][R + 1], class-major exclusive prefix over rows: cum[c][i] = sum of counts[0..i-1][c]; cum[c][R] = n_c
 *   thr      uint64 [n_classes]: thr[c] = floor(2^32 * sum of P(c') for c' <= c), and exactly 2^32 from the last class with pixels on
 * cum and thr are formed by the caller from counts; P is the caller's choice (emrt_amd: exp((1 - f_c) / T), or explicit weights).
 *
 * The redraw of sample b.  Philox4x32-10 with key and counter exactly as emrt_scene_draw: key = the words of `key`, counter = (low, high word
 * of *step_counter, rank * B + b, j).  Blocks j = 0..4 belong to the draw kernels, 5 to emrt_rot_scene_batch (emrt_hip_rot.h), 6 and 7 stay free, this library uses 8 and 9:
 *   block 8, word 0:    class mode iff word * 2^-32 < prob (float64); otherwise the row is left as it is
 *   block 8, word 1:    cls = the number of c with word >= thr[c], at most the last class with pixels
 *   block 8, words 2-3: k = the high half of value * n_cls (n_cls = cum[cls][R]): the k-th pixel of that class in bank order
 *   block 9, word 0:    dy = the high half of word * th;   word 1: dx = the high half of word * tw   (32 x 32 -> 64 bits)
 *   Ri = (the first i with cum[cls][i] > k) - 1,  j = k - cum[cls][Ri];  scene s = the last one with row_start[s] <= Ri,  y = Ri - row_start[s]
 *   x  = the column of the j-th byte of row y that label_lut maps to cls, counted from the left
 *   y0 = clamp(y - dy, 0, H - th),  x0 = clamp(x - dx, 0, W - tw);  columns 0, 1, 2 of the row become s, y0, x0
 * Columns 3 and up are never written: scale, offsets, flips and distortion keep the draw kernel's decisions.
 *
 * What is promised is a property of the SOURCE window: it contains the anchor pixel (y, x), at a uniformly drawn position inside the window
 * unless the window was clamped at a scene border.  The chain's later steps are unchanged, so a scale step above 1 followed by the crop may
 * still cut the anchor away; that is accepted.
 *
 * Every value read from a device table is brought into its range before it is used as an index, and a pixel that the scan does not find (a stale
 * or foreign index) leaves the row as the uniform draw wrote it: a wrong index moves windows to wrong places inside their scenes, never outside. */
#ifndef EMRT_HIP_SAMPLER_H
#define EMRT_HIP_SAMPLER_H
#include <stddef.h>
#include "emrt_hip.h" /* EmrtSceneEntry */

#ifdef __cplusplus
extern "C" {
#endif

#define EMRT_SMP_MAX_CLASSES 256
#define EMRT_SMP_BLOCK_CLASS 8
#define EMRT_SMP_BLOCK_OFFSET 9

const char* emrt_smp_last_error(void);
int emrt_smp_version(void); /* 1 */

/* counts[Ri][c] for every row of every label map of the bank: one wave per row, aligned 32-bit loads (bytes at the row's unaligned ends one by
 * one), one ballot and population count per class and byte lane.  Integers only and no atomics: the table is exact and the same from run to run.
 * scenes_host, row_start_host: HOST mirrors of scenes and row_start ([n_scenes + 1]); row_start must be the running sum of the scenes' heights
 * and total_rows its last entry.  label_lut: HOST, 256 bytes, or null for the identity.  counts: int32 [total_rows][n_classes], every entry written. */
int emrt_smp_row_counts(const unsigned char* bank, size_t bank_bytes, const EmrtSceneEntry* scenes, const EmrtSceneEntry* scenes_host, const long long* row_start, const long long* row_start_host, int n_scenes, const unsigned char* label_lut, int n_classes, int* counts, long long total_rows, void* stream);

/* The redraw described above on a table of emrt_scene_draw (draw_cols 10) or emrt_aug_scene_draw (draw_cols 18), after that launch and before the
 * sample launch, on the same stream: one wave per sample, the row scanned 256 bytes per pass by ballot and population count.  thresholds_host:
 * HOST mirror of thresholds; non-decreasing, at most 2^32, the last entry exactly 2^32.  class_cum is read on the device only (it is as large as
 * the index); its values are range-checked there.  th, tw: the source tile, as given to the draw launch.  0 <= prob <= 1. */
int emrt_smp_class_redraw(const long long* step_counter, const unsigned char* bank, size_t bank_bytes, const EmrtSceneEntry* scenes, const EmrtSceneEntry* scenes_host, const long long* row_start, const long long* row_start_host, int n_scenes, const long long* class_cum, const unsigned long long* thresholds, const unsigned long long* thresholds_host, int n_classes, const unsigned char* label_lut, long long key, int rank, int B, int th, int tw, double prob, int* draws, int draw_cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMRT_HIP_SAMPLER_H */
