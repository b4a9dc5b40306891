/* emrt_hip_augment.h -- C-ABI of libemrt_hip_augment.so: the training augmentation of emrt_hip.h (emrt_augment_tiles, emrt_scene_draw,
 * emrt_scene_sample) extended by RandomVerticalFlip and RandomDistort (brightness, contrast, saturation; hue is not offered).
 *
 * Why a second library: the ABI of emrt_hip.h is frozen at version 9 (its prototype, struct and member counts are pinned by the test suite), so
 * these entry points live beside it until a change that may raise that version folds them in.  The chains emrt_hip.h serves never call this
 * library; this library is a superset, and with no vertical flip and no distortion its output is bit-identical to the first library's.
 *
 * Conventions, as in emrt_hip.h: plain pointers and sizes; every launch goes to the caller's stream; nothing is allocated and nothing
 * synchronises; every argument is checked on the HOST before anything is launched; 0 on success, non-zero on refusal, and
 * emrt_aug_last_error() then gives this library's own thread-local message.  Pointers are device pointers unless marked HOST.
 *
 * The per-pixel arithmetic (float32, two roundings per blend, no fused multiply-add; PIL's ImageEnhance restated):
 *   x   = the geometry map's float32 channel (resize, pad, crop, flips) truncated to uint8         -- only when `distort` is non-zero
 *   L   = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16
 *   op: t = d + f * (x - d);  x = (uint8)t when 0 <= f <= 1, else 0 if t <= 0, 255 if t >= 255, else (uint8)t
 *       brightness d = 0;  contrast d = (int)(sum of L over the OH x OW tile as the op sees it, padding included / (OH * OW) + 0.5);
 *       saturation d = the pixel's own L
 *   out = (float)(((double)x - mean) * stdinv)
 * The contrast sum is an integer sum (64-bit vector atomics into the workspace): the result is the same from run to run. */
#ifndef EMRT_HIP_AUGMENT_H
#define EMRT_HIP_AUGMENT_H
#include <stddef.h>
#include "emrt_hip.h" /* EmrtSceneEntry */

#ifdef __cplusplus
extern "C" {
#endif

#define EMRT_AUG_OP_BRIGHTNESS 0
#define EMRT_AUG_OP_CONTRAST 1
#define EMRT_AUG_OP_SATURATION 2
#define EMRT_AUG_FLIP_H 1
#define EMRT_AUG_FLIP_V 2
#define EMRT_AUG_DRAW_COLS 18

const char* emrt_aug_last_error(void);
int emrt_aug_version(void); /* 1 */

/* Bytes of the caller's workspace for a batch of B samples: one 64-bit luminance sum per sample.  0 for B <= 0 (an error). */
size_t emrt_aug_workspace_bytes(int B);

/* One sample of emrt_aug_tiles: EmrtAugDesc of emrt_hip.h, then the flips as a bit mask and the colour ops in application order. */
typedef struct EmrtAugOpsDesc {
  long long img_off, lab_off;            /* byte offsets into src */
  int H, W;                              /* source size */
  int h, w;                              /* resized size */
  int off_y, off_x;                      /* crop offsets into the resized image padded bottom / right to the crop size */
  int flip;                              /* EMRT_AUG_FLIP_H | EMRT_AUG_FLIP_V, after the crop */
  int n_ops;                             /* 0..3 colour ops; must be 0 when `distort` is 0 */
  int op[3];                             /* EMRT_AUG_OP_*, each at most once */
  float factor[3];                       /* finite, >= 0 */
} EmrtAugOpsDesc;

/* emrt_augment_tiles with both flips and the colour ops.  descs: HOST.  distort != 0: the chain holds RandomDistort, every pixel is truncated
 * to uint8 before the ops (with n_ops == 0 too, as the CPU class does) and img_pad must lie in [0, 256).  workspace: emrt_aug_workspace_bytes(B)
 * bytes, used (zeroed on the stream, then summed into) only when some sample applies contrast.  Per chunk of 16 samples: a statistics launch
 * (only if a sample of the chunk applies contrast) and the apply launch.  The label follows both flips and nothing else. */
int emrt_aug_tiles(const void* src, size_t src_bytes, const EmrtAugOpsDesc* descs, int B, int OH, int OW, int distort, const double* mean, const double* stdinv, const float* img_pad, int label_pad, const unsigned char* label_lut, float* out, long long out_bs, long long* labels, void* workspace, size_t workspace_bytes, void* stream);

/* emrt_scene_draw with the new decisions.  Keys and counters as there (Philox4x32-10, key = the words of `key`, counter = (low, high word of
 * *step_counter, rank * B + b, j)); blocks j = 0, 1, 2 are used identically, so columns 0-8 equal emrt_scene_draw's for the same arguments.
 *   block 2, word 1:    vflip = word * 2^-32 < vflip_prob
 *   block 3, words 0-1: an integer below 24 = the lexicographic rank of the permutation of (brightness, contrast, saturation, hue); hue keeps its
 *                       place in the permutation and is never applied
 *   per op k (0 brightness, 1 contrast, 2 saturation) two words, (block 3 word 2, 3), (block 4 word 0, 1), (block 4 word 2, 3):
 *                       applied = distort && first word * 2^-32 < probs[k];  factor = (float)(lower + (upper - lower) * second word * 2^-32) in
 *                       float64 with lower = 1 - ranges[k], upper = 1 + ranges[k]
 * A row of draws, int32 [B][EMRT_AUG_DRAW_COLS]:
 *   0 scene, 1 y0, 2 x0, 3 scale_index, 4 h, 5 w, 6 off_y, 7 off_x, 8 hflip, 9 vflip, 10 permutation rank, 11 n_ops,
 *   12-14 the applied ops' codes in application order (unused: 0), 15-17 their factors' float32 bits (unused: 1.0f)
 * ranges, probs: HOST double[3]; 0 <= range <= 1 (factors stay >= 0), 0 <= prob <= 1; both must be given even when distort is 0. */
int emrt_aug_scene_draw(const long long* step_counter, const EmrtSceneEntry* scenes, const long long* cum_origins, const EmrtSceneEntry* scenes_host, const long long* cum_origins_host, int n_scenes, size_t bank_bytes, long long key, int rank, int B, int th, int tw, int OH, int OW, double flip_prob, double vflip_prob, int distort, const double* ranges, const double* probs, const int* scale_hw, int n_scales, int* draws, void* stream);

/* emrt_scene_sample on a table of emrt_aug_scene_draw: with distort != 0 the workspace is zeroed on the stream, a statistics launch sums the
 * luminance of every sample that applies contrast, and the apply launch follows; with distort == 0 only the apply launch runs and columns 11-17
 * are ignored.  Every value read from the table is clamped into its range (flips to 0 / 1, n_ops to 0..3, op codes to 0..2, factors to [0, 2],
 * NaN to 0): a stale or foreign table reads wrong pixels, never memory outside the bank.  With equal decisions the output is bit-identical to
 * emrt_aug_tiles on a contiguous copy of the window, and with vflip_prob = 0 and distort = 0 to emrt_scene_sample. */
int emrt_aug_scene_sample(const unsigned char* bank, size_t bank_bytes, const EmrtSceneEntry* scenes, const EmrtSceneEntry* scenes_host, int n_scenes, const int* draws, int B, int th, int tw, int OH, int OW, int distort, const double* mean, const double* stdinv, const float* img_pad, int label_pad, const unsigned char* label_lut, float* out, long long out_bs, long long* labels, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMRT_HIP_AUGMENT_H */
