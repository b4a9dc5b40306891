/* emrt_hip_rot.h -- C-ABI of libemrt_hip_rot.so: the quarter turn of the training augmentation, RandomRot90, as a post-pass over a
 * finished batch.
 *
 * Why a seventh library: emrt_hip.h is frozen at ABI 9 and the entry lists of the five side headers before this one are pinned by the test suite,
 * as is the table of the six libraries itself.  None of those libraries calls this one; a run with DATA.AUGMENT.ROT90_PROB 0 never loads it.
 *
 * Conventions, as in emrt_hip_sampler.h: plain pointers and sizes; every launch goes to the caller's stream; nothing is allocated and nothing
 * synchronises; every argument is checked on the HOST before anything is launched; 0 on success, non-zero on refusal, and emrt_rot_last_error()
 * then gives this library's own thread-local message.  Pointers are device pointers unless marked HOST.
 *
 * The turn.  images fp32 [B][3][n][n] and labels int64 [B][n][n], contiguous, are turned IN PLACE: sample b by turns[b] quarter turns
 * counter-clockwise in array coordinates, numpy's rot90(plane, k, axes=(0, 1)) on each of its four planes: after one turn out[i][j] = in[j][n-1-i].
 * Turn 0 leaves the sample untouched (its blocks exit at once).  The values are moved as bits: a NaN payload arrives as it left.
 * In the variant codes of emrt_hip_tta.h (t * 4 + fv * 2 + fh) the turns 0, 1, 2, 3 are the codes 0, 5, 3, 6.
 *
 * The kernel.  A quarter turn splits the plane into orbits of four pixels (pairs for k = 2; the centre of an odd plane is fixed).  The fundamental
 * domain, rows [0, ceil(n/2)) x columns [0, floor(n/2)), is cut into 32 x 32 tiles, partial at the edges; a block owns one tile of one plane,
 * loads the tile and its three images under the turn -- rectangles whose rows are contiguous in memory -- into LDS by rows, synchronises, and
 * stores each rectangle by rows from the rectangle k steps behind it in the orbit, read from LDS transposed.  No global access is column-strided,
 * no thread reads a pixel that another block writes, and there is no atomic.
 *
 * The draw of emrt_rot_scene_batch for sample b.  Philox4x32-10 with key and counter exactly as emrt_scene_draw: key = the words of `key`,
 * counter = (low, high word of *step_counter, rank * B + b, j).  Blocks j = 0..4 belong to the draw kernels of emrt_hip.h and emrt_hip_augment.h,
 * 8 and 9 to emrt_smp_class_redraw (emrt_hip_sampler.h); this library uses block 5 (6 and 7 stay free):
 *   block 5, word 0:    on = word * 2^-32 < prob (float64)
 *   block 5, words 1-2: k = 1 + the high half of value * 3 (value = word 2 << 32 | word 1): uniform over 1, 2, 3;  turn = on ? k : 0
 * No other block is read or written, so every other decision of the batch is what it is without this launch. */
#ifndef EMRT_HIP_ROT_H
#define EMRT_HIP_ROT_H

#ifdef __cplusplus
extern "C" {
#endif

#define EMRT_ROT_BLOCK 5
#define EMRT_ROT_CHUNK 64 /* samples per launch of emrt_rot_batch */
#define EMRT_ROT_MAX_SIDE 32768
#define EMRT_ROT_MAX_BATCH 65535 /* samples of one emrt_rot_scene_batch launch */

const char* emrt_rot_last_error(void);
int emrt_rot_version(void); /* 1 */

/* The tile path: turns is a HOST array of B values in 0..3, read before the call returns and handed to the kernel by value, one launch per chunk
 * of 64 samples (a chunk whose turns are all 0 launches nothing).  labels may be null: only the images are turned.  A turn outside 0..3, n < 1
 * and B < 1 are refused by name before any launch. */
int emrt_rot_batch(float* images, long long* labels, const int* turns, int B, int n, void* stream);

/* --data scenes: ONE launch for the whole batch, every host argument a constant of the run (it can sit inside a captured step).  Every block
 * derives its sample's turn from the device step counter by the draw above; one block per sample also writes it to turns_out (int32 [B], 0 when
 * not on).  labels may be null.  0 <= prob <= 1, 1 <= B <= 65535. */
int emrt_rot_scene_batch(const long long* step_counter, long long key, int rank, int B, int n, double prob, float* images, long long* labels, int* turns_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMRT_HIP_ROT_H */
