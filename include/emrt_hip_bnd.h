/* emrt_hip_bnd.h -- C-ABI of libemrt_hip_bnd.so: boundary-aware scene evaluation: the ISPRS metrics on ground truth whose class
 * boundaries are eroded, and Boundary IoU (Cheng et al., CVPR 2021), counted on the device from the maps a SceneEvaluator already holds there.
 *
 * Why an eighth library: emrt_hip.h is frozen at ABI 9 and the entry lists of the side headers before this one are pinned by the test suite, as
 * are the two tables of libraries before it.  None of those libraries calls this one; an evaluation without `boundary` never loads it.
 *
 * Conventions, as in emrt_hip_rot.h: plain pointers and sizes; every launch goes to the caller's stream; nothing is allocated and nothing
 * synchronises; every argument is checked on the HOST before anything is launched; 0 on success, non-zero on refusal, and emrt_bnd_last_error()
 * then gives this library's own thread-local message.  Every pointer is a device pointer.  No floating point anywhere.
 *
 * The band.  For a map M [H][W], a radius r in 1..EMRT_BND_MAX_RADIUS and a shape, w(dy) is the half-width of the structuring element at row
 * offset dy in -r..r:
 *   shape 1, square: w(dy) = r                                      (Chebyshev distance: r iterations of a 3 x 3 erosion)
 *   shape 0, disk:   w(dy) = the largest integer w with w*w + dy*dy <= r*r    (found on the host in integers, handed to the kernel by value)
 * band[y][x] = 1 iff some IN-IMAGE neighbour (y + dy, x + dx) with |dx| <= w(dy) holds a value other than M[y][x], else 0.  Neighbours outside the
 * image are skipped: the border of the scene is no class boundary.  Values are compared as they are stored; an ignore byte of a label map is a
 * value like any other here.  1 - band is the union over the values c of binary_erosion(M == c, element, border_value=1).
 *
 * Two passes, O(r) per pixel for both shapes:
 *   runs[y][x] = min(r, the largest k such that every in-image pixel of [x - k, x + k] in row y equals M[y][x])                  emrt_bnd_runs
 *   band[y][x] = 1 iff some in-image dy in -r..r has M[y + dy][x] != M[y][x] or runs[y + dy][x] < w(dy)                            emrt_bnd_band
 * Both stage their tile with its halo of r columns / r rows in LDS, so that every global access runs along rows.
 *
 * map_kind selects the element type of M with the values of emrt_segmentation_areas (emrt_hip.h): 0 = int32 (the evaluator's prediction),
 * 2 = uint8 (a label map of a scene bank: read byte by byte, so no alignment is asked of the pointer); any other value is refused.
 *
 * Refused by name before any launch: a null pointer; H or W outside 1..EMRT_BND_MAX_SIDE; a radius outside 1..32; a shape other than 0 and 1;
 * a map kind other than 0 and 2; num_classes outside 1..256; a negative n. */
#ifndef EMRT_HIP_BND_H
#define EMRT_HIP_BND_H

#ifdef __cplusplus
extern "C" {
#endif

#define EMRT_BND_MAX_RADIUS 32
#define EMRT_BND_MAX_SIDE 65536
#define EMRT_BND_DISK 0
#define EMRT_BND_SQUARE 1

const char* emrt_bnd_last_error(void);
int emrt_bnd_version(void); /* 1 */

/* The row pass: runs uint8 [H][W] from the map (above).  It depends on the radius only through the cap, not on the shape. */
int emrt_bnd_runs(const void* map, int map_kind, int H, int W, int radius, unsigned char* runs, void* stream);

/* The column pass: band uint8 [H][W], 0 or 1, from the map and the runs that emrt_bnd_runs wrote for the SAME map and radius. */
int emrt_bnd_band(const void* map, int map_kind, const unsigned char* runs, int H, int W, int radius, int shape, unsigned char* band, void* stream);

/* The counts: out int64 [2][3][num_classes], ACCUMULATED into (the caller zeroes it once per evaluation), over the n pixels whose label !=
 * ignore_index; pred int32, label uint8 at any byte offset, band_pred / band_label uint8 as emrt_bnd_band wrote them for pred and for label.
 * Predictions and labels outside [0, num_classes) are counted nowhere, as in emrt_segmentation_areas.
 *   out[0], eroded (the ISPRS "no boundary" protocol): intersect / prediction / label areas over the pixels with band_label == 0
 *   out[1], boundary:  [0][c] = #(label == c and pred == c and band_label and band_pred)
 *                      [1][c] = #(pred == c and band_pred)        [2][c] = #(label == c and band_label)
 *                      intersect / (prediction + label - intersect) of these is Boundary IoU of class c
 * Per-block integer counters in LDS, integer atomics to out: the result does not depend on the order. */
int emrt_bnd_areas(const int* pred, const unsigned char* label, const unsigned char* band_pred, const unsigned char* band_label, long long n, int num_classes, int ignore_index, long long* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMRT_HIP_BND_H */
