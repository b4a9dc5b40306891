/* emrt_hip_mstta.h -- C-ABI of libemrt_hip_mstta.so: multi-scale test-time augmentation of whole-scene inference, window by window.
 * Scale is one more axis of the window-level augmentation of emrt_hip_tta.h: a window of ch x cw model pixels is resampled from a FOOTPRINT of
 * fh x fw native pixels of the uint8 scene where it is cropped, and its logits are resampled back to the footprint where they are accumulated.
 *
 * Why a sixth library: emrt_hip.h is frozen at ABI 9 and the entry lists of emrt_hip_augment.h, emrt_hip_sampler.h, emrt_hip_loss.h and
 * emrt_hip_tta.h are pinned by the test suite.  None of those libraries calls this one; a prediction or evaluation without tta_scales never loads it.
 *
 * Conventions, as in emrt_hip_tta.h: plain pointers and sizes; every launch goes to the caller's stream; nothing is allocated and nothing
 * synchronises; every argument is checked on the HOST before anything is launched; 0 on success, non-zero on refusal, and emrt_mst_last_error()
 * then gives this library's own thread-local message.  scene, batch, logits, final and count are device pointers; origins_yx and codes are
 * HOST arrays, read before the call returns.
 *
 * Resampling, the same rule in both directions: bilinear with align_corners = false over the footprint alone (F.interpolate of the cropped
 * footprint), in integers.  For output index i of n_out reading a source of n_src: num = (2 i + 1) n_src - n_out, den = 2 n_out;
 *   num <= 0: i0 = 0, w = 0;   else i0 = num / den;   i0 >= n_src - 1: i0 = n_src - 1, w = 0;   else w = (float)(num - i0 den) / (float)den;
 *   i1 = min(i0 + 1, n_src - 1)
 * and in fp32 top = a + wx (b - a), bot likewise, v = top + wy (bot - top).  With n_src == n_out every weight is 0 and v is the sample itself.
 * Every size is 1..2048 and neither of a footprint and its window is more than 4 times the other, per axis.
 *
 * Variants: the codes of emrt_hip_tta.h, t * 4 + fv * 2 + fh, of the ch x cw window (rows reversed if fv, columns reversed if fh, then
 * transposed if t; a transposing code needs ch == cw).  `codes` holds G different codes (1 <= G <= 8); a launch takes n footprints with
 * n * G <= 64, and variant g of footprint j is image j * G + g of the batch.
 *
 * Nothing here uses a floating-point atomic: every output element is written by one thread in one fixed order, so two runs give the same bits. */
#ifndef EMRT_HIP_MSTTA_H
#define EMRT_HIP_MSTTA_H

#ifdef __cplusplus
extern "C" {
#endif

#define EMRT_MST_MAX_VARIANTS 8
#define EMRT_MST_MAX_IMAGES 64 /* n * G of one launch */
#define EMRT_MST_MAX_CLASSES 256
#define EMRT_MST_MAX_EDGE 2048 /* fh, fw, ch, cw */
#define EMRT_MST_MAX_RATIO 4   /* f <= 4 c and c <= 4 f */

const char* emrt_mst_last_error(void);
int emrt_mst_version(void); /* 1 */

/* scene: uint8 [H][W][3].  batch: fp32 [n * G][3][ch][cw] = the G variants of the n windows whose fh x fw footprints lie at origins_yx ([n][2],
 * y then x).  Window pixel (y, x) blends the bytes of each channel at the rule's taps (n_out = ch, n_src = fh; cw, fw for columns) in fp32 and
 * normalises the blend as (float)(((double)v - mean[c]) * stdinv[c]).  With fh == ch and fw == cw these are the bits of emrt_tta_crop_windows_u8.
 * A block stages a 32 x 32 tile of one window in LDS (blended and normalised once) and writes it into all G variants. */
int emrt_mst_crop_windows_u8(const unsigned char* scene, float* batch, const int* origins_yx, int n, const int* codes, int G, int H, int W, int fh, int fw, int ch, int cw, double mean0, double mean1, double mean2, double stdinv0, double stdinv1, double stdinv2, void* stream);

/* logits: fp32 [n * G][C][ch][cw], what the model made of the batch above.  For every native pixel p inside footprint j (in the order given)
 * and every g (in the order given) the C logits of p are blended from the four taps of inverse_g(logits[j * G + g]) (n_out = fh, n_src = ch;
 * fw, cw for columns; the inverse maps the tap coordinates, nothing is copied), and
 *   final[c][p] += softmax_c(the blended logits)        count[p] += G per covering footprint
 * with final fp32 [C][H][W] and count fp32 [H][W].  The softmax is emrt_tta_window_accumulate's: a fmaxf chain, expf terms added in class order,
 * one reciprocal.  One thread owns a pixel; the terms are added to the value final held, one after the other.  1 <= C <= 256. */
int emrt_mst_window_accumulate(const float* logits, float* final, float* count, const int* origins_yx, int n, const int* codes, int G, int C, int H, int W, int fh, int fw, int ch, int cw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMRT_HIP_MSTTA_H */
