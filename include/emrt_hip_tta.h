/* emrt_hip_tta.h -- C-ABI of libemrt_hip_tta.so: flip and rotation test-time augmentation of whole-scene inference, window by window.
 *
 * Why a fifth library: emrt_hip.h is frozen at ABI 9 and the entry lists of emrt_hip_augment.h, emrt_hip_sampler.h and emrt_hip_loss.h are pinned
 * by the test suite.  None of those libraries calls this one; a prediction or evaluation without test-time augmentation never loads it.
 *
 * Conventions, as in emrt_hip_loss.h: plain pointers and sizes; every launch goes to the caller's stream; nothing is allocated and nothing
 * synchronises; every argument is checked on the HOST before anything is launched; 0 on success, non-zero on refusal, and emrt_tta_last_error()
 * then gives this library's own thread-local message.  scene, batch, logits, final and count are device pointers; origins_yx and codes are
 * HOST arrays, read before the call returns.
 *
 * Variants.  A code is t * 4 + fv * 2 + fh.  For a window A [ch][cw] the variant is A with its rows reversed if fv and its columns reversed if
 * fh, then transposed if t:
 *   0 identity   1 horizontal flip   2 vertical flip   3 rotation by 180   4 transpose   5 rot90(A, 1)   6 rot90(A, -1)   7 anti-transpose
 * The inverse, applied to a map the model made from the variant, is: transposed if t, then the same reversals.  A transposing code needs
 * ch == cw.  `codes` holds G different codes (1 <= G <= 8); a launch takes n windows with n * G <= 64, and variant g of window j is image
 * j * G + g of the batch.
 *
 * Nothing here uses a floating-point atomic: every output element is written by one thread in one fixed order, so two runs give the same bits. */
#ifndef EMRT_HIP_TTA_H
#define EMRT_HIP_TTA_H

#ifdef __cplusplus
extern "C" {
#endif

#define EMRT_TTA_MAX_VARIANTS 8
#define EMRT_TTA_MAX_IMAGES 64 /* n * G of one launch */
#define EMRT_TTA_MAX_CLASSES 256

const char* emrt_tta_last_error(void);
int emrt_tta_version(void); /* 1 */

/* scene: uint8 [H][W][3].  batch: fp32 [n * G][3][ch][cw] = the G variants of the n windows at origins_yx ([n][2], y then x), every value
 * (float)(((double)u8 - mean[c]) * stdinv[c]), the bits of emrt_scene_crop_windows_u8.  A block stages a 32 x 32 tile of one window in LDS
 * (normalised once) and writes it into all G variants, so a scene byte is read once per window. */
int emrt_tta_crop_windows_u8(const unsigned char* scene, float* batch, const int* origins_yx, int n, const int* codes, int G, int H, int W, int ch, int cw, double mean0, double mean1, double mean2, double stdinv0, double stdinv1, double stdinv2, void* stream);

/* logits: fp32 [n * G][C][ch][cw], what the model made of the batch above.  For every scene pixel p and class c
 *   final[c][p] += sum over the windows j that cover p, in the order given, and over g in the order given, of softmax_c(inverse_g(logits[j * G + g]))[p]
 *   count[p]    += G * (the number of windows that cover p)
 * with final fp32 [C][H][W] and count fp32 [H][W].  The softmax is emrt_softmax_nchw_acc's: a fmaxf chain, expf terms added in class order, one
 * reciprocal.  One thread owns a pixel; the terms are added to the value final held, one after the other.  1 <= C <= 256. */
int emrt_tta_window_accumulate(const float* logits, float* final, float* count, const int* origins_yx, int n, const int* codes, int G, int C, int H, int W, int ch, int cw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMRT_HIP_TTA_H */
