/* emrt_hip_loss.h -- C-ABI of libemrt_hip_loss.so: cross entropy + Dice in one pass over the logits.
 *
 * Why a fourth library: emrt_hip.h is frozen at ABI 9 and the entry lists of emrt_hip_augment.h and emrt_hip_sampler.h are pinned by the test
 * suite.  None of those libraries calls this one; a run whose TRAIN.LOSS is not DiceCrossEntropyLoss never loads it.
 *
 * Conventions, as in emrt_hip_sampler.h: plain pointers and sizes; every launch goes to the caller's stream; nothing is allocated and nothing
 * synchronises; every argument is checked on the HOST before anything is launched; 0 on success, non-zero on refusal, and emrt_lx_last_error()
 * then gives this library's own thread-local message.  All pointers are device pointers.
 *
 * The loss of one head.  z = fp32 NCHW logits, y = int64 labels [N, H, W], v_i = [y_i != ignore_index], p_ic = softmax(z_i)_c, s = smooth:
 *   I_c = sum_i v_i p_ic [y_i = c]     P_c = sum_i v_i p_ic     T_c = sum_i v_i [y_i = c]          (sums over the whole batch, N * H * W)
 *   U_c = P_c + T_c + s                dice_c = (2 I_c + s) / U_c    (U_c = 0, possible only with s = 0: dice_c = 1 and no gradient)
 *   Dice = 1 - (1 / C) sum_c dice_c    (the mean over ALL C classes: a class absent from the batch contributes s / (P_c + s))
 *   CE   = sum_i v_i w[y_i] ce_i / sum_i v_i w[y_i]     (class_weight == NULL: w = 1, the mean over the non-ignored pixels; all ignored: 0)
 *   L    = ce_weight * CE + dice_weight * Dice
 * CE is emrt_wce_* of emrt_hip.h, accumulated with the same grid rule, block reduction and finalize arithmetic: with dice_weight = 0 and
 * ce_weight = 1, CE and L have the bits of that entry point's loss.  A label outside [0, C) that is not ignore_index is outside the contract.
 *
 * Gradient, with a_c = -2 dice_weight / (C U_c) and b_c = dice_weight (2 I_c + s) / (C U_c^2) (both 0 where U_c = 0), g_ic = a_c [y_i = c] + b_c:
 *   dz_ik = weight * upstream * v_i * ( ce_weight * w[y_i] / sum w * (p_ik - [y_i = k])  +  p_ik * (g_ik - sum_c p_ic g_ic) )
 * Ignored pixels get exact zeros.
 *
 * result: float[8] per head = {L, CE, Dice, sum w[y] (class_weight == NULL: the non-ignored count), the non-ignored count, 0, 0, 0}
 * coef:   float[2 C] per head = {a_0 .. a_(C-1), b_0 .. b_(C-1)}: written by the forward, read by the backward
 *
 * Forward: one streaming launch (256 threads, at most 1024 blocks per head, the head is the grid's second dimension) that keeps the sums of
 * eight classes in registers -- C <= 8 is one pass over the logits, a larger C one pass per eight classes -- and reduces them per block into
 * the workspace; then a one-block launch that adds the blocks' partial sums in float64 and writes result, coef and (pair) total.  Backward: one
 * launch, one read of the logits, one write of the gradient.  No floating-point atomics: every value is the same bits in every run, and the
 * pair entry points give each head the bits of the single ones. */
#ifndef EMRT_HIP_LOSS_H
#define EMRT_HIP_LOSS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMRT_LX_MAX_CLASSES 64

const char* emrt_lx_last_error(void);
int emrt_lx_version(void); /* 1 */

/* bytes of the forward's workspace for C classes and `heads` (1 or 2) heads; 0 for arguments the entry points refuse */
size_t emrt_lx_dice_ce_workspace_bytes(int C, int heads);

/* One head.  class_weight: float[C] or NULL.  ce_weight, dice_weight, smooth: >= 0, not NaN, the two weights not both 0. */
int emrt_lx_dice_ce_fwd(const float* logits, const long long* labels, const float* class_weight, int N, int C, int H, int W, int ignore_index, float ce_weight, float dice_weight, float smooth, float* result, float* coef, void* workspace, void* stream);

/* result, coef: as the forward wrote them.  upstream: a device scalar or NULL (= 1).  weight: the head's weight.  Every entry of dlogits is written. */
int emrt_lx_dice_ce_bwd(const float* logits, const long long* labels, const float* class_weight, const float* result, const float* coef, const float* upstream, float weight, float ce_weight, int N, int C, int H, int W, int ignore_index, float* dlogits, void* stream);

/* Two heads of equal shape on the same labels through the launches of one; total[0] = wa * L_a + wb * L_b. */
int emrt_lx_dice_ce_pair_fwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, int N, int C, int H, int W, int ignore_index, float wa, float wb, float ce_weight, float dice_weight, float smooth, float* res_a, float* res_b, float* coef_a, float* coef_b, float* total, void* workspace, void* stream);

int emrt_lx_dice_ce_pair_bwd(const float* logits_a, const float* logits_b, const long long* labels, const float* class_weight, const float* res_a, const float* res_b, const float* coef_a, const float* coef_b, const float* up_a, const float* up_b, float wa, float wb, float ce_weight, int N, int C, int H, int W, int ignore_index, float* dlogits_a, float* dlogits_b, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMRT_HIP_LOSS_H */
