/*
 * mage_hip_ext.h -- extension entry points of libmage_hip.so.
 *
 * The core table of include/mage_hip.h is frozen at 69 entry points (MAGE_ABI_VERSION 10); entry points added since are declared here and
 * bound from mage_amd/_lib.py's EXT_SIGNATURES in the same loop as the core table, so a stale library fails to load the same way.  The
 * conventions are mage_hip.h's: device pointers owned by the caller, `stream` a hipStream_t passed as void*, asynchronous calls, 0 on
 * success or a negative MAGE_E* code with a thread-local message in mage_last_error().
 */
#ifndef MAGE_HIP_EXT_H
#define MAGE_HIP_EXT_H

#include "mage_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-token statistics of the sampling policy: no site in the reference (it decodes greedily and reports no probability).  Serves
 * MAGE.set_logprobs(policy=, entropy=) and MAGE.score at the sites where mage_token_logprob is called (mage_amd/modules/mage_model.py: the
 * incremental loop, the sampled and the greedy full loop).
 * Row i reads K fp32 logits z with mage_argmax's input addressing (ld, group, in_group_stride, in_off) and uses index
 * (i / group)*tok_group_stride + i % group + tok_off of tokens (int64; may be null when policy_logprob is null) and of every output, as
 * mage_token_logprob does.  temperature, top_k, top_p are mage_sample_tokens' and are validated the same way.  With s = z * (float)(1.0 /
 * temperature) and N the set mage_sample_tokens draws from under these parameters (the sampler's own filter code runs again in the same
 * arithmetic, so N is its set bit for bit, also where rounded top-p masses keep a value more or less than the exact rule):
 *   kept           (int32)  |N|, exact;
 *   policy_logprob (fp32)   s_t - (s_max + log Z) for the row's token t in N, -inf for t outside N; Z = sum_{j in N} exp(s_j - s_max);
 *   policy_entropy (fp32)   log Z - (sum_{j in N} exp(s_j - s_max) (s_j - s_max)) / Z, in nats; exactly 0 when |N| = 1;
 *   entropy        (fp32)   the same formula over the whole row of z (temperature 1, no filter): the entropy of the distribution
 *                           mage_token_logprob scores under.
 * Each output is optional (null: not computed), at least one must be given; the row is read once whatever is asked for.  top_k == 1 is
 * greedy by definition, as in the sampler: N = { mage_argmax's first maximum of z }, kept = 1, policy_logprob 0 for that code and -inf for
 * any other, policy_entropy 0.  Every sum has a fixed order: a row's bits do not depend on `rows` or on its place in the launch, and with
 * temperature 1, top_k 0, top_p 1 policy_logprob equals mage_token_logprob's result bit for bit on NaN-free rows.
 * Special values: a NaN logit is in no set (and makes `entropy` NaN, as it does mage_token_logprob's result); a -inf logit counts in
 * `kept` when the filter keeps it and adds a zero term to the sums; a row with no selectable code (every logit NaN) gives kept = 0 and NaN
 * for policy_logprob and policy_entropy; a row whose largest kept s is not finite gives NaN for them (inf - inf).  A token outside [0, K) is
 * recorded for mage_check_device_errors (as mage_token_logprob's) and clamped.  K % 4 == 0, K <= MAGE_SAMPLE_MAX_K, ld % 4 == 0, ld >= K,
 * logits 16-byte aligned, strides and offsets >= 0, top_k in [0, K], top_p in (0, 1], temperature (and its reciprocal) finite and > 0:
 * MAGE_EINVAL otherwise, nothing launched. */
int mage_token_stats(const float* logits, int64_t rows, int32_t K, int64_t ld, int64_t group, int64_t in_group_stride, int64_t in_off,
                     const int64_t* tokens, int64_t tok_group_stride, int64_t tok_off, float temperature, int32_t top_k, float top_p,
                     float* policy_logprob, float* policy_entropy, int32_t* kept, float* entropy, void* stream);

/* Policy-gradient loss over given tokens, and its gradient with respect to the logits: no site in the reference (its only objective is the
 * mean cross-entropy).  Serves MAGE.policy_loss (mage_amd/modules/mage_train.py: train_forward / train_backward with a PolicyHead).
 * Row i is the K fp32 logits z at logits + i*ld with its token t = tokens[i] (int64), its advantage A = advantage[i / adv_div] (fp32;
 * adv_div = 1: one per row, adv_div = rows per clip: one per clip) and, when behaviour_logprob is given, b = behaviour_logprob[i] (fp32:
 * the log-probability under which the token was drawn).  The policy is mage_sample_tokens' under (temperature, top_k, top_p): with
 * s = z * (float)(1.0 / temperature) and N the set it draws from -- the sampler's own filter code runs again in the same arithmetic, as in
 * mage_token_stats -- the forward call writes, per row,
 *   cut      (uint32)  the filter's threshold on the order-preserving key of s: j is in N iff key(s_j) >= cut[i] (what the backward call reads
 *                      instead of running the filter again);
 *   logprob  (fp32)    s_t - (s_max + log Z), Z = sum_{j in N} exp(s_j - s_max); -inf for t outside N: mage_token_stats' policy_logprob,
 *                      bit for bit (the same operations in the same order);
 *   entropy  (fp32)    log Z - (sum_{j in N} exp(s_j - s_max) (s_j - s_max)) / Z: mage_token_stats' policy_entropy, bit for bit;
 *   row_loss (fp32)    l_i = -A logprob - entropy_coef entropy                                       (behaviour_logprob null: the
 *                      reward-weighted likelihood; A = 1, temperature 1, no filter, entropy_coef 0: cross-entropy's row loss), or
 *                      l_i = -min(rho A, clamp(rho, 1 - clip_lo, 1 + clip_hi) A) - entropy_coef entropy,  rho = expf(logprob - b)
 *                      (the clipped surrogate).  rho is one fp32 value, the bounds are (float)(1.0 - clip_lo) and (float)(1.0 + clip_hi);
 *                      the products and the sum are taken in fp64 and rounded once.
 * A row whose token lies outside a non-empty N (off-policy data the current filter could never draw) is an outside row: logprob -inf,
 * l_i = 0, a zero gradient row.  summary[0..5) are five means over `rows`, each summed in fp64 in a fixed order and rounded once to fp32:
 * l, entropy, b - logprob (0 without behaviour_logprob), the share of rows whose gradient the clip switched off (g_i = 0 below), the share of
 * outside rows; an outside row counts in the last one only.  Two launches on the same inputs give the same bits.  The partial sums pass
 * through one per-device buffer of the library: calls of mage_policy_loss on one device must be ordered (one stream, or events).
 * The backward call writes dlogits [rows, K] (contiguous; dl_dtype MAGE_F32 or MAGE_BF16, as mage_cross_entropy_bwd's):
 *   dlogits_ij = grad_out[0] / rows * inv_t * [ g_i (1[j = t] - p_j) + entropy_coef p_j (log p_j + entropy_i) ]   for j in N,
 *   exactly 0 for j outside N and for every j of an outside row; p = softmax of s over N, a p_j = 0 term counts as 0 (never 0 * inf);
 *   g_i = -A without behaviour_logprob; with it g_i = -A rho where the unclipped term of the min is the active one (A >= 0 and
 *   rho <= 1 + clip_hi, or A < 0 and rho >= 1 - clip_lo) and 0 otherwise.  It recomputes Z, entropy and rho with the forward call's
 *   operations, so both passes take the same branch; pass it the forward call's arguments.
 * Special values: a NaN logit is in no set; a row with no selectable code (every logit NaN) gives NaN for logprob, entropy and row_loss and
 * a zero gradient row; a row whose largest kept s is not finite gives NaN throughout (inf - inf), as mage_token_logprob does.  A token
 * outside [0, K) is recorded for mage_check_device_errors by the forward call and clamped by both.
 * top_k == 1 is refused: a greedy policy has log-probability 0 and no gradient, and its one-element set is not a threshold.  clip_lo in
 * [0, 1], clip_hi >= 0, entropy_coef finite, adv_div > 0; otherwise mage_token_stats' rules: K % 4 == 0, K <= MAGE_SAMPLE_MAX_K,
 * ld % 4 == 0, ld >= K, logits (and dlogits) 16-byte aligned, top_k in [0, K], top_p in (0, 1], temperature (and its reciprocal) finite
 * and > 0; every output required.  MAGE_EINVAL otherwise, nothing launched.
 * One wave per row, the row in registers in the sampler's layout (4 .. 64 values per lane by K), one kernel instance per filter
 * combination, every sum in a fixed order, accurate expf / logf. */
int mage_policy_loss(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage, int64_t adv_div,
                     const float* behaviour_logprob, float temperature, int32_t top_k, float top_p, float clip_lo, float clip_hi,
                     float entropy_coef, float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* summary, void* stream);
int mage_policy_loss_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                         int64_t adv_div, const float* behaviour_logprob, const uint32_t* cut, float temperature, float clip_lo,
                         float clip_hi, float entropy_coef, const float* grad_out, void* dlogits, int32_t dl_dtype, void* stream);

/* mage_policy_loss with a penalty against a frozen reference policy (the per-token KL term of PPO / GRPO-style fine-tuning), and its
 * gradient: no site in the reference.  Serves MAGE.policy_loss(reference_logprobs=, kl_coef=).
 * Everything mage_policy_loss / mage_policy_loss_bwd state holds; in addition row i reads r = reference_logprob[i] (fp32: the token's
 * log-probability under the reference policy, e.g. MAGE.token_policy_logprobs of a frozen copy).  With lp the row's logprob (unchanged, bit
 * for bit mage_token_stats' policy_logprob) and d = r - lp formed as one fp32 subtraction, the forward call also writes
 *   kl       (fp32)    kl_i = exp(d) - d - 1, the non-negative "k3" estimate of KL(policy || reference) at the drawn token,
 * and row_loss is l_i(mage_policy_loss' rule) + kl_coef kl_i, the sum taken in fp64 together with the rule's fp64 terms and rounded once.
 * The backward call uses g_i(mage_policy_loss_bwd's rule) + kl_coef (1 - exp(d)) in place of g_i (d kl / d logprob = 1 - exp(r - logprob);
 * the two parts are added in fp64 and rounded once to fp32); the rest of dlogits -- the entropy term, the kept set read from cut -- is
 * mage_policy_loss_bwd's formula.  A row whose gradient the clip switched off keeps its KL gradient.
 * Accuracy: both factors are evaluated in fp64 from the fp32 value d, 1 - exp(d) as -expm1(d) (no cancellation), kl_i as expm1(d) - d for
 * |d| >= 2^-8 (the subtraction costs at most 9 of fp64's 53 bits: relative error below 2^-42) and as the series
 * d^2 (1/2 + d/6 + d^2/24 + d^3/120 + d^4/720) below it (first dropped term below 2^-51 of the sum): each is far inside one fp32 ulp for every
 * d, down to |d| of 1e-12 and below, before its one rounding.  There is no clamp on d: a finite d large enough to overflow gives kl_i = +inf
 * (and a gradient factor of -inf), as the arithmetic says.
 * Exact cases: d == 0 (r has the bits of logprob) gives kl_i = 0 exactly, and a zero term is never added: that row's row_loss and dlogits
 * row are bit for bit mage_policy_loss' and mage_policy_loss_bwd's for any kl_coef; kl_coef == 0 gives row_loss, logprob, entropy, cut and
 * dlogits bit for bit theirs for any r (kl is still reported).
 * Special rows: an outside row (logprob -inf) stays all zeros, kl_i = 0 included, and counts in the outside share only.  A row whose r is
 * not finite (NaN, +-inf: e.g. -inf because the reference's filter could not draw the token) is an unanchored row: kl_i = 0, no KL gradient,
 * otherwise treated by mage_policy_loss' rule.  A NaN logprob gives a NaN kl_i.
 * summary[0..7): mage_policy_loss' five means (the loss mean now including the KL term), the mean of kl_i over `rows`, and the share of
 * unanchored rows (inside rows whose r is not finite) -- the same two-stage fixed-order fp64 reduction through the same per-device buffer:
 * two launches give the same bits, and calls of mage_policy_loss and mage_policy_loss_anchored on one device must be ordered.
 * Arguments: the plain pair's rules; reference_logprob (and kl) non-null and 4-byte aligned, kl_coef finite and >= 0: MAGE_EINVAL
 * otherwise, nothing launched.  The kernels are the plain pair's templates (one wave per row, one instance per filter combination) with the
 * anchor compiled in: the plain entry points run the instances without it. */
int mage_policy_loss_anchored(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                              int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature,
                              int32_t top_k, float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef, float* row_loss,
                              float* logprob, float* entropy, uint32_t* cut, float* kl, float* summary, void* stream);
int mage_policy_loss_anchored_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                  int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, const uint32_t* cut,
                                  float temperature, float clip_lo, float clip_hi, float entropy_coef, float kl_coef, const float* grad_out,
                                  void* dlogits, int32_t dl_dtype, void* stream);

/* Sum of squares of a flat fp32 buffer, and mage_adam with the gradient norm clipped: no site in the reference (it runs bare Adam).  Serve
 * FlatAdam(max_grad_norm=) (mage_amd/optim.py).
 * mage_sumsq: out[0] (fp64, device) = sum_i g[i]^2.  Every square is taken in fp64 (exact for fp32 values) and the sum is added in a fixed
 * order -- one partial per workgroup over its contiguous part of g, then a second stage over the partials: two launches give the same bits,
 * and the result does not depend on the alignment of g beyond the 4 bytes required (scalar loads only).  n > 0 is arbitrary (no n % 4 rule);
 * g 4-byte and out 8-byte aligned: MAGE_EINVAL otherwise, nothing launched.  The partials pass through one per-device buffer of the
 * library: calls of mage_sumsq on one device must be ordered (one stream, or events).
 * mage_adam_clipped: mage_adam's arguments and update, with the gradient scaled by torch.nn.utils.clip_grad_norm_'s rule.  sumsq (device,
 * fp64) holds the sum of squares of the whole (summed) gradient -- in a sharded step the all-reduced total of the shards' mage_sumsq.  Every
 * thread derives the same scale from that one value:
 *   norm = sqrt(*sumsq) * grad_scale  in fp64 (the norm of the averaged gradient);  coef = max_norm / (norm + 1e-6);
 *   scale = grad_scale where coef >= 1, (float)(grad_scale * coef) otherwise,
 * and the update is mage_adam's with `scale` for grad_scale (the same code): a step whose norm is within the limit leaves mage_adam's bits
 * in p, m and v.  norm_out (device, fp32, may be null) receives (float)norm from one thread.  Nothing is read on the host.  A norm that is
 * not finite propagates (NaN: the scale is NaN; +inf: the scale is 0 and 0 * inf = NaN where the gradient is infinite), as
 * clip_grad_norm_(error_if_nonfinite=False) does; the step that skips instead is mage_adam_guarded (below).  max_norm finite and > 0, sumsq
 * non-null and 8-byte aligned, otherwise mage_adam's rules: MAGE_EINVAL otherwise, nothing launched. */
int mage_sumsq(const float* g, int64_t n, double* out, void* stream);
int mage_adam_clipped(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int32_t step,
                      float grad_scale, const double* sumsq, float max_norm, float* norm_out, void* stream);

/* The Adam step that can run unattended: mage_adam_clipped's launch with a skip of non-finite steps, AdamW's decoupled weight decay and an
 * exponential moving average of the parameters: no site in the reference (bare Adam).  Serves FlatAdam(weight_decay=, no_decay=,
 * ema_decay=, skip_nonfinite=) (mage_amd/optim.py).  One launch over a flat shard in mage_adam's grid; every thread reads the one device
 * value *sumsq (when given) and derives the same decisions from it; nothing is read on the host.
 * Norm and scale: with sumsq given, norm = sqrt(*sumsq) * grad_scale in fp64 and norm_out (device fp32, may be null) receives (float)norm
 *   from one thread -- on a skipped step too, so the caller can see the inf or NaN.  max_norm > 0: the scale is mage_adam_clipped's, operation
 *   for operation (coef = max_norm / (norm + 1e-6); grad_scale where coef >= 1, (float)(grad_scale * coef) otherwise).  max_norm == 0: no
 *   clip, scale = grad_scale.
 * Guard: with skip_nonfinite != 0, a *sumsq that is not finite makes every thread return before it loads p, g, m, v or ema: the five
 *   buffers keep their bits.  Thread 0 of workgroup 0 then adds 1 to *skipped (device int64, may be null; one thread writes it and none
 *   reads it).  mage_sumsq takes every square in fp64, where the square of an fp32 value cannot overflow, inf squared is inf and NaN stays
 *   NaN, and adds non-negative terms: *sumsq is finite exactly when every gradient element is finite, so the guard is a test of the
 *   gradient, not of its magnitude.  `step` counts CALLS: a skipped call still consumes its step number (the caller's counter advances, and
 *   the bias corrections 1 - beta^step of the next call are those of step + 1).  This differs, on purpose, from "as if the call had not
 *   happened": the corrections stay host values computed as mage_adam computes them, and the kernel stays one launch without device-side
 *   state.  With skip_nonfinite == 0 a non-finite gradient propagates as in mage_adam / mage_adam_clipped.
 * Decay: element i < n_decay gets p = p * decay_mul (one fp32 product, rounded on its own) before the Adam update -- torch.optim.AdamW's
 *   order; the caller forms decay_mul = (float)(1.0 - (double)lr * weight_decay).  Elements >= n_decay are not decayed.  n_decay is any value
 *   in [0, n]: the test is per element, a 16-byte chunk may straddle it.
 * Update: the one statement mage_adam and mage_adam_clipped run (the same device function).  With finite gradients, ema null and
 *   n_decay == 0 it leaves mage_adam_clipped's bits in p, m and v (max_norm > 0), or mage_adam's (max_norm == 0, whatever sumsq is).
 * EMA: with ema (device fp32 [n], 16-byte aligned) non-null, ema = fma(ema_decay, ema, (1 - ema_decay) * p_new) after the update: 1 -
 *   ema_decay one fp32 subtraction, the product rounded once, then one fused multiply-add; p_new is the value just stored.
 * Arguments: mage_adam's rules (p, g, m, v non-null and 16-byte aligned, n > 0, step >= 1); ema null or 16-byte aligned; 0 <= n_decay <= n;
 * decay_mul finite and in (0, 1]; ema_decay in (0, 1) when ema is given; max_norm finite and >= 0; sumsq non-null whenever max_norm > 0 or
 * skip_nonfinite, 8-byte aligned when given; skipped null or 8-byte, norm_out null or 4-byte aligned: MAGE_EINVAL otherwise, nothing
 * launched.  One kernel instance per (ema given, n_decay > 0): the plain form carries no load or test of the other two. */
int mage_adam_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t n, int64_t n_decay, float lr, float beta1, float beta2,
                      float eps, int32_t step, float grad_scale, float decay_mul, float ema_decay, const double* sumsq, float max_norm,
                      int32_t skip_nonfinite, float* norm_out, int64_t* skipped, void* stream);

/* Per-frame MSE, PSNR and SSIM between generated frames and their targets: no site in the reference (it reports no metric).  Serves
 * MAGE.video_metrics and the built-in rewards of MAGE.rollout (mage_amd/modules/mage_model.py).
 * video and target are fp32 [clips, T, C, H, W] with a frame's C*H*W values contiguous, frames of a clip T*C*H*W apart and clip r of video
 * at video + r*video_clip_stride (elements); video clip r is compared with target clip r / tgt_div at target + (r / tgt_div) *
 * target_clip_stride (tgt_div = N: the N candidates of a clip share one ground truth; a target that is frames 1 .. L-1 of an [B, L, C, H, W]
 * batch is the pointer advanced one frame with target_clip_stride = L*C*H*W).  Outputs are fp32 [clips*T], entry r*T + t for frame t of
 * clip r; each is optional (null: not computed), at least one must be given:
 *   mse   the mean over C*H*W of (x - y)^2: differences, squares and the sum in fp64, rounded once;
 *   psnr  10 log10(data_range^2 / mse) from the fp64 mean; +inf where mse is 0;
 *   ssim  the mean over channels and window positions of
 *           ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)),  C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2,
 *         with the local moments under an 11 x 11 Gaussian window (sigma 1.5, normalised to sum 1, applied separably) at the (H-10) x (W-10)
 *         positions where the window lies inside the frame, biased: sx^2 = E[x^2] - mx^2, sxy = E[xy] - mx my.  All of it in fp64, rounded
 *         once (x*x, y*y and x*y of fp32 values are exact there).
 * Every sum has a fixed order and there are no floating-point atomics: two launches give the same bits, and a frame's bits depend on its own
 * pixels only -- not on clips, tgt_div or its place in the launch.  Both sides go through the same operations, so metrics(x, y) equals
 * metrics(y, x) bit for bit and metrics(x, x) is mse 0, psnr +inf, ssim 1 exactly.  A NaN pixel makes its own frame's outputs NaN.
 * ssim needs H >= 11 and W >= 11; clips, T, C, H, W > 0 with clips*T and C*H*W below 2^31; tgt_div >= 1; data_range finite and > 0; both
 * strides >= T*C*H*W; pointers 4-byte aligned: MAGE_EINVAL otherwise, nothing launched.
 * One workgroup per frame, which walks the frame in tiles of up to 28 x 30 window positions: a tile's pixels come from memory once into LDS
 * (only the 10-pixel halo is read again by the neighbouring tile), a row pass and a column pass form the five windowed moments through LDS. */
int mage_video_metrics(const float* video, int64_t video_clip_stride, const float* target, int64_t target_clip_stride, int64_t clips, int32_t T,
                       int32_t C, int32_t H, int32_t W, int64_t tgt_div, float data_range, float* mse, float* psnr, float* ssim, void* stream);

/* Per-clip rewards and group-relative advantages from per-frame rewards: no site in the reference.  Serves MAGE.rollout.
 * frame_reward is fp32 [groups*N*T]: T frame rewards for each of the N candidates of each group (clip).  reward (fp32 [groups*N]) is each
 * candidate's mean over its T frames, added in fp64 in order and rounded once.  With mean_g and std_g the mean and the population standard
 * deviation of a group's N rewards (fp64, fixed order), advantage (fp32 [groups*N]) is
 *   mode 0:  r - mean_g;          mode 1:  (r - mean_g) / (std_g + eps).
 * A reward equal to its group's mean gets exactly 0 in both modes (so a group of equal rewards is all zeros, also with eps = 0).  A group
 * holding a NaN or infinite reward gets NaN advantages throughout; nothing is checked on the host.  Two launches give the same bits.
 * groups > 0, N >= 2, T >= 1, mode 0 or 1, eps finite and >= 0, pointers non-null and 4-byte aligned: MAGE_EINVAL otherwise, nothing launched. */
int mage_group_advantages(const float* frame_reward, int64_t groups, int32_t N, int32_t T, int32_t mode, float eps, float* reward,
                          float* advantage, void* stream);

/* Per-frame reward-to-go returns and their group-relative advantages: no site in the reference.  Serves MAGE.rollout(credit='frame'): a
 * frame's tokens are drawn given the earlier frames only, so they are credited with the rewards of their own frame and the later ones.
 * frame_reward is fp32 [groups*N*T] in mage_group_advantages' layout.  returns (fp32 [groups*N*T]), in fp64 with gamma widened from fp32:
 *   S[c,T-1] = r[c,T-1];   S[c,t] = r[c,t] + gamma * S[c,t+1]  from the last frame down;   G[c,t] = S[c,t] / T, rounded once to fp32.
 * The product and the sum are rounded separately (no fma: a numpy restatement has the same bits).  gamma == 0 forms no product,
 * S[c,t] = r[c,t], so a non-finite later frame does not reach an earlier one as 0 * inf; at gamma == 1 frame 0's return is the candidate's
 * mean reward (mage_group_advantages' reward up to the order of the sum).
 * advantage is fp32 [groups*N*slots]: frame t of candidate c of group g goes to ((g*N + c)*slots) + slot_off + t, every slot outside
 * [slot_off, slot_off + T) is written as +0 (slots = L-1 and slot_off = k-1 under a context of k given frames: the layout of tokens).  With
 * mean and std the mean and the population standard deviation of a (group, frame)'s N returns AS STORED (the fp32 values widened to fp64,
 * added in candidate order) -- so advantage is a function of returns alone --
 *   mode 0:  d = G - mean;          mode 1:  d / (std + eps),
 * and d == 0 gives exactly +0 in both modes, mage_group_advantages' rule: a frame whose candidates all earned the same rewards from there
 * on is all +0, also with eps = 0.  A (group, frame) whose N returns hold a NaN or an infinity gets NaN for all N candidates at that
 * frame; through the recursion a non-finite reward at frame s reaches the frames t <= s of its group (gamma > 0) and no later one.
 * Nothing is checked on the host.  Two launches give the same bits, and the bits of a (group, frame) depend on that group's rewards
 * alone, not on groups or the group's place in the launch.  No floating-point atomics, plain vector-memory stores.
 * groups > 0, N >= 2, T >= 1, slot_off >= 0, slots >= slot_off + T, groups*N*slots (hence groups*N*T) below 2^31, gamma in [0, 1], mode 0
 * or 1, eps finite and >= 0, pointers non-null and 4-byte aligned: MAGE_EINVAL otherwise, nothing launched.
 * One launch, one wave per group: a lane per candidate walks the recursion and stores the returns, then, behind a workgroup barrier, a
 * lane per slot reads its frame's returns back and forms the statistics -- N > 64 and slots > 64 wrap over the lanes. */
int mage_frame_advantages(const float* frame_reward, int64_t groups, int32_t N, int32_t T, float gamma, int32_t mode, float eps, int32_t slots,
                          int32_t slot_off, float* returns, float* advantage, void* stream);

/* Seeded standard-normal noise of the randomness branch: the reference draws it with torch.randn (mage_model.py:661), unseeded and kept
 * nowhere.  Serves batch['noise_seed'] of MAGE.autoregressive_generate and MAGE.rollout(noise='candidate') (mage_amd/modules/mage_model.py:
 * _anchor_tail), whose recorded noise MAGE.policy_loss then conditions on.
 * seeds is int64 [B] on the device; clip b gets C * hw values.  Two optional fp32 outputs, at least one given: nchw [B, C, hw] (the public
 * video_noise layout, [B, C, h, w]) and rows [B * hw, C] (channel-last: what conv_d2's convolution reads).  The rule, for clip b, channel c,
 * pixel p, in uint64 wrap-around arithmetic on hash32 (mage_amd/csrc/common.h):
 *   e    = c * hw + p;   base = ((uint64)seeds[b] ^ 0x8000000000000000) * 0x9e3779b97f4a7c15;
 *   m1   = hash32(base + 2e) >> 8 (24 bits),  u1 = (m1 + 0.5) 2^-24;      m2 = hash32(base + 2e + 1) >> 9 (23 bits);
 *   z    = sqrt(-2 log(u1)) * cos(pi * (m2 + 0.5) 2^-22)                  (Box-Muller, one normal per element).
 * log(u1) is taken as mage_sample_tokens takes its Gumbel logarithm -- logf of u1 below 1/2, log1pf of -(1 - u1) above, either argument
 * exact in fp32 -- so u1 is never rounded; the angle (m2 + 0.5) 2^-22 in (0, 2) has 24 significant bits, is exact, and goes through cospif.
 * z is finite by construction: u1 >= 2^-25 gives |z| <= sqrt(2 log 2^25) < 5.89, and the cosine is never exactly 0.
 * A value depends on its clip's seed, its channel and its pixel only: not on B, the clip's place in the batch, which outputs are asked for,
 * or the launch geometry.  Every value is computed once per launch and stored to both layouts: they hold the same bits.
 * Domain separation from mage_sample_tokens: a rollout gives a candidate ONE seed s for both streams.  The sampler's counters are
 * s * 0x9e3779b97f4a7c15 + t, t = pos * K + j < 2^63; flipping bit 63 of the seed before the multiply moves the base by exactly
 * 2^63 * 0x9e3779b97f4a7c15 = 2^63 (mod 2^64: the multiplier is odd), so the noise counters are s * 0x9e3779b97f4a7c15 + 2^63 + t',
 * t' < 2^31 -- the two sets are disjoint for every seed as long as the sampler's stream is shorter than 2^63, which its own argument rules
 * guarantee.  (Under any affine scheme the noise of seed s is the sampler's stream of SOME other seed; here that seed is s ^ 2^63, never a
 * neighbour s + c of a rollout.)
 * B, C, hw > 0, at least one output, outputs 16-byte and seeds 8-byte aligned, C * hw <= 2^30 (the counters 2e + 1 stay below 2^31) and
 * B * C * hw <= 2^38: MAGE_EINVAL otherwise, nothing launched.  hw and C need not be multiples of 4: a lane owns a tile of 4 channels x 4
 * pixels and falls back from 16-byte to 4-byte stores where a quad crosses the end of its axis or is not 16-byte aligned.  No LDS, no
 * atomics, plain vector-memory stores. */
int mage_video_noise(const int64_t* seeds, int64_t B, int32_t C, int64_t hw, float* nchw, float* rows, void* stream);

/* Classifier-free guidance of the token logits: no site in the reference (it decodes one caption's logits).  Serves MAGE.set_guidance
 * (mage_amd/modules/mage_model.py: _generate_one runs the decoder over [clips under the caption | the same clips under the negative caption]
 * and combines the two logit rows of every position, in place on the caption's half, before the token is picked).
 * Row i of cond, uncond and out is K fp32 values at mage_argmax's input address, ((i / group) * in_group_stride + i % group + in_off) * ld, in
 * each buffer; row i uses s = scale[i / scale_div] (fp32, device; scale_div = rows per clip: one value per clip, as mage_policy_loss'
 * adv_div).  The rule, per element, in fp32:
 *   w = s - 1 (one subtraction per row);   d = c - u;   z = c where w == 0 or d == 0,   z = fma(w, d, c) otherwise (one rounding).
 * So z = c + (s - 1)(c - u), the usual u + s (c - u), written so that two cases are exact by construction: scale 1 returns cond's bits, and
 * uncond equal to cond returns cond's bits for every finite scale, the sign of a zero included (0 * w + (-0) would be +0: hence the selects).
 * Special values: NaN propagates -- a NaN in c, u or s gives NaN (the comparisons are false, the fma runs); inf - inf in d is NaN; an
 * infinite s with d == 0 still returns c.  A row's bits depend on its own two rows and its scale only, not on `rows` or the row's place in
 * the launch.  No reduction, no LDS, no atomics; 16-byte loads, plain 16-byte vector-memory stores; columns K .. ld of out are not written.
 * out may be cond itself, exactly (every lane reads the quads it writes, and no others, before it writes them); otherwise out must not
 * overlap either input.
 * K % 4 == 0, K <= MAGE_SAMPLE_MAX_K, ld % 4 == 0, ld >= K, cond / uncond / out non-null and 16-byte aligned, scale non-null and 4-byte
 * aligned, rows, group, scale_div > 0, in_group_stride and in_off >= 0: MAGE_EINVAL otherwise, nothing launched.  Row bases are 64-bit. */
int mage_guide_logits(const float* cond, const float* uncond, float* out, int64_t rows, int32_t K, int64_t ld, int64_t group,
                      int64_t in_group_stride, int64_t in_off, const float* scale, int64_t scale_div, void* stream);

/* Preference loss over ranked pairs of clips (DPO / IPO), its pair stage: no site in the reference (its only objective is the mean
 * cross-entropy).  Serves MAGE.preference_loss (mage_amd/modules/mage_train.py: train_forward with a PreferenceHead, after mage_token_logprob and
 * mage_clip_scores have reduced the logits to one log-likelihood per clip).
 * clip_logprob s and reference_logprob r are fp32 [clips] (a clip's summed token log-probabilities under the model and under the frozen
 * reference); pairs is int64 [n_pairs, 2] on the device, pair p = (w, l): the chosen row and the rejected row.  Everything is computed in
 * fp64 from the fp32 inputs (beta and label_smoothing eps widened from their fp32 values), each output rounded to fp32 once:
 *   a = s_w - r_w;   b = s_l - r_l;   u = a - b;   h = beta u;
 *   mode 0 (DPO):  l_p = -(1 - eps) logsig(h) - eps logsig(-h),  logsig(x) = min(x, 0) - log1p(exp(-|x|))   (never overflows; the eps term
 *                  is not formed at all when eps == 0, so a saturated pair is 0 and not 0 * inf);
 *                  g_p = dl/du = -beta [(1 - eps) sig(-h) - eps sig(h)],  sig(|h|) = 1 / (1 + e), sig(-|h|) = e / (1 + e), e = exp(-|h|);
 *   mode 1 (IPO):  l_p = (u - 1 / (2 beta))^2,  g_p = 2 (u - 1 / (2 beta));  label_smoothing must be 0.
 * Outputs: pair_loss [n_pairs] = l_p;  pair_margin [n_pairs] = h;
 *   clip_coef [clips]: clip_coef[c] = (sum_{p: w_p = c} g_p - sum_{p: l_p = c} g_p) / n_pairs, the derivative of the mean loss with respect to
 *   clip_logprob[c] (what mage_token_logprob_bwd takes as its weights): the terms are added in fp64 in increasing p, whichever side names c.
 *   A pair with w == l contributes nothing (its u is exactly 0: no preference); a clip in no pair gets +0.
 *   summary [5]: five means over the pairs -- l, the share of pairs with u > 0 (the accuracy), beta a (the chosen reward), beta b (the
 *   rejected reward), h (the margin) -- each a fixed-order fp64 sum (a workgroup's 256 pairs meet in an xor butterfly and its four waves in
 *   order; the workgroups' sums meet the same way), divided by n_pairs and rounded once.
 * The launch geometry is a function of clips and n_pairs alone and every sum has a fixed order: two launches give the same bits.  There are
 * no floating-point atomics.  A non-finite input propagates as the arithmetic says (inf - inf is NaN); nothing is checked on the host.  An
 * index outside [0, clips) is recorded for mage_check_device_errors and clamped, as mage_token_logprob's out-of-range token is.
 * Two launches: one thread per pair writes pair_loss, pair_margin, (w, l, g_p) and its workgroup's partial sums into per-device buffers of the
 * library (calls of mage_preference_loss on one device must be ordered: one stream, or events); then one thread per clip, 256 clips per
 * workgroup, walks all pairs, staged through LDS 256 at a time (16 bytes each): a wave looks at 64 staged pairs at once, one per lane,
 * ballots the ones that name one of ITS 64 clips and adds only those, in order.  The walk is n_pairs / 64 steps per wave plus one step per
 * pair naming one of the wave's clips; a clip's own terms are one dependent fp64 add each, whatever the kernel does.
 * Limits: clips and n_pairs in [1, 65536] (the per-device pair buffer holds 65536 entries); beta finite and > 0 (and 1 / (2 beta) finite);
 * label_smoothing in [0, 0.5), 0 in mode 1; mode 0 or 1; every pointer non-null and aligned to its element size (4 bytes, pairs 8):
 * MAGE_EINVAL otherwise, nothing launched. */
int mage_preference_loss(const float* clip_logprob, const float* reference_logprob, int64_t clips, const int64_t* pairs, int64_t n_pairs,
                         float beta, float label_smoothing, int32_t mode, float* pair_loss, float* pair_margin, float* clip_coef,
                         float* summary, void* stream);

/* Gradient of sum_i weight[i / weight_div] * logprob_i with respect to the logits, logprob_i being mage_token_logprob's value for row i (the
 * log-softmax of the row at temperature 1, no filter, gathered at tokens[i]): no site in the reference.  Serves the backward pass of
 * MAGE.preference_loss (mage_amd/modules/mage_train.py: train_backward), with mage_preference_loss' clip_coef as the weights and
 * weight_div = rows per clip.
 * Row i is the K fp32 logits z at logits + i*ld with its token t = tokens[i] (int64).  With c_i = grad_out[0] * weight[i / weight_div] (one
 * fp32 product) and p the softmax of the row in mage_cross_entropy_bwd's arithmetic (fp32: m = max_j z_j, w_j = expf(z_j - m), p_j = w_j *
 * (1 / sum_j w_j), the sum in a fixed order: a lane adds its own terms in register order, the lanes meet in an xor butterfly),
 *   dlogits_ij = c_i (1[j = t] - p_ij),
 * written contiguous ([rows, K]) as dl_dtype MAGE_F32 or MAGE_BF16.  A row with c_i == 0 is written as +0 throughout WITHOUT reading its
 * logits (most clips of a large rollout are in no pair; a NaN in such a row does not show).  A -inf logit gives p = 0 and so a zero at its
 * column; a token outside [0, K) gets no one-hot (mage_token_logprob, which runs before, records it); a NaN logit, or a row whose maximum is
 * not finite, makes the row NaN as it makes logprob_i NaN.  A row's bits depend on the row, its token and c_i alone.
 * One wave per row, the row in registers in the sampler's layout (4 .. 64 values per lane by K, code k = chunk*256 + lane*4 + e): every logit
 * is read once with a 16-byte load, and every output is written once with a 16-byte store -- for bf16 two neighbouring lanes exchange
 * their packed quads so that each stores eight consecutive values (K % 8 == 0; other K: 8-byte stores).
 * mage_token_stats' size rules: rows > 0, K % 4 == 0, 0 < K <= MAGE_SAMPLE_MAX_K, ld % 4 == 0, ld >= K, logits and dlogits 16-byte aligned;
 * weight_div > 0; tokens 8-byte, weight and grad_out 4-byte aligned; every pointer non-null: MAGE_EINVAL otherwise, nothing launched. */
int mage_token_logprob_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* weight,
                           int64_t weight_div, const float* grad_out, void* dlogits, int32_t dl_dtype, void* stream);

/* The decoder's H / W axial attention fused into its in_proj GEMM: q, k, v and the softmax numerators never reach memory (mage_model.py:20,75
 * inside the axial blocks :344,382; serves FlatAxialDecoder._pass for the blocks attending along H or W on the 16-bit LayerNorm-fold path).
 * Replaces the pair mage_gemm (QKV, LayerNorm-consuming form) -> mage_attention for 16 x 16 frames and head width 32 by ONE launch of the
 * one-wave-per-SIMD GEMM (csrc/gemm4.hip): per (frame, group of 4 heads) a Q K tile whose numerators stay in the registers of the wave that
 * computed them, then a half-width V tile over the same rows; the frame's LayerNorm statistics are fetched once per entry, no scratch buffer.
 * `desc` is filled as for mage_gemm's LayerNorm-consuming form (A = the 16-bit rows, bias = W beta + b, ln_stats, ln_colsum) with
 *   N = 3C, W = the folded in_proj rows [q; k; v] PACKED per group g of 4 heads (heads 4g .. 4g+3) as 384 rows:
 *            rows 384g .. 384g+255: head h of the group at rows 64h .. 64h+63 as [q_h | k_h], and within each 32 rows j the head dim
 *            (j%16/4)*8 + (j/16)*4 + j%4;
 *            rows 384g+256 .. 384g+383: the v rows 128g .. 128g+127, natural order;
 *            bias and ln_colsum in the same order;
 *   Y[yrow(m)][C] = the attention output rows, in desc->dtype, ldy >= C.
 * A 256-row tile of A is one frame: M % 256 == 0, a_off % 256 == 0, plain rows in (in_w == out_w; out_w >= M, or a_img_stride == out_w); the
 * output rows may be regrouped whole frames at a time (out_w % 256 == 0, y_img_stride, y_off) as mage_gemm regroups them.  axis 1 = H (a
 * sequence is a column of the frame), 2 = W (a row).  C % 128 == 0 (N % 384 == 0), K % 128 == 0 in [256, 1024], dtype MAGE_BF16 or MAGE_F16,
 * act none, no other epilogue stage.  `scale` is mage_attn_desc::scale.  Per output element the operations are those of the replaced pair
 * in their order: Y holds the same bits as mage_gemm followed by mage_attention.  Anything else: MAGE_EINVAL, nothing launched.
 * axis 0 = T, the temporal blocks of a full pass over clips of exactly 16 slots (causal: slot i attends to the slots <= i, mage_attn_desc::causal
 * with nq == nk == 16): rows [clip][slot][hw], and desc->out_w carries hw, the rows of one slot (in_w, a_img_stride and y_img_stride equal it:
 * the rows are described as groups of hw, nothing is regrouped).  hw % 16 == 0, M % (16 hw) == 0, a_off and y_off whole clips (multiples of
 * 16 hw), (15 hw + 16) * lda * 2 + 16384 < 2^32 (the kernel's 32-bit lane offsets inside a clip); a y_img_stride other than out_w (regrouped
 * output rows) is refused for this axis.  A tile is then 16 adjacent positions x the 16 slots of one clip; everything else as for axes 1 and 2,
 * the same bits as mage_gemm followed by mage_attention with q_axis_stride = kv_axis_stride = hw, outer strides 16 hw, causal. */
int mage_gemm_attn_fused_qkv(const mage_gemm_desc* desc, int32_t axis, float scale, void* stream);
/* The symbol of the kernel mage_gemm_attn_fused_qkv(desc, axis, ...) launches. */
int mage_gemm_attn_fused_qkv_kernel_name(const mage_gemm_desc* desc, int32_t axis, char* buf, int32_t len);

/* The decoder block's MLP, x + c_proj(QuickGELU(c_fc(ln_2(x)))) (mage_model.py:48-53), in ONE launch: the hidden rows never reach memory
 * (serves FlatAxialDecoder._pass on the 16-bit LayerNorm-fold path with the 16-bit stream).  Replaces the pair mage_gemm (c_fc: LayerNorm-consuming
 * form, QuickGELU) -> mage_gemm (c_proj: 16-bit residual added in the epilogue, optionally the LayerNorm partial sums) for C = 512, hidden = 2048
 * (csrc/gemm4m.hip: a workgroup owns 128 rows for both products and walks the hidden dimension 32 units at a time).
 *   x [.., ldx]: the 16-bit rows (row m of the call is row m + a_off); y [.., ldy]: the output rows m + y_off, y == x (in place, a_off == y_off) or
 *   another buffer; w1 [4C][ldw1] = gamma * W_fc, c1 [4C] = W_fc beta + b_fc, s1 [4C] = the row sums of w1, ln_stats [M][2] = (mean, rstd) per row;
 *   w2 [C][ldw2] = W_proj, b2 [C]; ln_part (may be null; [C/64][ln_part_rows][2], rows m + y_off) = mage_gemm's LayerNorm partial sums of the new rows.
 * dtype = w_dtype = y_dtype = MAGE_BF16 or MAGE_F16; C == 512; M > 0, M % 128 == 0; ldx, ldy >= C, ldw1 >= C, ldw2 >= 4C, all multiples of 8;
 * rows, weights and vectors 16-byte aligned, ln_stats and ln_part 8-byte aligned.  Per output element the operations are those of the replaced
 * pair in their order: y and ln_part hold the same bits.  Anything else: MAGE_EINVAL, nothing launched. */
int mage_mlp_fused(int32_t dtype, int32_t w_dtype, int32_t y_dtype, int64_t M, int32_t C, const void* x, int64_t ldx, int64_t a_off, void* y, int64_t ldy,
                   int64_t y_off, const void* w1, int64_t ldw1, const float* c1, const float* s1, const float* ln_stats, const void* w2, int64_t ldw2,
                   const float* b2, float* ln_part, int64_t ln_part_rows, void* stream);
/* The symbol of the kernel mage_mlp_fused(...) launches; refuses what mage_mlp_fused refuses, launches nothing. */
int mage_mlp_fused_kernel_name(int32_t dtype, int32_t w_dtype, int32_t y_dtype, int64_t M, int32_t C, const void* x, int64_t ldx, int64_t a_off, void* y,
                               int64_t ldy, int64_t y_off, const void* w1, int64_t ldw1, const float* c1, const float* s1, const float* ln_stats,
                               const void* w2, int64_t ldw2, const float* b2, float* ln_part, int64_t ln_part_rows, char* buf, int32_t len);

/* Given tokens over picked ones: no site in the reference (it generates every token after frame 0).  Serves MAGE.set_context and
 * batch['known_tokens'] (mage_amd/modules/mage_model.py: _generate_one, after each frame's pick and its log-probability / statistics
 * launches).
 * Row i in [0, rows) has c = i / group, j = i % group and uses index t = c*tok_group_stride + j + tok_off of tokens (int64) and of every
 * result buffer -- mage_token_logprob's token addressing, so a frame is forced where the pick kernels wrote it in either AR mode -- and
 * k = known[(c / known_clip_div)*known_group_stride + j + known_off] (int64; known_clip_div = N: a clip's N candidates share one row).
 *   k < 0   the slot is free: nothing at index t is written, in any buffer;
 *   k >= 0  tokens[t] = k, and each of the five result buffers that is non-null gets, at t, its value under a policy that takes the given
 *           token with certainty: logprob, policy_logprob, entropy, policy_entropy (fp32) 0, kept (int32) 1.  So clip totals
 *           (mage_clip_scores) are sums over the free tokens, and an importance ratio at a forced slot is 1.
 * k >= K is recorded for mage_check_device_errors and clamped to K - 1, as mage_token_logprob's out-of-range token is.
 * One thread per row, plain vector-memory stores, no LDS, no atomics; two rows that map to one index t must carry the same k.
 * tokens and known non-null, rows >= 0, group > 0, known_clip_div > 0, strides and offsets >= 0, K > 0: MAGE_EINVAL otherwise, nothing
 * launched.  rows == 0 is a no-op. */
int mage_apply_known_tokens(int64_t* tokens, int64_t rows, int64_t group, int64_t tok_group_stride, int64_t tok_off, const int64_t* known,
                            int64_t known_group_stride, int64_t known_off, int64_t known_clip_div, int32_t K, float* logprob,
                            float* policy_logprob, float* entropy, float* policy_entropy, int32_t* kept, void* stream);

/* mage_policy_loss / mage_policy_loss_anchored over the rows that were drawn, leaving out the rows that were given: no site in the reference.
 * Serves MAGE.policy_loss(given=) (mage_amd/modules/mage_train.py: PolicyHead with a 'given' argument) for tokens of a rollout that
 * continued given frames or filled in around given tokens (MAGE.rollout(context=, known_tokens=)).
 * The arguments are mage_policy_loss_anchored's plus given (uint8 [rows], one byte per row, non-zero: the row's token was given, not drawn; a
 * torch.bool tensor as it is) and norm (fp32 [1], device).  reference_logprob and kl may both be null: the plain rule of mage_policy_loss
 * (kl_coef must then be 0); both non-null: the anchored rule.
 *   A free row (given[i] == 0) is computed by the operations of the unmasked kernels (the same kernel instances, behind one wave-uniform
 *   branch): cut, logprob, entropy, kl and row_loss carry, bit for bit, what mage_policy_loss / mage_policy_loss_anchored write for that row.
 *   A given row is never read: not its logits (a NaN there does not show), not its advantage, behaviour or reference value; its token is not
 *   range-checked.  The forward call writes cut = 0 and logprob = entropy = kl = row_loss = +0; the backward call writes its dlogits row as +0
 *   with the stores the free rows use (fp32: 16 bytes, bf16: 8 bytes per lane).
 * summary[0..7) are the anchored call's seven means (under the plain rule the sixth and seventh are 0) taken OVER THE FREE ROWS, sum / n_free:
 * the same two-stage fixed-order fp64 reduction through the same per-device buffer -- a thread adds its free rows in ascending order -- so
 * the ordering rule between calls holds, and with nothing given the seven carry the unmasked call's bits.  summary[7] is the share of given
 * rows over `rows`.  The forward call also writes norm[0] = 1.0f / (float)n_free, the expression the unmasked backward call forms for
 * 1.0f / (float)rows; the backward call reads norm[0] in its place (dlogits of a free row = the unmasked rule with n_free for rows: its bits
 * depend on the row and on norm[0] alone).  Nothing is read on the host.
 * n_free == 0: norm[0] = 0, the seven means are +0, summary[7] = 1, dlogits is all zeros; no NaN anywhere.
 * The plain pair's argument rules; given non-null, norm non-null and 4-byte aligned, reference_logprob and kl both null or both non-null
 * (the backward call: reference_logprob alone decides), kl_coef == 0 without a reference: MAGE_EINVAL otherwise, nothing launched. */
int mage_policy_loss_masked(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                            int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature, int32_t top_k,
                            float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef, float* row_loss, float* logprob,
                            float* entropy, uint32_t* cut, float* kl, float* summary, float* norm, const uint8_t* given, void* stream);
int mage_policy_loss_masked_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, const uint32_t* cut,
                                float temperature, float clip_lo, float clip_hi, float entropy_coef, float kl_coef, const float* grad_out,
                                const float* norm, void* dlogits, int32_t dl_dtype, const uint8_t* given, void* stream);

/* The clipped surrogate with ONE importance ratio per group of consecutive rows -- a frame or a clip -- in place of one per token: the
 * length-normalised sequence ratio of GSPO (Zheng et al., "Group Sequence Policy Optimization", 2025) over the unit that is an action here
 * (all h*w tokens of a frame are drawn in one step).  No site in the reference.  Serves MAGE.policy_loss(ratio='frame' | 'clip')
 * (mage_amd/modules/mage_train.py: PolicyHead with a 'ratio_div' argument).
 * The arguments are mage_policy_loss_masked's -- here given MAY be null (every row free) -- plus ratio_div, group_logratio (fp32
 * [rows / ratio_div]) and group_count (int32 [rows / ratio_div]); the backward call takes mage_policy_loss_masked_bwd's plus ratio_div and
 * group_logratio as the forward call left it.
 *   Rows are ordered clip, frame, pixel; group g holds rows [g*ratio_div, (g+1)*ratio_div): ratio_div = h*w is a frame, (L-1)*h*w a clip.
 *   cut, logprob, entropy and kl come from mage_policy_loss_masked's row kernel instances, unchanged: they carry, bit for bit, what that
 *   call writes on the same inputs (without given and without a reference: what mage_policy_loss / mage_policy_loss_anchored write).
 *   A row COUNTS in its group if it is free (given[i] == 0, or no mask) and inside (logprob != -inf).  For a counted row
 *   d_i = logprob_i - b_i, one fp32 subtraction (the value the token rule feeds to expf).  Then
 *     n_g = the number of counted rows -> group_count[g];
 *     m_g = (float)((sum over the counted rows of (double)d_i) / n_g) -> group_logratio[g];   n_g == 0: m_g = +0.
 *   The sum is fp64 in a fixed order: a thread adds its rows in ascending order, the lanes meet in an xor butterfly, the waves are added in
 *   order.  A NaN d_i makes its group NaN.
 *   rho_g = expf(m_g).  Every counted row takes the token rule's clipped term with rho_g for its own rho, A = advantage[i / adv_div]:
 *     l_i = -min(rho_g A, clamp(rho_g, 1 - clip_lo, 1 + clip_hi) A) - entropy_coef H_i   [+ kl_coef kl_i under the anchored rule],
 *   the products and sums in fp64 and rounded once, as mage_policy_loss / mage_policy_loss_anchored form them.  An outside row and a given
 *   row are what they are in the masked call (+0).
 *   summary and norm: the masked call's eight values by the same two-stage fixed-order reduction through the same per-device buffer (so
 *   the ordering rule between calls holds); norm[0] = 1.0f / (float)n_free, n_free = rows without a mask.  summary[3], the clipped share,
 *   stays a share of ROWS: the rows of the groups whose gradient the clip switched off.
 *   Backward: rho_g = expf(group_logratio[g]) by the same operation, the same branch; g_i = -(A * rho_g) where the unclipped term is the
 *   active one, 0 otherwise, plus the anchored part as in mage_policy_loss_anchored_bwd; the rest of dlogits is
 *   mage_policy_loss_masked_bwd's formula.  Why g_i is not divided by n_g: the loss is (sum over rows of l_i) / n_free, the n_g counted rows
 *   of a group ALL carry the term -rho_g A, and d rho_g / d logprob_i = rho_g / n_g; so d(sum) / d logprob_i = n_g (-A rho_g / n_g) =
 *   -A rho_g -- the token rule's factor with rho_g substituted.
 *   Exact cases.  ratio_div == 1: (float)(double)d_i == d_i, so every output of both calls carries mage_policy_loss_masked's bits (without
 *   mask or reference: the plain / anchored pair's).  b_i with the bits of logprob_i on every counted row of a group: m_g = +0 and
 *   rho_g = 1 exactly.
 * Three steps on the stream: the row kernel, ONE group kernel (one wave per group up to 1024 rows, four groups per workgroup; one
 * workgroup of 1024 threads per group above), the two summary stages.  The group kernel reads logprob, b, given and the group's advantage,
 * writes group_logratio and group_count and rewrites row_loss of the counted rows.  No floating-point atomics, nothing read on the host:
 * two launches on the same inputs give the same bits.
 * The masked pair's argument rules (given aside); behaviour_logprob non-null; 1 <= ratio_div < 2^31; rows % ratio_div == 0;
 * adv_div % ratio_div == 0 (a group has one advantage); group_logratio, group_count and norm non-null and 4-byte aligned: MAGE_EINVAL
 * otherwise, nothing launched. */
int mage_policy_loss_grouped(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                             int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature, int32_t top_k,
                             float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef, float* row_loss, float* logprob,
                             float* entropy, uint32_t* cut, float* kl, float* summary, float* norm, const uint8_t* given, int64_t ratio_div,
                             float* group_logratio, int32_t* group_count, void* stream);
int mage_policy_loss_grouped_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                 int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, const uint32_t* cut,
                                 float temperature, float clip_lo, float clip_hi, float entropy_coef, float kl_coef, const float* grad_out,
                                 const float* norm, void* dlogits, int32_t dl_dtype, const uint8_t* given, int64_t ratio_div,
                                 const float* group_logratio, void* stream);

/* mage_token_logprob_bwd with given rows left out: no site in the reference.  Serves the backward pass of MAGE.preference_loss(given=).
 * mage_token_logprob_bwd's arguments plus given (uint8 [rows], as mage_policy_loss_masked's).  A given row is a row of c_i == 0: +0
 * throughout, its logits not read (a NaN there does not show); every other row carries mage_token_logprob_bwd's bits (one kernel template,
 * the mask behind a wave-uniform branch).  The forward side needs no kernel of its own: one mage_apply_known_tokens launch after
 * mage_token_logprob writes the given slots' 0, and mage_clip_scores then sums the free tokens.
 * mage_token_logprob_bwd's rules; given non-null: MAGE_EINVAL otherwise, nothing launched. */
int mage_token_logprob_bwd_masked(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* weight,
                                  int64_t weight_div, const float* grad_out, void* dlogits, int32_t dl_dtype, const uint8_t* given,
                                  void* stream);

/* Distillation loss: the KL divergence between a teacher's and a student's whole distribution over the K codes, per row: no site in the
 * reference (its only objective is the cross-entropy of one token per row).  Serves MAGE.distill_loss (mage_amd/modules/mage_train.py:
 * train_forward / train_backward with a DistillHead) against the logits MAGE.distill_targets returned.
 * Row i is the K fp32 student logits z at logits + i*ld and the K fp32 teacher logits at teacher + i*ld_t.  The rule for one row, in fp32,
 * with inv_t = (float)(1.0 / temperature) formed on the host:
 *   s_j = z_j * inv_t, t_j = teacher_j * inv_t (one multiply each: step 1 of the sampling rule); each row then goes through the
 *   arithmetic of mage_token_logprob's log-sum-exp (csrc/token_row.h: row_logsumexp): m = max_j (a NaN skipped), d_j = s_j - m,
 *   w_j = expf(d_j), Z = sum_j w_j, and sum_j w_j d_j for the entropy H = log Z - (sum_j w_j d_j) / Z; every sum in ONE order (a lane adds
 *   its own terms in register order with explicit roundings, the lanes meet in an xor butterfly).
 *   mode 0, forward KL(teacher || student):  row_kl = A / Z_T + (log Z_S - log Z_T),  A = sum_j w_T,j (d_T,j - d_S,j);
 *   mode 1, reverse KL(student || teacher):  the same with the two rows' roles exchanged.
 *   A term whose weight is 0 is not added (never 0 * inf).  A code to which the first distribution gives positive mass and the second
 *   gives a logit of -inf makes the row +inf.  The result is not clamped at 0: rounding may leave a small negative value.
 *   EQUAL ROWS GIVE EXACTLY +0: with the same bits in both rows every difference above is x - x = +0, A = +0 and row_kl = +0 + +0; the
 *   backward call's differences vanish the same way, so a model distilled against its own logits has a loss and a gradient of exactly 0
 *   (tests rely on this).  A NaN in either row makes row_kl NaN; so does a row of -inf only (inf - inf).
 * summary [5]: summary[0..4) are means over the free rows of row_kl, of the teacher's entropy and of the student's entropy (both at the
 *   given temperature) and of 1[argmax_j z_j == argmax_j teacher_j] (on the raw logits, mage_argmax's rule: NaNs skipped, the first maximum
 *   wins); summary[4] is the share of given rows over `rows`.  Each is a fixed-order fp64 sum, rounded once: workgroup b of the one
 *   row-reading launch owns the row quads b, b + G, ... (G = min(ceil(rows / 4), 16384)), a wave adds its rows in ascending order, the four
 *   waves meet in order; a second launch adds the G partial sums the same way through a per-device buffer of the library (calls of
 *   mage_distill_loss on one device must be ordered: one stream, or events).  The geometry depends on rows alone: two launches give the
 *   same bits, and there are no floating-point atomics.
 * norm[0] = 1.0f / (float)n_free (0 when every row is given: the four means are then +0 and nothing is NaN), the backward call's input.
 * given (uint8 [rows], may be null: every row free; a torch.bool tensor as it is): mage_policy_loss_masked's contract.  A given row is
 *   never read in either buffer (a NaN there does not show); its row_kl is +0 and its dlogits row is +0, written with the stores the free
 *   rows use.  A free row's bits depend on its two rows alone.
 * mage_distill_loss_bwd: dlogits [rows, K] contiguous, MAGE_F32 or MAGE_BF16, the gradient of grad_out[0] * summary[0] with respect to
 *   the student's logits.  With c = grad_out[0] * norm[0] * inv_t and p = w * (1 / Z) recomputed by the forward call's operations:
 *   mode 0:  c (p_S,j - p_T,j);    mode 1:  c p_S,j ((log p_S,j - log p_T,j) - row_kl_i), 0 where p_S,j == 0, with
 *   log p_S,j - log p_T,j = (d_S,j - d_T,j) - (log Z_S - log Z_T).  A row whose row_kl is not finite (+inf: the second distribution
 *   excludes a code the first one holds; NaN) is written as +0 throughout, without being read: such a row has no finite gradient, and
 *   zeros let the rest of the batch train (the forward call's summary[0] still shows the inf or NaN).
 * Both rows of a pair are read once with 16-byte loads; outputs are written once (fp32: 16 bytes, bf16: 8 bytes per lane and chunk).
 * mage_token_stats' size rules on both buffers: rows > 0, K % 4 == 0, 0 < K <= MAGE_SAMPLE_MAX_K, ld and ld_t % 4 == 0 and >= K, logits,
 * teacher and dlogits 16-byte aligned; temperature finite and > 0; mode 0 or 1; row_kl, summary, norm, grad_out non-null and 4-byte
 * aligned: MAGE_EINVAL otherwise, nothing launched. */
int mage_distill_loss(const float* logits, int64_t rows, int32_t K, int64_t ld, const float* teacher, int64_t ld_t, float temperature,
                      int32_t mode, const uint8_t* given, float* row_kl, float* summary, float* norm, void* stream);
int mage_distill_loss_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const float* teacher, int64_t ld_t, float temperature,
                          int32_t mode, const uint8_t* given, const float* row_kl, const float* grad_out, const float* norm, void* dlogits,
                          int32_t dl_dtype, void* stream);

/* Supervised cross entropy of one target code per row with class weights, label smoothing, a z-loss and a mask, and what the row predicts:
 * the reference's objective is F.cross_entropy(logits, target) with no option (mage_model.py:618, mage_cross_entropy here); this is
 * F.cross_entropy(weight=, label_smoothing=, ignore_index=) per row, plus the z-loss of PaLM (Chowdhery et al. 2022: zeta * log^2 Z) and the
 * rank of the target.  Serves MAGE.forward after MAGE.set_loss or with batch['given'] (mage_amd/modules/mage_train.py: SupervisedHead) and
 * MAGE.evaluate.
 * Row i is the K fp32 logits z at logits + i*ld and the target y = target[i] (int64; outside [0, K): recorded for
 * mage_check_device_errors as mage_token_logprob's bad token is, and clamped).  w = class_weight (fp32 [K], 16-byte aligned; null: all
 * ones), eps = label_smoothing, zeta = z_loss; c1 = (float)(1 - eps) and c2 = (float)(eps / K) are formed on the host in fp64.  The rule for
 * one free row, in fp32, one wave per row in csrc/token_row.h's layout:
 *   mx, Z       row_logsumexp's maximum and sum, so lse = mx + logf(Z) (row_lse) carries mage_token_logprob's bits;
 *   row_nll     = -(z_y - lse): THE NEGATION OF mage_token_logprob's VALUE ON THE SAME ROW, BIT FOR BIT (the same difference with its sign
 *               turned, so a token that holds all the mass gives -0 where the log-probability is +0);
 *   smooth      = sum_{k < K} w_k (lse - z_k), formed only when eps > 0: a lane adds its own codes in register order, each step one
 *               fma(w_k, lse - z_k, sum) on the rounded difference, and the lanes meet in the xor butterfly;
 *   row_loss    = fma(c2, smooth, (c1 w_y) nll) with eps > 0, (c1 w_y) nll (two products) otherwise: with eps = 0 and no weights row_loss
 *               has row_nll's bits.  The z-loss term zeta lse^2 is NOT in row_loss: it enters summary[0] and the gradient only;
 *   rank        = #{j < K : z_j > z_y} + #{j < y : z_j == z_y} (int32; may be null), counted exactly by ballots on the sampler's keys
 *               (sample_key at inv_t = 1: -0 == +0, a NaN logit is never above), so rank == 0 exactly where mage_argmax picks y; a NaN
 *               z_y gives rank K.
 *   Edges follow F.cross_entropy, nothing is clamped: a -inf logit with eps > 0 makes row_loss +inf (NaN if its weight is 0: 0 * inf, as
 *   in torch), z_y = -inf makes row_nll +inf, a NaN logit or a row of -inf only makes row_lse, row_nll and row_loss NaN.
 * given (uint8 [rows], may be null: every row free; a torch.bool tensor as it is): mage_distill_loss's contract.  A given row is never read
 *   (a NaN there does not show, its target is not range-checked); its row_loss, row_nll and row_lse are +0, its rank 0 and its dlogits row
 *   +0, written with the stores the free rows use.  A free row's bits depend on the row, its target and the weights alone.
 * norm [2]: norm[0] = (float)(1 / sum_free w_y), norm[1] = (float)(1 / n_free), each 0 when its sum is 0 (the means are then +0 and nothing
 *   is NaN); sum_free w_y is an fp64 sum and n_free an exact count from the same pass.  Without class weights norm[0] == norm[1] ==
 *   1.0f / (float)n_free.
 * summary [5], each rounded once from fp64:
 *   [0] (sum row_loss) / (sum_free w_y) + zeta (sum lse^2) / n_free: the objective, F.cross_entropy's 'mean' reduction plus the z-loss
 *       (the z term is formed only when zeta > 0);
 *   [1] the mean of row_nll over the free rows, unweighted;  [2] the share of free rows with rank == 0;  [3] the mean of lse^2;
 *   [4] the share of given rows over `rows`.
 *   The sums are fp64 in ONE order, mage_distill_loss's two-launch geometry: workgroup b of the row-reading launch owns the row quads b,
 *   b + G, ... (G = min(ceil(rows / 4), 16384)), a wave adds its rows in ascending order, the four waves meet in order; a second launch adds
 *   the G partial sums the same way through a per-device buffer of the library (calls of mage_token_xent on one device must be ordered: one
 *   stream, or events).  The geometry depends on rows alone: two launches give the same bits; no floating-point atomics.
 * mage_token_xent_bwd: dlogits [rows, K] contiguous, MAGE_F32 or MAGE_BF16, the gradient of grad_out[0] * summary[0].  With g = grad_out[0],
 *   p_k = expf(z_k - mx) * (1 / Z) recomputed by the forward call's operations and W = sum_k w_k in smooth's order ((float)K without
 *   weights):
 *     d_k = g [ norm[0] ((1 - eps) w_y (p_k - 1[k = y]) + (eps / K) (W p_k - w_k)) + norm[1] 2 zeta lse p_k ],   evaluated as
 *     B = (g norm[0]) (c1 w_y),  C = (g norm[0]) c2,  A = fma((g norm[1]) (2 zeta), lse, fma(C, W, B)),
 *     d_k = fma(-C, w_k, fma(A, p_k, -B 1[k = y]))        (the C and zeta steps only with eps > 0 and zeta > 0).
 *   Rows are not special-cased: a NaN row's gradient is NaN.  A row is read once with 16-byte loads and written once (fp32: 16 bytes,
 *   bf16: 8 bytes per lane and chunk), with vector stores.
 * Registers (VGPRs per lane of the NV = 4, 8, 16, 32, 64 instances; no instance has scratch or a spill): forward 58, 60, 77, 109, 171
 *   without smoothing and 58, 65, 89, 150, 256 + 14 AGPRs with it (a lane keeps its NV class weights across the rows of its wave);
 *   backward (fp32) 22, 31, 41, 61, 101 without smoothing and 23, 33, 51, 87, 159 with it.
 * mage_token_stats' size rules (rows > 0, K % 4 == 0, 0 < K <= MAGE_SAMPLE_MAX_K, ld % 4 == 0 and >= K, logits 16-byte aligned); target
 * non-null and 8-byte aligned; class_weight 16-byte aligned; label_smoothing in [0, 1); z_loss finite and >= 0; row_loss, row_nll,
 * row_lse, summary, norm, grad_out non-null and 4-byte aligned; dlogits 16-byte aligned, dl_dtype MAGE_F32 or MAGE_BF16: MAGE_EINVAL
 * otherwise, nothing launched. */
int mage_token_xent(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* target, const float* class_weight,
                    float label_smoothing, float z_loss, const uint8_t* given, float* row_loss, float* row_nll, float* row_lse, int32_t* rank,
                    float* summary, float* norm, void* stream);
int mage_token_xent_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* target, const float* class_weight,
                        float label_smoothing, float z_loss, const uint8_t* given, const float* grad_out, const float* norm, void* dlogits,
                        int32_t dl_dtype, void* stream);

/* Per-code counts and row sums of a quantised batch: no site in the reference (its codebook moves by the gradient of
 * mse(z_q_x, z_e_x.detach()) alone and nothing reports its use).  Serves VectorQuantizedVAE.set_codebook_update('ema') (every training
 * forward, right after mage_vq_nearest) and VectorQuantizedVAE.code_usage (mage_amd/modules/vqvae_model.py).
 * ids int64 [rows]; z fp32 rows [rows, ldz], of which the first D columns are read.
 *   counts (int64 [K])    counts[k] = the number of rows with ids == k, exact (integer adds);
 *   sums   (fp32 [K, D])  sums[k, :] = the sum of those rows of z.
 * z and sums may both be null: the counts-only form (D and ldz are then not looked at).  An id outside [0, K) is recorded for
 * mage_check_device_errors (as mage_token_logprob's bad token is) and counted nowhere: neither in counts nor in sums.
 * THE SUMS HAVE ONE ORDER.  The rows are cut into n_chunk = min(64, ceil(rows / 4096)) chunks of R = ceil(rows / n_chunk) rounded up to a
 * multiple of 8 rows: chunk c owns rows [c R, min(rows, (c + 1) R)) -- a function of `rows` alone.  Inside a chunk the rows of code k are
 * added to +0 one after the other in ascending row order, in fp32 (one LDS add per row, issued by the one wave that owns the channel);
 * sums[k, d] is then +0 + chunk 0's sum + chunk 1's sum + ..., chunks ascending, in fp32.  There is no floating-point atomic between
 * waves: two launches give the same bits, and the bits of sums[k, :] depend on the positions and values of code k's rows alone (the rows
 * of other codes may be permuted among themselves).  Error: a sum of n_k terms plus the n_chunk stage,
 * |err| <= (n_k + n_chunk) 2^-24 sum |z|.
 * scratch: 16-byte aligned, at least n_chunk * K * (D + 1) * 4 bytes (n_chunk * K * 4 for the counts-only form): the chunks' partial
 * tables, written before they are read.
 * Geometry: mage_embedding_bwd's deterministic form (a workgroup owns a chunk and a channel slice, an LDS table of the slice, its eight
 * waves split the slice's channels) with any D % 4 == 0, a 32-channel slice above 512 codes (K x slice x 4 B within 128 KiB), a row stride,
 * and one more workgroup per chunk that counts; a second launch adds the chunks.
 * rows in [1, 2^31), K in [1, 1024], with sums D % 4 == 0, D in [4, 1024], ldz >= D; ids and counts 8-byte, z 4-byte, sums and scratch
 * 16-byte aligned; scratch_bytes as above: MAGE_EINVAL otherwise, nothing launched. */
int mage_code_stats(const int64_t* ids, const float* z, int64_t rows, int32_t D, int64_t ldz, int32_t K, int64_t* counts, float* sums,
                    void* scratch, int64_t scratch_bytes, void* stream);

/* Exponential-moving-average codebook update (van den Oord et al. 2017, appendix A.1) with Laplace smoothing, the restart of dead codes
 * from encoder rows, and usage statistics: no site in the reference.  Serves VectorQuantizedVAE.set_codebook_update('ema'), after
 * mage_code_stats on the same (ids, z).
 * One launch updates in place codebook (fp32 [K, D]: e_k), cluster_size (fp32 [K]: N_k) and embed_sum (fp32 [K, D]: m_k) from counts
 * (int64 [K]) and sums (fp32 [K, D]).  With g = (double)decay, every right-hand side evaluated in fp64 from the fp32 (int64) operands, each
 * operation rounded on its own (no contraction), and rounded once to fp32 where it is stored:
 *   1. N_k' = (float)(g N_k + (1 - g) counts[k]);
 *   2. m_k' = (float)(g m_k + (1 - g) sums[k]), elementwise;
 *   3. n = sum_k N_k' over the stored fp32 values, in fp64, k ascending from 0.0;
 *   4. Nhat_k = (N_k' + eps) / (n + K eps) * n                                   (fp64, not stored);
 *   5. e_k = (float)(m_k' / Nhat_k).
 * Every workgroup derives n itself from the K values in that order: no cross-workgroup reduction, no floating-point atomic, the same bits
 * from every launch.  (One integer ticket orders the write of the K new sizes after every workgroup's read of the old ones: the workgroup
 * that arrives last writes them from its own copy.  No value passes between workgroups.  The ticket is one word per device: calls of
 * mage_codebook_ema on one device must be ordered -- one stream, or events.)
 * Restart, after steps 1 to 5, when restart_below > 0: a code with N_k' < restart_below (fp32 compare) is dead and takes an encoder row,
 *   r_k = ((uint64)hash32(seed * 0x9e3779b97f4a7c15 + step * K + k) * rows) >> 32   (uint64 wrap-around; hash32 and the seed multiplier
 *         are the dropout masks' and the sampler's: csrc/common.h),
 *   e_k = z[r_k, :D] copied bit for bit, N_k = restart_size, m_k = (float)((double)restart_size * z[r_k]).
 * Two dead codes may draw the same row: the quantiser's first-minimum rule then never picks the second one, which stays dead and draws
 * again at the next step (`step` changes the counter).  z (fp32 rows [rows, ldz]), rows and ldz are looked at only when restart_below > 0.
 * stats (fp64 [4], device, written by one thread): [0] perplexity exp(-sum_k p_k ln p_k), p_k = counts[k] / sum counts, k ascending in
 * fp64, a zero count adding 0 (never 0 * inf); [1] the number of codes with counts[k] > 0; [2] the number of codes restarted; [3] sum counts.
 * sum counts == 0 (every id was invalid): the state is left untouched, perplexity is NaN, the other three are 0.
 * K in [1, 1024]; D % 4 == 0, D in [4, 1024]; decay in [0, 1), eps > 0, restart_below >= 0, restart_size > 0, all finite; with
 * restart_below > 0 z non-null, rows in [1, 2^31), ldz >= D; codebook, embed_sum, sums 16-byte, counts and stats 8-byte, cluster_size and z
 * 4-byte aligned: MAGE_EINVAL otherwise, nothing launched.  Nothing is read on the host. */
int mage_codebook_ema(float* codebook, float* cluster_size, float* embed_sum, const int64_t* counts, const float* sums, const float* z,
                      int64_t rows, int64_t ldz, int32_t K, int32_t D, float decay, float eps, float restart_below, float restart_size,
                      uint64_t seed, uint64_t step, double* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
