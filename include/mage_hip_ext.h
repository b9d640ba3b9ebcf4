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

#ifdef __cplusplus
}
#endif
#endif
