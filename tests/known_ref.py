"""The rule of mage_apply_known_tokens (include/mage_hip_ext.h) restated in numpy, and constrained generation (MAGE.set_context,
batch['known_tokens']) restated on the CPU oracle's functions, for the CPU and GPU tests of given frames and tokens.

apply_known: row i has c = i // group, j = i % group, token index t = c*tok_group_stride + j + tok_off and known index
(c // known_clip_div)*known_group_stride + j + known_off.  A negative known value leaves everything at t as it is; any other value is stored
at tokens[t] (clamped to K - 1 when it is >= K) and every result buffer given gets the certain policy's value at t: log-probabilities and
entropies 0, kept 1.
"""
import numpy as np
import torch

from oracle import mage_oracle as O

RESULTS = (("logprob", np.float32, 0.0), ("policy_logprob", np.float32, 0.0), ("entropy", np.float32, 0.0),
           ("policy_entropy", np.float32, 0.0), ("kept", np.int32, 1))


def indices(rows, group, tok_group_stride, tok_off, known_group_stride, known_off, known_clip_div):
    """(token index, known index) of every row, int64 [rows] each."""
    i = np.arange(rows, dtype=np.int64)
    c, j = i // group, i % group
    return c * tok_group_stride + j + tok_off, (c // known_clip_div) * known_group_stride + j + known_off


def apply_known(tokens, known, *, rows, group, K, tok_group_stride=None, tok_off=0, known_group_stride=None, known_off=0, known_clip_div=1,
                **results):
    """Returns (tokens after the launch, {name: result buffer after the launch}, the number of values >= K met); the inputs (flat arrays,
    addressed from their first element) are not modified.  results: any of logprob, policy_logprob, entropy, policy_entropy (fp32), kept
    (int32); None entries are passed through as None."""
    tok_group_stride = group if tok_group_stride is None else tok_group_stride
    known_group_stride = group if known_group_stride is None else known_group_stride
    tokens = np.array(tokens, np.int64).reshape(-1)
    known = np.asarray(known, np.int64).reshape(-1)
    out = {n: None if b is None else np.array(b).reshape(-1) for n, b in results.items()}
    t, kix = indices(rows, group, tok_group_stride, tok_off, known_group_stride, known_off, known_clip_div)
    k = known[kix]
    forced = k >= 0
    bad = int((k >= K).sum())
    tokens[t[forced]] = np.minimum(k[forced], K - 1)
    for name, dt, val in RESULTS:
        b = out.get(name)
        if b is not None:
            assert b.dtype == dt
            b[t[forced]] = val
    return tokens, out, bad


# ---------------------------------------------------------------------------------------------------- constrained generation on the oracle
def merged_known(ctx_tokens, known, k, Lm1):
    """known int64 [B, L-1, h, w] (or None) with the given frames 1 .. k-1 (ctx_tokens int64 [B, k, h, w]) merged into slots 0 .. k-2."""
    B, _, h, w = ctx_tokens.shape
    kn = torch.full((B, Lm1, h, w), -1, dtype=torch.int64) if known is None else known.clone()
    kn[:, :k - 1] = ctx_tokens[:, 1:k]
    return kn


def teacher_forced_logits(sd, ctx0, text, speed, gen):
    """The oracle's logits [B, L-1, h, w, K] (fp32, no grad) for frames 1 .. L-1 given frame 0's tokens ctx0 [B, h, w] and the tokens
    gen [B, L-1, h, w] of the frames before each: the decoder is causal along time, so row i is what a generation that has produced
    gen[:, :i] sees when it picks frame i + 1."""
    Lm1 = gen.shape[1]
    with torch.no_grad():
        feats = O._frame_features(sd, torch.cat([ctx0[:, None], gen[:, :Lm1 - 1]], 1))
        return O.flat_axial_decoder(sd, "generate_model.", O.motion_anchor(sd, ctx0, text, speed), feats)


def generate(sd, batch, L, k=1, known=None, ctx_tokens=None):
    """Greedy constrained generation on the oracle's own trajectory: (tokens [B, L-1, h, w], the merged known tensor, the logits each frame
    was picked from [B, L-1, h, w, K]).  Frames 0 .. k-1 are given (encoded from batch['images'] unless ctx_tokens gives them)."""
    images = batch["images"]
    B, Lm1 = images.shape[0], L - 1
    if ctx_tokens is None:
        with torch.no_grad():
            ctx_tokens = torch.stack([O.vqvae_encode(sd, "first_stage_model.", images[:, j]) for j in range(k)], 1)
    kn = merged_known(ctx_tokens, known, k, Lm1)
    tok0 = ctx_tokens[:, 0]
    with torch.no_grad():
        ma = O.motion_anchor(sd, tok0, batch["text"], batch.get("speed"))
        cur = tok0[:, None].repeat(1, L, 1, 1)                                      # slot j: frame j; future slots hold frame 0
        picked = []
        for i in range(Lm1):
            logits = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, cur[:, :Lm1]))[:, i]
            picked.append(logits)
            tok = logits.max(-1)[1]
            cur[:, i + 1] = torch.where(kn[:, i] >= 0, kn[:, i], tok)
    return cur[:, 1:].clone(), kn, torch.stack(picked, 1)


def check_against_oracle(gen, kn, logits, tol, what=""):
    """gen int64 [B, L-1, h, w] (the tokens under test), kn the merged known tensor, logits the oracle's [B, L-1, h, w, K] teacher-forced on
    gen.  Forced slots hold the given tokens exactly; every free token is the oracle's argmax wherever its top-2 margin exceeds tol; the free
    positions at or under tol are at most 1 % of the free tokens.  Returns (free tokens, free positions at or under tol, free tokens that
    differ from the argmax)."""
    gen, kn = np.asarray(gen), np.asarray(kn)
    g = np.asarray(logits, np.float64)
    forced = kn >= 0
    assert np.array_equal(gen[forced], kn[forced]), f"{what}: a forced slot does not hold its given token"
    top2 = np.sort(g, axis=-1)[..., -2:]
    margin = top2[..., 1] - top2[..., 0]
    bad = (gen != g.argmax(-1)) & ~forced
    free = int((~forced).sum())
    under = int(((margin <= tol) & ~forced).sum())
    print(f"{what}: {free} free tokens ({int(forced.sum())} forced), {int(bad.sum())} differ from the oracle's argmax, "
          f"{under} free positions with a top-2 margin <= tol {tol:.1e}")
    assert not (bad & (margin > tol)).any(), f"{what}: {int((bad & (margin > tol)).sum())} free tokens differ where the margin exceeds {tol}"
    assert under <= free // 100, f"{what}: {under} of {free} free positions at or under tol"
    return free, under, int(bad.sum())


def mixed_known(ctx0, frame_tokens, Lm1=5, K=64):
    """The mixed pattern of the tests, for 4 clips of 16 x 16 tokens and L = 6: clip 0 free; clip 1 slot 0 = its own frame-1 tokens; clip 2
    rows 0..7, columns 4..11 of every slot held at the frame-0 tokens; clip 3 a quarter of random slots at random tokens and slot 4 = its
    frame-5 tokens.  ctx0 int64 [4, 16, 16]: the frame-0 tokens; frame_tokens int64 [4, L, 16, 16]: the encoder's tokens of every frame."""
    known = torch.full((4, Lm1, 16, 16), -1, dtype=torch.int64)
    known[1, 0] = frame_tokens[1, 1]
    known[2, :, 0:8, 4:12] = ctx0[2, 0:8, 4:12]
    g = torch.Generator().manual_seed(5)
    sc = torch.rand(5, 16, 16, generator=g) < 0.25
    rnd = torch.randint(0, K, (5, 16, 16), generator=g)
    known[3][sc] = rnd[sc]
    known[3, 4] = frame_tokens[3, 5]
    return known
