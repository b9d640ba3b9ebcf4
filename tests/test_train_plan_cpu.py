"""CPU: the launch plan of the training path -- mage_train.train_forward / train_backward (mage_train_prior behind them) and vqvae_train's
vq_train_* / vq8_train_* pairs: every call into mage_amd.ops, in order, with its arguments and with which buffer goes where -- against
tests/golden/train_plan.json, which tools/gen_train_plan.py recorded from the parent of the commit that gave the three training modules one
weight-gradient helper and one Linear backward.  The modules are pure orchestration: as long as the plan is the recorded one, the GPU work is
the same launch for launch.  No GPU, no library: the real ops functions run on CPU tensors over a library that launches nothing
(tools/gen_train_plan.py says what is recorded, how a tensor is normalised, and lists the cases).

Per case: the names of the ops calls issued from the three training modules with a digest of each call, the number of all calls, and the sha256
of the whole normalised trace (nested calls and the frozen first stage's included).  On a mismatch the first differing call is printed in full."""
import json
import os

import pytest

from tools import gen_train_plan as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "train_plan.json")) as f:
    GOLDEN = json.load(f)
_PLAN = []


def _plan():
    if not _PLAN:
        _PLAN.extend(gen.plan(gen.load(ROOT)))
    return _PLAN


def test_the_cases_are_the_recorded_ones():
    got, _ = _plan()
    assert sorted(got) == sorted(GOLDEN) == sorted(gen.specs())
    # the fixture itself shows that the cases take the routes they were chosen for
    n = lambda case, op: sum(o.split(":")[0] == op for o in GOLDEN[case]["ops"])       # noqa: E731
    assert n("b-bf16-train", "gemm_tn") > 0 and n("c-b-wgrad_transpose", "gemm_tn") == 0 and n("a-bf16-train", "gemm_tn") == 0
    assert n("c-b-wgrad_transpose", "transpose_colsum") > n("b-bf16-train", "transpose_colsum")
    assert n("c-b-no_taps", "cast") > n("b-bf16-train", "cast")                          # the padded-frame buffer is filled without ops.cast
    assert n("a-bf16-train", "dropout_add_layernorm") > 0 and n("c-a-train_emit=False", "dropout_add_layernorm") == 0
    assert n("c-a-train_emit=False", "dropout_add") > n("a-bf16-train", "dropout_add")
    for eval_case in ("a-bf16-eval", "a-fp32-eval"):
        assert n(eval_case, "dropout") == n(eval_case, "dropout_add") == n(eval_case, "dropout_add_layernorm") == 0
    assert n("a-fp32-train", "dropout_add") > 0 and n("a-fp32-train", "cast") == 0
    # train_dual=False: one act and one act_bwd per decoder block where the default has the dual / QUICKGELU_GRAD epilogues
    assert n("c-a-train_dual=False", "act_bwd") == n("a-bf16-train", "act_bwd") + 3
    assert n("c-a-train_dual=False", "act") == n("a-bf16-train", "act") + 3
    assert n("c-a-train_dual=False", "gemm") == n("a-bf16-train", "gemm")
    assert n("a-bf16-train", "split") > 0 and n("c-a-train_enc_split=False", "split") == 0 and n("a-fp32-train", "split") == 0
    assert GOLDEN["c-a-train_f32_branch=True"]["sha256"] != GOLDEN["a-bf16-train"]["sha256"]
    for d in ("d-bf16-train", "d-fp32-eval"):
        assert n(d, "reparam_kl") == n(d, "reparam_kl_bwd") == n(d, "adain_bwd") == 1 and n(d, "cross_entropy") == 1
    assert n("f-d-policy-noise", "adain_bwd") == 1 and n("f-d-policy-noise", "reparam_kl_bwd") == 0
    for e in ("e-bf16-train", "e-fp32-eval", "e-bf16-train-nospeed", "e-fp32-eval-nospeed"):
        assert n(e, "mse") == n(e, "mse_bwd") == n(e, "groupnorm_act") == 1 and n(e, "cross_entropy") == 0
        assert n(e, "add_scaled_rowvec") == (0 if e.endswith("nospeed") else 1)
    assert n("f-policy", "policy_loss") == n("f-policy", "policy_loss_bwd") == n("f-policy-all", "policy_loss_bwd") == 1
    assert GOLDEN["f-policy"]["sha256"] != GOLDEN["f-policy-all"]["sha256"]
    assert n("f-preference", "preference_loss") == n("f-preference-given", "preference_loss") == 1
    assert n("f-preference", "apply_known_tokens") == 0 and n("f-preference-given", "apply_known_tokens") == 1
    assert n("f-distill", "distill_loss") == n("f-distill", "distill_loss_bwd") == 1
    assert not [o for o in GOLDEN["f-logits"]["ops"] if "_bwd" in o or o.startswith("transpose")]
    assert n("g-f4-1ch", "bn_backward") > 0 and n("g-f8-3ch", "bn_backward") == 0 and n("g-f8-3ch", "maxpool2_bwd") == 3
    assert GOLDEN["g-f4-1ch"]["sha256"] != GOLDEN["g-f4-3ch"]["sha256"]


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_launch_plan_is_the_recorded_one(case):
    got, full = _plan()
    want, have = GOLDEN[case], got[case]
    if have != want:
        print(f"{case}: {len(have['ops'])} of {have['n_calls']} calls from the training modules (recorded: {len(want['ops'])} of {want['n_calls']})")
        for i, (h, w) in enumerate(zip(have["ops"] + [None] * len(want["ops"]), want["ops"] + [None] * len(have["ops"]))):
            if h != w:
                print(f"first differing call: #{i}: recorded {w}, now {h}:")
                print(json.dumps(full[case][i], sort_keys=True) if i < len(full[case]) else "(no such call now)")
                break
        else:
            print("the calls from the training modules are the recorded ones: a call beneath them (inside ops, or the first stage's) differs")
    assert have["ops"] == want["ops"]
    assert have["n_calls"] == want["n_calls"]
    assert have["sha256"] == want["sha256"]
