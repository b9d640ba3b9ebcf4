"""CPU: the launch plan of FlatAxialDecoder (_run, _inc_begin + _inc_step), MAEncoder._run and TransformerTextEncoder.forward -- every call into
mage_amd.ops, in order, with its arguments and with which buffer goes where -- against tests/golden/decoder_plan.json, which
tools/gen_decoder_plan.py recorded from the parent of the commit that merged the decoder's two passes.  The passes are pure orchestration: as
long as the plan is the recorded one, the GPU work is the same launch for launch.  No GPU, no library: the ops are recorders on CPU tensors
(tools/gen_decoder_plan.py says what is recorded, how a tensor is normalised, and lists the cases).

Per case: the routes the pass took (_fold, _stream_bf16, _stats_inline, _qkv_fuse, _mlp_fuse, _attn_split), the op names with a digest of each
call, and the sha256 of the whole normalised trace.  On a mismatch the first differing call is printed in full."""
import json
import os

import pytest

from tools import gen_decoder_plan as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "decoder_plan.json")) as f:
    GOLDEN = json.load(f)
_PLAN = []


def _plan():
    if not _PLAN:
        _PLAN.extend(gen.plan(*gen.load(ROOT)))
    return _PLAN


def test_the_cases_are_the_recorded_ones():
    got, _ = _plan()
    assert sorted(got) == sorted(GOLDEN)
    # the fixture itself shows that the cases take the routes they were chosen for
    took = lambda case, name: {v for n, v in GOLDEN[case]["routes"] if n == name}       # noqa: E731
    assert took("a-bf16/run", "_fold") == {False} and took("b-bf16/run", "_fold") == {True}
    assert took("b-bf16/run", "_qkv_fuse") == {True} and took("b-bf16/inc", "_qkv_fuse") == {False} and took("c-bf16/run", "_qkv_fuse") == {False}
    assert took("b-f16/run", "_mlp_fuse") == {True} and took("c-f16/run", "_mlp_fuse") == {False}
    assert took("d-bf16/inc", "_stats_inline") == {True} and took("b-bf16/inc", "_stats_inline") == {False}
    assert took("e-stream32-bf16/run", "_stream_bf16") == {False} and took("e-nofold-bf16/run", "_fold") == {False}
    assert took("b-f16x3/inc", "_attn_split") == {True} and took("f-attn32-f16x3/inc", "_attn_split") == {False}
    assert took("b-bf16x3/run", "_attn_split") == {False}


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_launch_plan_is_the_recorded_one(case):
    got, full = _plan()
    want, have = GOLDEN[case], got[case]
    if have != want:
        print(f"{case}: routes {have['routes']} (recorded: {want['routes']}); {len(have['ops'])} calls (recorded: {len(want['ops'])})")
        for i, (h, w) in enumerate(zip(have["ops"] + [None] * len(want["ops"]), want["ops"] + [None] * len(have["ops"]))):
            if h != w:
                print(f"first differing call: #{i}: recorded {w}, now {h}:")
                print(json.dumps(full[case][i], sort_keys=True) if i < len(full[case]) else "(no such call now)")
                break
    assert have["routes"] == want["routes"]
    assert have["ops"] == want["ops"]
    assert have["sha256"] == want["sha256"]
