"""graph_step.plan_refusal: whether a recorded step may replay as a launch plan is a pure function of the captured
hipGraph's node counts and of what the plan recorded — the three refusals, their texts and their precedence."""
from rec_pangu_amd.graph_step import plan_refusal


def test_plan_refusal_messages_and_precedence():
    # (kernel nodes, other nodes, the plan's launches, the streams they were issued on)
    assert plan_refusal(36, 0, 36, 1) is None
    assert plan_refusal(36, 2, 36, 1) == "the captured step holds 2 non-kernel node(s) (memset / memcpy)"
    assert plan_refusal(38, 0, 36, 1) == "the captured step holds 38 kernel nodes, 36 of them library launches"
    assert plan_refusal(36, 0, 36, 2) == "the library launches were issued on 2 streams"
    # two conditions at once: non-kernel nodes before the kernel count, the kernel count before the streams
    assert plan_refusal(38, 1, 36, 3) == "the captured step holds 1 non-kernel node(s) (memset / memcpy)"
    assert plan_refusal(38, 0, 36, 3) == "the captured step holds 38 kernel nodes, 36 of them library launches"
