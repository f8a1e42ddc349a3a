"""The fixed conv policy is pinned: before any forward at a batch size, fr_debug_plan reports the policy's kernel per
conv (csrc/convs.cpp default_choice), which depends on the plan and the shapes alone.  The plan text of every model
at B = 1, 8 and 256, with FR_OPT_BATCH_INVARIANT off and on, must equal the recorded one (tests/golden/plans/,
written by tests/conv_policy_plans.py at the commit before the conv selection moved into its table).  No embed call:
only the load-time packers run on the device.

The plan text does not show the plan's tensors, so their list (name, H, W, C, storage dtype, in plan order) is pinned
the same way (<name>_tensors.json, recorded at the commit before the plan builders moved into csrc/plan.cpp)."""
import pytest

from tests import conv_policy_plans as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(P.MODELS))
def test_fixed_policy_plan_matches_recorded(gpu, name):
    want = P.golden(name)
    got = P.plans(name)
    assert sorted(got) == sorted(want)
    assert len(want) == (3 if name.endswith("fp8") else 6)
    for key in want:
        assert any(l.startswith("conv ") for l in want[key]), key
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b]
        assert len(got[key]) == len(want[key]) and not diff, (name, key, diff[:5])


@pytest.mark.parametrize("name", list(P.MODELS))
def test_plan_tensors_match_recorded(gpu, name):
    want = P.golden(name + "_tensors")["tensors"]
    got = P.tensors(name)["tensors"]
    assert len(want) > 20 and all(len(t) == 5 for t in want)
    diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not diff, (name, diff[:5])
