"""The fixed conv policy is pinned: before any forward at a batch size, fr_debug_plan reports the policy's kernel per
conv (csrc/convs.cpp default_choice), which depends on the plan and the shapes alone.  The plan text of every model
at B = 1, 8 and 256, with FR_OPT_BATCH_INVARIANT off and on, must equal the recorded one (tests/golden/plans/,
written by tests/conv_policy_plans.py at the commit before the conv selection moved into its table).  No embed call:
only the load-time packers run on the device."""
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
