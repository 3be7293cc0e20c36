"""Code-object metadata of the kernels of the allocation sampler's split-merge move in the built gfx950 library
(DESIGN.md section 24): no private segment, no dynamic stack, no register spills of either kind; and the DP chain's scan,
whose body they share, keeps none either."""
import re

import pytest

from test_feature_select_codeobj import kernels  # noqa: F401  (the fixture)


@pytest.mark.parametrize("pattern", ["k_as_launch", "k_as_scan", "k_as_decide", "k_as_commit", "k_sm_scan"])
def test_no_private_segment_and_no_spills(kernels, pattern):  # noqa: F811
    names = [n for n in kernels if pattern in n]
    assert len(names) == 1, names
    blk = kernels[names[0]]
    field = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)  # noqa: E731
    print(names[0], {k: field(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
    assert field("private_segment_fixed_size") == "0"
    assert field("uses_dynamic_stack") == "false"
    assert field("vgpr_spill_count") == "0" and field("sgpr_spill_count") == "0"
