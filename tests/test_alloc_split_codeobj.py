"""Code-object metadata of the split-merge kernels in the built gfx950 library (DESIGN.md sections 15 and 24), both
flavours of each -- the DP chain's (ILb0E) and the allocation chain's (ILb1E): no private segment, no dynamic stack, no
register spills of either kind."""
import re

import pytest

from test_feature_select_codeobj import kernels  # noqa: F401  (the fixture)


@pytest.mark.parametrize("pattern", ["k_sm_%sILb%dE" % (k, f) for f in (1, 0) for k in ("launch", "scan", "decide", "commit")])
def test_no_private_segment_and_no_spills(kernels, pattern):  # noqa: F811
    names = [n for n in kernels if pattern in n]
    assert len(names) == 1, names
    blk = kernels[names[0]]
    field = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)  # noqa: E731
    print(names[0], {k: field(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
    assert field("private_segment_fixed_size") == "0"
    assert field("uses_dynamic_stack") == "false"
    assert field("vgpr_spill_count") == "0" and field("sgpr_spill_count") == "0"
