"""Code-object metadata of the missing-data kernels in the built gfx950 library: no private
segment, no dynamic stack, no register spills of either kind.  Metadata only: no instruction text is read."""
import re

import pytest

from test_pair_check_codeobj import kernels  # noqa: F401  (the fixture: kernel name -> metadata block)


# the fill, both forms of the census and of the draw, the rates and the word gather
@pytest.mark.parametrize("pattern,count", [("k_na_fill", 1), ("k_na_census", 2), ("k_na_phi", 1), ("k_na_draw", 2), ("k_na_words", 1)])
def test_no_private_segment_and_no_spills(kernels, pattern, count):  # noqa: F811
    names = [n for n in kernels if pattern in n]
    assert len(names) == count, names
    for name in names:
        blk = kernels[name]
        field = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)  # noqa: E731
        print(name, {k: field(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert field("private_segment_fixed_size") == "0"
        assert field("uses_dynamic_stack") == "false"
        assert field("vgpr_spill_count") == "0" and field("sgpr_spill_count") == "0"
