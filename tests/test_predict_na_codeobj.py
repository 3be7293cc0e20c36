"""Code-object metadata of the kernels of incomplete new rows in the built gfx950 library: no
private segment, no dynamic stack and no spilled vector register in any instantiation.  The scorers keep some scalars
in lanes of a vector register, as k_score does (its 64-accumulator form: over 300); their number is printed, the
vector registers that costs are inside vgpr_count.  Metadata only: no instruction text is read."""
import re

import pytest

from test_pair_check_codeobj import kernels  # noqa: F401  (the fixture: kernel name -> metadata block)


# the table builder, the LDS scorer at 13 accumulator counts and both group widths, the global scorer, the finish
@pytest.mark.parametrize("pattern,count", [("k_split_tables", 1), ("k_score_naI", 26), ("k_score_na_generic", 1),
                                           ("k_predict_cells_finish", 1)])
def test_no_private_segment_and_no_vector_spills(kernels, pattern, count):  # noqa: F811
    names = [n for n in kernels if pattern in n]
    assert len(names) == count, names
    for name in names:
        blk = kernels[name]
        field = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)  # noqa: E731
        print(name, {k: field(k) for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size")})
        assert field("private_segment_fixed_size") == "0"
        assert field("uses_dynamic_stack") == "false"
        assert field("vgpr_spill_count") == "0"
        assert int(field("vgpr_count")) <= 256  # 512 lanes per workgroup: two waves per SIMD
