"""Code-object metadata of k_ens_sweep in the built gfx950 library: no private segment, no dynamic
stack, no register spills of either kind, in either instantiation.  Metadata only: no instruction text is read."""
import os
import re
import subprocess

import pytest

from bmm_mcmc_amd import build


def _tool(name):
    root = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    for path in (os.path.join(root, "llvm", "bin", name), os.path.join(root, "lib", "llvm", "bin", name)):
        if os.path.exists(path):
            return path
    raise AssertionError("%s not found beside hipcc" % name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel name -> its metadata block, from the notes of the library's gfx950 code object"""
    if build.stale(build.LIB):
        build.build()
    d = tmp_path_factory.mktemp("codeobj")
    fat, co = str(d / "fat.bin"), str(d / "lib.co")
    subprocess.run([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", build.LIB, fat], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count")[1:]:
        out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = blk
    return out


def test_both_instantiations_are_there(kernels):
    names = sorted(n for n in kernels if "k_ens_sweep" in n)
    assert len(names) == 2, names  # the finite sampler and the DP


def test_no_private_segment_no_dynamic_stack_no_spills(kernels):
    names = [n for n in kernels if "k_ens_sweep" in n]
    assert names
    for name in names:
        blk = kernels[name]
        field = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)  # noqa: E731
        print(name, {k: field(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert field("private_segment_fixed_size") == "0", name
        assert field("uses_dynamic_stack") == "false", name
        assert field("vgpr_spill_count") == "0" and field("sgpr_spill_count") == "0", name
