"""Code-object metadata of k_ens_score in the built gfx950 library: every instantiation is there,
none has a private segment, a dynamic stack or a register spill of either kind; and k_ens_sweep is the kernel it was
before the scorer came to stand beside it.  Metadata only: no instruction text is read."""
import os
import re
import subprocess

import pytest

from bmm_mcmc_amd import build

# k_ens_sweep<DP> as the commit before this feature built it: vgpr_count, sgpr_count, group_segment_fixed_size
SWEEP_BEFORE = {"_ZN3bmm11k_ens_sweepILb0EEEvNS_7EnsArgsE": ("138", "102", "0"),
                "_ZN3bmm11k_ens_sweepILb1EEEvNS_7EnsArgsE": ("134", "106", "0")}


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


def _field(blk, key):
    return re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)


def test_every_instantiation_is_there(kernels):
    names = sorted(n for n in kernels if "k_ens_score" in n)
    # <DP, LOO>: the finite sampler and the DP, the predictive and the leave-one-out
    assert names == sorted("_ZN3bmm11k_ens_scoreILb%dELb%dEEEvNS_11EnsFoldArgsE" % (dp, loo) for dp in (0, 1) for loo in (0, 1)), names
    assert not any("k_ens_sweep" in n for n in names)


def test_no_private_segment_no_dynamic_stack_no_spills(kernels):
    names = [n for n in kernels if "k_ens_score" in n]
    assert names
    for name in names:
        blk = kernels[name]
        print(name, {k: _field(blk, k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert _field(blk, "private_segment_fixed_size") == "0", name
        assert _field(blk, "uses_dynamic_stack") == "false", name
        assert _field(blk, "vgpr_spill_count") == "0" and _field(blk, "sgpr_spill_count") == "0", name


def test_the_sweep_kernel_is_what_it_was(kernels):
    names = sorted(n for n in kernels if "k_ens_sweep" in n)
    assert names == sorted(SWEEP_BEFORE), names
    for name in names:
        got = tuple(_field(kernels[name], k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size"))
        assert got == SWEEP_BEFORE[name], (name, got)
