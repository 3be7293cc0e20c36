"""The two-tier draw of k_resample, without a device: bmm_spec.h's draw_tier1 (binary32 weights through exp2, which
says whether its count is proven) against draw_spec (the definition: expw_, binary64 running sum, count), both
compiled for the host by tests/draw_tier1/tier1_check.cpp.

Cases (all of them, for every category count from 2 to 56 and for 64): random score vectors of many spreads, ties,
-inf entries, all -inf, NaN, +inf; uniforms at, just below and just above every exact boundary cdf_k / tot one
step of the 52-bit grid at a time, around the edge of the band, at random, u = 0 and u = 1 - 2^-52; the binary32
exponential at its nominal value, an ulp up, an ulp down, mixed, and with tiny results flushed to zero.

Asserted by the program: whenever tier 1 says "certain" its count is the definition's; it is never certain at a
constructed boundary, nor of an impossible or NaN observation; and a band of width zero IS wrong at those
boundaries (so the test can fail)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "draw_tier1", "tier1_check.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")


def test_tier1_count_is_the_definitions_whenever_it_says_certain(tmp_path):
    exe = str(tmp_path / "tier1_check")
    # -ffp-contract=off: as the library is built (bmm_spec.h fuses only where it says fma_)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    sys.stderr.write(r.stderr[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
