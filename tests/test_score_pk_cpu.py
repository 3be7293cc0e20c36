"""The packed tier of k_resample_pk, without a device: bmm_spec.h's draw_pk (scores summed in binary32 from narrowed
table entries, binary32 weights, a band per observation) against draw_spec (the definition on the binary64 scores),
both compiled for the host by tests/score_pk/pk_check.cpp.

Cases: every category count from 2 to 32; 1, 7, 20 and 26 lookup groups; scores from about -2 down to about -700,
categories a fiftieth of a unit to sixty units apart, ties, impossible categories, all impossible, NaN, +inf; every
narrowed entry as it is, an ulp up, an ulp down and alternately; the exponential as tests/draw_tier1 pushes it;
uniforms at and one grid step at a time around every exact boundary cdf_k / tot, around the edge of the band, at
random, u = 0 and u = 1 - 2^-52.

Asserted by the program: a certain draw always has the definition's count; none is certain at a constructed boundary
or of an impossible or NaN observation; a band of width zero IS wrong at those boundaries; and the band is not
vacuous -- on tables built from C5's generator at steady state (K = 20, P = 100, statistics N_k theta) at most 0.5 %
of the observations come back uncertain (0.058 % when this was written)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "score_pk", "pk_check.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")


def test_packed_count_is_the_definitions_whenever_it_says_certain(tmp_path):
    exe = str(tmp_path / "pk_check")
    # -ffp-contract=off: as the library is built (bmm_spec.h fuses only where it says fma_)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    sys.stderr.write(r.stderr[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
