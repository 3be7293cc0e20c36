"""The middle settle tier of k_resample_pk, without a device: bmm_spec.h's draw_mid (the binary32 table entries the
packed loop reads, widened and summed in binary64, then the definition's maximum, expw_, running sum and count, with a
band per observation) against draw_spec (the definition on the binary64 scores), both compiled for the host by
tests/mid_tier/mid_check.cpp.

Cases: every category count from 2 to 32; 1, 7, 20 and 26 lookup groups; scores from about -2 down to about -700,
categories a fiftieth of a unit to sixty units apart, ties, impossible categories, a cluster of one row (an own score
of -inf), all impossible, NaN, +inf; every narrowed entry as it is, an ulp up, an ulp down and alternately; uniforms at
and one 2^-52 step at a time around every exact boundary cdf_k / tot, around the edge of the band, at random, u = 0 and
u = 1 - 2^-52.

Asserted by the program: a certain draw always has the definition's count; none is certain at a constructed boundary
or of an impossible or NaN observation; a band of width zero IS wrong at those boundaries; and the band is not vacuous
-- on tables built from C5's generator at steady state (K = 20, P = 100, statistics N_k theta; sixteen uniforms to
each of 200 000 observations) at most 20 % of the draws draw_pk leaves uncertain are left uncertain by draw_mid
(14.25 % when this was written: 312 of 2190; the ratio of the two bands there is 0.13).

mid_check.cpp is a stand-alone program: built with -fsanitize=address,undefined it runs clean (profiles/r12/README.md)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mid_tier", "mid_check.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")
# -ffp-contract=off: as the library is built (bmm_spec.h fuses only where it says fma_)
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-I", INC]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    sys.stderr.write(r.stderr[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-4000:], r.stderr[-2000:])


def test_middle_count_is_the_definitions_whenever_it_says_certain(tmp_path):
    exe = str(tmp_path / "mid_check")
    subprocess.run(["g++"] + FLAGS + [SRC, "-o", exe], check=True)
    _run(exe)

