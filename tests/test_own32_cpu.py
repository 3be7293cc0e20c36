"""The binary32 own-cluster score of k_resample_pk, without a device.

tests/own32/own32_check.cpp restates the kernel's own score on the host -- the "observation removed" terms grouped at
the shape's width, each binary64 entry narrowed once, summed in binary32 in group order (the image Tm32 of
k_count_tables) -- beside the scores Tq gives, and runs bmm_spec.h's draw_pk on them against draw_spec on the
definition's binary64 scores, whose own score is the width-3 sum.  Tables come from the count-table rules of
bmm_spec.h: C5's generator at steady state (K = 20, P = 100) and adversarial counts (clusters of one and of two rows,
features with s = 0 and s = n, N up to 1e9; P = 1, 37, 100, 128; 4, 8 and 20 labels), at both group widths; every
narrowed entry as it is, an ulp up, an ulp down and alternately; uniforms one 2^-52 step at a time around every CDF
boundary, around the band's edge, at random, 0 and 1 - 2^-52.

Asserted by the program: a certain draw always has the definition's count; every entry of both own images is <= 0 or
-inf; at most 0.5 % of C5's observations come back uncertain.  Measured when this was written, 200 000 observations:
0.0705 % at groups of five (0.0710 % on the same observations and uniforms with the own score narrowed from its
binary64 sum, as the parent commit forms it; the parent's pk_check, other observations: 0.058 %), 0.0845 % at groups
of four (0.0845 %).

The second test builds the same program under the address and undefined-behaviour sanitizers and runs a tenth of it.

Last, the LDS of a packed workgroup: the library's bmm_spec_pk_image_bytes against a restatement of the layout over
KT = 4..32 in steps of 4, P = 1..128 and both widths -- and no shape, at the width the width rule gives it, that had
the packed kernel with the binary64 Tm in LDS loses it to the image that holds Tm32 instead (1000 of the 1024 fitted
before, 1020 now; the image only grows where K x P is large at groups of five, and those shapes have groups of four)."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "own32", "own32_check.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")
# -ffp-contract=off: as the library is built (bmm_spec.h fuses only where it says fma_)
CXX = ["g++", "-std=c++17", "-ffp-contract=off", "-I", INC, SRC]


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=900)
    sys.stderr.write(r.stderr[-4000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-4000:], r.stderr[-4000:])


def test_certain_draws_with_the_binary32_own_score_are_the_definitions(tmp_path):
    exe = str(tmp_path / "own32_check")
    subprocess.run(CXX + ["-O2", "-o", exe], check=True)
    _run(exe)


def test_the_check_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "own32_check_san")
    subprocess.run(CXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe], check=True)
    _run(exe, "quick")


LDS_MAX = 160 * 1024
QUEUE = 4096


def _layout(KT, P, W):
    """doubles of the pieces of the table image (TableLayout, kernels.hip.h)"""
    G, M = -(-P // W), 1 << W
    nk_slots = (KT + 1) // 2 + (((KT + 1) // 2) & 1)
    gm_pad = -(-(-(-P // 3)) // 6) * 6
    return dict(tq=G * (KT // 2) * M, nk_e=nk_slots + 256, tm=gm_pad * KT * 8)


def _bytes_before(KT, P, W):
    l = _layout(KT, P, W)
    return (l["tq"] + l["nk_e"] + l["tm"]) * 8 + (KT * P + KT + 4 + QUEUE) * 4


def _bytes_now(KT, P, W):
    l = _layout(KT, P, W)
    return (2 * l["tq"] + l["nk_e"]) * 8 + (KT * P + KT + 4 + QUEUE) * 4


def test_no_shape_loses_the_packed_kernel_to_the_larger_image():
    from bmm_mcmc_amd import _capi
    f = _capi.lib().bmm_spec_pk_image_bytes
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] * 4
    assert _bytes_before(20, 100, 5) == 123888 and _bytes_now(20, 100, 5) == 129008   # C5
    assert f(0, 20, 100, 5) == 129008
    width = _capi.lib().bmm_spec_group_width_for
    fit_before = fit_now = 0
    lost, lost_elsewhere = [], []
    for W in (5, 4):
        for KT in range(4, 33, 4):
            for P in range(1, 129):
                now = f(0, KT, P, W)      # the finite sampler: K labels in KT = K accumulators
                assert now == _bytes_now(KT, P, W), (KT, P, W, now)
                before = _bytes_before(KT, P, W)
                if width(0, KT, P) != W:  # not a shape that runs: the rule gives (K, P) the other width
                    lost_elsewhere += [(KT, P, W)] if before <= LDS_MAX < now else []
                    continue
                fit_before += before <= LDS_MAX
                fit_now += now <= LDS_MAX
                if before <= LDS_MAX < now:
                    lost.append((KT, P, W))
    print("shapes at the width the rule gives them with the packed image in LDS: %d before, %d now; lost: %s; "
          "at the width the rule does not give them: %d would not fit any more" % (fit_before, fit_now, lost, len(lost_elsewhere)))
    assert not lost, lost
    assert f(0, 20, 129, 5) == -1 and f(0, 20, 100, 3) == -1 and f(0, 2000, 100, 5) == -1
