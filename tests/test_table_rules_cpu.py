"""The count-table rules of bmm_spec.h (const_arg, cat_consts, term_arg, term_of) without a device.  They are what
build_tables_self and k_state_tables evaluate; tests/table_rules/rules_check.cpp builds every row's scores from the
finite sweep's rule through group_entry, as a table image gives them, and compares them with score[] of the oracle's
oracle_collapsed_cond_spec -- exactly, -inf equal to -inf: the oracle's scores are that table arithmetic.

Reached, and counted by the program (a guard that never fired fails it): an empty label; a single-row label scored by
its own row and by another; features with s = 0 and s = n under the minus-self guards; P = 125; both group widths.
(k_count_tables writes its terms out itself in all four flavours and is held to the oracle chains on the device.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "table_rules", "rules_check.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")


def test_the_rules_give_the_oracles_scores_exactly(tmp_path):
    obj, exe = str(tmp_path / "bmm_oracle.o"), str(tmp_path / "rules_check")
    # -ffp-contract=off: as the library and the oracle are built (bmm_spec.h fuses only where it says fma_)
    subprocess.run(["gcc", "-std=gnu11", "-O2", "-mfma", "-ffp-contract=off", "-pthread", "-c", os.path.join(ORACLE, "bmm_oracle.c"),
                    "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, "-I", ORACLE, SRC, obj, "-o", exe, "-lm", "-pthread"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stderr.write(r.stderr[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
