"""Every count-table build and both tails of the stored-state scorer, held to the digests recorded from the commit
before they were folded into one (tests/state_score_pins.py: the cases, what is digested and how the file was
recorded).  A digest is of raw bytes: one reordered sum or one moved guard changes it."""
import pytest

import bmm_mcmc_amd as bm
import state_score_pins as pins

pytestmark = pytest.mark.gpu


def _check(name):
    want = pins.load_pins()[name]
    got = pins.digests(bm, name)
    print(name, len(got), "digests")
    assert sorted(got) == sorted(want), (name, sorted(set(got) ^ set(want)))
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, (name, differ)


def test_the_pins_cover_the_cases():
    assert sorted(pins.load_pins()) == sorted(pins.CASES)


@pytest.mark.parametrize("name", pins.PRODUCT_CASES)
def test_the_product_library_reproduces_the_recorded_bits(monkeypatch, name):
    pins.set_switches(None, monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
    _check(name)


@pytest.mark.parametrize("name", pins.SWITCHED_CASES)
def test_the_switched_forms_reproduce_the_recorded_bits(dbg_lib, name):
    pins.set_switches(pins.CASES[name].get("env"), dbg_lib.setenv, lambda v: dbg_lib.delenv(v, raising=False))
    _check(name)
