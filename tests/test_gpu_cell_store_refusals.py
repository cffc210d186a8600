"""GPU suite of the host side that describes what a context holds: the gh_set_cells_* entry points, the refusals of the
stores of blocks among each other, and the assembly of the smallest context of every cell kind.

The yardstick is tests/golden/cell_store_refusals.json, recorded by tests/make_golden_cell_refusals.py from the scripted
cases of tests/cell_store_cases.py on the library as it was before the stores were described by one table
(csrc/host_cells.h).  Everything is compared EXACTLY: return codes, gh_last_error's texts byte for byte -- with two
faults in one call, the text tells the order of the checks -- and, per cell kind, the SHA-256 of download_G()'s bytes
(the table forms, which never store G: of forward()'s), of weight()'s wm and of forward() of a fixed mw, kernel_stats()
and multi_info().  Two runs of the generator on the recording library agreed in every digest, so no quantity needs a
tolerance."""
import json
import os

import pytest

import cell_store_cases as cases
from conftest import GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "cell_store_refusals.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pkg(built_lib):
    import gravinv3dhmc_amd
    from gravinv3dhmc_amd import _lib, engine  # noqa: F401
    return gravinv3dhmc_amd


def test_the_case_lists_are_the_recorded_ones(golden):
    assert sorted(c[0] for c in cases.refusal_cases()) == sorted(golden["refusals"])
    assert sorted(c[0] for c in cases.BIT_CASES) == sorted(golden["bits"])


def test_refusals_codes_and_texts(pkg, golden):
    got = cases.run_refusals(pkg._lib)
    bad = ["%s step %d:\n    recorded %r\n    got      %r" % (name, i, want, have)
           for name, steps in sorted(golden["refusals"].items())
           for i, (want, have) in enumerate(zip(steps, got[name] + [None] * len(steps))) if want != have]
    refusing = sum(1 for steps in got.values() for rc, _ in steps if rc != 0)
    print("cell store refusals: %d cases, %d refusing steps, %d differ" % (len(got), refusing, len(bad)))
    assert not bad, "\n".join(bad)
    assert all(len(got[name]) == len(steps) for name, steps in golden["refusals"].items())


def test_every_refusal_case_is_a_refusal_or_a_clean_ok(golden):
    from gravinv3dhmc_amd import _lib
    codes = {rc for steps in golden["refusals"].values() for rc, _ in steps}
    assert codes <= {_lib.GH_OK, _lib.GH_ERR_ARG, _lib.GH_ERR_UNSUPPORTED}, codes
    assert all(msg for steps in golden["refusals"].values() for rc, msg in steps if rc != 0)


@pytest.mark.parametrize("case", cases.BIT_CASES, ids=[c[0] for c in cases.BIT_CASES])
def test_bits_of_every_kind(pkg, golden, case):
    got = cases.run_bit_case(pkg, case)
    want = golden["bits"][case[0]]
    print("cell store bits [%s]: %s" % (case[0], got["kernel_stats"]))
    assert got == want
