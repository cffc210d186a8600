"""GPU suite of the arithmetic the stores are assembled from: the prism corner (prism_each_corner, prism_v6) and the
tesseroid traversal (tess_traverse) of csrc/kernels.hip.h, through every kernel written on them.

The yardstick is tests/golden/geometry_bits.json, recorded by tests/make_golden_geometry_bits.py from the scripted cases
of tests/geometry_bit_cases.py on the library as it was while every kernel carried its own copy of that arithmetic.
Everything is compared EXACTLY: per case the SHA-256 of download_G()'s bytes, of weight()'s wm, of forward() of a model
that differs per cell and of every result pass, and kernel_stats().  Two runs of the generator on the recording library
agreed in every digest, so no quantity needs a tolerance."""
import json
import os

import pytest

import geometry_bit_cases as cases
from conftest import GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "geometry_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pkg(built_lib):
    import gravinv3dhmc_amd
    from gravinv3dhmc_amd import _lib, engine  # noqa: F401
    return gravinv3dhmc_amd


def test_the_case_list_is_the_recorded_one(golden):
    assert sorted(c[0] for c in cases.CASES) == sorted(golden)


def test_the_recorded_tesseroid_cases_ran_the_subdivision(golden):
    assert cases.subdivision_ran(golden) is None


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_bits(pkg, golden, case):
    got = case[2](pkg)
    print("geometry bits [%s]: %s %s" % (case[0], cases.all_stats(got), got.get("near_field", "")))
    assert got == golden[case[0]]
