"""Generate tests/golden/geometry_bits.json: the bits of the stores, result passes and matrix-free passes that the
scripted cases of tests/geometry_bit_cases.py assemble from the prism corner and the tesseroid traversal.

TEST INFRASTRUCTURE ONLY; the library has no CPU path, so it runs on the GPU machine, on the library whose bits are to be
kept (the commit BEFORE a change of that arithmetic):
    python tests/make_golden_geometry_bits.py [output.json]
GRAVHMC_LIB names another build of the library.  The file holds DATA only: SHA-256 digests, kernel_stats() and the
matrix-free near-field table's counts.  It is NOT written if a tesseroid case shows no more leaves than (point, cell)
pairs -- the subdivision has then not run and the case pins nothing of it --, if no case flags a cell or none fills a
near-field table (geometry_bit_cases.subdivision_ran).  Two runs on the same library write the same file (checked when
the fixture was made: every digest reproduced).
(Not collected by pytest: the name does not start with test_.)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import geometry_bit_cases as cases  # noqa: E402


def main(argv):
    import gravinv3dhmc_amd as pkg
    from gravinv3dhmc_amd import _lib, engine  # noqa: F401
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", "geometry_bits.json")
    doc = cases.run_all(pkg)
    for name, pairs, _ in cases.CASES:
        print("%-26s %s %s" % (name, cases.all_stats(doc[name]), doc[name].get("near_field", "")))
    missing = cases.subdivision_ran(doc)
    if missing:
        sys.exit("not written: " + missing)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (out, len(doc)))


if __name__ == "__main__":
    main(sys.argv[1:])
