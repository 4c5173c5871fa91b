"""GPU: the bits of the validation-path kernels (disease_loss forward and backward, calib_fit,
reliability_bins, confusion_grid) against tests/golden/valid_bits.json.

The cases, their inputs and the digests are those of tools/valid_bits.py, imported and not
restated; its docstring lists the shapes and what each exercises.  The kernels add in a fixed
order and count in integers, so every output is a function of the inputs alone and is compared
bit for bit: a change in the shared reduction (csrc/class_reduce.h) that reorders one addition
fails here.

Regenerating the file (tools/valid_bits.py --write) is legitimate after a compiler or ROCm
change, shown by a mismatch at an unchanged parent commit, and is done from that unchanged
parent.  It is never the answer to a kernel edit that fails this test.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import valid_bits as VB  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stored():
    with open(os.path.join(ROOT, "tests", "golden", "valid_bits.json")) as f:
        return json.load(f)


def test_stored_cases_are_the_tools_cases(dev, stored):
    assert sorted(stored["digests"]) == sorted(VB.CASES)


@pytest.mark.parametrize("kind", ["loss", "fit", "bins", "grid"])
def test_digests_match(dev, stored, kind):
    bad = []
    for name, (k, _) in VB.CASES.items():
        if k == kind:
            bad += VB.compare(name, *VB.run_case(name, dev), stored)
    print("\n".join(bad))
    assert not bad, f"{len(bad)} line(s) of mismatch against the file written at " \
                    f"{stored.get('commit')} (ROCm {stored.get('rocm')}):\n" + "\n".join(bad)
