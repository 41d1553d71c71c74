"""The channel-pair window kernels (K19 windowpair.hip, K23 windowxcorr.hip, K24 windowgranger.hip)
return the bits they returned before their plan, entry checks, batch walk and tile helpers were
moved into csrc/pair_window.h: every result of the cases of tests/golden/make_golden_pairwin_bits.py
has the SHA-256 digest that tests/golden/g26_pairwin_bits.npz recorded from the build before the
move.  Bits, so there is no tolerance; a NaN counts as a NaN whatever its payload."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_pairwin_bits",
                                               os.path.join(GOLDEN, "make_golden_pairwin_bits.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope="module")
def gold():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()      # fails loudly if the HIP library was not built
    with np.load(os.path.join(GOLDEN, "g26_pairwin_bits.npz")) as f:
        return dict(zip(f["keys"].tolist(), f["sha256"]))


def test_fixture_holds_these_cases(gold):
    assert {k.split(":")[1] for k in gold} == set(cases.CASES)


@pytest.mark.parametrize("case", list(cases.CASES))
def test_pair_window_kernels_kept_their_bits(gold, case):
    found = cases.digests(case)
    assert sorted(found) == sorted(k for k in gold if k.split(":")[1] == case)
    assert np.array_equal(found[f"in:{case}"], gold[f"in:{case}"]), f"{case}: the inputs changed, not the kernels"
    differ = [k for k in found if not np.array_equal(found[k], gold[k])]
    assert not differ, f"results with other bits than recorded: {differ}"
