"""The variant ledger (tests/kernel_variants.py) matches the instantiations of the built library, both ways."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rpeflow_amd", "csrc", "librpeflow_hip.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_coverage as K  # noqa: E402
from tests.kernel_variants import LEDGER  # noqa: E402


def test_ledger_entries_are_well_formed():
    for name, (kind, what) in LEDGER.items():
        assert kind in ("test", "reason") and isinstance(what, str) and what, name
        if kind == "reason":  # the one admissible reason left: a clock / probe kernel with a test of its own
            assert "probe" in what and "test_" in what, name
        if kind == "test" and what.startswith("tests/"):
            path = what.split("::")[0]
            assert os.path.exists(os.path.join(ROOT, path)), (name, what)


def test_ledger_matches_built_library():
    if not os.path.exists(LIB):
        pytest.skip("librpeflow_hip.so is not built")
    try:
        built = set(K.list_kernels(LIB))
    except FileNotFoundError as e:  # no demangler on this machine
        pytest.skip(str(e))
    missing = sorted(built - set(LEDGER))
    gone = sorted(set(LEDGER) - built)
    assert not missing, f"instantiations with no ledger entry: {missing}"
    assert not gone, f"ledger entries whose instantiation is gone: {gone}"


def test_normalise_matches_trace_names():
    assert K.normalise("void (anonymous namespace)::corr_backward_kernel<4, true>(float const*, float const*, int, int, int, float*)") \
        == "corr_backward_kernel<4, true>"
    assert K.normalise("attn_softmax_kernel(float const*, float const*, int, float const*, int, int, int, float, float*)") == "attn_softmax_kernel"
    assert K.normalise("void resize_frames_kernel<unsigned char>(unsigned char const*, float*)") == "resize_frames_kernel<unsigned char>"
