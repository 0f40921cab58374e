"""GPU: a fixed-seed slice of the differential fuzzer (tools/fuzz.py) -- every C-ABI entry point
against the oracle on randomised shapes, parameters and error cases.  The full fuzzer ran
72 168 cases over the final kernels without a mismatch (profiles/r01_fuzz_v3.txt, incl. the chunked host path; 59 633 on the
earlier ones, profiles/r01_fuzz.txt)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("block", range(4))
def test_fuzz_slice(block):
    from tools import fuzz
    for k in range(150):
        seed = 7_000_003 * (block + 1) + k
        fuzz.CASES[k % len(fuzz.CASES)](np.random.default_rng(seed))
    fuzz.case_umi_large(np.random.default_rng(11 * (block + 1)))


@pytest.mark.parametrize("block", range(2))
def test_fuzz_slice_other_encodings(block):
    """The quality-aware cases with the table drawn from tests/encodings.py (alignment, consensus, masking, the fused
    MSA + consensus)."""
    from tools import fuzz
    for k in range(120):
        seed = 9_000_011 * (block + 1) + k
        fuzz.ENC_CASES[k % len(fuzz.ENC_CASES)](np.random.default_rng(seed))
