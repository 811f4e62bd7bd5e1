"""lm_select_kernel alone (api.k_lm_select; lm_logits.hip) on the direct cases of synth/lm_logits_cases.py: every token equals the numpy-f32 processors
followed by the lowest-index arg-max EXACTLY -- the penalty is one correctly rounded f32 operation per seen logit, the ban a set, the choice a comparison: no
tolerance enters -- the words around the token output come back untouched, and two runs give the same bytes.

What the cases open: vocabularies 33 .. 103424 (a last partial quad at 33, 97, 10007; a partial last bitmap word at all but 103424; more than one pass of the 1024
threads x 4 quads at 103424), 1 / 3 / 16 rows, histories of 0, 1, n - 1, n, 255, 256, 257 and 1030 ids (around a quarter of the ban search's thread stride, and above it) drawn from six ids so that
bans are many, a match at i = 0 and at i = H - n, ids beyond the vocabulary, an n larger than every history, +-0, negative winners, NaNs, rows of NaN and of -inf
alone, all tokens banned but one, and equal maxima 1, 64, 256 and 1023 apart (one lane, another lane's quad, another wave, and about a workgroup's width of quads apart)."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import lm_logits_cases as LC

pytestmark = pytest.mark.gpu

CASES = LC.kernel_cases()
GUARD = 8
SENTINEL = np.int32(-0x5A5A5A5B)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_select_equals_the_numpy_processors_exactly(case):
    rows = case["logits"].shape[0]
    want = LC.kernel_expected(case)
    io = np.full(GUARD + rows + GUARD, SENTINEL, np.int32)
    got = api.k_lm_select(case["logits"], case["histories"], case["r"], case["n"], io, GUARD)
    again = api.k_lm_select(case["logits"], case["histories"], case["r"], case["n"], io, GUARD)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + rows:] == SENTINEL).all()
    assert np.array_equal(got[GUARD:GUARD + rows], want), (case["name"], got[GUARD:GUARD + rows], want)
    assert got.tobytes() == again.tobytes()
    if "equal_maxima" in case:      # the lower of two equal maxima is seen: the upper wins; unseen: the lower wins
        for j, (lo, d) in enumerate(case["equal_maxima"]):
            assert got[GUARD + 2 * j] == lo + d and got[GUARD + 2 * j + 1] == lo


def test_processors_off_is_the_plain_lowest_index_argmax():
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, (16, 1030)).astype(np.float32)        # few distinct values: many equal maxima
    hs = [[int(v) for v in rng.integers(0, 1030, 40)] for _ in range(16)]
    got = api.k_lm_select(x, hs, 1.0, 0, np.zeros(16, np.int32), 0)
    assert np.array_equal(got, np.asarray([LC.choose(r) for r in x], np.int32)) and np.array_equal(got, x.argmax(axis=1))
    assert np.array_equal(api.k_lm_select(x, hs, 1.0, 1, np.zeros(16, np.int32), 0), got)
