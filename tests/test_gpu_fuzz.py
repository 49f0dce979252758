"""Randomised differential tests (GPU): the fuzzers under scripts/ as regression tests, a few hundred cases each."""
import os
import runpy
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [11, 12])
def test_topk_fuzz(dev, seed):
    """K3 / K6 against a stable reference order over shapes around every size-class boundary, tie patterns, NaN / inf."""
    argv = sys.argv
    sys.argv = ["fuzz_topk.py", "250", str(seed)]
    try:
        with pytest.raises(SystemExit) as e:
            runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_topk.py"), run_name="__main__")
        assert e.value.code == 0
    finally:
        sys.argv = argv


def test_scoring_chain_fuzz(dev):
    """K2 -> K3 -> K4 -> K5 -> K6 against the oracle on random shapes (concept counts around ATen's 32-column groups, every K,
    ragged neuron counts, soft / hard WPMI, padded and unpadded S)."""
    argv = sys.argv
    sys.argv = ["fuzz_core.py", "150", "21"]
    try:
        with pytest.raises(SystemExit) as e:
            runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_core.py"), run_name="__main__")
        assert e.value.code == 0
    finally:
        sys.argv = argv


def test_front_fuzz(dev):
    """K1a, K1 (bit-exact in MKL's K-block order) on random (N, C, D) and leading dimensions; K0 on random hook outputs."""
    argv = sys.argv
    sys.argv = ["fuzz_front.py", "120", "31"]
    try:
        with pytest.raises(SystemExit) as e:
            runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_front.py"), run_name="__main__")
        assert e.value.code == 0
    finally:
        sys.argv = argv


def test_stress_chain_fuzz(dev):
    """K1s and K4s against float64 on random shapes (tile / slice / batch boundaries of both kernels)."""
    argv = sys.argv
    sys.argv = ["fuzz_stress.py", "150", "41"]
    try:
        with pytest.raises(SystemExit) as e:
            runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_stress.py"), run_name="__main__")
        assert e.value.code == 0
    finally:
        sys.argv = argv


def test_similarity_functions_fuzz(dev):
    """soft_wpmi, wpmi, cos_similarity, cos_similarity_cubed, rank_reorder (seeded) of the drop-in module against the oracle."""
    argv = sys.argv
    sys.argv = ["fuzz_sim.py", "25", "51"]
    try:
        with pytest.raises(SystemExit) as e:
            runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_sim.py"), run_name="__main__")
        assert e.value.code == 0
    finally:
        sys.argv = argv


# ---- the encoder side: tests/encoder_fuzz.py on the library, every operand in a frame -------------------------------------
import encoder_fuzz as E  # noqa: E402  (touches no GPU on import)


@pytest.fixture(scope="module")
def encoder_call(mcd, dev):
    return E.gpu_call(mcd._lib.load())


def _encoder_fuzz(entry, call, dev):
    """The committed case list of one entry (E.SEEDS): float64 and the headers' bit relations, read sets and frames."""
    case_list = E.cases(entry, E.SEEDS[entry])
    findings, ratio = E.run(entry, case_list, call, dev)
    print("%s: %d cases, %d findings, max err / bound %.3f" % (entry, len(case_list), len(findings), ratio))
    assert not findings, "\n".join(findings[:20])


@pytest.mark.parametrize("entry", E.ATTENTION)
def test_attention_family_fuzz(encoder_call, dev, entry):
    """K9, K9L, K9M, K9A, K9B over every (query wave, key tile, last-tile fill) class, lens at tile edges and clamped, rel NULL /
    zero / random, under every value regime (rising and falling scores, a dominant last-tile key, a zero K row, V = 100 + randn)."""
    _encoder_fuzz(entry, encoder_call, dev)


@pytest.mark.parametrize("entry", E.CLS_ROW)
def test_cls_row_fuzz(encoder_call, dev, entry):
    """K9C under random strides up to the four-wave split; K30 over every (H, D) instance, padded strides, and just above every
    token count at which its heads per pass fall (B = 1 there)."""
    _encoder_fuzz(entry, encoder_call, dev)


@pytest.mark.parametrize("entry", E.TOKEN_OPS)
def test_token_ops_fuzz(encoder_call, dev, entry):
    """K10 / K25 against float64 at their own tests' tolerances; K24, K26, K27, K28, K29 on the bits their headers spell out."""
    _encoder_fuzz(entry, encoder_call, dev)


# ---- the convolution side: tests/conv_fuzz.py on the library, every operand in a frame ------------------------------------
import conv_fuzz as CF  # noqa: E402  (touches no GPU on import)


@pytest.fixture(scope="module")
def conv_call(mcd, dev):
    return CF.gpu_call(mcd._lib.load())


def _conv_fuzz(entry, call, dev):
    """The committed case list of one entry (CF.SEEDS): float64, the headers' bit relations, read sets and frames."""
    case_list = CF.cases(entry, CF.SEEDS[entry])
    findings, ratio = CF.run(entry, case_list, call, dev)
    print("%s: %d cases, %d findings, max err / bound %.3f" % (entry, len(case_list), len(findings), ratio))
    assert not findings, "\n".join(findings[:20])


@pytest.mark.parametrize("entry", CF.TOWERS)
def test_conv_towers_fuzz(conv_call, dev, entry):
    """K12 - K15 and K0n, K16 - K18 and K18 with a residual, K19 - K21 over their tile edges, channel slices and k-step counts, one
    case past every grid cap, under exact, random, offset and dead data; every image alone, the batch reversed, permuted output
    channels, the ReLU flags against each other, one NaN pixel's read set."""
    _conv_fuzz(entry, conv_call, dev)


@pytest.mark.parametrize("entry", CF.SWIN)
def test_swin_fuzz(conv_call, dev, entry):
    """K31 at every (window, shift) pair, padded and unpadded grids of one to three windows a side, scores of +-100, a table that
    dominates q.k, a dominant key, every window of an unshifted grid alone; K32 against K10 on the gathered rows at every parity."""
    _conv_fuzz(entry, conv_call, dev)


# ---- the scoring side: tests/scoring_fuzz.py on the library, every operand in a frame -------------------------------------
import scoring_fuzz as SF  # noqa: E402  (touches no GPU on import)


@pytest.fixture(scope="module")
def scoring_call(mcd, dev):
    return SF.gpu_call(mcd._lib.load())


@pytest.mark.parametrize("entry", SF.ENTRIES)
def test_scoring_fuzz(scoring_call, dev, entry):
    """K1A, K1 (f32), K2, K4, K5, K7, the gathered row preparation and K8 over every class of their host dispatch
    (SF.dispatch: kernel form, template flags, persistent passes, panel width, npad), one case with 64-bit gather offsets: the
    oracle's bits or the entry's numeric rule, a row / neuron / segment alone, the batch reversed, the entry's twin forms
    (pitch, trusted, route) on the same bits, one NaN's read set, both guard fills."""
    import time
    t0 = time.perf_counter()
    case_list = SF.cases(entry, SF.SEEDS[entry])
    findings, ratio = SF.run(entry, case_list, scoring_call, dev)
    print("%s: %d cases, %d findings, max err / bound %.3f, %.1f s" % (entry, len(case_list), len(findings), ratio, time.perf_counter() - t0))
    assert not findings, "\n".join(findings[:20])
