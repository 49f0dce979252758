"""CPU: the framed-buffer checker of the C ABI contract tests (util.framed / util.check_frame) can fail.  Four numpy
"entries" with one planted defect each -- a write into a pad column, a write past the last row, a promised-zero pad left
unset, a result that depends on what an input's gap holds -- must each make check_frame raise; the clean one passes."""
import numpy as np
import pytest
import torch

from util import GAP_FILLS, OUT_FILL, check_frame, framed, framed_dense

ROWS, W, PX, PY, GUARD = 5, 7, 11, 12, 16
X = np.random.default_rng(0).standard_normal((ROWS, W)).astype(np.float32)


def entry(x, ldx, y, ldy, zero_pad, defect=None):
    """y[r, :W] = 2 * x[r, :W] on flat float32 arrays that start at the matrices' first elements (pitches ldx, ldy); with
    zero_pad the columns W..ldy-1 of every row are written as 0, as mcd_row_softmax promises."""
    for r in range(ROWS):
        row = x[r * ldx:r * ldx + W]
        y[r * ldy:r * ldy + W] = 2 * row + (0 * x[r * ldx + W] if defect == "reads_gap" and r == 2 else 0)
        if zero_pad and not (defect == "pad_unset" and r == 3):
            y[r * ldy + W:(r + 1) * ldy] = 0
    if defect == "pad_write":
        y[1 * ldy + W + 2] = 5.0
    if defect == "past_last_row":
        y[(ROWS - 1) * ldy + W + (ldy - W if zero_pad else 0)] = 5.0


def run(defect, zero_pad, gap, base_off=1):
    """The entry on framed CPU buffers; returns what check_frame needs for the output."""
    xf, xv = framed(ROWS, W, PX, base_off, GUARD, gap, torch.float32, "cpu")
    xv.copy_(torch.from_numpy(X))
    spec = (ROWS, W, PY, base_off, GUARD, OUT_FILL)
    yf, _ = framed(*spec, torch.float32, "cpu", tail=PY - W if zero_pad else 0)
    entry(xf.numpy()[GUARD + base_off:], PX, yf.numpy()[GUARD + base_off:], PY, zero_pad, defect)
    return yf, spec


@pytest.mark.parametrize("zero_pad", [False, True])
def test_the_clean_entry_passes(zero_pad):
    first = None
    for gap in GAP_FILLS:
        yf, spec = run(None, zero_pad, gap)
        check_frame(yf, spec, 2 * X, zero_pad=zero_pad)
        first = yf.clone() if first is None else first
        check_frame(yf, spec, torch.as_strided(first, (ROWS, W), (PY, 1), GUARD + 1), zero_pad=zero_pad)


@pytest.mark.parametrize("defect,zero_pad", [("pad_write", False), ("pad_write", True), ("past_last_row", False),
                                             ("past_last_row", True), ("pad_unset", True)])
def test_a_stray_or_missing_write_is_caught(defect, zero_pad):
    yf, spec = run(defect, zero_pad, 1.0e30)
    with pytest.raises(AssertionError, match="outside the logical region"):
        check_frame(yf, spec, 2 * X, zero_pad=zero_pad)


def test_a_result_that_depends_on_a_gap_is_caught():
    """0 * gap is NaN for a NaN gap and 0 for 1e30: the two runs' outputs differ in row 2, so the second run fails against
    the first run's bits (and the NaN run against the expected values)."""
    y_nan, spec = run("reads_gap", False, GAP_FILLS[0])
    y_big, _ = run("reads_gap", False, GAP_FILLS[1])
    check_frame(y_big, spec, 2 * X)
    with pytest.raises(AssertionError, match="logical region differ.*row 2"):
        check_frame(y_nan, spec, 2 * X)
    with pytest.raises(AssertionError, match="logical region differ.*row 2"):
        check_frame(y_nan, spec, torch.as_strided(y_big, (ROWS, W), (PY, 1), GUARD + 1))


def test_a_wrong_value_and_a_nan_payload_are_caught():
    yf, spec = run(None, False, 1.0e30)
    wrong = 2 * X
    wrong[4, 6] = np.nextafter(wrong[4, 6], np.float32(9))
    with pytest.raises(AssertionError, match=r"\(row 4, column 6\)"):
        check_frame(yf, spec, wrong)
    # NaNs compare by their bits: equal payloads pass, another payload does not
    a = np.array([[0x7fc00001]], np.int32)
    f, v = framed(1, 1, 1, 0, GUARD, OUT_FILL, torch.float32, "cpu")
    v.copy_(torch.from_numpy(a.view(np.float32)))
    check_frame(f, (1, 1, 1, 0, GUARD, OUT_FILL), a.view(np.float32))
    with pytest.raises(AssertionError):
        check_frame(f, (1, 1, 1, 0, GUARD, OUT_FILL), np.array([[0x7fc00002]], np.int32).view(np.float32))


@pytest.mark.parametrize("defect", [None, "one_past_the_end", "one_before_the_start", "wrong_element", "empty_but_written"])
def test_a_contiguous_nd_operand_is_a_frame_of_one_row(defect):
    """util.framed_dense: y [2, 3, 4] = 2 * x on a contiguous N-d output.  A store one element past the tensor or one in
    front of it lands in a guard and is caught, as is a wrong element; an empty output ([2, 0, 4]: nothing is written) must
    leave the whole allocation as it was, and one stray store into it is caught too."""
    shape = (2, 0, 4) if defect == "empty_but_written" else (2, 3, 4)
    x = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    yf, yv, spec = framed_dense(shape, 0, GUARD, OUT_FILL, torch.float32, "cpu")
    assert tuple(yv.shape) == shape and yv.is_contiguous() and spec[:2] == (1, x.size)
    yv.copy_(torch.from_numpy(2 * x))
    y = yf.numpy()
    if defect == "one_past_the_end":
        y[GUARD + x.size] = 5.0
    elif defect == "one_before_the_start":
        y[GUARD - 1] = 5.0
    elif defect == "wrong_element":
        y[GUARD + 13] = np.nextafter(y[GUARD + 13], np.float32(9))
    elif defect == "empty_but_written":
        y[GUARD] = 5.0
    if defect is None:
        check_frame(yf, spec, 2 * x)
        return
    match = r"\(row 0, column 13\)" if defect == "wrong_element" else "outside the logical region"
    with pytest.raises(AssertionError, match=match):
        check_frame(yf, spec, 2 * x)
