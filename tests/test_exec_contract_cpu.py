"""CPU: the checkers of the execution-contract tests can fail, and their case tables cover the headers.

1. util.framed_ws / check_ws_guards / check_ws_untouched / assert_same_bits (test_gpu_workspace_contracts.py,
   test_gpu_stream_contracts.py) on a numpy "entry" with one planted defect each -- a write one byte past the workspace, a
   result that depends on what the workspace held before the call (a mark read before it is written, K3's), a result that
   depends on stale output content (the mark kept in the output, K6's) -- must each fail; the clean entry passes.
2. Every prototype of include/mcd_hip.h and include/mcd_blaslt.h that takes a stream has a row in STREAM_TABLE, every
   *_workspace() function one in WS_TABLE, and neither table names anything the headers do not declare: an entry added later
   cannot skip these tests silently.  Importing the tables needs no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from util import (OUT_FILL, WS_ALIGN, WS_FILLS, WS_GUARD, assert_same_bits, check_ws_guards, check_ws_untouched, framed_ws,
                  ws_interior)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, W, NBYTES = 4, 6, 4 + 4 * 4 * 6          # the workspace: one int32 mark, then a [ROWS, W] fp32 scratch
X = np.random.default_rng(0).standard_normal((ROWS, W)).astype(np.float32)
IDX_STALE = (-77777, -1, 0)


def entry(x, ws, y, idx, defect=None):
    """y = 2 x + 1 through a scratch copy in ws, idx[r] = argmax of row r.  ws: the uint8 bytes FROM the workspace's first byte on
    (a correct entry touches NBYTES of them).  Row 0 is "left to a second pass" when its mark says -1 -- the mark is a word of
    the workspace, written (0) before it is read; the planted defects read it first, or keep it in idx[0]."""
    mark = ws[:4].view(np.int32)
    scratch = ws[4:NBYTES].view(np.float32).reshape(ROWS, W)
    if defect != "reads_ws_first":
        mark[0] = 0
    if defect == "mark_in_stale_output":
        mark[0] = idx[0]                        # whatever the output held: -1 means "a second pass does row 0"
    scratch[:] = 2 * x
    if defect == "past_the_end":
        ws[NBYTES] = 1
    for r in range(ROWS):
        if r == 0 and mark[0] == -1:
            continue                            # (no second pass in this entry: the row keeps what it held)
        y[r] = scratch[r] + 1
        idx[r] = int(np.argmax(x[r]))


def run(defect, fill, idx_fill=IDX_STALE[0]):
    flat, ptr, n = framed_ws(NBYTES, WS_GUARD, fill, "cpu")
    assert n == NBYTES and ptr % WS_ALIGN == 0 and ptr == flat.data_ptr() + flat.ws_start
    assert flat.ws_start >= WS_GUARD and flat.numel() - flat.ws_start - n >= WS_GUARD and bool((flat == fill).all())
    y = np.full((ROWS, W), OUT_FILL, np.float32)
    idx = np.full((ROWS,), idx_fill, np.int32)
    entry(X, flat.numpy()[flat.ws_start:], y, idx, defect)
    return flat, y, idx


def test_the_clean_entry_passes():
    runs = []
    for fill in WS_FILLS:
        for idx_fill in IDX_STALE:
            flat, y, idx = run(None, fill, idx_fill)
            check_ws_guards(flat, NBYTES, fill)
            assert np.array_equal(y, 2 * X + 1) and np.array_equal(idx, X.argmax(1))
            assert bool((ws_interior(flat, NBYTES)[4:].view(torch.float32) == torch.from_numpy(2 * X).reshape(-1)).all())
            runs.append(((fill, idx_fill), [y, idx]))
    assert_same_bits(runs)
    flat, _, _ = framed_ws(NBYTES, WS_GUARD, 0x7F, "cpu")
    check_ws_untouched(flat, 0x7F)


def test_a_write_one_byte_past_the_workspace_is_caught():
    flat, y, idx = run("past_the_end", 0xFF)
    assert np.array_equal(y, 2 * X + 1)                     # the result itself is right
    with pytest.raises(AssertionError, match="trailing guard changed, the first 1 bytes past its end"):
        check_ws_guards(flat, NBYTES, 0xFF)
    with pytest.raises(AssertionError, match="refused call wrote"):        # (a call that ran is no refused call)
        check_ws_untouched(flat, 0xFF)
    flat, _, _ = run(None, 0x00)
    flat[flat.ws_start - 1] = 9                             # and one byte in front of it
    with pytest.raises(AssertionError, match="leading guard changed, the first 1 bytes in front"):
        check_ws_guards(flat, NBYTES, 0x00)


def test_a_result_that_depends_on_the_workspace_content_is_caught():
    """The mark read before it is written: under 0x00 and 0x7F the entry behaves, under 0xFF (int32 -1) row 0 is never
    computed -- the run differs from the first one, and from the reference."""
    runs = [(fill, list(run("reads_ws_first", fill)[1:])) for fill in WS_FILLS]
    assert np.array_equal(runs[0][1][0], 2 * X + 1) and np.array_equal(runs[2][1][0], 2 * X + 1)
    with pytest.raises(AssertionError, match="output 0 of run 255 differs from run 0 in 6 elements"):
        assert_same_bits(runs)
    assert_same_bits([runs[0], runs[2]])


def test_a_result_that_depends_on_stale_output_content_is_caught():
    """The mark kept in idx[0]: a caller whose idx happens to hold -1 gets row 0 left undone; 0 and any other value pass."""
    runs = [(i, list(run("mark_in_stale_output", 0x00, i)[1:])) for i in IDX_STALE]
    with pytest.raises(AssertionError, match="run -1 differs from run -77777"):
        assert_same_bits(runs)
    assert_same_bits([runs[0], runs[2]])


def test_assert_same_bits_compares_nan_payloads():
    a = np.array([0x7fc00001, 5], np.int32).view(np.float32)
    b = np.array([0x7fc00002, 5], np.int32).view(np.float32)
    assert_same_bits([("a", [a]), ("a again", [a.copy()]), ("tensor", [torch.from_numpy(a.copy())])])
    with pytest.raises(AssertionError, match="flat index 0"):
        assert_same_bits([("a", [a]), ("b", [b])])


# ---- completeness --------------------------------------------------------------------------------------------------------
def prototypes(header):
    """{name: parameter text} of every function the header declares (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mcd_\w+)\s*\(([^;{}()]*)\)\s*;", text)}


def test_every_stream_and_workspace_prototype_has_a_row():
    import test_gpu_stream_contracts as S
    import test_gpu_workspace_contracts as Wc
    protos = {}
    for h in ("mcd_hip.h", "mcd_blaslt.h"):
        protos.update(prototypes(h))
    with_stream = sorted(n for n, args in protos.items() if re.search(r"\bmcd_(blaslt_)?stream_t\b", args))
    size_fns = sorted(n for n in protos if n.endswith("_workspace"))
    # the parser sees what it should: entries from both headers, of one line and of several
    assert {"mcd_normalize_rows", "mcd_image_minmax_normalize", "mcd_vit_attention_cls", "mcd_linear_residual_relu"} <= set(with_stream)
    assert {"mcd_col_topk_workspace", "mcd_linear_residual_workspace"} <= set(size_fns)
    assert "mcd_last_error" in protos and "mcd_last_error" not in with_stream
    assert sorted(S.STREAM_TABLE) == with_stream, sorted(set(S.STREAM_TABLE) ^ set(with_stream))
    assert all(len(rows) >= 1 for rows in S.STREAM_TABLE.values())
    assert sorted(Wc.WS_TABLE) == size_fns, sorted(set(Wc.WS_TABLE) ^ set(size_fns))
    for fn, (entries, cases) in Wc.WS_TABLE.items():
        assert len(cases) >= 1 and all(e in with_stream for e in entries), fn
        for e in entries:                    # the entry takes the pair the size function is for
            assert re.search(r"\bvoid\s*\*\s*ws\b", protos[e]) and re.search(r"\bsize_t\s+ws_bytes\b", protos[e]), e
    # every entry with a ws / ws_bytes pair is served by a size function of the table; other scratch is listed by hand
    paired = sorted(n for n, args in protos.items() if re.search(r"\bsize_t\s+ws_bytes\b", args))
    assert paired == sorted(e for entries, _ in Wc.WS_TABLE.values() for e in entries)
    scratch = sorted(n for n, args in protos.items() if re.search(r"\w+_ws\b", args))
    assert scratch == ["mcd_rank_reorder"] and set(scratch) <= set(Wc.WS_TABLE_NO_SIZE_FN)
    assert all(e in with_stream and len(c) >= 1 for e, c in Wc.WS_TABLE_NO_SIZE_FN.items())
