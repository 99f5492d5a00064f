"""CPU: the table of tests/test_gpu_stream_ops.py covers every entry of include/depgan.h that takes a stream.

The header is read through dep_gan_im_amd._lib, the parser the binding is derived from: every prototype with a
`void* hip_stream` or `void* stream` parameter must be a row of the table or stand in its exclusion dict with a reason.
An entry added later fails here until it gets a row.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_stream_ops as ops  # noqa: E402
from dep_gan_im_amd import _lib  # noqa: E402

MAX_EXCLUDED = 3


def stream_entries():
    """names of the prototypes with a `void* hip_stream` / `void* stream` parameter, in header order"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", _lib.read_header(), flags=re.S)
    found = re.findall(r"\b(depgan_\w+)\s*\(([^()]*)\)\s*;", text)
    names = [n for n, params in found if re.search(r"\bvoid\s*\*\s*(hip_stream|stream)\s*(,|$)", params.strip())]
    assert set(names) <= set(_lib.EXPORTS)
    return names


def test_the_header_has_the_entries_this_file_was_written_for():
    names = stream_entries()
    assert "depgan_set_stream" in names
    assert len(names) - 1 >= 80, len(names)                  # 80 when the table was written, plus depgan_set_stream
    assert len(set(names)) == len(names)


def test_every_stream_entry_is_a_row_or_an_explained_exclusion():
    rows = {fn for _, fn, _ in ops.ROWS}
    entries = [n for n in stream_entries() if n != "depgan_set_stream"]      # tests/test_gpu_stream_ctx.py
    missing = [n for n in entries if n not in rows and n not in ops.EXCLUDED]
    assert not missing, "entries that take a stream and have no row in tests/test_gpu_stream_ops.py: %s" % missing
    assert len(ops.EXCLUDED) <= MAX_EXCLUDED
    assert all(isinstance(r, str) and len(r) > 20 for r in ops.EXCLUDED.values())
    assert not (set(ops.EXCLUDED) & rows), "excluded and in the table"
    assert set(ops.EXCLUDED) <= set(entries)
    assert len([n for n in entries if n in rows]) >= len(entries) - MAX_EXCLUDED


def test_every_row_names_an_existing_entry_that_takes_a_stream():
    entries = set(stream_entries())
    for cid, fn, build in ops.ROWS:
        assert fn in _lib.EXPORTS and fn in entries, (cid, fn)
    ids = [cid for cid, _, _ in ops.ROWS]
    assert len(set(ids)) == len(ids)
    assert set(ops.NEGATIVE_CONTROL) <= set(ids)


def test_host_only_plan_entries_take_no_stream_and_have_no_row():
    """the entries that report a launcher's plan (`Host only` in the header) enqueue nothing: no stream parameter, no row;
    every depgan_debug_*_plan / *_choice prototype of the header stands in the list"""
    entries, rows = set(stream_entries()), {fn for _, fn, _ in ops.ROWS}
    assert len(set(ops.HOST_ONLY)) == len(ops.HOST_ONLY) >= 4
    for fn in ops.HOST_ONLY:
        assert fn in _lib.EXPORTS and fn not in entries and fn not in rows and fn not in ops.EXCLUDED, fn
    plans = [n for n in _lib.EXPORTS if re.fullmatch(r"depgan_debug_\w+_(plan|choice)", n)]
    assert sorted(plans) == sorted(ops.HOST_ONLY)
    assert "depgan_debug_deconv_fwd_plan" in plans and "depgan_op_deconv2x2_ex" in rows


def test_every_row_has_the_entrys_parameter_count_and_one_stream(lib):
    """the builders run on the host (they ask the library for scratch sizes, host-only calls): the argument list of every
    row has the length of the header's prototype and exactly one stream"""
    for cid, fn, build in ops.ROWS:
        case = build(lib)
        assert case.fn == fn, cid
        assert len(case.args) == len(_lib._HDR.prototypes[fn][1]), (cid, len(case.args))
        assert sum(a is ops.STREAM for a in case.args) == 1 and case.args[-1] is ops.STREAM, cid
        for a in case.args + case.extra:
            if isinstance(a, ops.In):
                assert a.poison in ("nan", "nan64", "bf16nan", "zero"), cid
                if a.data.dtype.kind in "iu" and a.data.dtype.itemsize != 2:
                    assert a.poison == "zero", "%s: an integer operand (a code, an index, a set) is poisoned with zero" % cid
