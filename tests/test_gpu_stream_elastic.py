"""GPU, the stream contract of depgan_data_augment_fields: the rows of this entry in the table of
tests/test_gpu_stream_ops.py, and the gated call of that file run on them.

tests/test_stream_table_cpu.py holds the table (test_gpu_stream_ops.ROWS) against the header: every entry that takes a
stream needs a row.  The rows of this entry are made HERE, with that file's own `row` decorator, when this module is
imported -- which pytest does while it collects the suite, before any test runs -- so the table is complete whenever
the suite is collected as a whole (with or without -m gpu).  The parametrised test of test_gpu_stream_ops.py took its
ids before these rows existed, so the gated call on them is the test below, the same statements on a table of these
rows alone.  Collected WITHOUT this file (tests/test_stream_table_cpu.py on its own, say) the table test reports the
entry as missing: run it together with this file.

Two rows, one for each way the kernel evaluates the fields: 9 x 7 per lane, 2 x 256 through LDS."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_gate as sg  # noqa: E402
import test_gpu_stream_ops as ops  # noqa: E402
from stream_gate import STREAM, Case, In, Out  # noqa: E402


def _fields(H, W):
    n_src, n, nicg, gh, gw = 3, 2, 1, 4, 5
    r = ops.rng_of("augment_fields")
    params = np.float32([[1, 0, 0.5, 0, 1, -1.25, 1.5, 0.1], [0.9, 0.1, 0, -0.1, 0.9, 1, 1, 0]])
    return Case("depgan_data_augment_fields",
                [In(ops.f32(r, n_src, H, W, nicg)), nicg, In(r.integers(0, 4, (n_src, H, W)).astype(np.uint8), "zero"), 1, 4,
                 In(np.array([2, 0], np.int64), "zero"), n_src, In(params), In(ops.f32(r, n, 3, gh, gw)), gh, gw, n, H, W,
                 1, -1.0, 3, ops.F(n * H * W * nicg), Out(n * H * W), ops.F(n * H * W * 3), STREAM], sync=False)


MINE = []
for _fn, _tag, _build in (("depgan_data_augment_fields", "lanes", lambda lib: _fields(9, 7)),
                          ("depgan_data_augment_fields", "row", lambda lib: _fields(2, 256))):
    _cid = _fn[len("depgan_"):] + "-" + _tag
    if _cid not in [r[0] for r in ops.ROWS]:             # a second import of this module adds nothing
        ops.row(_fn, _tag)(_build)
    MINE.append(_cid)


class Table:
    """test_gpu_stream_ops.Table over the rows above alone"""

    def __init__(self, lib):
        import torch
        self.bound, self.want, self.secs = {}, {}, {}
        for cid, fn, build in ops.ROWS:
            if cid in MINE:
                self.bound[cid] = b = sg.Bound(lib, build(lib))
                self.want[cid], self.secs[cid] = sg.null_run(b)
        self.ms = sg.gate_ms(max(self.secs.values()))
        self.gate = sg.Gate(sg.session_delay(), self.ms)
        self.s = torch.cuda.Stream()


@pytest.fixture(scope="module")
def table(lib):
    return Table(lib)


def test_the_rows_are_in_the_table():
    """no GPU: the rows exist, name an entry of the header that takes a stream, and end in it"""
    from dep_gan_im_amd import _lib
    rows = {cid: (fn, build) for cid, fn, build in ops.ROWS}
    for cid in MINE:
        fn, build = rows[cid]
        assert fn in _lib.EXPORTS
        case = build(None)
        assert len(case.args) == len(_lib._HDR.prototypes[fn][1]) and case.args[-1] is STREAM


@pytest.mark.gpu
@pytest.mark.parametrize("cid", MINE)
def test_entry_enqueues_everything_on_the_stream_it_is_given(table, cid):
    b, want = table.bound[cid], table.want[cid]
    assert int(want[0].view(np.int64)[0]) == 0, "%s: status %d on the null stream" % (cid, int(want[0].view(np.int64)[0]))
    got = sg.gated_run(b, table.gate, table.s)
    assert sg.same(got, want), "%s on a side stream differs from the null stream: %s" % (cid, sg.first_difference(b, got, want))
    bad, ro = b.guards_intact(got)
    assert not bad and not ro, "%s: wrote outside its outputs (guards of buffers %s, read-only buffers %s)" % (cid, bad, ro)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", MINE)
def test_the_gate_detects_a_call_on_the_wrong_stream(table, cid):
    """the negative control of test_gpu_stream_ops.py on these rows: handed the NULL stream the entry works on poison"""
    import torch
    b = table.bound[cid]
    b.reset()
    torch.cuda.synchronize()
    e_gate = torch.cuda.Event()
    with torch.cuda.stream(table.s):
        table.gate.delay.enqueue(table.ms)
        e_gate.record(table.s)
        for buf in b.bufs:
            buf.load()
    assert not e_gate.query(), "inconclusive: the gate was open before the call"
    rc, _ = b.call(0)
    table.s.synchronize()
    torch.cuda.synchronize()
    got = b.snapshot(rc)
    assert not sg.same(got, table.want[cid]), "%s on the wrong stream went unnoticed: the gate proves nothing" % cid
