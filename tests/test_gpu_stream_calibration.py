"""GPU, the stream contract of depgan_eval_calibration_census, depgan_eval_temperature_sums and
depgan_eval_apply_temperature: the rows of these three entries in the table of tests/test_gpu_stream_ops.py, and the
gated call of that file run on them.

tests/test_stream_table_cpu.py holds the table (test_gpu_stream_ops.ROWS) against the header: every entry that takes a
stream needs a row.  The rows of the three entries are made HERE, with that file's own `row` decorator, when this module
is imported -- which pytest does while it collects the suite, before any test runs -- so the table is complete whenever
the suite is collected as a whole (with or without -m gpu).  The parametrised test of test_gpu_stream_ops.py took its
ids before these rows existed, so the gated call on them is the test below, the same statements on a table of these
rows alone.  Collected WITHOUT this file (tests/test_stream_table_cpu.py on its own, say) the table test reports the
three entries as missing: run it together with this file.

Two census rows, one for each way a wave's peel loop runs: "uniform" (labels and confidences uniform: many distinct bins
per wave, many passes) and "skewed" (97 % background at confidence >= 0.99: one or two passes per table).  The census and
the temperature sums synchronise their stream and write host outputs (HostOut, sync=True); their scratch is a workspace.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_gate as sg  # noqa: E402
import test_gpu_stream_ops as ops  # noqa: E402
from stream_gate import STREAM, Case, HostOut, In, Out, Scratch  # noqa: E402

PN, CC, BINS = 3000, 4, 15


def _scratch_bytes(lib, npix, Cc, bins):
    """depgan_eval_calibration_scratch_bytes, restated so that a row can be built without the library"""
    nbytes = (min(-(-npix // 1024), 1024) + 1) * ((1 + Cc) * bins * 3 + 4 + 4) * 8
    assert lib is None or int(lib.depgan_eval_calibration_scratch_bytes(npix, Cc, bins)) == nbytes
    return nbytes


def _problem(skewed):
    r = ops.rng_of("calibration-" + ("skewed" if skewed else "uniform"))
    lab = r.integers(0, CC, PN).astype(np.uint8)
    conf = r.random(PN) * (1 - 1.0 / CC) + 1.0 / CC
    if skewed:
        hot = r.random(PN) < 0.97
        lab[hot] = 0
        conf[hot] = 0.99 + 0.01 * r.random(PN)[hot]
    top = np.where(r.random(PN) < 0.8, lab, r.integers(0, CC, PN))
    prob = np.repeat(((1 - conf) / (CC - 1))[:, None], CC, 1)
    prob[np.arange(PN), top] = conf
    return prob, lab


def _census(lib, skewed):
    prob, lab = _problem(skewed)
    return Case("depgan_eval_calibration_census",
                [In(prob), 1, CC, In(lab, "zero"), -1, None, PN, BINS, 1e-7, Scratch(_scratch_bytes(lib, PN, CC, BINS)),
                 HostOut(np.int64, (1 + CC) * BINS * 3 + 4), HostOut(np.float64, 2), STREAM], sync=True)


def _temperature(lib):
    prob, lab = _problem(False)
    mask = (ops.rng_of("calibration-mask").random(PN) > 0.2).astype(np.float32)
    return Case("depgan_eval_temperature_sums",
                [In(prob.astype(np.float32)), 0, CC, In(lab, "zero"), 2, In(mask), PN, 0.5, 1e-7,
                 Scratch(_scratch_bytes(lib, PN, CC, 1)), HostOut(np.float64, 4), STREAM], sync=True)


def _apply(lib):
    prob, _ = _problem(False)
    return Case("depgan_eval_apply_temperature", [In(prob.astype(np.float32)), 0, CC, 0.5, 1e-7, Out(PN * CC * 4), PN, STREAM],
                sync=False)


MINE = []
for _fn, _tag, _build in (("depgan_eval_calibration_census", "uniform", lambda lib: _census(lib, False)),
                          ("depgan_eval_calibration_census", "skewed", lambda lib: _census(lib, True)),
                          ("depgan_eval_temperature_sums", "", _temperature),
                          ("depgan_eval_apply_temperature", "", _apply)):
    _cid = _fn[len("depgan_"):] + ("-" + _tag if _tag else "")
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
    """no GPU: the rows exist, name entries of the header that take a stream, and end in it"""
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
