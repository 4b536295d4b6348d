"""The device arithmetic at the edges of its range contracts.

lib/libnttmul_probe.so (tests/probe/arith_probe.hip) runs each __device__ primitive of
csrc/modarith.hpp and each mac_add overload of csrc/mac_dev.hpp on its own, with the constants
the library's planner and make_params give a launch.  tests/arith_contracts.py states, per op, the
operand domains of the primitive's comment, the value of every output and the range it must lie
in; this module feeds each op the edge cross product of its domains, every twiddle pair of the
plan's two tables plus the edge twiddles, and seeded random tuples, and asserts value AND range: a
result that is congruent but outside its declared range fails."""
import pytest

import arith_contracts as C
import probe_lib
from test_gpu_parity import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

CLASS_Q = [(cls, q) for cls in ("Arith32", "Arith32P", "Arith32P3", "Arith32W", "Arith64")
           for q in C.MODULI[cls]]


def _rows_of(cls):
    """The rows that run in `cls` (mac_add's with their class; Arith32P3's on their own)."""
    return [r for r in C.ROWS if (r.op.split(".")[0] if not r.op.startswith("mac_add")
                                  else C.op_class(r.op)) == cls]


_TW = {}


def twiddles(q):
    """The plan's pair tables and scale pairs as the library built them, and the edge twiddles."""
    if q not in _TW:
        fw, iw, sg, fwp, iwp = probe_lib.tables(q)
        tw = C.twiddle_lists(q, fw, iw, sg, fwp, iwp)
        k = probe_lib.consts(q)
        bits = 32 if q < (1 << 32) else 64
        f = pow(256, -1, q) * (1 << bits) % q
        uform, sform = ("tw_u", "tw_s") if q < (1 << 31) else ("tw_m",) * 2 if bits == 32 else ("tw_h",) * 2
        for mul, name in ((1, ""), (4, "4"), (8, "8")):     # F, 4F, 8F and w F ..., w = iw[1]
            tw[uform].insert(0, (f * mul % q, k["f" + name], k["f" + name + "s"]))
            tw[sform].insert(0, (int(iwp[1]) * f * mul % q, k["wf" + name], k["wf" + name + "s"]))
        _TW[q] = tw
    return _TW[q]


@pytest.mark.parametrize("cls,q", CLASS_Q)
def test_primitives_meet_their_contracts(cls, q, torch_cuda):
    # (torch_cuda as in every GPU test: the process's HIP runtime is torch's, loaded first)
    rows = _rows_of(cls)
    assert rows
    tw = twiddles(q)
    failed = []
    for row in rows:             # every row runs: one broken contract does not hide the next
        words, values = C.tuples(row, q, tw)
        outs = probe_lib.run(row.op, q, words)
        try:
            C.check(row, q, values, outs)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
