"""ctypes binding of lib/libnttmul_probe.so (tests/probe/arith_probe.hip): the device primitives
of csrc/modarith.hpp / csrc/mac_dev.hpp one at a time.  Listing the ops and reading the plan's
tables needs no GPU; run() does."""
import ctypes
import os

import numpy as np

import nttmul

LIB_PATH = os.path.join(nttmul.PKG_DIR, "lib", "libnttmul_probe.so")
_LIB = None


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run __graft_entry__.build()")
        lib = ctypes.CDLL(LIB_PATH)
        vp, u64, i32p = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)
        lib.probe_op_name.argtypes = [ctypes.c_int]
        lib.probe_op_name.restype = ctypes.c_char_p
        lib.probe_op_shape.argtypes = [ctypes.c_char_p, i32p, i32p, i32p]
        lib.probe_tables.argtypes = [u64, vp, vp, vp]
        lib.probe_consts.argtypes = [u64, vp]
        lib.probe_run.argtypes = [ctypes.c_char_p, u64, vp, vp, ctypes.c_size_t]
        lib.nttmul_table.argtypes = [ctypes.c_uint32, u64, u64, ctypes.c_int, vp]
        _LIB = lib
    return _LIB


def _ok(st, what):
    if st != 0:
        raise RuntimeError(f"{what}: status {st}")


def ops():
    """The op names the library exports, in its order."""
    lib = load()
    return [lib.probe_op_name(i).decode() for i in range(lib.probe_op_count())]


def shape(op):
    """(operand words, result words, word bits) of an op."""
    nin, nout, bits = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _ok(load().probe_op_shape(op.encode(), nin, nout, bits), op)
    return nin.value, nout.value, bits.value


def tables(q, n=256):
    """The pair tables of the library's make_plan(256, q), the signed-form flags of its forward
    entries, and the tables' plain values (nttmul_table mixed_powers_rev / inv_mixed_powers_rev):
    (fw_pairs [n, 2], iw_pairs [n, 2], fw_signed [n], fw_plain [n], iw_plain [n])."""
    lib = load()
    fw, iw = np.zeros((n, 2), np.uint64), np.zeros((n, 2), np.uint64)
    sg = np.zeros(n, np.uint8)
    _ok(lib.probe_tables(q, fw.ctypes.data, iw.ctypes.data, sg.ctypes.data), "probe_tables")
    plain = []
    for which in (9, 11):
        t = np.zeros(n, np.uint64)
        _ok(lib.nttmul_table(n, q, 0, which, t.ctypes.data), "nttmul_table")
        plain.append(t)
    return fw, iw, sg, plain[0], plain[1]


CONSTS = ("f", "fs", "wf", "wfs", "f4", "f4s", "wf4", "wf4s", "f8", "f8s", "wf8", "wf8s",
          "qinv_neg", "c32", "as", "q2")


def consts(q):
    """The scale pairs of the plan and the constants make_params derives, by name."""
    out = np.zeros(len(CONSTS), np.uint64)
    _ok(load().probe_consts(q, out.ctypes.data), "probe_consts")
    return dict(zip(CONSTS, (int(v) for v in out)))


def run(op, q, words):
    """Run `op` at modulus q on the operand word arrays (uint64, one per operand word); returns
    one uint64 array per result word."""
    nin, nout, _ = shape(op)
    assert len(words) == nin, (op, len(words), nin)
    count = len(words[0])
    src = np.ascontiguousarray(np.stack(words), dtype=np.uint64)
    dst = np.zeros((nout, count), np.uint64)
    _ok(load().probe_run(op.encode(), q, src.ctypes.data, dst.ctypes.data, count), op)
    return list(dst)
