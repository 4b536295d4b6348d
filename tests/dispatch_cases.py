"""Case tables of the GPU suite and a pure-Python mirror of the library's kernel selection.

Two things live here, both plain data and arithmetic (no GPU, no library, no oracle):

* the axes the GPU tests are parametrised over (moduli, sizes, word widths, batches, modes), as
  `Case` rows, so that what the suite launches is written down in one place;
* `kernels_of(case)`: the kernels a case launches, as `nttmul.kernel_key` strings, restating the
  selection rules of csrc/kernels.hip (with_arith, with_io, product, xform, launch_pointwise,
  launch_bitrev, launch_fill, launch_check_range, launch_server), csrc/kernels_dev.hpp
  (launch_rows, rows_prio, xform_upg) and csrc/nttmul.cpp (run_device, run_server).

tests/test_kernel_ledger.py holds the two against the built library: every kernel of
libnttmul.so is either launched by a case or matched by an `UNREACHABLE` rule with its reason,
and every kernel a case names exists.  tests/test_gpu_ledger.py anchors the product part of the
mirror to the library's own dispatch (nttmul_kernel_name).
"""
from collections import namedtuple

Q0 = 12289
Q20 = 786433                # 3 * 2^18 + 1, 20 bits
Q31 = 2013265921            # 15 * 2^27 + 1, the benchmark modulus
Q30 = 1073479681            # < 2^30
Q32 = 4293918721            # 0xFFF00001, full 32-bit word
Q62 = 0x3FFFFFFFFFE80001    # 62-bit, 2^17 | q - 1
Q31HI = 2147352577          # the ends of the Arith32P3 range 2^30 < q < 2^31, 2^17 | q - 1
Q31LO = 1073872897
SEED33 = 33
Q33 = 7863402497            # test_gpu_parity._random_primes([33], 17, SEED33)[0]

PLANTARD = (Q31HI, Q31LO, Q31, Q20)     # Arith32P
WIDE = (Q32,)                           # Arith32W
ARITH64 = (Q62, Q33)                    # Arith64
# one modulus per arithmetic class
CLASS_MODULI = (Q31HI, Q32, Q62)

XF_MODES = (0, 2, 1, 3, 1 | 4, 3 | 4)   # nttmul.XF_INVERSE = 1, XF_REV2STD = 2, XF_UNSCALED = 4
ALL_N = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
MULTIPASS_N = (8192, 16384, 32768, 65536)
MI355X_CUS = 256

# op: "multiply" | "transform" | "pointwise" | "fill"
# path: "device" (the *_device entry points and the launch path of the host calls) or "server"
#   (a host multiply the resident server takes: run_server's eligibility holds)
# mode: transform mode bits;  validate: NTTMUL_FLAG_VALIDATE;  prio: nttmul_params.issue_prio;
# prio_ok: LaunchTables.prio_ok (0 after a product launch on another stream)
Case = namedtuple("Case", "op n q word_bits batch mode validate path prio prio_ok",
                  defaults=(0, False, "device", 0, 1))


def native_bits(q):
    return 32 if q < (1 << 32) else 64


def word_options(q):
    """The word widths a caller may pass for q: the native one, and 64 on a 32-bit modulus."""
    return (32, 64) if q < (1 << 32) else (64,)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def arith_class(q):
    """kernels.hip with_arith on planner.cpp's word_bits: the class follows q alone."""
    return "Arith32P" if q < (1 << 31) else "Arith32W" if q < (1 << 32) else "Arith64"


def p3_fold_ok(q):
    """arith_select.hpp p3_fold_ok."""
    if q >= (1 << 31) or q < 3:
        return False
    s1 = 4 * (q - 1) * (q - 1)
    return (s1 >> 32) * ((1 << 32) % q) + 0xFFFFFFFF + s1 < (1 << 64)


def _io(bits):
    return "u32" if bits == 32 else "u64"


def _logn(n):
    assert n & (n - 1) == 0 and 256 <= n <= 65536
    return n.bit_length() - 1


def square_split(n, q):
    """64-bit arithmetic at n = 65536 runs 256 x 256 (NTTMUL_C5_SQ)."""
    return n == 65536 and q >= (1 << 32)


def row_split(n, q):
    """(LOGS, L1): the row pass a product or transform of n words runs, after L1 column stages."""
    logn = _logn(n)
    if logn <= 12:
        return logn, 0
    return (8, 8) if square_split(n, q) else (12, logn - 12)


def xform_upg(n, q):
    """kernels_dev.hpp xform_upg: polynomials per thread group of a standalone transform."""
    return 2 if n <= 4096 and q < (1 << 32) else 1


def rows_prio(case, cus=MI355X_CUS):
    """launch_rows / rows_prio: the issue-prioritised fused product, u32 Plantard products only."""
    logs = _logn(case.n)
    if logs > 12 or arith_class(case.q) != "Arith32P" or case.word_bits != 32 or not case.batch:
        return False
    if case.prio:
        return case.prio > 0
    nt = 64 if logs == 10 else 256
    per_block = nt // ((1 << logs) // 16)
    blocks = (case.batch + per_block - 1) // per_block
    return blocks * (nt // 64) <= (cus if case.prio_ok else 0) * 16


def server_eligible(case):
    """nttmul.cpp run_server: u32 host products of at most 1024 words per operand, Plantard
    moduli, n <= 1024.  (Its twiddle-count condition never declines: the planner's tables hold
    exactly n pairs.)"""
    return (case.op == "multiply" and case.word_bits == 32 and case.n <= 1024
            and case.batch * case.n <= 1024 and arith_class(case.q) == "Arith32P")


def _product(case, cus):
    a, io, w = arith_class(case.q), _io(case.word_bits), _io(native_bits(case.q))
    logs, l1 = row_split(case.n, case.q)
    if l1 == 0:
        if a == "Arith32P" and logs == 12 and p3_fold_ok(case.q):
            a = "Arith32P3"
        prio = "true" if rows_prio(case, cus) else "false"
        return [f"k_rows<{a},{io},{io},{logs},0,{prio}>"]
    if square_split(case.n, case.q):
        return [f"k_cols8<{a},{io},{w},0,2>", f"k_rows<{a},{w},{w},8,8,false>",
                f"k_cols8<{a},{w},{io},1,1>"]
    return [f"k_cols_fwd<{a},{io},{l1},2>", f"k_rows<{a},{w},{w},{logs},{l1},false>",
            f"k_cols_inv<{a},{io},{l1}>"]


def _transform(case):
    a, io, w = arith_class(case.q), _io(case.word_bits), _io(native_bits(case.q))
    logs, l1 = row_split(case.n, case.q)
    inv = case.mode & 1
    out = []
    # run_device: the kernels run forward std2rev and inverse rev2std; the other two orders go
    # through a bit-reversal into the scratch and one in place on the output
    reorder = bool(inv) != bool(case.mode & 2)
    if reorder:
        out.append(f"k_bitrev<{io}>")
    if l1 == 0:
        out.append(f"k_xform<{a},{io},{io},{logs},0,{inv}>")
    elif square_split(case.n, case.q):
        out += ([f"k_cols8<{a},{io},{w},0,1>", f"k_xform<{a},{w},{io},8,8,0>"] if not inv else
                [f"k_xform<{a},{io},{w},8,8,1>", f"k_cols8<{a},{w},{io},1,1>"])
    else:
        out += ([f"k_cols_fwd<{a},{io},{l1},1>", f"k_xform<{a},{w},{io},{logs},{l1},0>"] if not inv
                else [f"k_xform<{a},{io},{w},{logs},{l1},1>", f"k_cols_inv<{a},{io},{l1}>"])
    if reorder:
        out.append(f"k_bitrev_inplace<{io}>")
    return out


def kernels_of(case, cus=MI355X_CUS):
    """The kernel_keys `case` launches, in launch order."""
    assert case.word_bits == 64 or case.q < (1 << 32), "io_ok refuses 32-bit words for q >= 2^32"
    io = _io(case.word_bits)
    if case.path == "server":
        assert server_eligible(case)
        return [f"k_server<Arith32P,{_logn(case.n)}>"]     # (validation runs on the host)
    out = [f"k_check_range<{io}>"] if case.validate else []
    if case.op == "multiply":
        return out + _product(case, cus)
    if case.op == "transform":
        return out + _transform(case)
    if case.op == "pointwise":
        a = arith_class(case.q)
        return out + [f"k_pointwise<{'Arith32' if a == 'Arith32P' else a},{io}>"]
    if case.op == "fill":
        return [f"k_fill<{io}>"]
    raise ValueError(case.op)


def product_keys(case, cus=MI355X_CUS):
    """The product kernels of `case` without the range check."""
    return [k for k in kernels_of(case, cus) if not k.startswith("k_check_range")]


# Kernels the library holds that no call can launch: (regular expression over the kernel_key,
# reason).  The first matching rule names a kernel's reason.
UNREACHABLE = (
    (r"k_\w+<Arith64,(u32(,.*)?|u64,u32,.*)>",
     "Arith64 on u32 caller words: io_ok refuses 32-bit words for q >= 2^32"),
    (r"k_cols_fwd<\w+,u\d+,5,2>|k_cols_inv<\w+,u\d+,5>|k_rows<\w+,u\d+,u\d+,11,5,false>",
     "the 32 x 2048 split of n = 65536 sits behind NTTMUL_SPLIT16 == 5 (settled at 4)"),
    (r"k_rows<Arith32P,u\d+,u\d+,12,0,(false|true)>",
     "p3_fold_ok holds for every prime q < 2^31, so n = 4096 always takes Arith32P3"),
    (r"k_cols_fwd<Arith64,u64,4,[12]>|k_cols_inv<Arith64,u64,4>|k_rows<Arith64,u64,u64,12,4,false>"
     r"|k_xform<Arith64,u64,u64,12,4,[01]>",
     "Arith64 at n = 65536 takes the square split (NTTMUL_C5_SQ), never 16 x 4096"),
)


# ---------------------------------------------------------------------------------------------
# Case tables: the new modules
# ---------------------------------------------------------------------------------------------

# 1a. multi-pass products in 64-bit words on 32-bit moduli (tests/test_gpu_u64_words.py)
U64_MULTIPASS = [(n, q) for n in MULTIPASS_N for q in (Q31HI, Q31LO, Q32)]
# (the fused products in 64-bit words: test_random_prime_sweep runs n = 256, 1024 and 4096 only)
U64_FUSED = [(n, q) for n in (256, 512, 1024, 2048, 4096) for q in (Q31HI, Q31LO, Q32)]
# 1b. every transform mode and pointwise, every size, one modulus per class, both word widths
# (negacyclic and cyclic), and three more moduli, negacyclic, at the sizes no other test runs
XF_SWEEP = ([(n, q, cyclic) for n in ALL_N for q in CLASS_MODULI for cyclic in (False, True)]
            + [(n, q, False) for n in (512, 2048, 32768) for q in (Q33, Q20, Q31LO)])
XF_SWEEP_BATCHES = (3, 1)
# 1c. the device path in 64-bit words
U64_DEVICE = [(4096, Q31, 37), (8192, Q31HI, 5), (65536, Q32, 3)]
# 1d. range validation
VALIDATE = [(1024, Q31), (8192, Q32)]
# 1e. the host path in several chunks
U64_HOST_CHUNKS = (4096, Q31, 600)
# 2. sub-batched transforms (scratch_mb = 1): n, q, word_bits, batch, modes
SUBBATCH = [
    (4096, Q31, 32, 129, (2, 1)),
    (8192, Q31, 32, 65, XF_MODES),
    (8192, Q31, 64, 65, (2, 3)),
    (65536, Q62, 64, 5, XF_MODES),
]
SUBBATCH_PRODUCT = (8192, Q31, 64, 65)
# 3. the resident server at every size it serves: (n, batch)
SERVER_SHAPES = [(512, 1), (512, 2), (1024, 1), (256, 2), (256, 3), (256, 4)]
SERVER_BITS = (14, 17, 20, 24, 28, 30, 31)
SERVER_NAMED = (Q0, Q31, Q31HI, Q31LO)

# 4. inputs that saturate a stage boundary (tests/test_gpu_saturation.py, tests/saturation.py)
SAT_N = (256, 1024, 4096, 8192, 65536)
# nttmul.find_prime(n, 31): the largest prime below 2^31 with 2n | q - 1
SAT_P31 = {256: 2147483137, 1024: 2147473409, 4096: 2147377153, 8192: Q31HI, 65536: Q31HI}
SAT_U64_N = (4096, 8192)        # 64-bit words on the 32-bit moduli
SAT_SERVER = (256, Q31HI)       # the same family call by call through the resident server
SAT_MAC_N = (256, 4096)
SAT_MAC_TERMS = 7


def sat_moduli(n):
    out = []
    for q in (Q31HI, SAT_P31[n], Q32, Q62):
        if q not in out:
            out.append(q)
    return out


def sat_products():
    """(n, q, word_bits): one launch each."""
    return [(n, q, w) for n in SAT_N for q in sat_moduli(n)
            for w in ((native_bits(q),) + ((64,) if q < (1 << 32) and n in SAT_U64_N else ()))]


def sat_batch(n):
    """Polynomials per launch: two value pairs and one random partner per m = 1, 2, ..., n."""
    return 3 * n.bit_length()


# ---------------------------------------------------------------------------------------------
# Case tables: the caller's memory (tests/test_gpu_footprint.py, tests/guarded.py)
# ---------------------------------------------------------------------------------------------

# A footprint case: the exported entry point it calls, the launch it makes (a Case row, so the
# kernel ledger sees it), and how it is called.  alias: "" (distinct buffers), "out=in" (a
# transform in place), "c=a" / "c=b" (a pointwise product over an operand).  host: "" for a
# *_device call, else the host path the call must report through nttmul_last_host_path:
# "staged" (0), "direct" (1), "zero_copy" (2), "server" (3).
Footprint = namedtuple("Footprint", "entry case cyclic scratch_mb alias host",
                       defaults=(False, 0, "", ""))

FP_N = (256, 512, 1024, 2048, 4096, 8192, 65536)
FP_CYCLIC_N = (256, 4096, 65536)
FP_INPLACE_N = (256, 4096, 8192, 65536)
FP_INPLACE_BATCH = 3
# the sub-batched path (scratch_mb = 1), shapes of SUBBATCH: sub-batches of 32 + 32 + 1 and
# 2 + 2 + 1 polynomials; one product and the two reordered transform modes
FP_SUBBATCH = [(8192, Q31, 32, 65), (65536, Q62, 64, 5)]
FP_SUBBATCH_MODES = (2, 1)
# NTTMUL_FLAG_VALIDATE, one case per arithmetic class (k_check_range<u32> and <u64>): the call
# returns OK, so the range check read no guard word (every guard word is >= q)
FP_VALIDATE = [(512, Q31HI, 32), (2048, Q32, 64), (256, Q62, 64)]
# Host-buffer calls.  Staged copies go through CopyPool::copy (csrc/copy_pool.hpp), which splits
# a copy of at least 2 MiB (parts = min(threads, bytes / 1 MiB) > 1) into pieces of
# ceil(bytes / parts) rounded up to 4 KiB.  At n = 4096 in 32-bit words (16 KiB per polynomial)
# two pieces are always equal (batch * 8 KiB is whole pages); the smallest batch with unequal
# pieces is 193: 3,162,112 bytes, three parts, pieces of 1,056,768 + 1,056,768 + 1,048,576 bytes.
FP_STAGED_SPLIT = (4096, Q31, 32, 193)
FP_HOST_BATCH = 3
FP_HOST_SHAPES = {
    # path: (n, q, word_bits) for multiply, forward, inverse, pointwise and transform
    "staged": [(1024, Q32, 64), (8192, Q62, 64)],
    "direct": [(4096, Q31, 32), (8192, Q62, 64)],
    # chunks of at most 64 KiB per operand (the default zero_copy_kb) at n <= 4096; a non-Plantard
    # modulus, so the small products are not the resident server's
    "zero_copy": [(1024, Q32, 32), (512, Q62, 64)],
}
FP_SERVER = [(256, Q31HI, 1), (256, Q31HI, 3)]


def fp_batches(n):
    """1 and 33 up to n = 4096: 33 leaves exactly one live unit in the last block for every
    units-per-block value of the code (2, 4, 8, 16, 32) and a half-empty last pair of the
    two-polynomial transforms.  1 and 3 above (3 x 65536 x 8 B = 1.5 MiB per operand)."""
    return (1, 33) if n <= 4096 else (1, 3)


def fp_device_shapes():
    """(n, q, cyclic): every size and class negacyclic, three sizes cyclic."""
    return ([(n, q, False) for n in FP_N for q in CLASS_MODULI]
            + [(n, q, True) for n in FP_CYCLIC_N for q in CLASS_MODULI])


def footprint_cases():
    out = []
    F = Footprint

    def xf(n, q, w, batch, mode, **kw):
        return Case("transform", n, q, w, batch, mode=mode, **kw)

    for n, q, cyclic in fp_device_shapes():
        for w in word_options(q):
            for batch in fp_batches(n):
                out += [F("nttmul_fill_random_device", Case("fill", n, q, w, batch), cyclic),
                        F("nttmul_multiply_batch_device", Case("multiply", n, q, w, batch), cyclic),
                        F("nttmul_forward_batch_device", xf(n, q, w, batch, 0), cyclic),
                        F("nttmul_inverse_batch_device", xf(n, q, w, batch, 3), cyclic),
                        F("nttmul_pointwise_batch_device", Case("pointwise", n, q, w, batch), cyclic)]
                out += [F("nttmul_transform_device", xf(n, q, w, batch, m), cyclic) for m in XF_MODES]
    for n, q, w, batch in FP_SUBBATCH:
        out.append(F("nttmul_multiply_batch_device", Case("multiply", n, q, w, batch), scratch_mb=1))
        out += [F("nttmul_transform_device", xf(n, q, w, batch, m), scratch_mb=1)
                for m in FP_SUBBATCH_MODES]
    for n, q, w in FP_VALIDATE:
        b = fp_batches(n)[1]
        out += [F("nttmul_multiply_batch_device", Case("multiply", n, q, w, b, validate=True)),
                F("nttmul_forward_batch_device", xf(n, q, w, b, 0, validate=True)),
                F("nttmul_pointwise_batch_device", Case("pointwise", n, q, w, b, validate=True))]
    # in place
    b = FP_INPLACE_BATCH
    for n in FP_INPLACE_N:
        for q in CLASS_MODULI:
            for cyclic in (False, True):
                for w in word_options(q):
                    out += [F("nttmul_transform_device", xf(n, q, w, b, m), cyclic, alias="out=in")
                            for m in XF_MODES]
                    out += [F("nttmul_pointwise_batch_device", Case("pointwise", n, q, w, b), cyclic,
                              alias=al) for al in ("c=a", "c=b")]
    for n, q, w, batch in FP_SUBBATCH:
        out += [F("nttmul_transform_device", xf(n, q, w, batch, m), scratch_mb=1, alias="out=in")
                for m in XF_MODES]
    # host buffers
    n, q, w, batch = FP_STAGED_SPLIT
    out.append(F(f"nttmul_multiply_batch_u{w}", Case("multiply", n, q, w, batch), host="staged"))
    b = FP_HOST_BATCH
    for path, shapes in FP_HOST_SHAPES.items():
        for n, q, w in shapes:
            out += [F(f"nttmul_multiply_batch_u{w}", Case("multiply", n, q, w, b), host=path),
                    F(f"nttmul_forward_batch_u{w}", xf(n, q, w, b, 0), host=path),
                    F(f"nttmul_inverse_batch_u{w}", xf(n, q, w, b, 3), host=path),
                    F(f"nttmul_pointwise_batch_u{w}", Case("pointwise", n, q, w, b), host=path),
                    F(f"nttmul_transform_batch_u{w}", xf(n, q, w, b, 2), host=path),
                    # and in place, as the ntt256 shims call them
                    F(f"nttmul_transform_batch_u{w}", xf(n, q, w, b, 1), host=path, alias="out=in"),
                    F(f"nttmul_pointwise_batch_u{w}", Case("pointwise", n, q, w, b), host=path,
                      alias="c=a")]
    for n, q, batch in FP_SERVER:
        out.append(F("nttmul_multiply_batch_u32", Case("multiply", n, q, 32, batch, path="server"),
                     host="server"))
    # the one-polynomial entry points: the server on 32-bit words, zero-copy on 64-bit words
    out.append(F("nttmul_multiply_u32", Case("multiply", 256, Q31HI, 32, 1, path="server"),
                 host="server"))
    out.append(F("nttmul_multiply_u64", Case("multiply", 256, Q62, 64, 1), host="zero_copy"))
    return out


def units_per_block(case, cus=MI355X_CUS):
    """{kernel_key: (units per workgroup, units of the launch, words per unit)} for the kernels
    `case` launches.
    A unit is what one thread group of the kernel owns and what its end-of-batch predicate counts:

    * k_rows: rows of 2^LOGS words, PB = rows_threads(LOGS) / (2^LOGS / 16) per workgroup with
      rows_threads(10) = 64, else 256 (csrc/kernels_dev.hpp:545, :591, `live` :600); a multi-pass
      row pass runs batch * 2^L1 rows;
    * k_xform: 256 / (2^LOGS / 16) thread groups of xform_upg = 2 polynomials on 32-bit
      arithmetic with L1 == 0, else 1 (kernels_dev.hpp:1126, :1134, `live` / `live2` :1141;
      csrc/kernels.hip:151 sizes the grid with the same product);
    * k_cols8: one workgroup per 16 columns, the grid is exact (kernels_dev.hpp:1307);
    * k_cols_fwd / k_cols_inv: one column per thread, 256 per workgroup, 2^LOGS columns per
      polynomial (kernels_dev.hpp:1216, :1254; kernels.hip:44, :173);
    * k_pointwise, k_fill, k_bitrev, k_bitrev_inplace, k_check_range: one word per thread, 256 per
      workgroup (kernels_dev.hpp:1199, :1395, :1409, :1416, :1429);
    * k_server: one resident workgroup, results leave through the library's own mailbox and a
      host memcpy of batch * n words (csrc/nttmul.cpp:686)."""
    import re
    out = {}
    for key in kernels_of(case, cus):
        name, args = re.fullmatch(r"(\w+)<(.*)>", key).groups()
        args = args.split(",")
        if name == "k_rows":
            logs, l1 = int(args[3]), int(args[4])
            out[key] = ((64 if logs == 10 else 256) // ((1 << logs) // 16), case.batch << l1, 1 << logs)
        elif name == "k_xform":
            logs, l1 = int(args[3]), int(args[4])
            upg = 2 if l1 == 0 and args[0] != "Arith64" else 1
            out[key] = (256 // ((1 << logs) // 16) * upg, case.batch << l1, 1 << logs)
        elif name == "k_cols8":
            out[key] = (1, case.batch * 16, 4096)
        elif name in ("k_cols_fwd", "k_cols_inv"):
            out[key] = (256, case.batch * (case.n >> int(args[2])), 1)
        elif name == "k_server":
            out[key] = (1, case.batch, case.n)
        else:
            assert name in ("k_pointwise", "k_fill", "k_bitrev", "k_bitrev_inplace",
                            "k_check_range"), key
            out[key] = (256, case.batch * case.n, 1)
    return out


DEFAULT_SCRATCH_MB = 512


def chunks(case, scratch_mb=0):
    """csrc/nttmul.cpp run_device / sub_batch: the sub-batches of a device call.  A multi-pass
    product or transform and a reordered transform go through the scratch, at most scratch_mb MiB
    per buffer in whole polynomials (of the native word for a multi-pass call, of the caller's
    word for a reordered fused transform), never less than one; every other call is one launch
    over the whole batch."""
    multipass = case.n > 4096 and case.op in ("multiply", "transform")
    reorder = case.op == "transform" and bool(case.mode & 1) != bool(case.mode & 2)
    if not (multipass or reorder) or not case.batch:
        return [case.batch]
    poly = case.n * ((native_bits(case.q) if multipass else case.word_bits) // 8)
    chunk = max(1, min(case.batch, ((scratch_mb or DEFAULT_SCRATCH_MB) << 20) // poly))
    return [min(chunk, case.batch - p) for p in range(0, case.batch, chunk)]


# Kernels whose launches never end in a partial workgroup, whatever the batch: (regular expression
# over the kernel_key, reason).  Every other multi-unit kernel needs a footprint case with one.
FP_ALWAYS_WHOLE = (
    (r"k_(pointwise|fill|bitrev|bitrev_inplace|check_range)<.*>|k_cols_(fwd|inv)<.*>",
     "one word or column per thread: batch * n and batch * 2^LOGS are multiples of 256"),
    (r"k_(rows|xform)<\w+,u\d+,u\d+,8,8,\w+>",
     "the square split's row pass runs batch * 256 rows, 16 per workgroup"),
)


def fp_guard_words(case):
    """The guard width tests/guarded.py gives a libnttmul call: one batch entry is n words."""
    from guarded import guard_words
    return guard_words(case.n)


# ---------------------------------------------------------------------------------------------
# Case tables: the parametrisations of tests/test_gpu_parity.py
# ---------------------------------------------------------------------------------------------

PARITY_MODULI = [Q31, Q30, Q32, Q62, Q31HI, Q31LO]
PARITY_FUSED_N = [256, 512, 1024, 2048, 4096]          # test_random_vs_oracle
PARITY_MULTIPASS_N = [8192, 16384, 32768, 65536]       # test_multipass_vs_oracle
PARITY_XF_N = [256, 1024, 4096, 8192, 65536]           # test_transforms_vs_oracle
PARITY_XF_MODULI = [Q31, Q30, Q32, Q62, Q31HI]
PARITY_XF_MODES = [(256, Q30), (1024, Q31), (4096, Q31), (4096, Q32), (4096, Q62), (8192, Q30),
                   (16384, Q32), (65536, Q62)]          # test_transform_modes_vs_oracle
PARITY_PRIO = [(256, Q31), (512, Q31), (1024, Q31), (1024, Q30), (2048, Q31), (4096, Q31),
               (4096, Q31HI)]                           # test_issue_priority_variants
PARITY_SWEEP_N = [256, 1024, 4096]                     # test_random_prime_sweep, also in u64


def prio_limit(n, cus=MI355X_CUS):
    """The largest batch of n-word u32 Plantard products that still runs prioritised."""
    return 16 * cus * max(1, 64 // (n // 16)) // max(1, n // 16 // 64)


def parity_cases(cus=MI355X_CUS):
    out = []
    for q in PARITY_MODULI:
        for n in PARITY_FUSED_N + PARITY_MULTIPASS_N:
            out.append(Case("multiply", n, q, native_bits(q), 17, validate=n > 4096))
    for n in PARITY_SWEEP_N:        # one prime of each class stands for the sweep's bit lengths
        out += [Case("multiply", n, q, 64, 5) for q in (Q30, Q31, Q32, Q62)]
    for n, q in PARITY_PRIO:
        lim = prio_limit(n, cus)
        out += [Case("multiply", n, q, 32, lim), Case("multiply", n, q, 32, lim + 17)]
    out.append(Case("multiply", 1024, Q31, 32, 300, prio=-1))
    out.append(Case("multiply", 1024, Q31, 32, 256, prio_ok=0))
    for n in PARITY_XF_N:
        for q in PARITY_XF_MODULI:
            w = native_bits(q)
            out += [Case("transform", n, q, w, 3, mode=0), Case("transform", n, q, w, 3, mode=3),
                    Case("pointwise", n, q, w, 3)]
    for n, q in PARITY_XF_MODES:
        out += [Case("transform", n, q, native_bits(q), 2, mode=m) for m in XF_MODES]
    out += [Case("fill", 4096, Q31, 32, 8), Case("fill", 65536, Q62, 64, 8)]
    out += [Case("multiply", n, Q31, 32, 1024 // n, path="server") for n in (256, 512, 1024)]
    return out


def new_cases():
    out = []
    for n, q in U64_MULTIPASS:
        out += [Case("multiply", n, q, 64, 3), Case("multiply", n, q, 32, 3)]
    out += [Case("multiply", n, q, 64, 3) for n, q in U64_FUSED]
    for n, q, _ in XF_SWEEP:
        for w in word_options(q):
            for batch in XF_SWEEP_BATCHES:
                out += [Case("transform", n, q, w, batch, mode=m) for m in XF_MODES]
                out.append(Case("pointwise", n, q, w, batch))
    for n, q, batch in U64_DEVICE:
        out += [Case("fill", n, q, 64, batch), Case("multiply", n, q, 64, batch),
                Case("transform", n, q, 64, batch, mode=0), Case("pointwise", n, q, 64, batch),
                Case("transform", n, q, 64, batch, mode=3), Case("transform", n, q, 64, batch, mode=2)]
    for n, q in VALIDATE:
        for w in (32, 64):
            out += [Case("multiply", n, q, w, 2, validate=True),
                    Case("transform", n, q, w, 2, mode=0, validate=True),
                    Case("transform", n, q, w, 2, mode=3, validate=True),
                    Case("pointwise", n, q, w, 2, validate=True)]
    n, q, batch = U64_HOST_CHUNKS
    out += [Case("multiply", n, q, 64, 256), Case("transform", n, q, 64, 256, mode=0),
            Case("transform", n, q, 64, 256, mode=3)]
    for n, q, w, batch, modes in SUBBATCH:
        out += [Case("transform", n, q, w, batch, mode=m) for m in modes]
    n, q, w, batch = SUBBATCH_PRODUCT
    out.append(Case("multiply", n, q, w, batch))
    for n, batch in SERVER_SHAPES:
        out += [Case("multiply", n, q, 32, batch, path="server") for q in SERVER_NAMED]
    out += [Case("multiply", n, q, w, sat_batch(n)) for n, q, w in sat_products()]
    for n in SAT_N:
        for q in sat_moduli(n):
            w = native_bits(q)
            out += [Case("transform", n, q, w, n.bit_length(), mode=0),
                    Case("transform", n, q, w, n.bit_length(), mode=3)]
    out.append(Case("multiply", SAT_SERVER[0], SAT_SERVER[1], 32, 1, path="server"))
    out += [f.case for f in footprint_cases()]
    # the launches of the call sequences over long-lived contexts (tests/test_gpu_lifetime.py)
    from lifetime_cases import lifetime_cases
    out += lifetime_cases()
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("plain")
    return out


def all_cases(cus=MI355X_CUS):
    return parity_cases(cus) + new_cases()
