"""Case tables of tests/test_gpu_ctlin.py, test_gpu_ctlin_footprint.py and test_gpu_ctlin_scale.py,
and a pure-Python mirror of the dispatch behind include/nttmul_ctlin.h (csrc/ctlin.hip combine and
tensor, csrc/ctlin_plan.hpp ctlin_grid): plain data and arithmetic, no GPU.

tests/test_ctlin_ledger.py holds the mirror against the cross-compiled lib/libnttmul_ctlin.so (the
kernels it holds beyond libnttmul_level.so's are exactly the ones the mirror names over these
cases); test_gpu_ctlin.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_ctlin_kernel_name).

The shapes are the smallest at which the kernels can go wrong.  A workgroup of either kernel takes
256 vectors of 16 bytes of one limb's stream [batch][n]: at n = 256 that is 4 whole batch entries
on 32-bit words and 2 on 64-bit words, at n = 512 it is 2 on 32-bit words, so there batch 1, 3 and
5 each end in a partial workgroup and 5 has whole ones before it.  From n = 512 on 64-bit words
and n = 1024 on 32-bit words a workgroup is a part of one entry and no batch leaves a partial one:
the third batch there is 2.  L = 3 on the mixed-size chains of tests/basis_cases.py."""
from collections import namedtuple

import basis_cases as BC

OPS = ("combine", "tensor")
ALL_N = tuple(1 << e for e in range(8, 17))
PARITY_N = (256, 512, 4096, 8192)
L = 3
PROFILE = {32: "chain32", 64: "chain64"}
MAX_TERMS, MAX_COMPS = 16, 3
CHAIN_N = 256

# A term of a case: (kind, index of its x among the case's x buffers, or None: the constant term)
ONE, SCALAR, PLAIN = "one", "scalar", "plain"
KIND_CODE = {ONE: 0, SCALAR: 1, PLAIN: 2}

# op combine: terms as above, inplace: the indices of the x buffers that are out.  op tensor:
# pairs, square.  validate: the context has NTTMUL_FLAG_VALIDATE
Case = namedtuple("Case", "op bits n batch comps terms pairs square inplace validate",
                  defaults=(1, False, (), False))

_MIXED16 = ((ONE, 0), (SCALAR, 1), (PLAIN, 2), (SCALAR, None), (PLAIN, None), (PLAIN, 0),
            (ONE, 3), (SCALAR, 3), (PLAIN, 4), (ONE, 1), (PLAIN, 1), (SCALAR, 0), (PLAIN, 5),
            (ONE, 5), (SCALAR, 2), (PLAIN, 3))
_DOT16 = tuple((PLAIN, i) for i in range(16))

# (which batch, comps, terms): every value of every factor, every kind alone and mixed, both
# constant terms, the same x in two terms, 1, 2 and 16 terms
ROWS = (
    (0, 1, ((ONE, 0),)),
    (1, 2, ((SCALAR, 0),)),
    (2, 3, ((PLAIN, 0),)),
    (1, 3, ((ONE, 0), (ONE, 1))),                                   # ct + ct'
    (0, 2, ((PLAIN, 0), (ONE, 1))),                                 # pt o ct + ct'
    (2, 2, ((ONE, 0), (PLAIN, None))),                              # ct + pt
    (1, 1, ((SCALAR, 0), (SCALAR, None))),                          # c ct + constant
    (2, 1, _MIXED16),
    (0, 3, _DOT16),                                                 # sum of pt_i o ct_i
    (1, 2, ((PLAIN, 0), (PLAIN, 0))),                               # the same x (and w) twice
)
TENSOR_ROWS = ((0, 1, False), (1, 3, False), (2, 1, True), (1, 3, True))  # batch, pairs, square


def batches(n, bits):
    """1, 3 and a batch that ends in a partial workgroup after whole ones, where one exists."""
    return (1, 3, 5 if grid(1, n, bits)["per"] > 1 else 2)


def moduli_of(case_or_bits):
    """The basis of a case (or of a word class): L limbs of mixed sizes, unsorted."""
    bits = case_or_bits if isinstance(case_or_bits, int) else case_or_bits.bits
    return BC.basis(PROFILE[bits], L, 0)[0]


def special_of(bits):
    """One prime of the chain's P: the special basis of the NttCtMul that tensor's d_2 is held to."""
    return BC.basis(PROFILE[bits], L, 1)[1]


def x_count(case):
    return 1 + max([i for _, i in case.terms if i is not None], default=-1)


def parity_cases():
    out = []
    for bits in (32, 64):
        for n in PARITY_N:
            bs = batches(n, bits)
            for b, comps, terms in ROWS:
                out.append(Case("combine", bits, n, bs[b], comps, terms))
            for b, pairs, square in TENSOR_ROWS:
                out.append(Case("tensor", bits, n, bs[b], 3, (), pairs, square))
    return out


WORST_N = (256, 4096)


def worst_cases():
    """Every word q_l - 1 in 16 PLAIN terms and in 16 ONE terms."""
    return [Case("combine", bits, n, 2, 3, tuple((kind, i) for i in range(16)))
            for bits in (32, 64) for n in WORST_N for kind in (PLAIN, ONE)]


# out == x_0, and out == x_0 == x_3, against the out-of-place result
INPLACE_TERMS = ((PLAIN, 0), (ONE, 1), (SCALAR, 2), (ONE, 3), (PLAIN, None))
INPLACE_N = (256, 8192)


def inplace_cases():
    out = []
    for bits in (32, 64):
        for n in INPLACE_N:
            b = batches(n, bits)[2]
            out.append(Case("combine", bits, n, b, 2, INPLACE_TERMS, inplace=(0,)))
            # x_3 is x_0: the same buffer in two terms, and out
            same = tuple((k, 0 if i == 3 else i) for k, i in INPLACE_TERMS)
            out.append(Case("combine", bits, n, b, 2, same, inplace=(0,)))
    return out


VALIDATE = (256, 5)                          # n, batch
VALIDATE_TERMS = ((ONE, 0), (PLAIN, 1), (SCALAR, 2))
HOST = ((256, 5), (8192, 2))                 # (n, batch)
HOST_TERMS = ((PLAIN, 0), (ONE, 1), (SCALAR, 0), (SCALAR, None), (PLAIN, None))

# The caller's memory (tests/test_gpu_ctlin_footprint.py): host "" for the *_device call, "host"
# for the host form
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SIZES = ((256, 5), (8192, 3))             # (n, batch)
FP_TERMS = ((PLAIN, 0), (ONE, 1), (SCALAR, 1), (PLAIN, None), (SCALAR, None))
FP_PAIRS = 2


def footprint_cases():
    out = []
    for bits in (32, 64):
        for n, batch in FP_SIZES:
            for inplace in ((), (0,)):
                case = Case("combine", bits, n, batch, 2, FP_TERMS, inplace=inplace)
                out.append(Footprint("nttmul_ctlin_combine_device", case))
                out.append(Footprint("nttmul_ctlin_combine", case, "host"))
            for square in (False, True):
                case = Case("tensor", bits, n, batch, 3, (), FP_PAIRS, square)
                out.append(Footprint("nttmul_ctlin_tensor_device", case))
                out.append(Footprint("nttmul_ctlin_tensor", case, "host"))
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: one batch entry of the widest operand."""
    from guarded import guard_words
    return guard_words(max(case.comps, 2 * case.pairs) * L * case.n)


# ---------------------------------------------------------------------------------------------
# Scale cases (tests/test_gpu_ctlin_scale.py): the rule of tests/scale_cases.py -- the launch
# holds at least MIN_WAVES = 2 * 8192 waves, with the smallest batch that meets it and ends in a
# partial last workgroup: n = 256, where a workgroup holds several batch entries in both classes
# ---------------------------------------------------------------------------------------------

SCALE_N = 256
SCALE_TERMS = ((PLAIN, 0), (ONE, 1), (SCALAR, 2), (PLAIN, None), (SCALAR, None))
SCALE_PAIRS = 2
WAVE, MIN_WAVES = 64, 2 * 8192


def ends_partial(case):
    """Every kernel of the case that takes several units per workgroup ends in a partial one."""
    return all(per == 1 or units % per for per, units, _ in units_per_block(case).values())


def scale_cases():
    """One row per kernel: combine at comps 1, 2, 3 and tensor, both word classes."""
    out = []
    for bits in (32, 64):
        makers = [lambda b, c=comps: Case("combine", bits, SCALE_N, b, c, SCALE_TERMS)
                  for comps in (1, 2, 3)]
        makers.append(lambda b: Case("tensor", bits, SCALE_N, b, 3, (), SCALE_PAIRS, False))
        for make in makers:
            b = 1
            while min(launch_waves(make(b)).values()) < MIN_WAVES or not ends_partial(make(b)):
                b += 1
            out.append(make(b))
    return out


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py):
    all but the scale and the 4 GiB cases, whose batches exist to fill the machine."""
    out = parity_cases() + worst_cases() + inplace_cases()
    n, batch = VALIDATE
    out += [Case("combine", bits, n, batch, 2, VALIDATE_TERMS, validate=True) for bits in (32, 64)]
    out += [Case("tensor", bits, n, batch, 3, (), 2, sq, validate=True) for bits in (32, 64)
            for sq in (False, True)]
    out += [Case("combine", bits, n, batch, 2, HOST_TERMS) for bits in (32, 64)
            for n, batch in HOST]
    out += [Case("tensor", bits, n, batch, 3, (), 2, False) for bits in (32, 64)
            for n, batch in HOST]
    out += [f.case for f in footprint_cases()]
    return out


def all_cases():
    return referenced_cases() + scale_cases()


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def kernel_name(case):
    """ctlin.hip combine / tensor: one kernel per operation (and per comps for combine) at every
    n; the class follows the word size alone.  What nttmul_ctlin_kernel_name returns."""
    assert case.op in OPS and case.bits in (32, 64)
    cls, io = ("Arith32P", "u32") if case.bits == 32 else ("Arith64", "u64")
    if case.op == "tensor":
        return f"k_ctlin_tensor<{cls},{io}>"
    assert 1 <= case.comps <= MAX_COMPS and 1 <= len(case.terms) <= MAX_TERMS
    return f"k_ctlin_combine<{cls},{io},{case.comps}>"


def vec_words(bits):
    """Words of one 16-byte access."""
    return 128 // bits


def grid(batch, n, bits):
    """ctlin_plan.hpp ctlin_grid (ctmul_high_grid): a lane takes one vector at one slot of one
    batch entry in every component, a workgroup 256 consecutive vectors of one limb's stream
    [batch][n]: per = max(1, 256 vec / n) whole entries or one of n / (256 vec) parts of one;
    tail: the vectors of the last, partial workgroup."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    vec = vec_words(bits)
    pv = n // vec
    vectors = batch * pv
    return dict(vectors=vectors, wgx=-(-vectors // 256), vec=vec, per=max(1, 256 // pv),
                tail=vectors % 256)


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    (libnttmul_rns.so's kernel: per term its x, then its w; for tensor x_hat and once more for a
    y_hat that is not x_hat), then the one kernel."""
    io = "u32" if case.bits == 32 else "u64"
    if case.op == "tensor":
        count = 1 if case.square else 2
    else:
        count = sum((i is not None) + (kind != ONE) for kind, i in case.terms)
    return [f"k_rns_check_range<{io}>"] * (count * case.validate) + [kernel_name(case)]


def units_per_block(case):
    """{kernel_key: (units per workgroup and grid row, units of the launch per grid row, words per
    unit, component and workgroup)}.  A unit is a batch entry of the limb's stream; per whole ones
    where 256 vectors hold several (n words of each), else one (the 256 vec words of the
    workgroup's part)."""
    g = grid(case.batch, case.n, case.bits)
    return {kernel_name(case): (g["per"], case.batch, min(case.n, 256 * g["vec"]))}


def grid_rows(case):
    """{kernel_key: gridDim.y}: the limbs."""
    return {kernel_name(case): L}


def bpu(case):
    """Workgroups per run of units: the parts of a polynomial."""
    return max(1, case.n // (256 * vec_words(case.bits)))


def launch_waves(case):
    rows = grid_rows(case)
    return {k: -(-units // per) * bpu(case) * rows[k] * (256 // WAVE)
            for k, (per, units, _) in units_per_block(case).items()}


def combine_byte_units(comps, terms):
    """Limb polynomials combine moves per batch entry: comps per term with an x, comps written.
    (Plaintexts and scalars are shared by the batch and amortised away.)"""
    return comps * (1 + sum(i is not None for _, i in terms))


def tensor_byte_units(pairs):
    """Limb polynomials tensor moves per batch entry: 4 per pair read, 3 written."""
    return 4 * pairs + 3


# Kernels of libnttmul_ctlin.so beyond libnttmul_level.so's that no call can launch.  None:
# ctlin.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
