"""Call sequences over one long-lived context of a limb-aware library, and a pure-Python mirror of
the scratch state each of them keeps between calls: csrc/rnsmp.cpp (MpScratch), csrc/mdntt.cpp
(MdScr), csrc/ksntt.cpp (KnScr) and csrc/xconv.cpp (XcScr).  The four files carry the same state
machine, each written out by hand: `ensure` grows buffer i after an event synchronise on the last
use, a stream wait is issued when the stream changes, sub-batches run through the scratch, the
event is recorded after the launches, the host forms run on the context's own stream.  Plain data
and arithmetic: no GPU, and no library is loaded at import.  tests/lifetime_cases.py is the same
thing for csrc/nttmul.cpp.

* `SEQUENCES`: named (Ctx, steps) lists, each on one context from its first call to its last.
  tests/test_gpu_limb_lifetime.py runs them, every step on inputs of its own.
* `walk(ctx, state, step)`: what one call does to the state: the three buffer sizes, `used`,
  `last`, whether the event exists, the sub-batch list, whether the call is validated.  The chunk
  of a call comes from the libraries' own mirrors (mdntt_cases, xconv_cases, ksntt_cases,
  rnsmp_cases, macn_cases, hoist_cases), never from a rule restated here.  `model(name)` walks a
  whole sequence.
* `TRANSITIONS`: (name, file, function, regex, pairs) rows; the regex matches exactly one line of
  that function of that file.  The names of COMMON exist for every one of the four files.
  `EXEMPT`: the paths only a failing HIP call reaches, with the reason in place of the pairs.
* `inputs(name, index, salt)` and `expected(ctx, step, ins)`: every step's operands, seeded, and
  what the CPU references make of them: every output word of every entry at every n (the
  conversions through tests/full_ref.py).

tests/test_limb_lifetime_ledger.py holds the tables against the sources and the model."""
import copy
import os
from collections import namedtuple

import hoist_cases as HC
import ksntt_cases as KC
import level_cases as LC
import macn_cases as NC
import mdntt_cases as MC
import rnsmp_cases as RC
import xconv_cases as XC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "ntt-based-polynomial-multiplier-fpga_amd", "csrc")
FILES = {"rnsmp": "rnsmp.cpp", "mdntt": "mdntt.cpp", "ksntt": "ksntt.cpp", "xconv": "xconv.cpp"}
SCALE = 65537                               # xconv's t

# lib: "rnsmp" (nttmul.RnsMpHoistContext), "mdntt" (NttModDown), "ksntt" (NttLevelKeySwitch; the
#   CHAIN's: NttKeySwitch), "xconv" (NttExactConv)
# shape: rnsmp (limbs,); mdntt (L, K); ksntt (L, K, alpha); xconv (L, K, scale)
# basis: "level": a level of level_cases' chain (every ksntt context, and the CHAIN's mdntt one)
Ctx = namedtuple("Ctx", "lib n bits shape scratch_mb validate ndev share_devices basis",
                 defaults=(1, False, 1, False, ""))

# entry: rnsmp "multiply" | "forward" | "inverse" | "inverse_inplace" (out == in) | "mac" (mac_ntt,
#   b_hat per batch entry) | "macn" (comps operands, b_hat shared) | "hoist" (hoist_ntt);
#   mdntt "moddown"; ksntt "modup" | "mac"; xconv "extend" | "moddown"
# place: device operands on caller stream "A", "B" or the "null" stream; "host": the host form, on
#   the context's own stream
# status: "OK", or "ERANGE" on a validating context: polynomial `bad` of the first operand holds
#   one word equal to its limb's modulus
# view: (top_q_limbs, top_terms) of a key mac whose b_hat was made for the chain's top level
# dev: the device of a device form (sequence G_dev1)
Step = namedtuple("Step", "entry place batch terms comps rots status bad view dev",
                  defaults=(1, 1, 0, "OK", None, None, 0))

PLACES = ("A", "B", "null", "host")
SALT = 1000                                 # test_sequence, the chain
THREAD_SALTS = (5000, 105000)               # the two threads of a pair

# nttmul_*_last_error after NTTMUL_ERANGE, per (lib, entry is the key mac)
ERANGE_TEXT = {("rnsmp", False): "input coefficient >= its limb's modulus",
               ("mdntt", False): "input word >= its limb's modulus",
               ("ksntt", False): "input word >= its limb's modulus",
               ("ksntt", True): "operand word >= its limb's modulus",
               ("xconv", False): "input word >= its limb's modulus"}


def moduli_of(cp):
    """rnsmp: the basis; the others: (q, p)."""
    if cp.lib == "rnsmp":
        return (RC.BASIS32 if cp.bits == 32 else RC.BASIS64)[:cp.shape[0]]
    if cp.basis == "level":
        assert cp.shape[1] == LC.K
        return LC.level_bases(cp.bits, cp.shape[0])
    assert cp.lib != "ksntt"
    import ks_ref
    return ks_ref.bases(cp.bits, cp.shape[0], cp.shape[1])


def S(entry, place, batch, **kw):
    assert place in PLACES
    return Step(entry, place, batch, **kw)


# ---------------------------------------------------------------------------------------------
# The sub-batches of a call, from the libraries' mirrors
# ---------------------------------------------------------------------------------------------

def chunks(cp, step):
    """The sub-batch list of a call (polynomials; output units for "hoist"), as the library's own
    mirror gives it.  Where two mirrors cover the same call they must agree."""
    n, mb, b = cp.n, cp.scratch_mb, step.batch
    if cp.lib == "mdntt":
        return MC.chunks(MC.Case(cp.bits, n, b, *cp.shape, False, mb))
    if cp.lib == "xconv":
        L, K, t = cp.shape
        out = XC.chunks(XC.Case(step.entry, cp.bits, n, b, L, K, t, False, mb))
        assert out == MC.chunks(MC.Case(cp.bits, n, b, L, K, False, mb))
        return out
    if cp.lib == "ksntt":
        L, K, alpha = cp.shape
        if step.entry == "mac":
            return KC.chunks(KC.Mac(cp.bits, n, b, L, K, step.terms, step.comps, (1,) * step.rots))
        return KC.chunks(KC.Up(cp.bits, n, b, L, K, alpha, False, mb))
    m = moduli_of(cp)
    assert cp.lib == "rnsmp"
    if step.entry == "hoist":
        ks = HC.draw(n, step.rots, 1)
        return HC.chunks(HC.Case(n, m, b, step.terms, step.comps, ks, False, mb))
    if step.entry == "macn":
        out = NC.chunks(NC.Case(n, m, b, step.terms, step.comps, True, False, mb))
        if step.comps <= step.terms:        # then a's bytes bound the chunk, as for mac_ntt
            assert out == RC.chunks(RC.Case("mac", n, m, b, step.terms, True, False, mb))
        return out
    op = {"inverse_inplace": "inverse"}.get(step.entry, step.entry)
    out = RC.chunks(RC.Case(op, n, m, b, step.terms, False, False, mb))
    if op == "mac":                         # the mac against one operand is macn's comps = 1
        assert out == NC.chunks(NC.Case(n, m, b, step.terms, 1, False, False, mb))
    return out


def chunk_of(cp, entry, **kw):
    """The largest sub-batch `entry` ever gets on cp."""
    return chunks(cp, Step(entry, "A", 1 << 20, **kw))[0]


def _wb(cp):
    return cp.bits // 8


def needs(cp, step, chunk):
    """[(buffer index, bytes)] the call asks of `ensure`, in order (rnsmp.cpp run / run_units,
    mdntt.cpp run, ksntt.cpp run_modup, xconv.cpp run)."""
    n, wb = cp.n, _wb(cp)
    if cp.lib in ("mdntt", "xconv"):
        L, K = cp.shape[:2]
        y, t = K * n * wb, L * n * wb
        return [(0, chunk * y)] + ([(1, chunk * y), (2, chunk * t)] if n > 4096 else [])
    if cp.lib == "ksntt":
        y = cp.shape[0] * n * wb
        return [(0, chunk * y)] + ([(1, chunk * y)] if n > 4096 else [])
    poly = cp.shape[0] * n * wb
    if step.entry == "hoist":
        return [(2, chunk * poly * step.comps)]
    if step.entry == "multiply":
        return [(0, chunk * poly), (1, chunk * poly), (2, chunk * poly)]
    if step.entry in ("mac", "macn"):
        return [(0, chunk * poly * step.terms), (2, chunk * poly * step.comps)]
    return [(0, chunk * poly)]


# ---------------------------------------------------------------------------------------------
# The sequences
# ---------------------------------------------------------------------------------------------

def _ctx_r(bits, **kw):
    return Ctx("rnsmp", 8192, bits, (3,), 1, **kw)


def _seq_r(bits):
    cp = _ctx_r(bits)
    chunk = chunk_of(cp, "multiply")
    return (cp, [
        S("forward", "A", 1),                               # 0 first use: buf[0] alone
        S("multiply", "A", 3),                              # 1 buf[0] grows, buf[1] and buf[2] new
        S("mac", "B", 2, terms=3),                          # 2 other stream; buf[0] to chunk * apoly
        S("macn", "B", 4, terms=1, comps=2),                # 3 buf[2] to chunk * cpoly
        S("hoist", "A", 2, terms=2, comps=2, rots=3),       # 4 run_units: buf[2] alone
        S("multiply", "null", 2 * chunk + 3),               # 5 three sub-batches, a short last one
        S("multiply", "host", 2),                           # 6 the context's own stream
        S("inverse_inplace", "A", 3),                       # 7 out == in
        S("forward", "B", 1),                               # 8 no growth
    ])


# R_overlap: nothing orders the calls but the library; each issues at least OVERLAP_SUBS
# sub-batches, so the next call's first launch is enqueued behind a queue of the previous call's
OVERLAP_SUBS = 16
OVERLAP_ROUNDS = 3


def _seq_r_overlap(scale=1):
    cp = _ctx_r(32)
    k = OVERLAP_SUBS * scale
    macn = dict(terms=1, comps=2)
    rnd = [S("multiply", "A", k * chunk_of(cp, "multiply")),
           S("forward", "B", k * chunk_of(cp, "forward")),
           S("macn", "null", k * chunk_of(cp, "macn", **macn), **macn)]
    return (cp, rnd * OVERLAP_ROUNDS)


SEQ_R_ERANGE = (_ctx_r(32, validate=True), [
    S("multiply", "A", 2),
    S("multiply", "A", 2, status="ERANGE", bad=1),
    S("multiply", "host", 2),
    S("hoist", "B", 1, rots=1),                             # run_units' check, after the failure
    S("hoist", "B", 2, rots=1, status="ERANGE", bad=1),
    S("hoist", "A", 1, rots=1),
    S("forward", "A", 1),
])


def _seq_m(n, **kw):
    return (Ctx("mdntt", n, 32, (3, 2), 1, **kw), [
        S("moddown", "A", 1),
        S("moddown", "A", 35),                              # the scratch grows
        S("moddown", "B", 35),
        S("moddown", "host", 2),
        S("moddown", "null", 3),
        S("moddown", "A", 35),
    ])


SEQ_M_ERANGE = (Ctx("mdntt", 256, 32, (3, 2), 1, True), [
    S("moddown", "A", 3),
    S("moddown", "A", 3, status="ERANGE", bad=1),
    S("moddown", "host", 2),
    S("moddown", "B", 3),
])

K_SHAPE = (LC.CHAIN_LEVEL, LC.K, LC.ALPHA)  # level 3 of level_cases' five-limb chain
K_MAC = dict(terms=LC.terms_of(LC.CHAIN_LEVEL), comps=2, rots=1)
K_VIEWED = dict(terms=LC.terms_of(LC.CHAIN_LEVEL), comps=1, rots=3, view=LC.VIEW)


def _seq_k(n):
    cp = Ctx("ksntt", n, 32, K_SHAPE, 1, basis="level")
    chunk = chunk_of(cp, "modup")
    return (cp, [
        S("modup", "A", 1),
        S("mac", "A", 2, **K_MAC),                          # no scratch: streams and flag only
        S("modup", "B", 9),
        S("mac", "B", 2, **K_VIEWED),                       # the top-level key through a view
        S("modup", "host", 2),
        S("modup", "null", min(2 * chunk + 3, 23)),         # n = 8192: 10 + 10 + 3
        S("mac", "host", 2, **K_MAC),
    ])


SEQ_K_ERANGE = (Ctx("ksntt", 256, 32, K_SHAPE, 1, True, basis="level"), [
    S("modup", "A", 2),
    S("modup", "A", 2, status="ERANGE", bad=1),
    S("modup", "host", 2),
    S("modup", "B", 2),
    S("mac", "B", 2, **K_MAC),
    S("mac", "B", 2, status="ERANGE", bad=1, **K_MAC),
    S("mac", "host", 2, **K_VIEWED),                        # the viewed operand's own check
    S("mac", "A", 2, **K_MAC),
])


def _seq_x(n):
    return (Ctx("xconv", n, 32, (3, 2, SCALE), 1), [
        S("extend", "A", 1),
        S("moddown", "B", 35),
        S("extend", "A", 35),
        S("moddown", "host", 2),
        S("extend", "null", 3),
        S("moddown", "A", 35),
    ])


SEQ_X_ERANGE = (Ctx("xconv", 256, 32, (3, 2, SCALE), 1, True), [
    S("extend", "A", 3),
    S("moddown", "A", 3, status="ERANGE", bad=1),
    S("extend", "host", 2),
    S("moddown", "B", 3),
    S("extend", "B", 3),                                    # the same stream again
])

# G: two device entries of one context (on a machine with one GPU both on device 0: the second is
# set up and freed, and never found by a call); G_dev1 adds the calls on device 1
_G_CTX = Ctx("mdntt", 256, 32, (3, 2), 1, False, 2, True)
_G_STEPS = [S("moddown", "host", 2), S("moddown", "A", 3), S("moddown", "host", 1),
            S("moddown", "B", 35)]
SEQ_G = (_G_CTX, _G_STEPS)
SEQ_G_DEV1 = (_G_CTX, _G_STEPS + [S("moddown", "A", 3, dev=1), S("moddown", "host", 2),
                                  S("moddown", "B", 35, dev=1), S("moddown", "A", 1)])
G_DEV1_DEVICES = 2                          # the device count G_dev1 needs and is modelled with

SEQUENCES = {"R": _seq_r(32), "R_u64": _seq_r(64), "R_overlap": _seq_r_overlap(),
             "R_erange": SEQ_R_ERANGE,
             "M": _seq_m(8192), "M_256": _seq_m(256), "M_erange": SEQ_M_ERANGE,
             "K": _seq_k(8192), "K_256": _seq_k(256), "K_erange": SEQ_K_ERANGE,
             "X": _seq_x(8192), "X_256": _seq_x(256), "X_erange": SEQ_X_ERANGE,
             "G": SEQ_G}

# CHAIN: one caller stream, three iterations with no host synchronisation between them, each
# NttKeySwitch.modup -> mac -> NttModDown.moddown on the same two contexts; the batches.  The mac
# has comps = 2 and one rotation, so the moddown's batch is twice the iteration's
CHAIN_N, CHAIN_BATCHES, CHAIN_SHAPE, CHAIN_K = 256, (1, 5, 2), (3, 2, 2), 5
CHAIN_CTX = {"ks": Ctx("ksntt", CHAIN_N, 32, CHAIN_SHAPE, 0, basis="level"),
             "md": Ctx("mdntt", CHAIN_N, 32, CHAIN_SHAPE[:2], 0, basis="level")}
CHAIN_MAC = dict(terms=-(-CHAIN_SHAPE[0] // CHAIN_SHAPE[2]), comps=2, rots=1)
SEQ_CHAIN_KS = (CHAIN_CTX["ks"], [s for b in CHAIN_BATCHES
                                  for s in (S("modup", "A", b), S("mac", "A", b, **CHAIN_MAC))])
SEQ_CHAIN_MD = (CHAIN_CTX["md"], [S("moddown", "A", 2 * b) for b in CHAIN_BATCHES])

MODEL_SEQUENCES = {**SEQUENCES, "G_dev1": SEQ_G_DEV1, "CHAIN_ks": SEQ_CHAIN_KS,
                   "CHAIN_md": SEQ_CHAIN_MD}
# two host threads, a context each: the pairs of sequences that run together
THREAD_PAIRS = (("R", "X"), ("M", "K"))


def devices_of(name):
    return G_DEV1_DEVICES if name == "G_dev1" else 1


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def new_state(cp):
    """A context after create: per device entry the scratch (bytes of the three buffers, the event,
    used, last, the operation of the last use), and whether the last validated call failed."""
    return {"failed": False,
            "dev": [{"bytes": [0, 0, 0], "ev": False, "used": False, "last": None, "op": None}
                    for _ in range(cp.ndev)]}


def entry_index(cp, step, devices=1):
    """The device entry a call runs on: dev[0] for a host form, the first entry on the step's
    device for a device form (limb_ctx.hpp find_dev; entry i is on device i mod the count)."""
    if step.place == "host":
        return 0
    ids = [i % devices for i in range(cp.ndev)]
    assert step.dev in ids, "NTTMUL_ENODEV"
    return ids.index(step.dev)


Walk = namedtuple("Walk", "state tags subs validated entry")


def walk(cp, before, step, devices=1):
    """One call on a context in state `before`: Walk(state after, the transition names driven,
    the sub-batch list ([] when the call never reaches the scratch), whether the range check ran,
    the device entry)."""
    st = copy.deepcopy(before)
    lib, tags = cp.lib, set()
    e = entry_index(cp, step, devices)
    key_mac = lib == "ksntt" and step.entry == "mac"
    units = step.entry == "hoist"
    pre = lib + (".mac." if key_mac else ".units." if units else ".")

    def tag(name, own=False):
        tags.add((pre if own else lib + ".") + name)

    erange = step.status == "ERANGE"
    assert not erange or (cp.validate and step.bad is not None and step.bad < step.batch)
    if cp.validate:
        if erange:
            tag("validate.erange", True)
            st["failed"] = True
            return Walk(st, frozenset(tags), [], True, e)
        if st["failed"]:
            tag("validate.after_erange", True)
        st["failed"] = False
        if key_mac and step.view:
            tag("validate.viewed", True)
    if step.place == "host":
        tag("host_form", True)
    if key_mac:                                 # one launch, no scratch
        tag("viewed" if step.view else "dense", True)
        return Walk(st, frozenset(tags), [step.batch], cp.validate, e)

    sc = st["dev"][e]
    stream = f"own{e}" if step.place == "host" else step.place
    subs = chunks(cp, step)
    if not sc["ev"]:
        tag("first_use")
        sc["ev"] = True
    if sc["used"]:
        tag("same_stream" if sc["last"] == stream else "wait_other_stream")
    if lib == "xconv" and sc["op"] not in (None, step.entry):
        tag("op_switch")
    for i, need in needs(cp, step, subs[0]):
        if sc["bytes"][i] >= need:
            tag("no_growth")
            continue
        tag("grow_after_use" if sc["used"] else "alloc_unused")
        if sc["bytes"][i]:
            tag("regrow")
        sc["bytes"][i] = need
    count = len(needs(cp, step, 1))
    if units:
        tag("single_buffer", True)
    elif lib == "rnsmp":                        # run's `two` (the product), `three` (and the macs)
        tag({1: "buffers.one", 2: "buffers.mac", 3: "buffers.two"}[count])
        if count >= 2:
            tag("buffers.three")
        if step.entry == "macn":
            tag("comps_sizing")
    else:
        tag("buffers.one" if count == 1 else "buffers.above_4096")
    if len(subs) > 1:
        tag("sub_batches", units)
        if lib == "xconv":
            tag("sub_batch_stride")
    tag("event_recorded")
    sc["used"], sc["last"], sc["op"] = True, stream, step.entry
    return Walk(st, frozenset(tags), subs, cp.validate, e)


def model(name, devices=None):
    """[Walk] of a sequence, one per step, from a fresh context."""
    cp, steps = MODEL_SEQUENCES[name]
    devices = devices_of(name) if devices is None else devices
    st, out = new_state(cp), []
    for step in steps:
        out.append(walk(cp, st, step, devices))
        st = out[-1].state
    return out


def state_before(name, index):
    cp, _ = MODEL_SEQUENCES[name]
    return new_state(cp) if index == 0 else model(name)[index - 1].state


def drives(transition, name, index):
    """The predicate of a transition over (state before, step) of a sequence."""
    cp, steps = MODEL_SEQUENCES[name]
    return transition in walk(cp, state_before(name, index), steps[index], devices_of(name)).tags


# ---------------------------------------------------------------------------------------------
# The transitions
# ---------------------------------------------------------------------------------------------

# name: "<lib>.<what>", as `walk` calls it;  file: the key of FILES;  func: the first words of the
# line that opens the function;  line: a regular expression that matches exactly one line of that
# function;  pairs: (sequence, step index) that drive it
Transition = namedtuple("Transition", "name file func line pairs")

# what every one of the four files has, under its own prefix
COMMON = ("first_use", "wait_other_stream", "same_stream", "alloc_unused", "grow_after_use",
          "regrow", "no_growth", "sub_batches", "event_recorded", "host_form", "validate.erange",
          "validate.after_erange")

_ENSURE = {
    "alloc_unused": r"LIMB_TRY\(\w+->err, hipMalloc\(&sc\.buf\[i\], need\)\);",
    "grow_after_use": r"if \(sc\.used\) LIMB_TRY\(\w+->err, hipEventSynchronize\(sc\.ev\)\);",
    "regrow": r"if \(sc\.buf\[i\]\) \(void\)hipFree\(sc\.buf\[i\]\);",
    "no_growth": r"if \(sc\.bytes\[i\] >= need\) return NTTMUL_OK;",
}
_FIRST_USE = (r"if \(!sc\.ev\) LIMB_TRY\(\w+->err, "
              r"hipEventCreateWithFlags\(&sc\.ev, hipEventDisableTiming\)\);")
_WAIT = r"if \(sc\.used && sc\.last != s\) LIMB_TRY\(\w+->err, hipStreamWaitEvent\(s, sc\.ev, 0\)\);"
_LAST = r"sc\.last = s;"
_RECORD = r"const hipError_t e = hipEventRecord\(sc\.ev, s\);"
_SUBS = r"for \(size_t k = 0; k < S\.subs && !st; k\+\+\) \{"
_VALIDATES = r"if \(P\.flags & NTTMUL_FLAG_VALIDATE\) \{"
_CHECK = r"if \(const int st = check_range\("


def _rows(lib, run, host_func, host_line, pairs):
    """The COMMON rows of one of the three files that keep the state machine inside `run`."""
    def T(what, func, line):
        return Transition(f"{lib}.{what}", lib, func, line, pairs[what])
    return tuple([T("first_use", run, _FIRST_USE), T("wait_other_stream", run, _WAIT),
                  T("same_stream", run, _LAST)]
                 + [T(what, "int ensure(", line) for what, line in _ENSURE.items()]
                 + [T("sub_batches", run, _SUBS), T("event_recorded", run, _RECORD),
                    T("host_form", host_func, host_line),
                    T("validate.erange", run, _CHECK), T("validate.after_erange", run, _VALIDATES)])


def _row(lib):
    """Rows of one file: (what, func, line, *pairs) -> Transition."""
    def row(what, func, line, *pairs):
        return Transition(f"{lib}.{what}", lib, func, line, pairs)
    return row


_R, _M, _K, _X = _row("rnsmp"), _row("mdntt"), _row("ksntt"), _row("xconv")

TRANSITIONS = (
    # csrc/rnsmp.cpp: scratch_begin, ensure and scratch_end serve run and run_units alike
    _R("first_use", "int scratch_begin(", _FIRST_USE, ("R", 0), ("R_u64", 0), ("R_overlap", 0)),
    _R("wait_other_stream", "int scratch_begin(", _WAIT,
       ("R", 2), ("R", 4), ("R", 5), ("R", 6), ("R", 7), ("R", 8), ("R_overlap", 1),
       ("R_overlap", 2), ("R_overlap", 3), ("R_erange", 2)),
    _R("same_stream", "int scratch_end(", _LAST, ("R", 1), ("R", 3), ("R_u64", 3)),
    _R("alloc_unused", "int ensure(", _ENSURE["alloc_unused"], ("R", 0), ("R_overlap", 0)),
    _R("grow_after_use", "int ensure(", _ENSURE["grow_after_use"],
       ("R", 1), ("R", 2), ("R", 3), ("R", 4), ("R", 5), ("R_u64", 1), ("R_u64", 5)),
    _R("regrow", "int ensure(", _ENSURE["regrow"], ("R", 1), ("R", 2), ("R", 3), ("R", 4), ("R", 5)),
    _R("no_growth", "int ensure(", _ENSURE["no_growth"],
       ("R", 2), ("R", 3), ("R", 6), ("R", 7), ("R", 8), ("R_overlap", 1), ("R_overlap", 3)),
    _R("sub_batches", "int run(", r"for \(size_t k = 0; k < mp_subs\(batch, chunk\) && !st; k\+\+\) \{",
       ("R", 5), ("R_u64", 2), ("R_u64", 3), ("R_overlap", 0), ("R_overlap", 1), ("R_overlap", 2)),
    _R("event_recorded", "int scratch_end(", _RECORD, ("R", 0), ("R", 4), ("R", 6), ("R_overlap", 8)),
    _R("host_form", "int host_op(", r'return staged_op\(r->err, d\.base, "rnsmp", ops, 3,',
       ("R", 6), ("R_u64", 6), ("R_erange", 2)),
    _R("validate.erange", "int validate(", r"return check_range\(r->err, d\.base\.flag, d\.base\.q,",
       ("R_erange", 1)),
    _R("validate.after_erange", "int run(",
       r"if \(const int st = validate\(r, d, a, words\[1\], b, words\[2\], s\)\) return st;",
       ("R_erange", 2)),
    _R("units.validate.erange", "int run_units(",
       r"if \(const int st = validate\(r, d, a, words\[1\], b, words\[2\], s\)\) return st;",
       ("R_erange", 4)),
    _R("units.validate.after_erange", "int validate(",
       r"if \(!\(r->flags & NTTMUL_FLAG_VALIDATE\)\) return NTTMUL_OK;", ("R_erange", 5)),
    _R("units.single_buffer", "int run_units(", r"int st = ensure\(r, sc, 2, chunk \* cunit\);",
       ("R", 4), ("R_u64", 4), ("R_erange", 3)),
    _R("units.sub_batches", "int run_units(",
       r"for \(size_t k = 0; k < mp_subs\(units, chunk\) && !st; k\+\+\) \{", ("R", 4), ("R_u64", 4)),
    _R("buffers.one", "int run(", r"int st = ensure\(r, sc, 0, chunk \* apoly\);",
       ("R", 0), ("R", 7), ("R", 8), ("R_overlap", 1)),
    _R("buffers.two", "int run(", r"if \(!st && two\) st = ensure\(r, sc, 1, chunk \* poly\);",
       ("R", 1), ("R", 5), ("R", 6), ("R_overlap", 0)),
    _R("buffers.three", "int run(", r"if \(!st && three\) st = ensure\(r, sc, 2, chunk \* cpoly\);",
       ("R", 1), ("R", 2), ("R", 3), ("R_overlap", 2)),
    _R("buffers.mac", "int run(",
       r"const size_t apoly = op == kRnsMac \? poly \* terms : poly, cpoly = poly \* comps;",
       ("R", 2), ("R", 3), ("R_u64", 2)),
    _R("comps_sizing", "int run(",
       r"const size_t chunk = mp_chunk\(\(size_t\)r->scratch_mb << 20, apoly, cpoly, batch\);",
       ("R", 3), ("R_u64", 3), ("R_overlap", 2), ("R_overlap", 5), ("R_overlap", 8)),
) + _rows("mdntt", "int run(", "int nttmul_mdntt_moddown(",
          r'return staged_op\(h->err, d\.base, "mdntt", ops, 2,', {
    "first_use": (("M", 0), ("M_256", 0), ("G", 0), ("CHAIN_md", 0)),
    "wait_other_stream": (("M", 2), ("M", 3), ("M", 4), ("M", 5), ("M_256", 2), ("G", 1), ("G", 2),
                          ("G_dev1", 5), ("M_erange", 2)),
    "same_stream": (("M", 1), ("M_256", 1), ("CHAIN_md", 1), ("CHAIN_md", 2)),
    "alloc_unused": (("M", 0), ("M_256", 0), ("G_dev1", 4)),
    "grow_after_use": (("M", 1), ("M_256", 1), ("G", 1), ("G", 3), ("CHAIN_md", 1), ("G_dev1", 6)),
    "regrow": (("M", 1), ("M_256", 1), ("G", 3)),
    "no_growth": (("M", 2), ("M", 3), ("M", 4), ("M", 5), ("M_256", 5), ("G", 2), ("CHAIN_md", 2)),
    "sub_batches": (("M", 1), ("M", 2), ("M", 5)),
    "event_recorded": (("M", 0), ("M", 5), ("M_256", 3), ("G", 3)),
    "host_form": (("M", 3), ("M_256", 3), ("G", 0), ("G", 2), ("M_erange", 2)),
    "validate.erange": (("M_erange", 1),),
    "validate.after_erange": (("M_erange", 2),),
}) + (
    _M("buffers.one", "int run(", r"int st = ensure\(h, sc, kMdY, S\.chunk \* S\.y_bytes\);",
       ("M_256", 0), ("M_256", 1), ("G", 1)),
    _M("buffers.above_4096", "int run(",
       r"if \(!st && S\.t_bytes\) st = ensure\(h, sc, kMdT, S\.chunk \* S\.t_bytes\);",
       ("M", 0), ("M", 1), ("M", 3)),
) + _rows("ksntt", "int run_modup(", "int nttmul_ksntt_modup(",
          r'return staged_op\(h->err, d\.base, "ksntt", ops, 2,', {
    "first_use": (("K", 0), ("K_256", 0), ("CHAIN_ks", 0)),
    "wait_other_stream": (("K", 2), ("K", 4), ("K", 5), ("K_256", 2), ("K_erange", 2), ("K_erange", 3)),
    "same_stream": (("CHAIN_ks", 2), ("CHAIN_ks", 4)),
    "alloc_unused": (("K", 0), ("K_256", 0)),
    "grow_after_use": (("K", 2), ("K", 5), ("K_256", 2), ("K_256", 5), ("CHAIN_ks", 2)),
    "regrow": (("K", 2), ("K", 5), ("K_256", 2), ("CHAIN_ks", 2)),
    "no_growth": (("K", 4), ("K_256", 4), ("CHAIN_ks", 4), ("K_erange", 2)),
    "sub_batches": (("K", 5),),
    "event_recorded": (("K", 0), ("K", 5), ("K_256", 4)),
    "host_form": (("K", 4), ("K_256", 4), ("K_erange", 2)),
    "validate.erange": (("K_erange", 1),),
    "validate.after_erange": (("K_erange", 2),),
}) + (
    _K("buffers.one", "int run_modup(", r"int st = ensure\(h, sc, kMdY, S\.chunk \* S\.y_bytes\);",
       ("K_256", 0), ("K_256", 2), ("CHAIN_ks", 0)),
    _K("buffers.above_4096", "int run_modup(",
       r"if \(!st && P\.n > 4096\) st = ensure\(h, sc, kMdYLazy, S\.chunk \* S\.y_bytes\);",
       ("K", 0), ("K", 2), ("K", 4)),
    # the key mac: no scratch, the same streams and the same range-check flag
    _K("mac.dense", "int run_mac(", r": launch_ksntt_mac\(view\(h, d\), c, a, b, H, batch, terms, s\);",
       ("K", 1), ("K", 6), ("K_256", 1), ("CHAIN_ks", 1), ("K_erange", 4)),
    _K("mac.viewed", "int run_mac(", r"const hipError_t e = V \? V->launch\(",
       ("K", 3), ("K_256", 3), ("K_erange", 6)),
    _K("mac.host_form", "int mac_host(", r'return staged_op\(h->err, d\.base, "ksntt", ops, 3,',
       ("K", 6), ("K_256", 6), ("K_erange", 6)),
    _K("mac.validate.erange", "int run_mac(", _CHECK, ("K_erange", 5)),
    _K("mac.validate.after_erange", "int run_mac(", _VALIDATES, ("K_erange", 6)),
    _K("mac.validate.viewed", "int run_mac(", r"if \(const int st = V->check\(", ("K_erange", 6)),
) + _rows("xconv", "int run(", "int run_host(",
          r'return staged_op\(h->err, d\.base, "xconv", ops, 2,', {
    "first_use": (("X", 0), ("X_256", 0), ("X_erange", 0)),
    "wait_other_stream": (("X", 1), ("X", 2), ("X", 3), ("X", 4), ("X", 5), ("X_256", 1),
                          ("X_erange", 2), ("X_erange", 3)),
    "same_stream": (("X_erange", 4),),
    "alloc_unused": (("X", 0), ("X_256", 0)),
    "grow_after_use": (("X", 1), ("X_256", 1)),
    "regrow": (("X", 1), ("X_256", 1)),
    "no_growth": (("X", 2), ("X", 3), ("X", 4), ("X", 5), ("X_256", 2), ("X_erange", 2)),
    "sub_batches": (("X", 1), ("X", 2), ("X", 5)),
    "event_recorded": (("X", 0), ("X", 5), ("X_256", 3)),
    "host_form": (("X", 3), ("X_256", 3), ("X_erange", 2)),
    "validate.erange": (("X_erange", 1),),
    "validate.after_erange": (("X_erange", 2),),
}) + (
    _X("buffers.one", "int run(", r"int st = ensure\(h, sc, kMdY, S\.chunk \* S\.y_bytes\);",
       ("X_256", 0), ("X_256", 1), ("X_erange", 0)),
    _X("buffers.above_4096", "int run(",
       r"if \(!st && S\.t_bytes\) st = ensure\(h, sc, kMdT, S\.chunk \* S\.t_bytes\);",
       ("X", 0), ("X", 1), ("X", 3)),
    # extend and moddown differ in in_words and share the buffers
    _X("op_switch", "int run(",
       r"xconv_shape\(\(size_t\)h->scratch_mb << 20, P\.n, P\.L, P\.K, P\.word_bits, batch, op\);",
       ("X", 1), ("X", 2), ("X", 3), ("X", 4), ("X", 5), ("X_256", 1), ("X_erange", 3)),
    _X("sub_batch_stride", "int run(",
       r"\(const char \*\)in \+ u\.p \* S\.in_words \* wb, u\.cnt, sc\.buf, s\);",
       ("X", 1), ("X", 2), ("X", 5)),
)

# Paths no sequence drives, because only a failing HIP call reaches them: the line each would pin
# and, in place of the pairs, the reason.  No failure hook is added for them.
_NO_ENSURE = ("reached only when hipEventSynchronize or hipMalloc inside ensure fails: the call "
              "returns before any launch and before the event is recorded")
_NO_LAUNCH = ("reached only when a sub-batch launch fails: the loop stops and the event is still "
              "recorded after the failure, because what was enqueued still uses the scratch")
_NO_RECORD = "reached only when hipEventRecord itself fails after successful launches"
_LAUNCH_FAILS = r'if \(e != hipSuccess\) st = fail\(\w+->err, e, "sub-batch launch"\);'
_RECORD_FAILS = r'if \(!st && e != hipSuccess\) st = fail\(\w+->err, e, "hipEventRecord\(scratch\)"\);'


def _exempt(lib, run, end=None):
    E = lambda what, func, line, why: Transition(f"{lib}.{what}", lib, func, line, why)  # noqa: E731
    return (E("ensure_fails", run, r"^  if \(st\) return st;", _NO_ENSURE),
            E("launch_fails", run, _LAUNCH_FAILS, _NO_LAUNCH),
            E("record_fails", end or run, _RECORD_FAILS, _NO_RECORD))


EXEMPT = (_exempt("rnsmp", "int run(", "int scratch_end(")
          + (Transition("rnsmp.units.ensure_fails", "rnsmp", "int run_units(", r"^  if \(st\) return st;",
                        _NO_ENSURE),
             Transition("rnsmp.units.launch_fails", "rnsmp", "int run_units(", _LAUNCH_FAILS, _NO_LAUNCH))
          + _exempt("mdntt", "int run(") + _exempt("ksntt", "int run_modup(")
          + (Transition("ksntt.mac.launch_fails", "ksntt", "int run_mac(",
                        r'return e == hipSuccess \? NTTMUL_OK : fail\(h->err, e, "mac launch"\);',
                        "the failure branch is reached only when the one launch of the key mac fails"),)
          + _exempt("xconv", "int run("))


# ---------------------------------------------------------------------------------------------
# Operands and CPU references
# ---------------------------------------------------------------------------------------------

def dtype_of(cp):
    import numpy as np
    return np.uint32 if cp.bits == 32 else np.uint64


def ks_of(cp, step):
    """The rotations of a hoist or key-mac step."""
    if cp.lib == "rnsmp":
        return HC.draw(cp.n, step.rots, 1)
    if cp == CHAIN_CTX["ks"]:
        return (CHAIN_K,)
    return LC.ks_of(cp.n, step.rots)


def shapes(cp, step):
    """{operand: (shape, moduli of its second-last axis)} of a step's inputs, and the output's
    shape: (ins, out)."""
    n, b = cp.n, step.batch
    m = moduli_of(cp)
    if cp.lib == "rnsmp":
        Lm, t, c, r = len(m), step.terms, step.comps, step.rots
        if step.entry == "multiply":
            return {"a": ((b, Lm, n), m), "b": ((b, Lm, n), m)}, (b, Lm, n)
        if step.entry in ("forward", "inverse", "inverse_inplace"):
            return {"a": ((b, Lm, n), m)}, (b, Lm, n)
        if step.entry == "mac":
            return {"a": ((b, t, Lm, n), m), "b": ((b, t, Lm, n), m)}, (b, Lm, n)
        if step.entry == "macn":
            return {"a": ((b, t, Lm, n), m), "b": ((c, t, Lm, n), m)}, (b, c, Lm, n)
        assert step.entry == "hoist"
        return {"a": ((b, t, Lm, n), m), "b": ((r, c, t, Lm, n), m)}, (b, r, c, Lm, n)
    q, p = m
    L, K = len(q), len(p)
    if cp.lib == "mdntt":
        return {"a": ((b, L + K, n), q + p)}, (b, L, n)
    if cp.lib == "xconv":
        if step.entry == "extend":
            return {"a": ((b, K, n), p)}, (b, L, n)
        return {"a": ((b, L + K, n), q + p)}, (b, L, n)
    assert cp.lib == "ksntt"
    if step.entry == "modup":
        return {"a": ((b, L, n), q)}, (b, -(-L // cp.shape[2]), L + K, n)
    t, c, r = step.terms, step.comps, step.rots
    if step.view:
        q_top, _ = LC.chain_bases(cp.bits)
        assert q_top[:L] == q and step.view == (len(q_top), LC.TOP_TERMS)
        key = ((r, c, step.view[1], len(q_top) + K, n), q_top + p)
    else:
        key = ((r, c, t, L + K, n), q + p)
    return {"a": ((b, t, L + K, n), q + p), "b": key}, (b, r, c, L + K, n)


def _seed(name, index, salt):
    return salt * 1000 + 37 * sorted(MODEL_SEQUENCES).index(name) + index


def draw(cp, step, seed):
    """A step's operands: seeded canonical words, every limb below its own modulus; with
    status "ERANGE", word 5 of limb 1 of polynomial `bad` of a is that limb's modulus."""
    import numpy as np
    import bconv_ref as B
    rng = np.random.default_rng(seed)
    ins = {}
    for k, (shape, m) in shapes(cp, step)[0].items():
        lead = int(np.prod(shape[:-2]))
        ins[k] = B.random_words(rng, m, lead, cp.n, dtype_of(cp)).reshape(shape)
    if step.status == "ERANGE":
        shape, m = shapes(cp, step)[0]["a"]
        ins["a"].reshape(shape[0], -1, len(m), cp.n)[step.bad, 0, 1, 5] = m[1]
    return ins


def inputs(name, index, salt=SALT):
    """The operands of step `index` of a sequence: inputs no other step of any run has."""
    cp, steps = MODEL_SEQUENCES[name]
    return draw(cp, steps[index], _seed(name, index, salt))


def band_count(cp, step, ins):
    """The coefficients of an xconv step's input inside the guard band (tests/test_xconv_ref.py's
    check of seeded_gpu_inputs): through the oracle's inverse transform of the P part."""
    from fractions import Fraction
    import xconv_ref
    q, p = moduli_of(cp)
    x = ins["a"]
    xp = x if step.entry == "extend" else x[:, len(q):]
    coef = inverse(xp, p)
    return xconv_ref.count_in_band(coef, p, cp.shape[2], Fraction(len(p), 1 << XC.BAND_LOG2))


def forward(x, moduli):
    """[.., limbs, n] canonical coefficients -> NTT order, per limb by the oracle's loop
    (hoist_ref.forward, over all polynomials of a limb at once)."""
    return _transforms(x, moduli, "mulntt_ct_std2rev", "mixed_powers_rev", False)


def inverse(x_hat, moduli):
    """[.., limbs, n] NTT order -> canonical coefficients scaled by n^-1 (hoist_ref.inverse_one)."""
    return _transforms(x_hat, moduli, "nttmul_gs_rev2std", "inv_mixed_powers_rev", True)


def _transforms(x, moduli, fn, table, scaled):
    import numpy as np
    import hoist_ref as H
    x = np.asarray(x)
    n = x.shape[-1]
    flat = x.reshape(-1, len(moduli), n)
    out = np.empty_like(flat)
    for l, q in enumerate(moduli):
        rows = np.ascontiguousarray(flat[:, l], dtype=np.uint64)
        out[:, l] = H.plan(n, q).transform_batch(fn, rows, table, pow(n, -1, q) if scaled else 0)
    return out.reshape(x.shape)


def products(a, b, moduli):
    """a * b mod (x^n + 1, q_l) per (polynomial, limb) of [.., limbs, n] operands: the oracle's
    whole-batch product."""
    import numpy as np
    import hoist_ref as H
    n = a.shape[-1]
    fa, fb = a.reshape(-1, len(moduli), n), b.reshape(-1, len(moduli), n)
    out = np.empty_like(fa)
    for l, q in enumerate(moduli):
        P = H.plan(n, q)
        x, y = np.ascontiguousarray(fa[:, l]), np.ascontiguousarray(fb[:, l])
        if q < (1 << 31):
            out[:, l] = P.fast_batch_u32(x.astype(np.uint32), y.astype(np.uint32))[0]
        else:
            out[:, l] = P.product_batch(x.astype(np.uint64), y.astype(np.uint64))[0]
    return out.reshape(a.shape)


def _sum_terms(prods, moduli, axis):
    """The sum over `axis` of [.., limbs, n] products, modulo each limb's modulus."""
    import numpy as np
    total = prods.astype(object).sum(axis=axis)
    for l, q in enumerate(moduli):
        total[..., l, :] %= q
    return total.astype(prods.dtype)


def device_operands(cp, step, ins):
    """What the call is given: for "mac" and "macn" b goes in as its forward transform."""
    if cp.lib == "rnsmp" and step.entry in ("mac", "macn"):
        return {"a": ins["a"], "b": forward(ins["b"], moduli_of(cp))}
    return ins


def expected(cp, step, ins):
    """The CPU reference's result for a step on inputs `ins` (as `draw` gives them): every output
    word, at every n (the conversions through tests/full_ref.py)."""
    import numpy as np
    m = moduli_of(cp)
    a = ins["a"]
    if cp.lib == "rnsmp":
        if step.entry == "multiply":
            return products(a, ins["b"], m)
        if step.entry == "forward":
            return forward(a, m)
        if step.entry in ("inverse", "inverse_inplace"):
            return inverse(a, m)
        if step.entry == "mac":
            return _sum_terms(products(a, ins["b"], m), m, 1)
        if step.entry == "macn":
            b = np.broadcast_to(ins["b"][None], (a.shape[0],) + ins["b"].shape)
            wide = np.broadcast_to(a[:, None], b.shape)
            return _sum_terms(products(np.ascontiguousarray(wide), np.ascontiguousarray(b), m), m, 2)
        import hoist_ref
        return hoist_ref.hoist(a, ins["b"], ks_of(cp, step), m)
    q, p = m
    if cp.lib == "ksntt" and step.entry == "mac":
        import ksntt_ref
        import level_ref
        key = ins["b"]
        if step.view:
            key = level_ref.gather(key, step.view, len(q), step.terms)
        return ksntt_ref.mac(a, key, ks_of(cp, step), q + p)
    import full_ref
    if cp.lib == "mdntt":
        return full_ref.reference("mdntt", "moddown", a, q, p)
    if cp.lib == "xconv":
        return full_ref.reference("xconv", step.entry, a, q, p, cp.shape[2])
    return full_ref.reference("ksntt", "modup", a, q, p, cp.shape[2])
