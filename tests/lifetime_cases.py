"""Call sequences over one long-lived context, and a pure-Python mirror of the state the context
keeps between calls (csrc/nttmul.cpp).  Plain data and arithmetic: no GPU, no library, no oracle.

Three things live here:

* `SEQUENCES`: named (context parameters, steps) lists.  A `Step` names the entry point, where its
  operands live, the word width, the batch, the transform mode and the status the call returns.
  tests/test_gpu_lifetime.py runs them, every step on inputs of its own and against the oracle.
* `walk(ctx, state, step)`: what one call does to the state, restated from nttmul.cpp: the host
  path (run_server's eligibility, then direct / zero-copy / staged), the pipeline slots of each
  device slice (ensure_slots), every scratch a launch goes through (scratch_acquire, ensure,
  scratch_release), the resident server's `running` mark, prod_s and last_prod.  It returns the
  state after the call, the names of the transitions the call drives, and the launches it makes as
  dispatch_cases.Case rows.  `model(name)` walks a whole sequence.
* `TRANSITIONS`: one row per state transition: the function of nttmul.cpp and a regular expression
  that matches exactly one line of that function, the line that implements the transition, and
  the (sequence, step index) pairs that drive it.  `drives(transition, ctx, state, step)` is the
  pure predicate over (state before, step) behind each row.

`SERVER_SEQUENCES` are the sequences over the resident server's failure and retry paths: their
steps arm failure points of the diagnostic library (include/nttmul_diag.h), and the model's
"server" entry carries the failure count, the cool-down, the permanent switch to the launch path
and whether the go word equals the last one served.  tests/test_gpu_server_failures.py runs them.

tests/test_lifetime_ledger.py holds the table against the source and the model without a GPU.
"""
import copy
import os
import re
from collections import namedtuple

import dispatch_cases as D
from dispatch_cases import Case, Q0, Q31, Q31HI, Q32, Q62

SLOTS = 3                       # nttmul.cpp kSlots
CHUNK_BYTES = 8 << 20           # kChunkBytes
ZERO_COPY = 64 << 10            # nttmul_params.zero_copy_kb default
SERVER_WORDS = 1024             # launch.hpp ServerBox::kWords
PATHS = ("staged", "direct", "zero_copy", "server")     # nttmul_last_host_path 0, 1, 2, 3

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "ntt-based-polynomial-multiplier-fpga_amd", "csrc", "nttmul.cpp")


def _server_constants():
    """kServerRetryCalls and kServerMaxFailures as nttmul.cpp states them."""
    m = re.findall(r"constexpr unsigned kServerRetryCalls = (\d+), kServerMaxFailures = (\d+);",
                   open(SOURCE).read())
    assert len(m) == 1, m
    return int(m[0][0]), int(m[0][1])


RETRY_CALLS, MAX_FAILURES = _server_constants()
# include/nttmul_diag.h: the failure points in the order server_alloc passes them, then the launch
ALLOC_SITES = ("BOX_ALLOC", "BOX_MAP", "STREAM", "REQ_ALLOC", "REQ_MAP")
SITES = ALLOC_SITES + ("LAUNCH", "STALL_BEFORE_GO")
# the error an armed site returns: hipErrorOutOfMemory (fail() maps it to NTTMUL_ENOMEM, the
# status server_unavailable retries) or hipErrorInvalidValue (NTTMUL_EHIP: no retry)
ENOMEM, EINVAL = "ENOMEM", "EINVAL"

# lib: "plain" (nttmul.Context), "mac" (nttmul.MacContext) or "diag" (nttmul.Context on
#   nttmul.load_diag_library(): the failure points of SERVER_SEQUENCES)
Ctx = namedtuple("Ctx", "n q lib scratch_mb validate ndev share_devices",
                 defaults=("plain", 0, False, 1, False))

# entry: "multiply" | "multiply_one" (nttmul_multiply_u32) | "forward" | "inverse" | "pointwise" |
#   "transform" | "mac" | "fill" (nttmul_fill_random_device) | "shim256" (ntt256_product1, the
#   library's own n = 256 context)
# place: device operands on caller stream "A", "B" or the "null" stream; "host" (pageable) or
#   "pinned" (nttmul.host_empty) host arrays
# status: "OK", or "ERANGE" on a validating context: polynomial `bad` of a holds one coefficient q
# arm: failure points armed before the call, (site, error, skip) each: after `skip` further passes
#   the site's runtime call is not made and returns `error` (STALL_BEFORE_GO: error None)
Step = namedtuple("Step", "entry place bits batch mode status terms bad arm",
                  defaults=(0, "OK", 0, None, ()))

HOST_PLACES = ("host", "pinned")


def op_of(step):
    return {"multiply_one": "multiply", "forward": "transform", "inverse": "transform",
            "shim256": "multiply"}.get(step.entry, step.entry)


def mode_of(step):
    return {"forward": 0, "inverse": 3}.get(step.entry, step.mode)


def _h(entry, batch, bits=32, place="host", **kw):
    return Step(entry, place, bits, batch, **kw)


def _d(entry, place, bits, batch, **kw):
    return Step(entry, place, bits, batch, **kw)


# A. every host path on one context, the server stopped and relaunched in between
SEQ_A = (Ctx(256, Q31HI), [
    _h("multiply", 1),                          # 0 server, first launch
    _h("multiply", 4),                          # 1 server, resident
    _h("multiply", 5),                          # 2 zero-copy; slots allocated at 5 KiB
    _h("forward", 5),                           # 3
    _h("inverse", 5),                           # 4
    _h("multiply", 64),                         # 5 zero-copy at exactly 64 KiB; slots grow
    _h("multiply", 65),                         # 6 staged
    _h("multiply", 2),                          # 7 server, relaunched after the quiesce
    _h("pointwise", 3),                         # 8 never the server's: quiesces it
    _h("multiply", 3 * 8192 + 5),               # 9 staged, four chunks over three slots, 8 MiB
    _h("multiply", 3),                          # 10 server
    _d("multiply", "A", 32, 7),                 # 11 a device call stops the server
    _h("multiply", 200, place="pinned"),        # 12 direct
    _h("multiply_one", 1),                      # 13 server, through nttmul_multiply_u32
    _h("shim256", 1),                           # 14 the library's own context beside this one
    _h("multiply", 4),                          # 15 server, still resident
    _d("fill", "B", 32, 3),                     # 16 a fill stops the server
    _h("multiply", 1),                          # 17 server, relaunched
])

# B. both word widths on one context (Arith32W: no server)
SEQ_B = (Ctx(1024, Q32), [
    _h("multiply", 3),                          # 0
    _h("transform", 3, mode=2),                 # 1 perm of slot 0, 4-byte words
    _h("multiply", 3, bits=64),                 # 2 slots double
    _h("transform", 3, bits=64, mode=1),        # 3 perm grows in 8-byte words
    _h("multiply", 8195),                       # 4 staged: 4 x 2048 + 3
    _h("transform", 3, mode=1),                 # 5
    _h("multiply", 8195, bits=64),              # 6 staged: 8 x 1024 + 3
    _h("transform", 3, bits=64, mode=2),        # 7
    _h("multiply", 1),                          # 8
])

# C. multi-pass scratch on two caller streams, 32 polynomials per sub-batch
SEQ_C = (Ctx(8192, Q31, scratch_mb=1), [
    _d("multiply", "A", 32, 1),                 # 0 first use
    _d("multiply", "A", 32, 3),                 # 1 grows, same stream
    _d("transform", "B", 32, 3, mode=2),        # 2 other stream; perm's first use beside buf
    _d("multiply", "B", 64, 65),                # 3 buf to its cap, three sub-batches
    _d("transform", "A", 64, 65, mode=1),       # 4 perm grows in 8-byte words, buf reused
    _d("forward", "B", 32, 2),                  # 5 buf only, no growth
    _d("multiply", "null", 32, 33),             # 6
])

# D. the square split, 2 polynomials per sub-batch
SEQ_D = (Ctx(65536, Q62, scratch_mb=1), [
    _d("multiply", "A", 64, 1),
    _d("multiply", "B", 64, 5),
    _d("transform", "A", 64, 3, mode=3 | 4),
    _d("transform", "B", 64, 5, mode=2),
])

# E. calls long enough to overlap when nothing orders them: a buf user and a perm user in flight
E_BATCH = 1200
SEQ_E = (Ctx(16384, Q31, scratch_mb=32), [
    s for _ in range(3) for s in (_d("multiply", "A", 32, E_BATCH),
                                  _d("transform", "B", 32, E_BATCH, mode=2))])

# F. a call that fails in the middle, then three calls that must be exact
F_BATCH = 1537                                  # four host chunks of 512 + 512 + 512 + 1
SEQ_F_HOST = (Ctx(4096, Q31, validate=True), [
    _h("multiply", F_BATCH, status="ERANGE", bad=2 * 512 + 7),      # chunk 2
    _h("multiply", 513),
    _d("multiply", "B", 32, 5),
    _h("transform", 3, mode=2),
])
SEQ_F_DEVICE = (Ctx(4096, Q31, validate=True), [
    _d("multiply", "A", 32, F_BATCH, status="ERANGE", bad=2 * 512 + 7),
    _h("multiply", 3),
    _d("multiply", "B", 32, 5),
    _d("transform", "A", 32, 3, mode=2),
])
SEQ_F_SUB = (Ctx(8192, Q31, scratch_mb=1, validate=True), [
    _d("multiply", "A", 32, 65, status="ERANGE", bad=64),           # the third sub-batch's range
    _h("multiply", 3),
    _d("multiply", "B", 32, 33),
    _d("transform", "A", 32, 33, mode=2),
])
SEQ_F_SERVER = (Ctx(256, Q31HI, validate=True), [
    _h("multiply", 2),
    _h("multiply", 2, status="ERANGE", bad=1),
    _h("multiply", 2),
])

# G. two slices on one device: each DevState grows its own slots
SEQ_G = (Ctx(2048, Q31, ndev=2, share_devices=True),
         [_h("multiply", b) for b in (1, 9, 1, 4100, 3)])

# H. the fused multiply-accumulate between server calls
SEQ_H = (Ctx(256, Q31HI, lib="mac"), [
    _h("multiply", 2),
    _d("mac", "A", 32, 5, terms=3),
    _h("multiply", 1),
    _h("mac", 3, terms=2),
    _h("multiply", 4),
])

SEQUENCES = {"A": SEQ_A, "B": SEQ_B, "C": SEQ_C, "D": SEQ_D, "E": SEQ_E, "F_host": SEQ_F_HOST,
             "F_device": SEQ_F_DEVICE, "F_sub": SEQ_F_SUB, "F_server": SEQ_F_SERVER, "G": SEQ_G,
             "H": SEQ_H}


# ---------------------------------------------------------------------------------------------
# The resident server's failure and retry paths (diagnostic library)
# ---------------------------------------------------------------------------------------------

STALL = ("STALL_BEFORE_GO", None, 0)


def _cool(first=0, n=None, top=4):
    """kServerRetryCalls eligible calls (the cool-down), batches 1 .. top in turn."""
    return [_h("multiply", 1 + (first + i) % top) for i in range(RETRY_CALLS if n is None else n)]


# S1. the kernel has left through its idle exit while a request waits: relaunched inside the spin
# loop, served; then smaller requests over the larger one's words in box->c
SEQ_S1 = (Ctx(256, Q31HI, lib="diag"), [
    _h("multiply", 4),                          # 0 first launch
    _h("multiply", 4, arm=(STALL,)),            # 1 relaunch in the spin loop
    _h("multiply", 1),                          # 2 one product: 768 older words stay in box->c
    _h("multiply", 2, arm=(STALL,)),            # 3
    _h("multiply", 3),                          # 4
])


def _s2(n, big):
    """S2. a relaunch refused in the middle of a request, the cool-down, the retry.  Step 1 leaves
    the server stopped, so step 2 launches once on entry whatever the time since step 0 (the host's
    idle margin would otherwise decide) and LAUNCH with skip 1 is the relaunch in the spin loop."""
    cool = _cool(1, top=big)
    cool.insert(20, _h("multiply", 1, status="ERANGE", bad=0))      # neither consumes cool-down
    cool.insert(41, _h("pointwise", 2))
    return (Ctx(n, Q31HI, lib="diag", validate=True), [
        _h("multiply", big),                    # 0 served
        _h("pointwise", 1),                     # 1 never the server's: quiesces it
        _h("multiply", max(1, big // 2), arm=(("LAUNCH", ENOMEM, 1), STALL)),   # 2 refused
    ] + cool + [
        _h("multiply", 1),                      # served again: the retry
        _h("multiply", big),
    ])


SEQ_S2 = _s2(256, 4)
SEQ_S2_512 = _s2(512, 1)
SEQ_S2_1024 = _s2(1024, 1)

# S3. the cap: the third out-of-memory failure leaves the launch path for good
SEQ_S3 = (Ctx(256, Q31HI, lib="diag"),
          [_h("multiply", 2, arm=(("LAUNCH", ENOMEM, 0),))] + _cool(0)
          + [_h("multiply", 3, arm=(("LAUNCH", ENOMEM, 0),))] + _cool(1)
          + [_h("multiply", 4, arm=(("LAUNCH", ENOMEM, 0),))] + _cool(2, 10))

# S4. a failure that is not out of memory: permanent at once
SEQ_S4 = (Ctx(256, Q31HI, lib="diag"),
          [_h("multiply", 3, arm=(("LAUNCH", EINVAL, 0),))] + _cool(0, 6))


def _s5(site):
    """S5. a setup that fails half-way: nothing is left behind, and the retry allocates again."""
    return (Ctx(256, Q31HI, lib="diag"),
            [_h("multiply", 4, arm=((site, ENOMEM, 0),))] + _cool(0)
            + [_h("multiply", 2), _h("multiply", 4)])


# S6. nttmul_destroy on a context in cool-down and on a permanently switched one (the test then
# serves on a fresh context: sequence S6_fresh)
SEQ_S6_COOL = (Ctx(256, Q31HI, lib="diag"),
               [_h("multiply", 4),
                _h("pointwise", 1),
                _h("multiply", 2, arm=(("LAUNCH", ENOMEM, 1), STALL))] + _cool(0, 3))
SEQ_S6_OFF = (Ctx(256, Q31HI, lib="diag"),
              [_h("multiply", 1, arm=(("BOX_MAP", EINVAL, 0),))] + _cool(0, 3))
SEQ_S6_FRESH = (Ctx(256, Q31HI, lib="diag"), [_h("multiply", 4), _h("multiply", 1)])

SERVER_SEQUENCES = {"S1": SEQ_S1, "S2": SEQ_S2, "S2_512": SEQ_S2_512, "S2_1024": SEQ_S2_1024,
                    "S3": SEQ_S3, "S4": SEQ_S4,
                    **{"S5_" + site.lower(): _s5(site) for site in ALLOC_SITES},
                    "S6_cool": SEQ_S6_COOL, "S6_off": SEQ_S6_OFF, "S6_fresh": SEQ_S6_FRESH}
ALL_SEQUENCES = {**SEQUENCES, **SERVER_SEQUENCES}

# I. one caller stream through the four libraries (the stages are listed in
# tests/test_gpu_lifetime.py; the scratch state the limb-aware libraries keep per context is
# modelled in tests/limb_lifetime_cases.py); n, batch, terms
CHAIN = (1024, 3, 2)
# J. two host threads, a context each: the pairs of sequences that run together
THREAD_PAIRS = (("A", "C"), ("A", "B"))


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def _scratch():
    return {"buf": 0, "perm": 0, "used": False, "last": None}


def new_state(cp):
    """A context after nttmul_create.  server: running, launches and served as the host counts
    them; failures, cooldown, disabled (small_server == -1) and reason = (failure number, status
    name, retried, site) of server_unavailable; go_is_served: req->go == S.served, which holds whenever
    no request is in flight; allocated / stream: the mailbox and the stream exist; spin and stops:
    relaunches inside the spin loop and stop requests; armed: site -> [error, passes to skip]."""
    return {"last_path": -1, "failed": False, "last_prod": None,
            "server": {"running": False, "launches": 0, "served": 0, "failures": 0, "cooldown": 0,
                       "disabled": False, "reason": None, "go_is_served": True,
                       "allocated": False, "stream": False, "spin": 0, "stops": 0, "armed": {},
                       "last_batch": 0},
            "dev": [{"slot_bytes": 0, "slot_bits": 0, "slot_op": None, "prod_s": None, "dscr": _scratch(),
                     "sscr": [_scratch() for _ in range(SLOTS)]} for _ in range(cp.ndev)]}


def server_takes(cp, step):
    """run_server's first condition (dispatch_cases.server_eligible, and a context of one device)
    behind run_host's: a u32 multiply."""
    return (step.place in HOST_PLACES and op_of(step) == "multiply" and step.entry != "shim256"
            and step.bits == 32 and cp.ndev == 1
            and D.server_eligible(Case("multiply", cp.n, cp.q, 32, step.batch)))


def zero_copy_chunk(cp, nbytes):
    return nbytes <= ZERO_COPY and cp.n <= 4096


def host_path(cp, step, server=True):
    """The nttmul_last_host_path number a host step reports (run_host / run_server; server=False:
    run_server has declined the call)."""
    assert step.place in HOST_PLACES
    if server and server_takes(cp, step):
        return 3
    pbytes = cp.n * step.bits // 8
    chunk = max(1, CHUNK_BYTES // pbytes)
    if step.place == "pinned":
        return 1
    return 2 if zero_copy_chunk(cp, min(chunk, max(1, step.batch // cp.ndev)) * pbytes) else 0


def slices(cp, batch):
    """[p0, p1) of each context device (run_host)."""
    return [(batch * i // cp.ndev, batch * (i + 1) // cp.ndev) for i in range(cp.ndev)]


Walk = namedtuple("Walk", "state tags cases path")


def walk(cp, before, step, in_vram=True):
    """One call on a context in state `before`: Walk(state after, transition names driven, the
    launches as Case rows, the host path reported or None for a device call).  in_vram: the
    request half of the mailbox goes to fine-grained device memory (server_alloc then never
    reaches REQ_ALLOC and REQ_MAP); the GPU test passes what the machine did."""
    st = copy.deepcopy(before)
    tags, cases = set(), []
    n, q, bits = cp.n, cp.q, step.bits
    logn = n.bit_length() - 1
    io_poly, w_poly = n * bits // 8, n * D.native_bits(q) // 8
    scratch_bytes = (cp.scratch_mb or 512) << 20
    op, mode = op_of(step), mode_of(step)
    erange = step.status == "ERANGE"
    assert not erange or (cp.validate and step.bad is not None and step.bad < step.batch)
    S = st["server"]

    def quiesce(site):
        if S["running"]:
            tags.update(("server.quiesce", "server.quiesce." + site))
            S["running"] = False
            S["stops"] += 1

    for site, error, skip in step.arm:
        assert site in SITES and (error is None) == (site == "STALL_BEFORE_GO")
        assert cp.lib == "diag"
        S["armed"][site] = [error, skip]

    def fires(site):
        """failpoint_fires: the armed error (True for the stall) once `skip` passes are through."""
        f = S["armed"].get(site)
        if f is None:
            return None
        if f[1]:
            f[1] -= 1
            return None
        del S["armed"][site]
        return f[0] or True

    def unavailable(kind, error, site):
        """server_unavailable after fail() at `site`: this call takes the launch path."""
        status = "ENOMEM" if error == ENOMEM else "EHIP"
        S["running"] = False
        S["failures"] += 1
        retry = status == "ENOMEM" and S["failures"] < MAX_FAILURES
        tags.update(("server.unavailable." + kind, "server.status_locked"))
        if retry:
            tags.add("server.retry_armed")
            S["cooldown"] = RETRY_CALLS
        else:
            tags.add("server.permanent.cap" if status == "ENOMEM" else "server.permanent.other")
            S["disabled"] = True
        S["reason"] = (S["failures"], status, retry, site)
        return False

    def serve():
        """run_server past its eligibility and range checks; False: the launch path."""
        if S["cooldown"]:
            tags.add("server.cooldown")
            S["cooldown"] -= 1
            return False
        first = not S["allocated"]
        if first:
            for site in ALLOC_SITES:
                if site == "STREAM" and S["stream"]:
                    continue
                if site in ("REQ_ALLOC", "REQ_MAP") and in_vram:
                    continue
                error = fires(site)
                if error:
                    tags.add("server.alloc_rollback")
                    return unavailable("alloc", error, site)
                if site == "STREAM":
                    S["stream"] = True
            S["allocated"] = True
        if S["running"]:
            tags.add("server.resident")
        else:
            tags.add("server.launch_first" if first else "server.relaunch")
            error = fires("LAUNCH")
            if error:
                return unavailable("launch", error, "LAUNCH")
            S["launches"] += 1
            S["running"] = True
        if fires("STALL_BEFORE_GO"):
            # the kernel has left; the request is posted, found unanswered and the kernel finished
            tags.add("server.spin_relaunch")
            S["go_is_served"] = False
            error = fires("LAUNCH")
            S["go_is_served"] = True            # server_launch takes the go word back first
            if error:
                tags.add("server.take_back")
                return unavailable("relaunch", error, "LAUNCH")
            S["launches"] += 1
            S["spin"] += 1
        if S["served"]:
            tags.add("server.served_advance")
        S["served"] += 1
        S["last_batch"] = step.batch
        return True

    def done(path=None):
        if not erange:
            st["failed"] = False
        return Walk(st, frozenset(tags), cases, path)

    def run_device(dev, sc, stream, p0, count):
        """nttmul.cpp run_device on polynomials [p0, p0 + count) of the call; False: ERANGE."""
        d = st["dev"][dev]
        if cp.validate:
            if st["failed"]:
                tags.add("validate.after_erange")
            if erange and p0 <= step.bad < p0 + count:
                tags.add("validate.erange")
                cases.append(Case(op, n, q, bits, count, mode=mode, validate=True))
                return False
        multipass = logn > 12 and op != "pointwise"
        reorder = op == "transform" and bool(mode & 1) != bool(mode & 2)
        if not multipass and not reorder:
            prio_ok = 1
            if op == "multiply":
                tag = (dev, stream)
                if d["prod_s"] is not None and d["prod_s"] != tag:
                    prio_ok = 0
                    tags.add("prod.stream_change")
                d["prod_s"] = tag
                st["last_prod"] = (count, bits, prio_ok)
                tags.add("err_mu.note_product")
            cases.append(Case(op, n, q, bits, count, mode=mode, validate=cp.validate,
                              prio_ok=prio_ok))
            return True
        chunk = max(1, min(count, scratch_bytes // (w_poly if multipass else io_poly)))
        if not sc["used"]:
            tags.add("scratch.first_use")
        elif sc["last"] != stream:
            tags.add("scratch.wait_other_stream")
        else:
            tags.add("scratch.same_stream")

        def ensure(which, need):
            if sc[which] >= need:
                tags.add("scratch.no_growth")
                return
            tags.add("scratch.grow_after_use" if sc["used"] else "scratch.alloc_unused")
            if sc[which]:
                tags.add(f"scratch.{which}_regrow")
            sc[which] = need
        if multipass:
            ensure("buf", chunk * w_poly)
        if reorder:
            ensure("perm", chunk * io_poly)
            if multipass:
                tags.add("scratch.buf_and_perm")
            if io_poly != w_poly:
                tags.add("scratch.perm_caller_words")
        for s0 in range(0, count, chunk):
            cases.append(Case(op, n, q, bits, min(chunk, count - s0), mode=mode,
                              validate=cp.validate and s0 == 0))
        if count > chunk:
            tags.add("scratch.sub_batches")
            if io_poly != w_poly:
                tags.add("scratch.sub_batch_stride")
        if op == "multiply":
            st["last_prod"] = (chunk, bits, 1)
            tags.update(("prod.note_sub_batch", "err_mu.note_product"))
        sc["used"], sc["last"] = True, stream
        return True

    if step.entry == "shim256":             # another context: this one's state stays
        tags.add("shim.ctx256")
        cases.append(Case("multiply", 256, Q0, 32, 1, path="server"))
        return done()
    if step.entry == "fill":
        quiesce("fill")
        cases.append(Case("fill", n, q, bits, step.batch))
        return done()
    if step.entry == "mac":                 # k_mac: tests/mac_cases.py has its rows
        assert cp.lib == "mac" and logn <= 12
        quiesce("mac_host" if step.place in HOST_PLACES else "mac_device")
        tags.add("mac.host" if step.place in HOST_PLACES else "mac.device")
        return done()
    if step.place not in HOST_PLACES:
        quiesce("device_op")
        if not run_device(0, st["dev"][0]["dscr"], step.place, 0, step.batch):
            st["failed"] = True
        return done()

    served = False
    if server_takes(cp, step) and not S["disabled"]:
        if erange:                          # the range check of run_server, on the host
            tags.add("server.erange")
            st["failed"] = True
            return done(None)
        served = serve()
    if served:
        if st["failed"] and cp.validate:
            tags.add("server.after_erange")
        cases.append(Case("multiply", n, q, 32, step.batch, path="server"))
        path = 3
    else:
        quiesce("run_host")
        path = host_path(cp, step, server=False)
        direct = path == 1
        chunk = max(1, CHUNK_BYTES // io_poly)
        for i, (p0, p1) in enumerate(slices(cp, step.batch)):
            if p1 <= p0:
                tags.add("slices.empty")
                continue
            if i:
                tags.add("slices.thread")
            d = st["dev"][i]
            need, old = min(chunk, p1 - p0) * io_poly, d["slot_bytes"]
            if old >= need:
                tags.add("slots.reuse")
            else:
                tags.add("slots.grow" if old else "slots.alloc_first")
                d["slot_bytes"] = need
            if d["slot_bits"] not in (0, bits):
                tags.add("slots.width_switch")
            if d["slot_op"] not in (None, op):
                tags.add("slots.op_switch")
            d["slot_bits"], d["slot_op"] = bits, op
            for k, c0 in enumerate(range(p0, p1, chunk)):
                cnt = min(chunk, p1 - c0)
                if not direct:
                    tags.add("copy_pool.shared")
                    if k >= SLOTS:
                        tags.add("slots.retire_copy_out")
                zero_copy = not direct and zero_copy_chunk(cp, cnt * io_poly)
                if zero_copy and 0 < old < need:
                    tags.add("slots.pin_dev_after_growth")
                if zero_copy and path == 0:
                    tags.add("host.zero_copy_tail")
                if not run_device(i, d["sscr"][k % SLOTS], f"xs{i}.{k % SLOTS}", c0, cnt):
                    st["failed"] = True
                    if k:
                        tags.add("host.drain_after_error")
                    break
    if st["last_path"] not in (-1, path):
        tags.add("path.change")
    tags.add("path." + PATHS[path])
    st["last_path"] = path
    return done(path)


def model(name, in_vram=True):
    """[Walk] of a sequence, one per step, from a fresh context."""
    cp, steps = ALL_SEQUENCES[name]
    st, out = new_state(cp), []
    for step in steps:
        out.append(walk(cp, st, step, in_vram))
        st = out[-1].state
    return out


def state_before(name, index, in_vram=True):
    cp, _ = ALL_SEQUENCES[name]
    return new_state(cp) if index == 0 else model(name, in_vram)[index - 1].state


def drives(transition, cp, before, step, in_vram=True):
    """The predicate of a transition over (state before, step)."""
    return transition in walk(cp, before, step, in_vram).tags


def lifetime_cases():
    """Every launch the sequences make, as dispatch_cases.Case rows (each distinct row once)."""
    out = []
    for name in ALL_SEQUENCES:
        for w in model(name):
            for c in w.cases:
                if c not in out:
                    out.append(c)
    # I: the plain context's fill
    fill = Case("fill", CHAIN[0], D.Q31LO, 32, CHAIN[1] * CHAIN[2] * 3)
    return out + ([fill] if fill not in out else [])


# ---------------------------------------------------------------------------------------------
# The transitions
# ---------------------------------------------------------------------------------------------

# name: what `walk` calls it;  func: the first words of the line that opens the function of
# csrc/nttmul.cpp;  line: a regular expression that matches exactly one line of that function;
# pairs: (sequence, step index) that drive it
Transition = namedtuple("Transition", "name func line pairs")
T = Transition

TRANSITIONS = (
    # Scratch: dscr of the device calls, sscr[slot] of the host pipeline
    T("scratch.first_use", "int scratch_acquire(", r"if \(!sc\.ev\) HIP_TRY",
      (("C", 0), ("D", 0), ("B", 1))),
    T("scratch.wait_other_stream", "int scratch_acquire(", r"hipStreamWaitEvent\(s, sc\.ev",
      (("C", 2), ("C", 4), ("C", 5), ("C", 6), ("D", 1), ("E", 1), ("E", 2), ("F_sub", 3))),
    T("scratch.same_stream", "int scratch_release(", r"sc\.last = s;",
      (("C", 1), ("C", 3), ("B", 3))),
    T("scratch.alloc_unused", "int ensure(", r"for \(int i = 0; i < nb; i\+\+\) HIP_TRY\(ctx, hipMalloc",
      (("C", 0), ("B", 1), ("F_host", 3))),
    T("scratch.grow_after_use", "int ensure(", r"if \(sc\.used\) HIP_TRY\(ctx, hipEventSynchronize",
      (("C", 1), ("C", 2), ("C", 3), ("C", 4), ("D", 1), ("B", 3))),
    T("scratch.buf_regrow", "int run_device(", r"ensure\(ctx, sc, sc\.buf, 3, &sc\.bytes, chunk \* w_poly\)",
      (("C", 1), ("C", 3), ("D", 1))),
    T("scratch.perm_regrow", "int ensure(", r"if \(bufs\[i\]\) \(void\)hipFree\(bufs\[i\]\);",
      (("C", 4), ("B", 3))),
    T("scratch.no_growth", "int ensure(", r"if \(\*have >= need\) return NTTMUL_OK;",
      (("C", 4), ("C", 5), ("D", 2), ("E", 2), ("B", 5))),
    T("scratch.buf_and_perm", "int run_device(", r"launch_xform\(T, sc\.perm, cp, cnt, io_bits, inv, sc\.buf, s\)",
      (("C", 2), ("C", 4), ("D", 3), ("E", 1))),
    T("scratch.perm_caller_words", "int run_device(", r"&sc\.perm_bytes, chunk \* io_poly\)",
      (("C", 4), ("B", 3), ("B", 7))),
    T("scratch.sub_batches", "int run_device(", r"for \(size_t p = 0; p < batch && !st; p \+= chunk\)",
      (("C", 3), ("C", 4), ("C", 6), ("D", 1), ("D", 2), ("D", 3), ("E", 0))),
    T("scratch.sub_batch_stride", "int run_device(", r"const char \*ap = \(const char \*\)a \+ p \* io_poly;",
      (("C", 3), ("C", 4))),
    # Host slots
    T("slots.alloc_first", "int ensure_slots(", r"hipStreamCreateWithFlags\(&d\.xs\[s\]",
      (("A", 2), ("B", 0), ("G", 0), ("G", 1))),
    T("slots.reuse", "int ensure_slots(", r"if \(d\.slot_bytes >= bytes\) return NTTMUL_OK;",
      (("A", 3), ("A", 8), ("A", 12), ("B", 8), ("G", 2))),
    T("slots.grow", "int ensure_slots(", r"if \(d\.pin\[s\]\[k\]\) \(void\)hipHostFree\(d\.pin\[s\]\[k\]\);",
      (("A", 5), ("A", 6), ("A", 9), ("B", 2), ("B", 4), ("G", 1), ("G", 3))),
    T("slots.pin_dev_after_growth", "int ensure_slots(", r"hipHostGetDevicePointer\(&d\.pin_dev\[s\]\[k\]",
      (("A", 5), ("A", 9), ("B", 2), ("B", 4), ("G", 1))),
    T("slots.width_switch", "int run_host(", r"J\.pbytes = \(size_t\)ctx->plan\.n \* \(io_bits / 8\);",
      (("B", 2), ("B", 4), ("B", 6), ("B", 8))),
    T("slots.op_switch", "int run_host_dev(", r"const bool two = J\.op == OP_MULTIPLY \|\| J\.op == OP_POINTWISE;",
      (("A", 3), ("A", 5), ("A", 8), ("A", 9), ("B", 1), ("B", 2))),
    T("slots.retire_copy_out", "int run_host_dev(", r"if \(!J\.direct\) pcopy\(ctx, \(char \*\)J\.c \+ pd\.off, d\.pin\[s\]\[2\]",
      (("A", 9), ("B", 4), ("B", 6))),
    T("host.zero_copy_tail", "int run_host_dev(", r"const bool zero_copy = !J\.direct && zero_copy_chunk\(ctx, bytes\);",
      (("A", 9), ("B", 4), ("B", 6), ("G", 3))),
    T("host.drain_after_error", "int run_host_dev(", r"const int r = retire\(s\);", (("F_host", 0),)),
    # Host paths
    T("path.staged", "int run_host(", r"ctx->last_path = J\.direct \? 1 : zero_copy_chunk",
      (("A", 6), ("A", 9), ("B", 4), ("G", 3), ("F_host", 0))),
    T("path.direct", "int run_host(", r"J\.direct = host_pinned\(a, total\)", (("A", 12),)),
    T("path.zero_copy", "bool zero_copy_chunk(", r"return bytes <= ctx->zero_copy && ctx->plan\.logn <= 12;",
      (("A", 2), ("A", 5), ("A", 8), ("B", 0), ("G", 0))),
    T("path.server", "int run_server(", r"ctx->last_path = 3;",
      (("A", 0), ("A", 7), ("A", 13), ("H", 0), ("F_server", 2))),
    T("path.change", "int nttmul_last_host_path(", r"return ctx \? ctx->last_path : NTTMUL_EINVAL;",
      (("A", 2), ("A", 6), ("A", 7), ("A", 8), ("A", 9), ("A", 10), ("A", 12), ("A", 13),
       ("B", 4), ("B", 5))),
    # The resident server
    T("server.launch_first", "int run_server(", r"if \(!S\.req\) \{", (("A", 0), ("H", 0), ("F_server", 0))),
    T("server.resident", "int run_server(", r"if \(S\.running && \(now - S\.last_done > kServerIdleHost",
      (("A", 1), ("A", 15))),
    T("server.relaunch", "int server_launch(", r"__atomic_store_n\(&S\.box->done, S\.served, __ATOMIC_RELEASE\);",
      (("A", 7), ("A", 10), ("A", 13), ("H", 2), ("H", 4))),
    T("server.served_advance", "int run_server(", r"S\.served = seq;",
      (("A", 1), ("A", 7), ("A", 15), ("H", 2), ("F_server", 2))),
    T("server.quiesce", "int server_quiesce(", r"return ctx->server\.running \? server_stop\(ctx\) : NTTMUL_OK;",
      (("A", 2), ("A", 8), ("A", 11), ("H", 1), ("H", 3))),
    T("server.quiesce.run_host", "int run_host(", r"server_quiesce\(ctx\)", (("A", 2), ("A", 8))),
    T("server.quiesce.device_op", "static int device_op(", r"server_quiesce\(ctx\)", (("A", 11),)),
    T("server.quiesce.fill", "int nttmul_fill_random_device(", r"server_quiesce\(ctx\)", (("A", 16),)),
    T("server.quiesce.mac_device", "int nttmul_mac_ntt_device(", r"server_quiesce\(ctx\)", (("H", 1),)),
    T("server.quiesce.mac_host", "static int mac_host(", r"server_quiesce\(ctx\)", (("H", 3),)),
    # ... its failure and retry paths (SERVER_SEQUENCES)
    T("server.cooldown", "int run_server(", r"S\.cooldown--;", (("S2", 3), ("S3", 1), ("S5_box_map", 64))),
    T("server.unavailable.alloc", "int run_server(", r"const int st = server_alloc\(ctx, d\);",
      (("S5_box_alloc", 0), ("S5_box_map", 0), ("S5_stream", 0), ("S6_off", 0))),
    T("server.unavailable.launch", "int run_server(", r"const int st = server_launch\(ctx, d\);",
      (("S3", 0), ("S3", RETRY_CALLS + 1), ("S3", 2 * RETRY_CALLS + 2), ("S4", 0))),
    T("server.unavailable.relaunch", "int run_server(", r"if \(rst\) return server_unavailable\(ctx, rst\);",
      (("S2", 2), ("S2_512", 2), ("S2_1024", 2), ("S6_cool", 2))),
    T("server.retry_armed", "int server_unavailable(", r"S\.cooldown = kServerRetryCalls;",
      (("S2", 2), ("S3", 0), ("S3", RETRY_CALLS + 1), ("S5_box_map", 0))),
    T("server.permanent.cap", "int server_unavailable(",
      r"const bool retry = st == NTTMUL_ENOMEM && S\.failures < kServerMaxFailures;",
      (("S3", 2 * RETRY_CALLS + 2),)),
    T("server.permanent.other", "int server_unavailable(", r"ctx->small_server = -1;",
      (("S4", 0), ("S6_off", 0))),
    T("server.spin_relaunch", "int run_server(", r"const int rst = server_launch\(ctx, d\);",
      (("S1", 1), ("S1", 3), ("S2", 2), ("S6_cool", 2))),
    T("server.take_back", "int server_launch(", r"post_go\(S, S\.served\);",
      (("S2", 2), ("S2_512", 2), ("S2_1024", 2), ("S6_cool", 2))),
    T("server.alloc_rollback", "int server_alloc(", r"if \(st\) server_free_mailbox\(S\);",
      (("S5_box_alloc", 0), ("S5_box_map", 0), ("S5_stream", 0), ("S6_off", 0))),
    T("server.status_locked", "int nttmul_server_status(", r"std::lock_guard<std::mutex> l\(g_err_mu\);",
      (("S2", 2), ("S3", 0), ("S4", 0), ("S5_box_map", 0))),
    T("server.erange", "int run_server(", r"if \(pa\[i\] >= P\.q \|\| pb\[i\] >= P\.q\) \{",
      (("F_server", 1), ("S2", 23))),
    T("server.after_erange", "int run_server(", r"for \(size_t i = 0; i < words; i\+\+\) bc\[i\] = ServerBox::kPending;",
      (("F_server", 2),)),
    # prod_s, last_prod, d.flag, err
    T("prod.stream_change", "int run_device(", r"if \(prev && prev != tag\) T\.prio_ok = 0;",
      (("A", 9), ("A", 11), ("A", 12), ("B", 4), ("F_host", 2))),
    T("prod.note_sub_batch", "int run_device(", r"note_product\(ctx, d, chunk, io_bits, T\.prio_ok\);",
      (("C", 0), ("C", 3), ("D", 1), ("E", 0), ("F_sub", 2))),
    T("validate.erange", "int run_device(", r"if \(bad\) \{",
      (("F_host", 0), ("F_device", 0), ("F_sub", 0))),
    T("validate.after_erange", "int run_device(", r"hipMemsetAsync\(d\.flag, 0, sizeof\(int\), s\)",
      (("F_host", 1), ("F_device", 1), ("F_sub", 1))),
    # Process-wide state: one copy per shared library
    T("copy_pool.shared", "void pcopy(", r"CopyPool::get\(\)\.copy\(dst, src, bytes, ctx->copy_threads\);",
      (("A", 6), ("A", 9), ("B", 4), ("B", 6), ("G", 3))),
    T("err_mu.note_product", "void note_product(", r"std::lock_guard<std::mutex> lk\(g_err_mu\);",
      (("A", 2), ("A", 11), ("C", 0), ("G", 1))),
    T("shim.ctx256", "static nttmul_ctx *ctx256(", r"std::call_once\(g_once256\[cyclic\]", (("A", 14),)),
    # Slices
    T("slices.empty", "int run_host(", r"if \(p1 > 0\) status\[0\] = run_host_dev\(ctx, ctx->dev\[0\], J, 0, p1\);",
      (("G", 0), ("G", 2))),
    T("slices.thread", "int run_host(", r"th\.emplace_back\(\[ctx, &J, &status, i, p0, p1\] \{",
      (("G", 0), ("G", 1), ("G", 3), ("G", 4))),
    # libnttmul_mac.so's calls on the same context
    T("mac.device", "static int mac_run(", r"launch_mac\(tables_for\(ctx, d\), a, b_hat, c, batch, terms", (("H", 1),)),
    T("mac.host", "static int mac_host(", r"const hipError_t e = hipStreamSynchronize\(d\.stream\);", (("H", 3),)),
)

# Paths of run_server that no sequence drives, with the line each would pin and the reason.
EXEMPT = (
    T("server.query_error", "int run_server(", r"return fail\(ctx, q, \"device server\"\);",
      "a real error of hipStreamQuery means the device is gone, and a staged one leaves a live "
      "kernel the host has disowned"),
    T("server.timeout", "int run_server(", r"set_err\(ctx, \"device server: no answer within 5 s\"\);",
      "needs a resident kernel that hangs for 5 s"),
)
