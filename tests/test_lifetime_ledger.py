"""The lifetime ledger: tests/lifetime_cases.py held against csrc/nttmul.cpp and against its own
model, without a GPU.

* Every TRANSITIONS row names a function of nttmul.cpp and a regular expression that matches
  exactly one line of that function: a refactor that moves the state must move the table.
* Every transition is driven by some (sequence, step) according to model(), every pair a row
  claims is confirmed by the transition's predicate on the state before that step, and no pair
  points outside its sequence.
* The launches of the sequences are rows of dispatch_cases.all_cases(), so the kernel ledger keeps
  describing everything the suite launches.
* The host-path choice of the model at the boundary batches of sequence A.
* The resident server's failure and retry paths (SERVER_SEQUENCES): the cool-down and the cap are
  read from the source, every failure path has its row, and the two paths no sequence can stage
  are EXEMPT rows with their reasons."""
import re

import dispatch_cases as D
import lifetime_cases as L

SOURCE = L.SOURCE


def _function(lines, opening):
    """The lines of the function whose definition starts with `opening` (to the closing brace in
    column 0; a one-line function is its own body)."""
    starts = [i for i, ln in enumerate(lines) if ln.startswith(opening)]
    assert len(starts) == 1, (opening, starts)
    i = starts[0]
    if lines[i].rstrip().endswith("}"):
        return lines[i:i + 1]
    j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith("}"))
    return lines[i:j + 1]


def test_every_transition_matches_one_line_of_its_function():
    lines = open(SOURCE).read().split("\n")
    names = [t.name for t in L.TRANSITIONS]
    assert len(names) == len(set(names))
    for t in L.TRANSITIONS + L.EXEMPT:
        hits = [ln for ln in _function(lines, t.func) if re.search(t.line, ln)]
        assert len(hits) == 1, (t.name, t.func, hits)


def test_every_transition_is_driven_and_every_claim_confirmed():
    driven = {}
    for name in L.ALL_SEQUENCES:
        for in_vram in (True, False):
            for i, w in enumerate(L.model(name, in_vram)):
                for tag in w.tags:
                    driven.setdefault(tag, []).append((name, i))
    table = {t.name for t in L.TRANSITIONS}
    assert sorted(set(driven) - table) == [], "the model names transitions the table lacks"
    for t in L.EXEMPT:                      # a reason instead of a step, and no step after all
        assert t.name not in table and t.name not in driven and len(t.pairs) > 20, t.name
    for t in L.TRANSITIONS:
        assert driven.get(t.name), f"no step of any sequence drives {t.name}"
        assert t.pairs, t.name
        for name, i in t.pairs:
            cp, steps = L.ALL_SEQUENCES[name]
            assert 0 <= i < len(steps), (t.name, name, i)
            assert L.drives(t.name, cp, L.state_before(name, i), steps[i]), (t.name, name, i)


def test_predicates_depend_on_the_state_before():
    """The same step on a fresh context drives other transitions than in its sequence: the pairing
    is about the state, not the step alone."""
    cp, steps = L.SEQUENCES["C"]
    fresh = L.new_state(cp)
    assert L.drives("scratch.wait_other_stream", cp, L.state_before("C", 2), steps[2])
    assert not L.drives("scratch.wait_other_stream", cp, fresh, steps[2])
    assert L.drives("scratch.first_use", cp, fresh, steps[2])
    cp, steps = L.SEQUENCES["A"]
    assert L.drives("server.relaunch", cp, L.state_before("A", 7), steps[7])
    assert L.drives("server.launch_first", cp, L.new_state(cp), steps[7])
    assert L.drives("slots.grow", cp, L.state_before("A", 5), steps[5])
    assert L.drives("slots.alloc_first", cp, L.new_state(cp), steps[5])


def test_the_sequences_hold_what_the_plan_asks_for():
    paths = [w.path for w in L.model("A")]
    assert {p for p in paths if p is not None} == {0, 1, 2, 3}
    # A: four chunks over three slots with a partial last one, slots at 8 MiB afterwards
    cp, steps = L.SEQUENCES["A"]
    assert steps[9].batch == 3 * 8192 + 5
    assert L.model("A")[9].state["dev"][0]["slot_bytes"] == 8 << 20
    assert L.model("A")[5].state["dev"][0]["slot_bytes"] == 64 << 10
    assert sum(s.batch for s in steps if L.op_of(s) == "multiply" and s.entry != "shim256") > 24581
    # B: slots double with the word width; 2048 then 1024 polynomials per chunk
    b = L.model("B")
    assert [b[i].state["dev"][0]["slot_bytes"] for i in (0, 2, 4, 6)] == \
        [3 * 4096, 3 * 8192, 8 << 20, 8 << 20]
    assert b[1].state["dev"][0]["sscr"][0]["perm"] == 3 * 4096
    assert b[3].state["dev"][0]["sscr"][0]["perm"] == 3 * 8192
    # C: 32 polynomials per sub-batch; buf in 4-byte plan words, perm in the caller's 8-byte words
    c = L.model("C")
    scr = [w.state["dev"][0]["dscr"] for w in c]
    assert [s["buf"] for s in scr] == [32768, 3 * 32768, 3 * 32768] + [1 << 20] * 4
    assert [s["perm"] for s in scr] == [0, 0, 3 * 32768, 3 * 32768] + [2 << 20] * 3
    assert [s["last"] for s in scr] == ["A", "A", "B", "B", "A", "B", "null"]
    # D: two polynomials per sub-batch
    assert L.model("D")[1].state["dev"][0]["dscr"]["buf"] == 1 << 20
    assert L.model("D")[1].state["last_prod"] == (2, 64, 1)
    # E alternates a buf user and a perm user, sized as test_device_calls_on_two_streams
    cp, steps = L.SEQUENCES["E"]
    assert (cp.n, cp.q, cp.scratch_mb, L.E_BATCH) == (16384, D.Q31, 32, 1200)
    assert [(s.entry, s.place, s.mode) for s in steps] == [("multiply", "A", 0), ("transform", "B", 2)] * 3
    # F: the bad coefficient lies in chunk 2 of four, and in the third sub-batch
    cp, steps = L.SEQUENCES["F_host"]
    chunk = L.CHUNK_BYTES // (cp.n * 4)
    assert chunk == 512 and steps[0].batch == 3 * chunk + 1 and steps[0].bad // chunk == 2
    cp, steps = L.SEQUENCES["F_sub"]
    assert steps[0].bad // ((1 << 20) // (cp.n * 4)) == 2
    for name in ("F_host", "F_device", "F_sub"):
        steps = L.SEQUENCES[name][1]
        assert [s.status for s in steps] == ["ERANGE", "OK", "OK", "OK"]
        assert steps[1].place == "host" and steps[2].place == "B" and L.op_of(steps[3]) == "transform"
    assert L.model("F_server")[2].path == 3
    # G: slice 0 gets nothing of a batch of 1; each DevState grows its own slots
    g = L.model("G")
    assert [[d["slot_bytes"] for d in w.state["dev"]] for w in g] == \
        [[0, 8192], [4 * 8192, 5 * 8192], [4 * 8192, 5 * 8192], [8 << 20, 8 << 20], [8 << 20, 8 << 20]]
    # J runs sequences that exist, and its second pair shares the staged path's CopyPool
    for pair in L.THREAD_PAIRS:
        assert all(p in L.SEQUENCES for p in pair)
    assert all(any("copy_pool.shared" in w.tags for w in L.model(p)) for p in L.THREAD_PAIRS[1])


def test_the_launches_are_rows_of_the_kernel_ledger():
    rows = L.lifetime_cases()
    assert len(rows) > 60 and len(rows) == len(set(rows))
    have = set(D.all_cases())
    assert [r for r in rows if r not in have] == []
    for r in rows:
        assert D.kernels_of(r)
    # each kind of launch the sequences make
    assert {r.op for r in rows} == {"multiply", "transform", "pointwise", "fill"}
    assert {r.path for r in rows} == {"device", "server"}
    assert any(r.validate for r in rows) and any(not r.prio_ok for r in rows)


def test_host_path_choice_at_the_boundaries():
    """Sequence A's context, n = 256 in 32-bit words (1 KiB per polynomial): the server takes up to
    1024 words per operand, zero-copy up to 64 KiB per chunk, staged beyond; page-locked operands
    go direct whatever the batch, except where the server takes them first."""
    cp = L.SEQUENCES["A"][0]

    def path(batch, place="host", bits=32, entry="multiply"):
        return L.host_path(cp, L.Step(entry, place, bits, batch))
    assert [path(b) for b in (1, 4, 5, 64, 65, 8192, 24581)] == [3, 3, 2, 2, 0, 0, 0]
    assert path(4, "pinned") == 3 and path(5, "pinned") == 1 and path(200, "pinned") == 1
    assert [path(b, bits=64) for b in (1, 4, 32, 33)] == [2, 2, 2, 0]      # u64: never the server
    assert [path(b, entry="forward") for b in (1, 64, 65)] == [2, 2, 0]    # nor a transform
    assert path(4, entry="pointwise") == 2
    # n = 1024: one polynomial is the server's whole mailbox; n = 2048 is past it
    assert L.host_path(L.Ctx(1024, D.Q31), L.Step("multiply", "host", 32, 1)) == 3
    assert L.host_path(L.Ctx(1024, D.Q31), L.Step("multiply", "host", 32, 2)) == 2
    assert L.host_path(L.Ctx(2048, D.Q31), L.Step("multiply", "host", 32, 1)) == 2
    # not a Plantard modulus, two slices, or n > 4096: no server, no zero-copy
    assert L.host_path(L.Ctx(1024, D.Q32), L.Step("multiply", "host", 32, 1)) == 2
    assert L.host_path(L.Ctx(256, D.Q31HI, ndev=2), L.Step("multiply", "host", 32, 1)) == 2
    assert L.host_path(L.Ctx(8192, D.Q31), L.Step("multiply", "host", 32, 1)) == 0
    # two slices: the first chunk is sized by batch / ndev
    g = L.SEQUENCES["G"][0]
    assert [L.host_path(g, L.Step("multiply", "host", 32, b)) for b in (1, 16, 17, 18)] == [2, 2, 2, 0]


def test_the_server_failure_sequences_hold_what_the_plan_asks_for():
    """SERVER_SEQUENCES against the constants of nttmul.cpp: how long the cool-down lasts, when
    the server is tried again, where the cap falls, and that no step leaves a request posted."""
    src = open(SOURCE).read()
    R, M = L.RETRY_CALLS, L.MAX_FAILURES
    assert f"kServerRetryCalls = {R}, kServerMaxFailures = {M};" in src and R > 8 and M == 3
    for name, (cp, steps) in L.SERVER_SEQUENCES.items():
        assert cp.lib == "diag" and cp.ndev == 1
        assert all(s.place == "host" and 1 <= s.batch <= 4 for s in steps), name
        for in_vram in (True, False):
            for w in L.model(name, in_vram):
                S = w.state["server"]
                assert S["go_is_served"] and S["failures"] <= M, name
                assert S["disabled"] == (w.state["server"]["reason"] is not None
                                         and not S["reason"][2]), name
    srv = lambda name, i, v=True: L.model(name, v)[i].state["server"]     # noqa: E731
    # S1: both stalled calls are served by the relaunch inside the spin loop
    s1 = L.model("S1")
    assert [w.path for w in s1] == [3] * 5 and srv("S1", 4)["failures"] == 0
    assert [w.state["server"]["spin"] for w in s1] == [0, 1, 1, 2, 2]
    assert [w.state["server"]["launches"] for w in s1] == [1, 2, 2, 3, 3]
    assert L.SEQUENCES is not L.ALL_SEQUENCES and "S1" not in L.SEQUENCES
    # S2: refused in the middle of a request with the larger request's words behind it, R eligible
    # calls on the launch path, the range failure and the pointwise call not among them
    for name, n in (("S2", 256), ("S2_512", 512), ("S2_1024", 1024)):
        cp, steps = L.SERVER_SEQUENCES[name]
        m = L.model(name)
        assert cp.n == n and cp.validate and steps[0].batch == (4 if n == 256 else 1)
        assert steps[2].batch <= steps[0].batch and len(steps[2].arm) == 2
        assert m[0].path == 3 and m[2].path in (0, 1, 2) and m[2].state["server"]["failures"] == 1
        assert m[2].state["server"]["reason"] == (1, "ENOMEM", True, "LAUNCH")
        cool = m[3:3 + R + 2]
        assert [s.status for s in steps[3:3 + R + 2]].count("ERANGE") == 1
        assert [s.entry for s in steps[3:3 + R + 2]].count("pointwise") == 1
        assert all(w.path != 3 for w in cool) and cool[-1].state["server"]["cooldown"] == 0
        assert sum("server.cooldown" in w.tags for w in cool) == R
        retry = m[3 + R + 2]
        assert retry.path == 3 and steps[3 + R + 2].batch == 1 and "server.relaunch" in retry.tags
        assert retry.state["server"]["failures"] == 1 and len(m) == R + 7
    # S3: three failures, each after its cool-down; ten calls on the launch path after the third
    cp, steps = L.SERVER_SEQUENCES["S3"]
    armed = [i for i, s in enumerate(steps) if s.arm]
    assert armed == [0, R + 1, 2 * R + 2] and len(steps) == armed[-1] + 1 + 10
    assert [srv("S3", i)["reason"] for i in armed] == \
        [(k, "ENOMEM", k < M, "LAUNCH") for k in (1, 2, 3)]
    assert all(w.path == 2 for w in L.model("S3")) and srv("S3", len(steps) - 1)["failures"] == M
    assert not srv("S3", armed[1])["disabled"] and srv("S3", armed[2])["disabled"]
    # S4: any other error is permanent at once
    assert srv("S4", 0)["reason"] == (1, "EHIP", False, "LAUNCH") and srv("S4", 0)["disabled"]
    assert all(w.path == 2 for w in L.model("S4"))
    # S5: every allocation site, the retry after the cool-down served; the request half's sites
    # are passed only where the request half is not in device memory
    for site in L.ALLOC_SITES:
        name = "S5_" + site.lower()
        for in_vram in (True, False):
            reached = not (in_vram and site.startswith("REQ"))
            m = L.model(name, in_vram)
            assert (m[0].path == 3) == (not reached), (site, in_vram)
            assert m[0].state["server"]["failures"] == int(reached)
            assert m[0].state["server"]["allocated"] == (not reached)
            assert ("server.alloc_rollback" in m[0].tags) == reached
            assert [w.path for w in m[R + 1:]] == [3, 3] and m[-1].state["server"]["allocated"]
            assert m[-1].state["server"]["failures"] == int(reached)
    # S6: destroyed in cool-down, and permanently switched
    assert 0 < srv("S6_cool", 5)["cooldown"] < R and not srv("S6_cool", 5)["disabled"]
    assert srv("S6_off", 3)["disabled"] and not srv("S6_off", 3)["allocated"]
    assert [w.path for w in L.model("S6_fresh")] == [3, 3]
