"""The lifetime ledger: tests/lifetime_cases.py held against csrc/nttmul.cpp and against its own
model, without a GPU.

* Every TRANSITIONS row names a function of nttmul.cpp and a regular expression that matches
  exactly one line of that function: a refactor that moves the state must move the table.
* Every transition is driven by some (sequence, step) according to model(), every pair a row
  claims is confirmed by the transition's predicate on the state before that step, and no pair
  points outside its sequence.
* The launches of the sequences are rows of dispatch_cases.all_cases(), so the kernel ledger keeps
  describing everything the suite launches.
* The host-path choice of the model at the boundary batches of sequence A."""
import os
import re

import dispatch_cases as D
import lifetime_cases as L

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "ntt-based-polynomial-multiplier-fpga_amd", "csrc", "nttmul.cpp")


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
    for t in L.TRANSITIONS:
        hits = [ln for ln in _function(lines, t.func) if re.search(t.line, ln)]
        assert len(hits) == 1, (t.name, t.func, hits)


def test_every_transition_is_driven_and_every_claim_confirmed():
    driven = {}
    for name in L.SEQUENCES:
        for i, w in enumerate(L.model(name)):
            for tag in w.tags:
                driven.setdefault(tag, []).append((name, i))
    table = {t.name for t in L.TRANSITIONS}
    assert sorted(set(driven) - table) == [], "the model names transitions the table lacks"
    for t in L.TRANSITIONS:
        assert driven.get(t.name), f"no step of any sequence drives {t.name}"
        assert t.pairs, t.name
        for name, i in t.pairs:
            cp, steps = L.SEQUENCES[name]
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
