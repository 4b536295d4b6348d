"""The limb-library lifetime ledger: tests/limb_lifetime_cases.py held against csrc/rnsmp.cpp,
mdntt.cpp, ksntt.cpp and xconv.cpp and against its own model, without a GPU.

* Every TRANSITIONS and EXEMPT row names one of the four files, a function of it and a regular
  expression that matches exactly one line of that function.
* Every transition is driven by some (sequence, step) according to model(), every pair a row claims
  is confirmed on the state before that step, and no pair points outside its sequence.
* The four files have the same set of common transition names: a copy of the state machine that
  loses a line fails by name.
* Every sequence's model ends in the state its last step implies, and holds what the plan asks for
  (the sub-batch counts, which buffers exist, R_overlap's floor of sixteen sub-batches per call).
* Every xconv input the GPU test feeds the library has no coefficient inside the guard band, so
  that no GPU assertion depends on the seeds."""
import os
import re

import pytest

import limb_lifetime_cases as L
from test_lifetime_ledger import _function


def _lines(lib):
    return open(os.path.join(L.CSRC, L.FILES[lib])).read().split("\n")


def test_every_row_matches_one_line_of_its_function_of_its_file():
    names = [t.name for t in L.TRANSITIONS + L.EXEMPT]
    assert len(names) == len(set(names))
    src = {lib: _lines(lib) for lib in L.FILES}
    for t in L.TRANSITIONS + L.EXEMPT:
        assert t.name.startswith(t.file + "."), t.name
        hits = [ln for ln in _function(src[t.file], t.func) if re.search(t.line, ln)]
        assert len(hits) == 1, (t.name, t.func, hits)


def test_every_transition_is_driven_and_every_claim_confirmed():
    driven = {}
    for name in L.MODEL_SEQUENCES:
        for i, w in enumerate(L.model(name)):
            for tag in w.tags:
                driven.setdefault(tag, []).append((name, i))
    table = {t.name for t in L.TRANSITIONS}
    assert sorted(set(driven) - table) == [], "the model names transitions the table lacks"
    for t in L.EXEMPT:                      # a reason instead of a step, and no step after all
        assert t.name not in table and t.name not in driven, t.name
        assert isinstance(t.pairs, str) and len(t.pairs) > 20, t.name
    for t in L.TRANSITIONS:
        assert driven.get(t.name), f"no step of any sequence drives {t.name}"
        assert t.pairs, t.name
        for name, i in t.pairs:
            cp, steps = L.MODEL_SEQUENCES[name]
            assert cp.lib == t.file and 0 <= i < len(steps), (t.name, name, i)
            assert L.drives(t.name, name, i), (t.name, name, i, driven[t.name])


def test_the_four_files_have_the_same_common_transitions():
    per = {lib: {t.name[len(lib) + 1:] for t in L.TRANSITIONS if t.file == lib} for lib in L.FILES}
    for lib, names in per.items():
        assert sorted(set(L.COMMON) - names) == [], lib
    shared = set.intersection(*per.values())
    assert shared >= set(L.COMMON)
    # and the same failure paths are set aside in each
    ex = {lib: {t.name[len(lib) + 1:] for t in L.EXEMPT if t.file == lib} for lib in L.FILES}
    for lib, names in ex.items():
        assert names >= {"ensure_fails", "launch_fails", "record_fails"}, lib
    # the range-check text of each file is what the GPU test expects of last_error
    for (lib, _), text in L.ERANGE_TEXT.items():
        assert f'"{text}"' in "\n".join(_lines(lib)), (lib, text)


def test_predicates_depend_on_the_state_before():
    cp, steps = L.SEQUENCES["R"]
    fresh = L.new_state(cp)
    assert L.drives("rnsmp.wait_other_stream", "R", 2)
    assert "rnsmp.wait_other_stream" not in L.walk(cp, fresh, steps[2]).tags
    assert "rnsmp.first_use" in L.walk(cp, fresh, steps[2]).tags
    assert "rnsmp.alloc_unused" in L.walk(cp, fresh, steps[4]).tags
    assert L.drives("rnsmp.grow_after_use", "R", 4)


def _scr(name, i=-1, entry=0):
    return L.model(name)[i].state["dev"][entry]


def test_every_sequence_ends_in_the_state_its_last_step_implies():
    for name, (cp, steps) in L.MODEL_SEQUENCES.items():
        trace = L.model(name)
        assert len(trace) == len(steps)
        for e in range(cp.ndev):
            users = [(s, w) for s, w in zip(steps, trace) if w.entry == e and w.subs
                     and not (cp.lib == "ksntt" and s.entry == "mac")]
            sc = trace[-1].state["dev"][e]
            if not users:
                assert sc == L.new_state(cp)["dev"][e], (name, e)
                continue
            last, w = users[-1]
            assert sc["used"] and sc["ev"], name
            assert sc["last"] == (f"own{e}" if last.place == "host" else last.place), name
            # each buffer holds the largest sub-batch any call asked of it
            want = [0, 0, 0]
            for s, w in users:
                for i, need in L.needs(cp, s, w.subs[0]):
                    want[i] = max(want[i], need)
            assert sc["bytes"] == want, name
            assert all(b <= max(cp.scratch_mb, 512 * (not cp.scratch_mb)) << 20 for b in want), name
        assert trace[-1].state["failed"] == (steps[-1].status == "ERANGE"), name
        for s, w in zip(steps, trace):
            assert w.validated == cp.validate and sum(w.subs) in (0, s.batch, s.batch * max(1, s.rots))
            assert (w.subs == []) == (s.status == "ERANGE"), name


def test_the_sequences_hold_what_the_plan_asks_for():
    for bits, name in ((32, "R"), (64, "R_u64")):
        cp, steps = L.SEQUENCES[name]
        poly = 3 * 8192 * bits // 8
        r = L.model(name)
        assert (cp.n, cp.bits, cp.scratch_mb) == (8192, bits, 1)
        assert [s.entry for s in steps] == ["forward", "multiply", "mac", "macn", "hoist", "multiply",
                                            "multiply", "inverse_inplace", "forward"]
        assert [s.place for s in steps] == ["A", "A", "B", "B", "A", "null", "host", "A", "B"]
        assert r[0].state["dev"][0]["bytes"] == [poly, 0, 0]                # buf[0] alone
        assert r[1].state["dev"][0]["bytes"] == [3 * poly] * 3
        assert len(r[5].subs) == 3 and r[5].subs[2] < r[5].subs[0] == r[5].subs[1]
        assert (steps[2].terms, steps[3].comps, steps[4].rots) == (3, 2, 3)
        assert r[3].state["dev"][0]["bytes"][2] == r[3].subs[0] * 2 * poly  # chunk * cpoly
        assert "rnsmp.no_growth" in r[8].tags and "rnsmp.grow_after_use" not in r[8].tags
    r = L.model("R")
    assert r[2].state["dev"][0]["bytes"][0] == 2 * 3 * 3 * 8192 * 4         # chunk * apoly
    # R_overlap: every call at least sixteen sub-batches, three rounds over three streams
    cp, steps = L.SEQUENCES["R_overlap"]
    assert [(s.entry, s.place) for s in steps] == \
        [("multiply", "A"), ("forward", "B"), ("macn", "null")] * L.OVERLAP_ROUNDS
    assert L.OVERLAP_SUBS == 16 and all(len(w.subs) >= 16 for w in L.model("R_overlap"))
    assert all("rnsmp.wait_other_stream" in w.tags for w in L.model("R_overlap")[1:])
    # M, X: one buffer at n = 256, three at n = 8192; 35 is four sub-batches there
    for name, small in (("M", "M_256"), ("X", "X_256")):
        assert [s.batch for s in L.SEQUENCES[name][1]] == [1, 35, 35, 2, 3, 35]
        assert [s.place for s in L.SEQUENCES[name][1]] == ["A", "B" if name == "X" else "A",
                                                          "A" if name == "X" else "B", "host",
                                                          "null", "A"]
        assert all(b > 0 for b in _scr(name)["bytes"]) and _scr(small)["bytes"][1:] == [0, 0]
        assert L.model(name)[1].subs == [10, 10, 10, 5] and L.model(small)[1].subs == [35]
    assert [s.entry for s in L.SEQUENCES["X"][1]] == ["extend", "moddown"] * 3
    assert L.SEQUENCES["X"][0].shape == (3, 2, 65537)
    # K: level 3 of the five-limb chain; two buffers above n = 4096; the macs never touch them
    cp, steps = L.SEQUENCES["K"]
    assert cp.shape == (3, 2, 2) and steps[3].view == (5, 3) and steps[5].place == "null"
    assert [s.entry for s in steps] == ["modup", "mac", "modup", "mac", "modup", "modup", "mac"]
    assert _scr("K")["bytes"][2] == 0 and _scr("K")["bytes"][1] > 0 and _scr("K_256")["bytes"][1] == 0
    assert len(L.model("K")[5].subs) == 3
    for i in (1, 3, 6):
        assert L.model("K")[i].state["dev"] == L.model("K")[i - 1].state["dev"]
    # the range failures: a clean call, the failure, a host form, a device form on the other stream
    for name in ("R_erange", "M_erange", "K_erange", "X_erange"):
        cp, steps = L.SEQUENCES[name]
        assert cp.validate and cp.n == (8192 if name[0] == "R" else 256)
        assert [s.status for s in steps[:4]] == ["OK", "ERANGE", "OK", "OK"]
        assert steps[2].place == "host" and steps[3].place == "B" and steps[0].place == "A"
    # G: two entries; on one GPU both calls and host forms use entry 0, G_dev1 reaches entry 1
    cp, steps = L.SEQ_G
    assert (cp.ndev, cp.share_devices) == (2, True)
    assert _scr("G", entry=1) == L.new_state(cp)["dev"][1]
    assert {w.entry for w in L.model("G_dev1")} == {0, 1} and _scr("G_dev1", entry=1)["used"]
    assert [w.entry for w in L.model("G")] == [0] * 4 == [w.entry for w in L.model("G", devices=2)]
    with pytest.raises(AssertionError, match="NTTMUL_ENODEV"):
        L.model("G_dev1", devices=1)
    # CHAIN and the thread pairs
    assert (L.CHAIN_N, L.CHAIN_BATCHES) == (256, (1, 5, 2))
    assert L.moduli_of(L.CHAIN_CTX["ks"]) == L.moduli_of(L.CHAIN_CTX["md"])
    assert L.THREAD_PAIRS == (("R", "X"), ("M", "K"))
    assert all(p in L.SEQUENCES for pair in L.THREAD_PAIRS for p in pair)


def _xconv_runs():
    """(sequence, salt) of every run of an xconv sequence the GPU test makes."""
    out = [(name, L.SALT) for name, (cp, _) in L.SEQUENCES.items() if cp.lib == "xconv"]
    for pair in L.THREAD_PAIRS:
        out += [(name, salt) for name, salt in zip(pair, L.THREAD_SALTS)
                if L.SEQUENCES[name][0].lib == "xconv"]
    return out


@pytest.mark.parametrize("name,salt", _xconv_runs())
def test_no_xconv_input_has_a_coefficient_inside_the_band(name, salt):
    """What tests/test_xconv_ref.py asks of xconv_cases.seeded_gpu_inputs(), of the inputs of
    limb_lifetime_cases.inputs(): zero in-band coefficients."""
    cp, steps = L.SEQUENCES[name]
    for i, step in enumerate(steps):
        assert L.band_count(cp, step, L.inputs(name, i, salt)) == 0, (name, i, salt)
    assert ("X", L.THREAD_SALTS[1]) in _xconv_runs() and len(_xconv_runs()) == 4


def test_inputs_are_distinct_canonical_and_reproducible():
    import numpy as np
    seeds = [L._seed(name, i, salt) for salt in (L.SALT,) + L.THREAD_SALTS
             for name, (_, steps) in L.MODEL_SEQUENCES.items() for i in range(len(steps))]
    assert len(seeds) == len(set(seeds))
    for name in ("M_erange", "K_erange", "CHAIN_ks"):
        cp, steps = L.MODEL_SEQUENCES[name]
        for i, step in enumerate(steps):
            ins = L.inputs(name, i)
            again = L.inputs(name, i)
            for k, (shape, m) in L.shapes(cp, step)[0].items():
                assert ins[k].shape == shape and np.array_equal(ins[k], again[k])
                over = [int((ins[k][..., l, :] >= q).sum()) for l, q in enumerate(m)]
                assert sum(over) == (1 if step.status == "ERANGE" and k == "a" else 0), (name, i, k)


def test_the_cpu_references_agree_with_the_references_they_batch():
    """forward, inverse and products of limb_lifetime_cases run the oracle over whole batches:
    held to hoist_ref's one-polynomial forms, and the mac to ksntt_ref through a gathered key."""
    import numpy as np
    import hoist_ref as H
    cp, steps = L.SEQUENCES["R_erange"]
    m = L.moduli_of(cp)
    ins = L.draw(cp, steps[0], 7)
    assert np.array_equal(L.forward(ins["a"], m), H.forward(ins["a"], m))
    back = L.inverse(ins["a"], m)
    assert np.array_equal(back[1, 2], H.inverse_one(ins["a"][1, 2].astype(np.uint64), cp.n, m[2]))
    assert np.array_equal(L.inverse(L.forward(ins["a"], m), m), ins["a"])
    prod = L.expected(cp, steps[0], ins)
    P = H.plan(cp.n, m[1])
    assert np.array_equal(prod[1, 1], P.product_merged(ins["a"][1, 1], ins["b"][1, 1]))
    # macn: component i is the mac against b[i]
    step = L.S("macn", "A", 2, terms=2, comps=2)
    ins = L.draw(cp, step, 8)
    c = L.expected(cp, step, ins)
    for i in range(2):
        one = L.expected(cp, L.S("mac", "A", 2, terms=2),
                         {"a": ins["a"], "b": np.broadcast_to(ins["b"][i], ins["a"].shape)})
        assert np.array_equal(c[:, i], one)
