"""The scale cases (tests/scale_cases.py) against their rule, without a GPU.

* Every row meets the rule: each launch holds at least 2 * 8192 waves and ends in a partial last
  workgroup where the kernel can have one; a sub-batched row meets it in every sub-batch but the
  ragged last.  All of it is computed from the case modules' own mirrors.
* Every kernel the nine libraries' ledgers name is launched by a scale case or excused by a
  SCALE_EXEMPT rule with its reason; no rule is idle and none excuses a covered kernel.
* The rows are rows of their module's all_cases(), so the kernel ledgers see them.
* The sample rule of tests/test_gpu_scale.py selects what it claims, and its checker reports a
  single wrong word at each place the rule names.
"""
import re

import numpy as np
import pytest

import dispatch_cases as D
import scale_cases as S

FAMILIES = tuple(S.FAMILIES)


def _ledger_keys():
    """Every kernel_key the mirrors name over their modules' case tables."""
    out = {}
    for family, (mod, _) in S.FAMILIES.items():
        for case in mod.all_cases():
            for key in mod.kernels_of(case):
                out.setdefault(key, family)
    return out


def _covered():
    return {l.key for s in S.scale_cases() for l in S.launches(s)}


def test_the_bound_is_the_hardware_limit():
    assert (S.WAVE, S.CU_WAVES, D.MI355X_CUS) == (64, 32, 256)
    assert S.RESIDENT_WAVES == 8192 and S.MIN_WAVES == 16384


@pytest.mark.parametrize("family", FAMILIES)
def test_every_scale_case_meets_the_rule(family):
    rows = S.rows_of(family)
    assert rows
    for s in rows:
        assert S.violations(s) == [], s
        ls = S.launches(s)
        held = ls[:len(ls) - S.last_sub_batch_launches(s)]
        # the rule once more, from the launch geometry alone
        for l in held:
            blocks = -(-l.units // l.per) * l.bpu * l.rows
            assert blocks * l.threads >= 2 * 256 * 32 * 64, (s, l)
            assert l.threads % 64 == 0 and l.threads <= 1024
            if l.per > 1 and l.upp % l.per and not S.always_whole(l.key):
                assert l.units % l.per, (s, l)
        # the smallest such batch: one polynomial fewer breaks the rule
        if not s.sub and S.batch_of(s) > 1:
            fewer = s._replace(case=s.case._replace(batch=S.batch_of(s) - 1))
            assert S.violations(fewer) or any(
                S.violations(o._replace(case=o.case._replace(batch=S.batch_of(s) - 1)))
                for o in rows if o.family == "plain" and o.case.n == s.case.n
                and o.case.q == s.case.q and not o.sub), s


def test_the_issues_worked_example():
    """k_rns_xform<Arith32P,u32,12,0> with L = 3 takes two polynomials per workgroup: 4097
    workgroups need 1366 per limb, and batch 2731 leaves a partial last one on every limb."""
    s, = [s for s in S.rows_of("rns")
          if s.case.op == "forward" and s.case.n == 4096 and s.case.moduli == S.R.BASIS32]
    l, = S.launches(s)
    assert (l.key, l.per, l.rows, l.threads) == ("k_rns_xform<Arith32P,u32,12,0>", 2, 3, 256)
    assert s.case.batch == 2731 and S.blocks_x(l) == 1366 and S.waves(l) == 1366 * 3 * 4


def test_block_threads_restates_the_launches():
    assert S.block_threads("k_rows<Arith32P,u32,u32,10,0,false>", 1024) == 64
    assert S.block_threads("k_rows<Arith32P,u32,u32,12,1,false>", 8192) == 256
    assert S.block_threads("k_rns_rows<Arith64,u64,10>", 1024) == 64
    assert S.block_threads("k_rns_rows<Arith32P3,u32,12>", 4096) == 256
    assert S.block_threads("k_xform<Arith32P,u32,u32,10,0,0>", 1024) == 256
    # min(1024, max(n / M, 1024) / 4)
    assert S.block_threads("k_galois_coeff<u32,0>", 256) == 256
    assert S.block_threads("k_galois_coeff<u32,0>", 4096) == 1024
    assert S.block_threads("k_galois_coeff<u64,2>", 65536) == 1024


def test_the_plain_sub_batch_rule():
    """dispatch_cases.chunks on the shapes whose sub-batches the tables already state
    (FP_SUBBATCH: 32 + 32 + 1 and 2 + 2 + 1 polynomials with scratch_mb = 1)."""
    for (n, q, w, batch), want in zip(D.FP_SUBBATCH, ([32, 32, 1], [2, 2, 1])):
        assert D.chunks(D.Case("multiply", n, q, w, batch), 1) == want
        assert D.chunks(D.Case("transform", n, q, w, batch, mode=1), 1) == want
        assert D.chunks(D.Case("pointwise", n, q, w, batch), 1) == [batch]
        assert D.chunks(D.Case("multiply", n, q, w, batch)) == [batch]
    # a fused transform goes through the scratch only when it is reordered, in caller words
    assert D.chunks(D.Case("transform", 4096, D.Q31, 32, 129, mode=0), 1) == [129]
    assert D.chunks(D.Case("transform", 4096, D.Q31, 32, 129, mode=2), 1) == [64, 64, 1]
    assert D.chunks(D.Case("transform", 4096, D.Q31, 64, 129, mode=2), 1) == [32] * 4 + [1]
    assert D.chunks(D.Case("multiply", 4096, D.Q31, 32, 129), 1) == [129]


def test_sub_batched_rows():
    rows = [s for s in S.scale_cases() if s.sub]
    assert sorted(s.family for s in rows) == ["hoist", "macn", "plain", "rnsmp"]
    for s in rows:
        subs = S.sub_batches(s)
        assert len(subs) == 3 and subs[0] == subs[1] > subs[2] >= 1, s
        assert s.case.n > 4096
        if s.family != "plain":
            assert s.case.scratch_mb == s.sub
        # one MiB less and a whole sub-batch falls below the rule
        less = s._replace(sub=s.sub - 1) if s.family == "plain" else \
            s._replace(sub=s.sub - 1, case=s.case._replace(scratch_mb=s.sub - 1))
        assert any("waves" in v for v in S.violations(less)), s


def test_the_rows_are_rows_of_their_modules_tables():
    for family, (mod, _) in S.FAMILIES.items():
        have = set(mod.all_cases())
        for s in S.rows_of(family):
            assert s.case in have, s


def test_the_tables_cover_what_the_issue_names():
    rows = S.scale_cases()

    def at(family, **kw):
        return [s for s in rows if s.family == family
                and all(getattr(s.case, k) == v for k, v in kw.items())]

    for q, w in ((D.Q31, 32), (D.Q62, 64)):
        for n in (256, 1024, 4096, 8192, 65536):
            assert at("plain", op="multiply", n=n, q=q, word_bits=w)
            assert at("plain", op="pointwise", n=n, q=q, word_bits=w)
            for mode in (0, 3):
                assert {s.alias for s in at("plain", op="transform", n=n, q=q, word_bits=w,
                                            mode=mode)} == {"", "out=in"}
        for n in (4096, 8192):
            assert at("plain", op="transform", n=n, q=q, mode=2)
    assert "k_cols8<Arith64,u64,u64,0,2>" in _covered()          # Q62 at n = 65536: the square split
    for n in (256, 4096):
        for w in (32, 64):
            assert {s.case.shared for s in at("mac", n=n, word_bits=w, terms=3)} == {False, True}
    for family, mod, ns in (("rns", S.R, (256, 4096)), ("rnsmp", S.M, (8192, 65536))):
        for n in ns:
            for basis in mod.BASES:
                assert len(basis) == 3
                assert {s.case.op for s in at(family, n=n, moduli=basis)} == set(mod.OPS)
                assert at(family, n=n, moduli=basis, op="mac", terms=3)
    for n in (256, 4096, 8192, 65536):
        for basis in S.N.cases_of(n).BASES:
            assert at("macn", n=n, moduli=basis, comps=2, terms=3)
            h = at("hoist", n=n, moduli=basis, comps=2, terms=3)
            assert h and all(len(s.case.ks) == 3 and len(set(s.case.ks)) == 3 and 1 not in s.case.ks
                             for s in h)
    for bits in (32, 64):
        for n in (256, 4096):
            assert {s.case.op for s in at("bconv", bits=bits, n=n, L=4, K=5)} == {"convert", "moddown"}
        assert S.B.CADENCE[bits] < 4 or bits == 64          # L = 4 crosses the fold cadence
        assert 5 % S.B.TILE != 0                              # K = 5 leaves a padded tile
        for n in (256, 65536):
            assert {s.case.op for s in at("ks", bits=bits, n=n, L=4, K=2, alpha=2)} == \
                {"modup", "moddown"}
    for basis in S.G.BASES:
        assert at("galois", op="coeff", n=65536, moduli=basis)
        assert at("galois", op="ntt", moduli=basis)
        assert all(len(s.case.ks) == 4 for s in at("galois", op="ntt_many", moduli=basis))
    # coeff staged in two and in four residue classes
    assert {"k_galois_coeff<u32,1>", "k_galois_coeff<u64,1>", "k_galois_coeff<u64,2>"} <= _covered()


def test_every_kernel_is_covered_or_exempt():
    keys, covered = _ledger_keys(), _covered()
    assert len(keys) > 300
    assert sorted(covered - set(keys)) == []
    missing = sorted(k for k in keys if k not in covered and not S.exempt_reason(k))
    assert not missing, f"kernels no scale case launches and no rule excuses: {missing}"
    both = sorted(k for k in covered if S.exempt_reason(k))
    assert not both, f"rules that excuse a covered kernel: {both}"
    for pattern, reason in S.SCALE_EXEMPT:
        assert any(re.fullmatch(pattern, k) for k in keys), f"idle rule: {pattern}"
        assert len(reason) > 20 and "not yet" not in reason.lower()


def test_a_degree_rule_lies_between_covered_degrees():
    """Every kernel excused as a degree between two covered ones has a covered kernel of the same
    template on both sides."""
    covered = _covered()

    def degree(key):
        name, args = re.fullmatch(r"(\w+)<(.*)>", key).groups()
        # (at n = 4096 the fused product templates run as Arith32P3: the same template, three
        # base blocks)
        args = args.replace("Arith32P3", "Arith32P").split(",")
        if name in ("k_rows", "k_xform"):
            i = 3 if args[4] == "0" else 4
        elif name in ("k_mac",):
            i = 3
        elif name == "k_rnsmp_rows":
            i = 1
        else:
            i = 2
        return (name, tuple(args[:i] + args[i + 1:])), int(args[i])

    for key in _ledger_keys():
        if (S.exempt_reason(key) or "").startswith("a degree strictly between"):
            template, d = degree(key)
            others = [degree(k)[1] for k in covered
                      if re.match(r"k_(rows|xform|mac|cols_fwd|cols_inv|rns|rnsmp)", k)
                      and degree(k)[0] == template]
            assert others and min(others) < d < max(others), (key, sorted(others))


# ---------------------------------------------------------------------------------------------
# The sample rule
# ---------------------------------------------------------------------------------------------

def _row(family, kw):
    s, = [s for s in S.rows_of(family) if not s.sub and not s.alias
          and all(getattr(s.case, k) == v for k, v in kw.items())]
    return s


SAMPLED = [
    # row, the partial last workgroup's polynomials, the first workgroup of the second wave's
    (("rns", dict(op="forward", n=4096, moduli=S.R.BASIS32)), [2730], [1364, 1365]),
    # 16 polynomials per workgroup and limb, 1366 workgroups per limb: workgroup 2048 is
    # blockIdx (682, 1)
    (("rns", dict(op="multiply", n=256, moduli=S.R.BASIS64)), [21840], list(range(10912, 10928))),
    # 456 * 3 workgroups per limb, the rotation fastest: workgroup 2048 is blockIdx (680, 1),
    # rotation 680 % 3 of polynomial 680 // 3
    (("hoist", dict(n=4096, moduli=S.R.BASIS32)), [], [226]),
    # one row of 4096 per workgroup, two rows per polynomial, 1366 workgroups per limb
    (("rnsmp", dict(op="multiply", n=8192, moduli=S.M.BASIS32)), [], [341]),
]


@pytest.mark.parametrize("row,partial,second", SAMPLED)
def test_the_sample_holds_what_the_rule_names(row, partial, second):
    s = _row(*row)
    batch, ls = S.batch_of(s), S.launches(s)
    polys = S.sample(ls, batch)
    assert polys == sorted(set(polys)) and len(polys) >= 256
    assert polys[0] == 0 and polys[-1] == batch - 1
    assert set(partial) <= set(polys) and set(second) <= set(polys)
    for i in range(64):                                     # one from each 1 / 64 of the batch
        assert any(i * batch <= 64 * p < (i + 1) * batch for p in polys), i
    # the hand-computed places are what the rule's own functions give
    if partial:
        main, = [l for l in ls if l.units % l.per]
        assert list(S.block_polys(main, S.blocks_x(main) - 1)) == partial
    rowk = [l for l in ls if "cols" not in l.key][0]
    assert list(S.block_polys(rowk, S.second_wave_block(rowk))) == second


def test_a_small_batch_is_sampled_whole():
    s = _row("rnsmp", dict(op="mac", n=65536, moduli=S.M.BASIS64))
    assert S.sample(S.launches(s), S.batch_of(s)) == list(range(86))


@pytest.mark.parametrize("row,partial,second", SAMPLED[:2])
def test_the_checker_reports_one_wrong_word_at_each_named_place(row, partial, second):
    s = _row(*row)
    batch = S.batch_of(s)
    polys = S.sample(S.launches(s), batch)
    rng = np.random.default_rng(5)
    want = rng.integers(0, 1 << 31, (batch, 3, 8), dtype=np.uint64)      # a synthetic batch
    places = [0, batch - 1, partial[-1], second[0]]
    for p in places:
        got = want.copy()
        got[p, 2, 7] ^= 1                                                # one wrong word
        idx = np.array(polys)
        assert S.mismatching(got[idx], want[idx], polys) == [p]
    assert S.mismatching(want[np.array(polys)], want[np.array(polys)], polys) == []
