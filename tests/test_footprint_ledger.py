"""The footprint ledger: what tests/test_gpu_footprint.py covers, held without a GPU.

* Entry points: every function the four headers export is called by a Footprint row of
  tests/dispatch_cases.py, mac_cases.py, rns_cases.py or bconv_cases.py, or matched by an EXEMPT
  rule that says why it needs none.
* Units per block: for every kernel a footprint row launches that takes more than one unit per
  workgroup, some row launching it ends in a partial workgroup after at least one whole one
  (units % units_per_block != 0 and units > units_per_block), or the kernel is listed as never
  having one, which is then checked over every row.
* Guard widths: the guard each row's arena gets covers one whole workgroup's span of every kernel
  the row launches and one whole batch entry of its widest operand.
* The deal: test_gpu_footprint.groups() hands every row to exactly one test."""
import re

import bconv_cases as B
import dispatch_cases as D
import guarded as G
import mac_cases as M
import nttmul
import rns_cases as R
import test_gpu_footprint as T

TABLES = (D, M, R, B)

# Exported functions without a footprint row: (regular expression over the name, reason)
EXEMPT = (
    (r"ntt256_product[14]|ntt_red256_product[14]",
     "fixed int32[256] shims over nttmul_multiply_u32 (the server's host memcpy of n words), "
     "covered by the golden tests"),
    (r"i?ntt256_(ct|gs)_\w+|mulntt256_ct_\w+|inttmul256_gs_\w+",
     "fixed int32[256] in-place shims over nttmul_transform_batch_u32, covered by the golden "
     "tests"),
    (r"nttmul_(rns_|bconv_)?(create\w*|destroy|host_alloc|host_free)",
     "create and release contexts and blocks; write one handle"),
    (r"nttmul_(rns_|bconv_)?(strerror|last_error|last_host_path|server_status|get_info|limb_info"
     r"|last_kernel_name)|nttmul_(mac_|rns_|bconv_)?kernel_name(_batch)?",
     "diagnostics and queries: one small struct or a string of at most cap bytes, no launch"),
    (r"nttmul_(is_prime|find_prime|table|bconv_plan)",
     "host-only planner functions: no device, no batch (tests/test_planner_io.py, "
     "tests/test_bconv_abi.py)"),
    (r"nttmul_(print_array|read_coefficients|read_hex|write_hex)",
     "host-only text formats (tests/test_planner_io.py)"),
)


def _exported():
    return (nttmul.exported_symbols() + nttmul.mac_exported_symbols()
            + nttmul.rns_exported_symbols() + nttmul.bconv_exported_symbols())


def _rows():
    return [(mod, f) for mod in TABLES for f in mod.footprint_cases()]


def _exempt_reason(name):
    for pattern, reason in EXEMPT:
        if re.fullmatch(pattern, name):
            return reason
    return None


def test_every_exported_entry_point_has_a_row_or_an_exemption():
    exported = _exported()
    assert len(exported) == len(set(exported)) > 80
    named = {f.entry for _, f in _rows()}
    assert sorted(named - set(exported)) == [], "rows name functions no header exports"
    missing = sorted(s for s in exported if s not in named and not _exempt_reason(s))
    assert not missing, f"exported without a footprint row or an exemption: {missing}"
    both = sorted(s for s in named if _exempt_reason(s))
    assert not both, f"exempt but covered by a row: {both}"
    for pattern, reason in EXEMPT:
        assert any(re.fullmatch(pattern, s) for s in exported), f"rule matches nothing: {pattern}"
        assert reason.strip() and "\n" not in reason
    # everything that takes a batch of caller buffers is covered by rows, not by exemptions
    batchy = [s for s in exported if re.search(r"_device$|_batch_u(32|64)$|_u(32|64)$", s)
              or re.fullmatch(r"nttmul_(rns|bconv)_(multiply|forward|inverse|mac_ntt|convert|moddown)", s)]
    assert len(batchy) == 33 and set(batchy) <= named


def _always_whole(key):
    for pattern, reason in D.FP_ALWAYS_WHOLE:
        if re.fullmatch(pattern, key):
            return reason
    return None


def test_every_multi_unit_kernel_has_a_row_with_a_partial_last_workgroup():
    seen, partial = {}, set()
    for mod, f in _rows():
        for key, (upb, units, _) in mod.units_per_block(f.case).items():
            seen[key] = upb
            if _always_whole(key):
                assert units % upb == 0, (key, f)
            elif upb > 1 and units % upb != 0 and units > upb:
                partial.add(key)
    multi = {k for k, upb in seen.items() if upb > 1 and not _always_whole(k)}
    assert len(multi) > 60
    assert sorted(multi - partial) == []
    for pattern, reason in D.FP_ALWAYS_WHOLE:
        assert any(re.fullmatch(pattern, k) for k in seen), pattern
        assert reason.strip() and "\n" not in reason
    # the values the code has: 2, 4, 8, 16 and 32 units per workgroup, each with such a row
    assert {seen[k] for k in multi} == {2, 4, 8, 16, 32}


def test_units_per_block_names_the_kernels_the_rows_launch():
    """units_per_block speaks about exactly the kernels kernels_of names (the range check of the
    limb-aware libraries aside: no footprint row of theirs validates)."""
    for mod, f in _rows():
        assert set(mod.units_per_block(f.case)) == set(mod.kernels_of(f.case)), f


def test_guards_cover_a_workgroup_span_and_a_batch_entry():
    entry = {D: lambda c: c.n, M: lambda c: c.terms * c.n,
             R: lambda c: c.terms * len(c.moduli) * c.n, B: lambda c: (c.K + c.L) * c.n}
    for mod, f in _rows():
        guard = mod.fp_guard_words(f.case)
        assert guard >= G.GUARD_MIN and guard >= entry[mod](f.case), f
        for key, (upb, _, words) in mod.units_per_block(f.case).items():
            assert guard >= upb * words, (f, key)
    assert G.GUARD_MIN == 32 * 256 == 2 * 4096


def test_every_row_is_dealt_to_exactly_one_test():
    dealt = [f for params in T.groups().values() for rows in params.values() for f in rows]
    rows = [f for _, f in _rows()]
    assert len(dealt) == len(rows)
    assert sorted(map(repr, dealt)) == sorted(map(repr, rows))
    assert all(params for params in T.groups().values())


def test_the_tables_hold_what_the_plan_asks_for():
    rows = D.footprint_cases()
    dev = [f for f in rows if T._plain(f)]
    ops = {(f.entry, f.case.mode) for f in dev}
    assert {e for e, _ in ops} == {
        "nttmul_multiply_batch_device", "nttmul_forward_batch_device",
        "nttmul_inverse_batch_device", "nttmul_pointwise_batch_device",
        "nttmul_transform_device", "nttmul_fill_random_device"}
    assert {m for e, m in ops if e == "nttmul_transform_device"} == set(D.XF_MODES)
    shapes = {(f.case.n, f.case.q, f.case.word_bits, f.cyclic) for f in dev}
    assert shapes == ({(n, q, w, False) for n in D.FP_N for q in D.CLASS_MODULI
                       for w in D.word_options(q)}
                      | {(n, q, w, True) for n in D.FP_CYCLIC_N for q in D.CLASS_MODULI
                         for w in D.word_options(q)})
    assert {f.case.batch for f in dev if f.case.n <= 4096} == {1, 33}
    assert {f.case.batch for f in dev if f.case.n > 4096} == {1, 3}
    assert {f.host for f in rows if f.host} == {"staged", "direct", "zero_copy", "server"}
    assert {f.alias for f in rows} == {"", "out=in", "c=a", "c=b"}
    assert {(f.case.n, f.case.q, f.case.word_bits, f.case.batch) for f in rows if f.scratch_mb} == \
        {s[:4] for s in D.SUBBATCH if s[:4] in D.FP_SUBBATCH} == set(D.FP_SUBBATCH)
    # the staged copy that splits into unequal pieces (csrc/copy_pool.hpp CopyPool::copy)
    n, q, w, batch = D.FP_STAGED_SPLIT
    part, page = 1 << 20, 4096

    def pieces(b, threads=8):
        size = b * n * (w // 8)
        parts = min(threads, size // part)
        if parts <= 1:
            return [size]
        step = (-(-size // parts) + page - 1) // page * page
        return [min(step, size - o) for o in range(0, size, step)]
    assert len(set(pieces(batch))) > 1 and len(pieces(batch)) >= 2
    assert all(len(set(pieces(b))) == 1 for b in range(1, batch))
    assert pieces(batch) == [1056768, 1056768, 1048576]
