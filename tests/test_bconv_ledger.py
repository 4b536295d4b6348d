"""The kernel ledger of lib/libnttmul_bconv.so, in the style of tests/test_rns_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_bconv.so = libnttmul_rns.so's kernels, bit for bit, plus the k_bconv
kernels, and every one of those is launched by a case of tests/bconv_cases.py (whose mirror
test_gpu_bconv.py anchors to nttmul_bconv_kernel_name on the GPU)."""
import re

import pytest

import bconv_cases as B
import nttmul


@pytest.fixture(scope="module")
def rns():
    return nttmul.kernel_hashes(nttmul.RNS_LIB_PATH)


@pytest.fixture(scope="module")
def bconv():
    return nttmul.kernel_hashes(nttmul.BCONV_LIB_PATH)


def _launched():
    out = {}
    for case in B.all_cases():
        for key in B.kernels_of(case):
            out.setdefault(key, case)
    return out


def _unreachable_reason(key):
    for pattern, reason in B.UNREACHABLE:
        if re.fullmatch(pattern, key):
            return reason
    return None


def test_common_kernels_are_the_rns_librarys_bit_for_bit(rns, bconv):
    assert len(rns) > 265
    assert sorted(set(rns) - set(bconv)) == []
    assert {k: bconv[k] for k in rns} == rns


def test_the_additional_kernels_are_exactly_what_the_cases_launch(rns, bconv):
    extra = set(bconv) - set(rns)
    launched = _launched()
    assert all(k.startswith("k_bconv") for k in extra), sorted(extra)
    ours = {k for k in launched if not k.startswith("k_rns_check_range")}
    assert all(k.startswith("k_bconv") and k not in rns for k in ours), sorted(ours)
    assert all(k in rns for k in set(launched) - ours)       # the range check is the RNS library's
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    for pattern, reason in B.UNREACHABLE:
        assert any(re.fullmatch(pattern, k) for k in extra), f"rule matches no kernel: {pattern}"
        assert reason.strip() and "\n" not in reason
    # per word size (2): convert and moddown, for every n, L and K
    assert extra == {"k_bconv<u32,0>", "k_bconv<u32,1>", "k_bconv<u64,0>", "k_bconv<u64,1>"}


def test_mirror_restates_the_selection_rules():
    assert B.bconv_kernel("convert", 4096, 32) == "k_bconv<u32,0>"
    assert B.bconv_kernel("moddown", 256, 64) == "k_bconv<u64,1>"
    assert B.kernels_of(B.Case("moddown", 64, 256, 2, 2, 2, True)) == \
        ["k_rns_check_range<u64>", "k_bconv<u64,1>"]
    f, t = B.bases(32, 3, 2)
    assert B.word_bits(f, t) == 32 and B.word_bits(*B.bases(64, 1, 1)) == 64
    with pytest.raises(AssertionError):
        B.word_bits(f, B.bases(64, 1, 1)[0])                  # mixed classes
    with pytest.raises(AssertionError):
        B.word_bits(f, f[:1])                                 # a prime in both bases
    with pytest.raises(AssertionError):
        B.bconv_kernel("convert", 8192, 32)


def test_the_case_bases_are_what_create_accepts():
    """bases(): disjoint primes of one class with 2 * 4096 | q - 1, so each serves every n; the
    tile and the cadences the cases are built around are the sources' own."""
    for bits in (32, 64):
        f, t = B.bases(bits, 64, 7)
        assert len(set(f + t)) == 71 and B.word_bits(f, t) == bits
        assert all(nttmul.is_prime(q) and (q - 1) % (2 * 4096) == 0 for q in f + t)
        assert nttmul.bconv_plan(4096, f[:3], t[:2])
    import os
    csrc = os.path.join(nttmul.PKG_DIR, "csrc")
    assert f"kBconvTile = {B.TILE};" in open(os.path.join(csrc, "bconv.hpp")).read()
    dev = open(os.path.join(csrc, "bconv_dev.hpp")).read()
    assert re.findall(r"kCadence = (\d+);", dev) == [str(B.CADENCE[32]), str(B.CADENCE[64])]
    assert B.TILE - 1 in [K for _, K in B.SHAPES] and B.TILE + 1 in [K for _, K in B.SHAPES]
    for bits, cad in B.CADENCE.items():
        assert {cad - 1, cad, cad + 1} <= set(B.CADENCE_L[bits])
