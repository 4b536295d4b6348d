"""The kernel ledger of lib/libnttmul_rnsmp.so, in the style of tests/test_bconv_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_rnsmp.so = libnttmul_bconv.so's kernels, bit for bit, plus the k_rnsmp_*
kernels, and every one of those is launched by a case of tests/rnsmp_cases.py (whose mirror
test_gpu_rnsmp.py anchors to nttmul_rnsmp_kernel_name on the GPU)."""
import re

import pytest

import dispatch_cases as D
import nttmul
import rnsmp_cases as R


@pytest.fixture(scope="module")
def bconv():
    return nttmul.kernel_hashes(nttmul.BCONV_LIB_PATH)


@pytest.fixture(scope="module")
def rnsmp():
    return nttmul.kernel_hashes(nttmul.RNSMP_LIB_PATH)


def _launched():
    out = {}
    for case in R.all_cases():
        for key in R.kernels_of(case):
            out.setdefault(key, case)
    return out


def _unreachable_reason(key):
    for pattern, reason in R.UNREACHABLE:
        if re.fullmatch(pattern, key):
            return reason
    return None


def test_common_kernels_are_the_bconv_librarys_bit_for_bit(bconv, rnsmp):
    assert len(bconv) > 269
    assert sorted(set(bconv) - set(rnsmp)) == []
    assert {k: rnsmp[k] for k in bconv} == bconv


def test_the_additional_kernels_are_exactly_what_the_cases_launch(bconv, rnsmp):
    extra = set(rnsmp) - set(bconv)
    launched = _launched()
    assert all(k.startswith("k_rnsmp_") for k in extra), sorted(extra)
    ours = {k for k in launched if not k.startswith("k_rns_check_range")}
    assert all(k.startswith("k_rnsmp_") and k not in bconv for k in ours), sorted(ours)
    assert all(k in bconv for k in set(launched) - ours)     # the range check is the RNS library's
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    assert R.UNREACHABLE == ()
    # per class (2) and L1 (4): two forward column passes (NPOLY 1, 2), one inverse column pass,
    # the product rows, two row transforms (DIR 0, 1) and the mac
    assert len(extra) == 2 * 4 * (2 + 1 + 1 + 2 + 1)
    assert not [k for k in extra if "Arith32W" in k or "Arith32P3" in k]
    for cls, io in (("Arith32P", "u32"), ("Arith64", "u64")):
        for l1 in (1, 2, 3, 4):
            assert {f"k_rnsmp_cols_fwd<{cls},{io},{l1},1>", f"k_rnsmp_cols_fwd<{cls},{io},{l1},2>",
                    f"k_rnsmp_cols_inv<{cls},{io},{l1}>", f"k_rnsmp_rows<{cls},{l1}>",
                    f"k_rnsmp_xform<{cls},{io},{l1},0>", f"k_rnsmp_xform<{cls},{io},{l1},1>",
                    f"k_rnsmp_mac<{cls},{io},{l1}>"} <= extra


@pytest.mark.parametrize("path", ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH"])
def test_the_older_libraries_do_not_grow(path):
    """The four older libraries keep their ABI and kernels: the new entry points and the
    k_rnsmp_* kernels are in the fifth library only."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert "nttmul_rnsmp" not in out and "k_rnsmp" not in out
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "k_rnsmp" in k]


def test_the_bases_serve_every_n():
    """Each modulus is prime with 2 * 65536 | q - 1, the bases hold at least three distinct primes
    of one word class, and the validate cases' bad value is in range for the neighbour they
    name."""
    for basis in (R.BASIS32_5, R.BASIS64):
        assert len(set(basis)) == len(basis) >= 3
        for q in basis:
            assert nttmul.is_prime(q) and (q - 1) % (1 << 17) == 0, q
    assert len(R.BASIS32) >= 3 and R.BASIS32_5[:3] == R.BASIS32 and len(R.BASIS32_5) == 5
    assert R.word_bits(R.BASIS32_5) == 32 and R.word_bits(R.BASIS64) == 64
    assert max(R.RNSMP_N) == 65536
    for n, moduli, limb, other in R.VALIDATE:
        assert moduli[limb] < moduli[other]


def test_mirror_restates_the_selection_rules():
    assert R.sequence("multiply", 8192, R.BASIS32) == [
        "k_rnsmp_cols_fwd<Arith32P,u32,1,2>", "k_rnsmp_rows<Arith32P,1>",
        "k_rnsmp_cols_inv<Arith32P,u32,1>"]
    # 64-bit words at n = 65536 take 16 x 4096 as well (no square split here)
    assert R.sequence("multiply", 65536, R.BASIS64) == [
        "k_rnsmp_cols_fwd<Arith64,u64,4,2>", "k_rnsmp_rows<Arith64,4>",
        "k_rnsmp_cols_inv<Arith64,u64,4>"]
    assert R.sequence("forward", 16384, R.BASIS32_5) == [
        "k_rnsmp_cols_fwd<Arith32P,u32,2,1>", "k_rnsmp_xform<Arith32P,u32,2,0>"]
    assert R.sequence("inverse", 32768, R.BASIS64[:1]) == [
        "k_rnsmp_xform<Arith64,u64,3,1>", "k_rnsmp_cols_inv<Arith64,u64,3>"]
    # the mac is three launches for any number of terms, shared or not
    mac = ["k_rnsmp_cols_fwd<Arith64,u64,1,1>", "k_rnsmp_mac<Arith64,u64,1>",
           "k_rnsmp_cols_inv<Arith64,u64,1>"]
    assert R.kernels_of(R.Case("mac", 8192, R.BASIS64, 3, 1)) == mac
    assert R.kernels_of(R.Case("mac", 8192, R.BASIS64, 3, 7, True)) == mac
    assert R.kernel_name("mac", 8192, R.BASIS64) == " + ".join(mac)
    assert R.kernels_of(R.Case("mac", 8192, R.BASIS64, 3, 2, True, True)) == \
        ["k_rns_check_range<u64>"] * 2 + mac
    assert R.kernels_of(R.Case("forward", 8192, R.BASIS32, 3, 1, False, True))[0] == \
        "k_rns_check_range<u32>"
    # sub-batches: the sequence once per chunk of whole polynomials
    for n, moduli, batch, want, terms, mbatch, mwant in R.SUBBATCH:
        case = R.Case("multiply", n, moduli, batch, scratch_mb=1)
        assert R.chunks(case) == list(want) and sum(want) == batch
        assert R.kernels_of(case) == R.sequence("multiply", n, moduli) * len(want)
        mcase = R.Case("mac", n, moduli, mbatch, terms, scratch_mb=1)
        assert R.chunks(mcase) == list(mwant) and sum(mwant) == mbatch
    assert R.chunks(R.Case("multiply", 8192, R.BASIS32, 23)) == [23]
    assert [x[3] for x in R.SUBBATCH] == [(10, 10, 3), (1, 1)]
    assert [x[6] for x in R.SUBBATCH] == [(3, 3, 2), (1, 1)]
    with pytest.raises(AssertionError):
        R.sequence("multiply", 8192, (D.Q31, D.Q62))           # mixed classes
    with pytest.raises(AssertionError):
        R.sequence("multiply", 8192, (D.Q31, D.Q32))           # [2^31, 2^32)
    with pytest.raises(AssertionError):
        R.sequence("multiply", 8192, (D.Q31, D.Q31))           # two equal primes
    with pytest.raises(AssertionError):
        R.sequence("mac", 4096, R.BASIS32)                     # nttmul_rns_*'s
    with pytest.raises(AssertionError):
        R.sequence("mac", 131072, R.BASIS32)
