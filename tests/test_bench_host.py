"""Host-side logic of bench.py that the driver's numbers depend on (CPU only): Infinity-Cache
rotation, the fail-closed profile lookups keyed by code object, the code-object id of the built
library, and the workload labels."""
import json
import os
import struct

import numpy as np
import pytest

import bench
import nttmul


def test_buffer_sets():
    assert bench.buffer_sets(3 * 4096 * 4 * 65536) == 1            # C3: 3 GiB, HBM anyway
    c2 = 3 * 1024 * 4 * 4096                                        # C2: 48 MiB
    assert bench.buffer_sets(c2) == 16 and 16 * c2 >= 3 * bench.IC_BYTES
    assert bench.buffer_sets(c2, 1) == 1                            # explicit --rotate 1
    assert bench.buffer_sets(bench.IC_BYTES) == 3


def test_workload_names():
    assert bench.workload_name(4096, 2013265921, 65536, 1) == "C3"
    assert bench.workload_name(4096, 2013265921, 1 << 20, 8) == "C4"
    assert bench.workload_name(1024, 2013265921, 4096, 1) == "C2"
    assert bench.workload_name(65536, 0x3FFFFFFFFFE80001, 1024, 1) == "C5"
    assert bench.workload_name(2048, 2013265921, 10, 1) == "custom"


def _elf(sections: dict) -> bytes:
    """A minimal ELF64 image holding a .shstrtab and the given {name: bytes} sections."""
    names = b"\0.shstrtab\0" + b"".join(k.encode() + b"\0" for k in sections)
    blobs, off = [], 64 + len(names)
    for data in sections.values():
        blobs.append((off, data))
        off += len(data)
    sh_off = off + (-off) % 8
    nsec = 2 + len(sections)
    hdr = bytearray(64)
    hdr[:4] = b"\x7fELF"
    hdr[4] = 2                                   # ELFCLASS64
    hdr[5] = 1
    struct.pack_into("<Q", hdr, 0x28, sh_off)    # e_shoff
    struct.pack_into("<HHH", hdr, 0x3A, 64, nsec, 1)  # e_shentsize, e_shnum, e_shstrndx
    secs = bytearray(64 * nsec)
    struct.pack_into("<IIQQQQ", secs, 64, 1, 3, 0, 0, 64, len(names))         # .shstrtab
    name_off = 11
    for i, (k, (o, data)) in enumerate(zip(sections, blobs)):
        struct.pack_into("<IIQQQQ", secs, 64 * (2 + i), name_off, 1, 0, 0, o, len(data))
        name_off += len(k) + 1
    body = bytes(hdr) + names + b"".join(d for _, d in blobs)
    return body + b"\0" * (sh_off - len(body)) + bytes(secs)


def _elf_with_fatbin(path, payload: bytes):
    """A minimal ELF64 with a .hip_fatbin section."""
    with open(path, "wb") as f:
        f.write(_elf({".hip_fatbin": payload}))


def _bundle(entries) -> bytes:
    """A clang offload bundle of (triple, image) entries."""
    head = len(b"__CLANG_OFFLOAD_BUNDLE__") + 8 + sum(24 + len(t) for t, _ in entries)
    out, table, off = b"", b"", head
    for triple, image in entries:
        table += struct.pack("<QQQ", off, len(image), len(triple)) + triple
        off += len(image)
    out = b"__CLANG_OFFLOAD_BUNDLE__" + struct.pack("<Q", len(entries)) + table
    return out + b"".join(image for _, image in entries)


def test_code_object_id_reads_machine_code(tmp_path):
    """The id follows each amdgcn code object's .text / .rodata / .note and ignores its symbol
    tables (the compiler's __hip_cuid_* marker changes with any source edit) and host entries."""
    def lib(path, text, dynsym, host=b"host"):
        co = _elf({".note": b"meta", ".dynsym": dynsym, ".rodata": b"kd", ".text": text})
        _elf_with_fatbin(path, _bundle([(b"host-x86_64-unknown-linux-gnu-", host),
                                        (b"hipv4-amdgcn-amd-amdhsa--gfx950", co)]))
        return nttmul.code_object_id(str(path))
    base = lib(tmp_path / "a.so", b"\x01\x02", b"__hip_cuid_1111")
    assert lib(tmp_path / "b.so", b"\x01\x02", b"__hip_cuid_2222") == base   # cuid only
    assert lib(tmp_path / "c.so", b"\x01\x02", b"__hip_cuid_1111", b"h2") == base
    assert lib(tmp_path / "d.so", b"\x01\x03", b"__hip_cuid_1111") != base   # a kernel changed


def test_code_object_id(tmp_path):
    a, b = tmp_path / "a.so", tmp_path / "b.so"
    _elf_with_fatbin(a, b"kernels v1")
    _elf_with_fatbin(b, b"kernels v2")
    ia, ib = nttmul.code_object_id(str(a)), nttmul.code_object_id(str(b))
    assert len(ia) == 16 and ia != ib
    assert nttmul.code_object_id(str(a)) == ia                      # deterministic
    (tmp_path / "x.txt").write_bytes(b"not an elf")
    with pytest.raises(ValueError):
        nttmul.code_object_id(str(tmp_path / "x.txt"))
    if os.path.exists(nttmul.LIB_PATH):                              # the built library has one
        assert len(nttmul.code_object_id()) == 16


def test_profile_lookup_fails_closed(tmp_path, monkeypatch):
    """Profiles are looked up kernel by kernel: an entry matches only when every kernel the step
    dispatches has the hash the entry was measured on (no whole-code-object key)."""
    prof = tmp_path / "profiles"
    prof.mkdir()
    ka = {"k_rows<A,u32,u32,12,0,false>": "aaaa"}
    entry = {"n": 4096, "q": 2013265921, "batch": 65536, "kernels": ka,
             "hbm_bytes_per_launch": 2.0e9, "source": "x_pmc.json", "method": "m"}
    legacy = dict(entry, kernels=None, code_object="aaaa", hbm_bytes_per_launch=9.0)
    (prof / "pmc_traffic.json").write_text(json.dumps({"entries": [legacy, entry]}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    t, src = bench.load_traffic(4096, 2013265921, 32768, ka)
    assert t == 1.0e9 and "aaaa" in src                            # scaled to the batch
    t, src = bench.load_traffic(4096, 2013265921, 65536, {"k_rows<A,u32,u32,12,0,false>": "bbbb"})
    assert t is None and "bbbb" in src                             # that kernel changed
    two = dict(ka, **{"k_cols8<A,u64,u64,1,1>": "cccc"})
    assert bench.load_traffic(4096, 2013265921, 65536, two)[0] is None   # a kernel more
    assert bench.load_traffic(4096, 2013265921, 65536, None)[0] is None
    assert bench.load_valu_bound(4096, 2013265921, ka) is None      # no file: None


def test_valu_roofline_sums_the_launches():
    """valu_roofline: cycles per wave x waves per polynomial, summed over a step's launches."""
    vb = {"per_kernel": [{"kernel": "a", "valu_per_wave": 10, "cycles_per_wave": 100.0,
                          "waves_per_unit": 64},
                         {"kernel": "b", "valu_per_wave": 20, "cycles_per_wave": 300.0,
                          "waves_per_unit": 64}]}
    vr = bench.valu_roofline(vb, 1024, 1.0, {"a": "1", "b": "2"})
    cyc = (100.0 + 300.0) * 64 * 1024 / bench.SIMDS
    assert vr["cycles_per_simd"] == pytest.approx(cyc)
    assert vr["bound_ms"] == pytest.approx(cyc / 2.4e9 * 1e3) and vr["frac"] == vr["bound_ms"]
    assert [k["kernel"] for k in vr["kernels"]] == ["a", "b"] and "cycles_per_wave" not in vr
    one = bench.valu_roofline({"per_kernel": vb["per_kernel"][:1]}, 65536, 2.0, {"a": "1"})
    assert one["cycles_per_wave"] == 100.0 and one["waves_per_simd"] == 64 * 65536 / 1024


def test_power_probe_summary():
    """bench.power_probe: medians over the gfx-busy samples, the cap, the PPT-limiter count, and
    None without a reader (amdsmi replaced by a canned sampler)."""
    it = iter(range(10 ** 6))

    def read():
        i = next(it)
        return {"w": 1399 if i % 2 else 1397, "mhz": 1900 + (i % 3) * 50, "busy": 100 if i else 0,
                "ppt": True, "ppt_pct": 100}

    steps = []
    out = bench.power_probe(lambda: steps.append(1), lambda: None, 0.7, (read, 1400.0, 3),
                            units_per_step=1000)
    assert out["board_uj_per_unit"] == pytest.approx(
        out["socket_power_w_median"] / out["rate_during_probe"] * 1e6)
    assert steps and out["amd_smi_gpu"] == 3 and out["socket_power_cap_w"] == 1400.0
    assert out["busy_samples"] == out["samples"] - 1 >= 1
    assert out["socket_power_w_median"] in (1397, 1398, 1399)
    assert out["ppt_limiter_active"] == f"{out['busy_samples']}/{out['busy_samples']}"
    assert bench.power_probe(lambda: None, lambda: None, 0.01, None) is None
    assert bench.power_reader("", 0) is None or callable(bench.power_reader("", 0)[0])


def test_host_cores_rule(monkeypatch):
    """cpu_baseline's thread count: every core of the affinity mask, capped by the cgroup quota
    and OMP_NUM_THREADS (each reported beside the choice)."""
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    c = bench.host_cores()
    assert c["threads"] == min(x for x in (c["sched_getaffinity"], c["cgroup_cpu_quota"], 3) if x)
    assert c["OMP_NUM_THREADS"] == 3 and c["os_cpu_count"] >= c["sched_getaffinity"] >= 1
    monkeypatch.delenv("OMP_NUM_THREADS")
    c = bench.host_cores()
    assert c["OMP_NUM_THREADS"] is None and c["threads"] <= c["sched_getaffinity"]


def test_c1_single_product_line():
    """BASELINE configs[0] (C1): one unoptimized-CT product on one core, checked vs the oracle."""
    c1 = bench.c1_single(target_s=0.05)
    assert c1["matches_oracle"] and c1["cores"] == 1 and c1["n"] == 1024
    assert c1["q"] == 2013265921 and c1["value"] > 0
    assert c1["us_per_polymult"] == pytest.approx(1e6 / c1["value"])


def test_default_batch_per_gpu():
    """--batch-per-gpu defaults to C3's 65536 per GPU at 1, 2 and 4 ranks and to C4's
    2^20 / 8 at 8 ranks, so the driver's 8-GPU line is BASELINE configs[3] (verdict r5 item 4)."""
    assert bench.parse([]).batch_per_gpu is None
    assert bench.parse(["--batch-per-gpu", "7"]).batch_per_gpu == 7
    for world, per in ((1, 65536), (2, 65536), (4, 65536), (8, 131072)):
        assert bench.default_batch(4096, world) == per
    assert bench.workload_name(4096, 2013265921, 8 * bench.default_batch(4096, 8), 8) == "C4"
    assert bench.workload_name(4096, 2013265921, bench.default_batch(4096, 1), 1) == "C3"
    assert bench.workload_name(4096, 2013265921, 4 * bench.default_batch(4096, 4), 4) == "C3"
    assert bench.default_batch(65536, 8) == 65536     # other n: the explicit flag sets the load


def test_settle_runs_untimed_chunks_until_the_wall_time():
    """bench.settle: synchronised chunks doubling while under 10 ms, stopping once `ms` passed."""
    t = {"now": 0.0, "steps": 0, "syncs": 0}

    def step():
        t["steps"] += 1
        t["now"] += 1e-3          # each step costs 1 ms of (fake) wall time

    def sync():
        t["syncs"] += 1

    n, ms = bench.settle(step, 100.0, sync, clock=lambda: t["now"])
    assert n == t["steps"] and ms >= 100.0
    assert n < 200                # chunks stop doubling at 10 ms, so little overshoot
    assert t["syncs"] >= 5        # paced: never one unsynchronised burst
    assert bench.settle(step, 0, sync) == (0, 0.0)


def test_op_defaults_to_the_product():
    """The default step is the product (the BASELINE metric); --op forward / inverse / pointwise
    time the standalone entry points with their own unit and bytes moved."""
    assert bench.parse([]).op == "multiply"
    assert bench.OPS["multiply"] == ("polymults/s", 3)
    assert bench.OPS["forward"][1] == bench.OPS["inverse"][1] == 2   # read x, write its transform
    assert bench.OPS["pointwise"][1] == 3
    assert bench.parse(["--op", "inverse"]).op == "inverse"
    with pytest.raises(SystemExit):
        bench.parse(["--op", "square"])


def test_plain_run_is_the_default_and_full_is_an_option():
    """Without --full the legs after the timed region (power, in-kernel clock, CPU baseline) stay
    off; their own switches keep their defaults for a --full run."""
    plain = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and plain.dump_outputs == "" and plain.steps == 20
    full = bench.parse(["--full"])
    assert full.full is True and not full.no_cpu_baseline
    assert full.power_seconds > 0 and full.clock_seconds > 0 and full.cpu_seconds > 0
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_dump_rows_are_a_fixed_sample_within_the_budget():
    """--dump-outputs: every row when the output fits the budget, else a sorted sample with both
    ends that is the same on every call; the arrays stay under 64 MB at C3, C2 and C5."""
    assert np.array_equal(bench.dump_rows(5, 4096, 32), np.arange(5))
    assert np.array_equal(bench.dump_rows(4096, 1024, 32), np.arange(4096))     # C2: 32 MiB, all
    for count, n, wb in ((65536, 4096, 32), (131072, 4096, 32), (1024, 65536, 64), (3000, 4096, 64)):
        rows = bench.dump_rows(count, n, wb)
        assert np.array_equal(rows, bench.dump_rows(count, n, wb))
        assert rows[0] == 0 and rows[-1] == count - 1 and np.all(np.diff(rows) > 0)
        assert len(rows) < count
        per_row = n * 8 * (1 if wb == 32 else 2)
        assert bench.DUMP_BYTES // 2 < len(rows) * per_row <= bench.DUMP_BYTES
        assert (len(rows) * (per_row + 8)) < 64e6


# what the library dispatches for the three bench configurations (pinned on the GPU by
# tests/test_gpu_parity.py::test_dispatch_names_of_the_bench_configs)
BENCH_DISPATCH = {
    (4096, 2013265921, 65536): "k_rows<Arith32P3,u32,u32,12,0>",
    (1024, 2013265921, 4096): "k_rows<Arith32P,u32,u32,10,0,prio>",
    (65536, 0x3FFFFFFFFFE80001, 1024):
        "k_cols8<Arith64,u64,fwd> + k_rows<Arith64,u64,u64,8,8> + k_cols8<Arith64,u64,inv>",
}


def test_committed_profiles_describe_the_shipped_kernels():
    """Each committed profile entry bench.py reports for C3, C2 and C5 (PMC traffic and the VALU
    bound) was measured on exactly the kernels the in-tree libnttmul.so dispatches: every entry's
    per-kernel hash equals the in-tree kernel's (nttmul.kernel_hashes).  A device-code edit of a
    product kernel fails this until that configuration is re-profiled; edits of other kernels or
    of host code do not (verdict r5 item 1)."""
    if not os.path.exists(nttmul.LIB_PATH):
        pytest.skip("libnttmul.so not built")
    for (n, q, batch), names in BENCH_DISPATCH.items():
        kernels = nttmul.dispatched_kernel_hashes(names)
        traffic, why = bench.load_traffic(n, q, batch, kernels)
        assert traffic is not None, why
        vb = bench.load_valu_bound(n, q, kernels)
        assert vb is not None, f"no VALU bound of {kernels} at n={n}"
        assert [k["kernel"] for k in vb["per_kernel"]] == list(kernels)


def _code_object(funcs) -> bytes:
    """A minimal amdgcn-like ELF64: .text holding each (name, code) back to back, .rodata one
    64-byte descriptor <name>.kd per kernel (entry offset = distance to its code), .symtab."""
    text, rodata, syms = b"", b"", []
    strtab = b"\0"
    for name, code in funcs:
        syms.append((len(strtab), 0x12, 2, len(text), len(code)))           # FUNC in .text
        strtab += name.encode() + b"\0"
        kd = bytearray(64)
        struct.pack_into("<q", kd, 16, len(text) - len(rodata))             # moves with layout
        kd[48:52] = b"rsrc"
        syms.append((len(strtab), 0x11, 3, len(rodata), 64))                # OBJECT in .rodata
        strtab += (name + ".kd").encode() + b"\0"
        text += code
        rodata += bytes(kd)
    symtab = bytes(24) + b"".join(struct.pack("<IBBHQQ", nm, info, 0, sec, val, size)
                                  for nm, info, sec, val, size in syms)
    secs = [(".text", 1, text, 0), (".rodata", 1, rodata, 0), (".strtab", 3, strtab, 0),
            (".symtab", 2, symtab, 4)]  # section 0 null, 1 .shstrtab, 2.. these
    names = b"\0.shstrtab\0" + b"".join(k.encode() + b"\0" for k, _, _, _ in secs)
    off = 64 + len(names)
    body = bytearray(64) + names
    heads = [struct.pack("<IIQQQQIIQQ", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
             struct.pack("<IIQQQQIIQQ", 1, 3, 0, 0, 64, len(names), 0, 0, 1, 0)]
    name_off = 11
    for k, typ, data, link in secs:
        heads.append(struct.pack("<IIQQQQIIQQ", name_off, typ, 0, 0, off, len(data), link, 0, 8,
                                 24 if typ == 2 else 0))
        name_off += len(k) + 1
        body += data
        off += len(data)
    sh_off = off + (-off) % 8
    body += bytes(sh_off - len(body))
    body[:4] = b"\x7fELF"
    body[4], body[5] = 2, 1
    struct.pack_into("<Q", body, 0x28, sh_off)
    struct.pack_into("<HHH", body, 0x3A, 64, len(heads), 1)
    return bytes(body) + b"".join(heads)


def test_kernel_hashes_are_per_kernel(tmp_path):
    """nttmul.kernel_hashes: one hash per kernel over its own code and descriptor; growing another
    kernel (which moves every later kernel and its descriptor's entry offset) changes only that
    kernel's hash; the short names follow the template arguments."""
    rows = "_ZN6nttmul6k_rowsINS_9Arith32P3EjjLi12ELi0ELb0EEEvNS_7KParamsIT_EEPKT0_S7_PT1_m"
    cols = "_ZN6nttmul7k_cols8INS_7Arith64EmmLi1ELi1EEEvNS_7KParamsIT_EEPKT0_S7_PS5_S8_m"

    def lib(path, first):
        _elf_with_fatbin(path, _bundle([(b"hipv4-amdgcn-amd-amdhsa--gfx950",
                                         _code_object([(cols, first), (rows, b"\x11" * 32)]))]))
        return nttmul.kernel_hashes(str(path))
    a = lib(tmp_path / "a.so", b"\x22" * 16)
    b = lib(tmp_path / "b.so", b"\x22" * 48)                          # k_cols8 grew
    assert set(a) == {"k_rows<Arith32P3,u32,u32,12,0,false>", "k_cols8<Arith64,u64,u64,1,1>"}
    assert a["k_rows<Arith32P3,u32,u32,12,0,false>"] == b["k_rows<Arith32P3,u32,u32,12,0,false>"]
    assert a["k_cols8<Arith64,u64,u64,1,1>"] != b["k_cols8<Arith64,u64,u64,1,1>"]


def test_dispatch_names_map_to_kernels():
    """nttmul.dispatch_key fills in the template arguments the dispatch's short names omit, and
    every bench configuration's kernels exist in the built library."""
    assert nttmul.dispatch_key("k_rows<Arith32P,u32,u32,10,0,prio>") == \
        "k_rows<Arith32P,u32,u32,10,0,true>"
    assert nttmul.dispatch_key("k_rows<Arith32P3,u32,u32,12,0>") == \
        "k_rows<Arith32P3,u32,u32,12,0,false>"
    assert nttmul.dispatch_key("k_cols8<Arith64,u64,fwd>") == "k_cols8<Arith64,u64,u64,0,2>"
    assert nttmul.dispatch_key("k_cols8<Arith64,u32,inv>") == "k_cols8<Arith64,u64,u32,1,1>"
    assert nttmul.dispatch_key("k_cols_fwd<Arith32P,u32,4>") == "k_cols_fwd<Arith32P,u32,4,2>"
    assert nttmul.kernel_key("_ZN6nttmul10k_cols_fwdINS_8Arith32TILb1EEEmLi2ELi2EEEvNS_7KParams"
                             "IT_EEPKT0_S8_PNS4_4wordESA_mi") == "k_cols_fwd<Arith32T<true>,u64,2,2>"
    if not os.path.exists(nttmul.LIB_PATH):
        pytest.skip("libnttmul.so not built")
    table = nttmul.kernel_hashes()
    assert not [k for k in table if k.startswith("_Z")]              # every kernel demangled
    for names in BENCH_DISPATCH.values():
        assert len(nttmul.dispatched_kernel_hashes(names)) == len(names.split("+"))
