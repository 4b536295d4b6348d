"""Python host mirror of the nttmul C ABI (include/nttmul.h), over ctypes.

This is the reference-side binding a Python caller uses: it exposes the reference's product entry
points with their names and argument meaning (ntt256_product1/4, ntt_red256_product1/4:
NTT/ntt256.h:85-86, NTT-RED/ntt_red256.h:87,90 — output array c, inputs a, b, n = 256,
q = 12289) plus the generic batched API multiply(a, b) for any (n, q).  All compute runs in
lib/libnttmul.so on the GPU; there is no CPU fallback: if the library or a GPU is missing the calls
raise.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul.so")
# the diagnostic build (include/nttmul_diag.h): same kernels plus in-kernel clock stamps
DIAG_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_diag.so")
# products against NTT-domain operands (include/nttmul_mac.h): the same ABI and kernels plus k_mac
MAC_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_mac.so")
HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul.h")
MAC_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_mac.h")

NTTMUL_OK = 0
NTTMUL_EINVAL = -1
NTTMUL_ENODEV = -2
NTTMUL_EHIP = -3
NTTMUL_ENOMEM = -4
NTTMUL_ERANGE = -5
NTTMUL_EUNSUPPORTED = -6
NTTMUL_FLAG_VALIDATE = 1
NTTMUL_FLAG_CYCLIC = 2
NTTMUL_FLAG_SHARE_DEVICES = 4
# transform modes (include/nttmul.h nttmul_transform_*)
XF_FORWARD = 0
XF_INVERSE = 1
XF_STD2REV = 0
XF_REV2STD = 2
XF_UNSCALED = 4
# the reference's n = 256 wrapper set (NTT/ntt256.h:20-69), exported under the same names
NTT256_WRAPPERS = [
    "ntt256_ct_rev2std", "ntt256_gs_rev2std", "ntt256_ct_std2rev", "ntt256_gs_std2rev",
    "intt256_ct_rev2std", "intt256_gs_rev2std", "intt256_ct_std2rev", "intt256_gs_std2rev",
    "mulntt256_ct_rev2std", "mulntt256_ct_std2rev", "inttmul256_gs_rev2std", "inttmul256_gs_std2rev",
]
TABLES = [  # nttmul_table `which` order = the tables of NTT/ntt.h:63-183 (ntt256_tables.h:29-43)
    "psi_powers", "inv_psi_powers", "inv_psi_powers_rev", "scaled_inv_psi_powers",
    "omega_powers", "omega_powers_rev", "inv_omega_powers", "inv_omega_powers_rev",
    "mixed_powers", "mixed_powers_rev", "inv_mixed_powers", "inv_mixed_powers_rev",
]

SEED = 0x4E54544D554C  # "NTTMUL", SURVEY §8d


class NttmulError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"nttmul status {status}: {msg}")
        self.status = status


class _Params(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("q", ctypes.c_uint64), ("psi", ctypes.c_uint64),
                ("ndev", ctypes.c_int), ("first_dev", ctypes.c_int), ("flags", ctypes.c_uint32),
                ("issue_prio", ctypes.c_int32), ("zero_copy_kb", ctypes.c_int32),
                ("copy_threads", ctypes.c_int32), ("scratch_mb", ctypes.c_uint32),
                ("small_server", ctypes.c_int32)]


class Info(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q", ctypes.c_uint64),
                ("psi", ctypes.c_uint64), ("omega", ctypes.c_uint64),
                ("inv_psi", ctypes.c_uint64), ("inv_omega", ctypes.c_uint64),
                ("inv_n", ctypes.c_uint64), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int), ("kernel", ctypes.c_int), ("cyclic", ctypes.c_uint32)]


# include/nttmul_diag.h: the device server's failure points (nttmul_diag_server_failpoint sites)
DIAG_SITES = ("BOX_ALLOC", "BOX_MAP", "STREAM", "REQ_ALLOC", "REQ_MAP", "LAUNCH", "STALL_BEFORE_GO")
# hipError_t values an armed site returns: the one fail() maps to NTTMUL_ENOMEM, and another
HIP_ERROR_OUT_OF_MEMORY = 2
HIP_ERROR_INVALID_VALUE = 1


class DiagServerState(ctypes.Structure):
    """include/nttmul_diag.h nttmul_diag_server_state_t."""
    _fields_ = [("go", ctypes.c_uint32), ("done", ctypes.c_uint32), ("served", ctypes.c_uint32),
                ("seq", ctypes.c_uint32), ("running", ctypes.c_int32), ("cooldown", ctypes.c_uint32),
                ("failures", ctypes.c_uint32), ("small_server", ctypes.c_int32),
                ("box_pair", ctypes.c_int32), ("req_pair", ctypes.c_int32),
                ("req_in_vram", ctypes.c_int32), ("launches", ctypes.c_uint32),
                ("spin_relaunches", ctypes.c_uint32), ("stops", ctypes.c_uint32)]


_LIB: Optional[ctypes.CDLL] = None
_DIAG_LIB: Optional[ctypes.CDLL] = None


def load_library() -> ctypes.CDLL:
    """Load lib/libnttmul.so (built by `make -C ntt-based-polynomial-multiplier-fpga_amd`)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run __graft_entry__.build() or make -C {PKG_DIR}")
    _LIB = _bind(ctypes.CDLL(LIB_PATH))
    return _LIB


def load_diag_library() -> ctypes.CDLL:
    """Load lib/libnttmul_diag.so (include/nttmul_diag.h): the same ABI, kernels with in-kernel
    clock stamps; used by bench.py for the clock the product kernel holds, never for results.
    It also holds the device server's failure points and state read-out (diag_server_failpoint,
    diag_server_state), for the tests of the server's failure and retry paths."""
    global _DIAG_LIB
    if _DIAG_LIB is not None:
        return _DIAG_LIB
    if not os.path.exists(DIAG_LIB_PATH):
        raise ImportError(f"{DIAG_LIB_PATH} not built")
    lib = _bind(ctypes.CDLL(DIAG_LIB_PATH))
    lib.nttmul_diag_clock_stamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.nttmul_diag_server_failpoint.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_uint]
    lib.nttmul_diag_server_state.argtypes = [ctypes.c_void_p, ctypes.POINTER(DiagServerState)]
    _DIAG_LIB = lib
    return lib


def _bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    vp, sz, u64, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.nttmul_create.argtypes = [ctypes.POINTER(vp), u32, u64, i32]
    lib.nttmul_create_ex.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(_Params)]
    lib.nttmul_create_sized.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(_Params), sz]
    lib.nttmul_destroy.argtypes = [vp]
    lib.nttmul_destroy.restype = None
    lib.nttmul_strerror.argtypes = [i32]
    lib.nttmul_strerror.restype = ctypes.c_char_p
    lib.nttmul_last_error.argtypes = [vp]
    lib.nttmul_last_error.restype = ctypes.c_char_p
    lib.nttmul_get_info.argtypes = [vp, ctypes.POINTER(Info)]
    lib.nttmul_kernel_name.argtypes = [vp, i32, ctypes.c_char_p, sz]
    lib.nttmul_kernel_name_batch.argtypes = [vp, i32, sz, ctypes.c_char_p, sz]
    lib.nttmul_last_kernel_name.argtypes = [vp, ctypes.c_char_p, sz]
    lib.nttmul_last_host_path.argtypes = [vp]
    if hasattr(lib, "nttmul_server_status"):  # (round 6; tools/bench_ab.py loads older builds)
        lib.nttmul_server_status.argtypes = [vp, ctypes.c_char_p, sz]
    for name in ("nttmul_multiply_u32", "nttmul_multiply_u64"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp]
    for name in ("nttmul_multiply_batch_u32", "nttmul_multiply_batch_u64"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, sz]
    lib.nttmul_multiply_batch_device.argtypes = [vp, vp, vp, vp, sz, i32, i32, vp]
    for op in ("forward", "inverse"):
        for w in ("u32", "u64"):
            getattr(lib, f"nttmul_{op}_batch_{w}").argtypes = [vp, vp, vp, sz]
        getattr(lib, f"nttmul_{op}_batch_device").argtypes = [vp, vp, vp, sz, i32, i32, vp]
    for w in ("u32", "u64"):
        getattr(lib, f"nttmul_pointwise_batch_{w}").argtypes = [vp, vp, vp, vp, sz]
    lib.nttmul_pointwise_batch_device.argtypes = [vp, vp, vp, vp, sz, i32, i32, vp]
    lib.nttmul_fill_random_device.argtypes = [vp, vp, vp, u64, sz, u64, i32, i32, vp]
    lib.nttmul_is_prime.argtypes = [u64]
    lib.nttmul_smallest_psi.argtypes = [u32, u64]
    lib.nttmul_smallest_psi.restype = u64
    lib.nttmul_smallest_omega.argtypes = [u32, u64]
    lib.nttmul_smallest_omega.restype = u64
    lib.nttmul_find_prime.argtypes = [u32, i32, i32, ctypes.POINTER(u64)]
    lib.nttmul_table.argtypes = [u32, u64, u64, i32, vp]
    lib.nttmul_fpga_R.argtypes = [u32, i32]
    lib.nttmul_fpga_R.restype = u64
    lib.nttmul_fpga_twiddles.argtypes = [u32, u64, u64, u64, u32, vp, sz]
    lib.nttmul_fpga_twiddles.restype = sz
    lib.nttmul_read_coefficients.argtypes = [ctypes.c_char_p, vp, i32]
    lib.nttmul_read_hex.argtypes = [ctypes.c_char_p, vp, i32]
    lib.nttmul_write_hex.argtypes = [ctypes.c_char_p, vp, i32]
    lib.nttmul_print_array.argtypes = [vp, vp, i32]
    for name in ("ntt256_product1", "ntt256_product4", "ntt_red256_product1", "ntt_red256_product4"):
        getattr(lib, name).argtypes = [vp, vp, vp]
        getattr(lib, name).restype = None
    for w in ("u32", "u64"):
        getattr(lib, f"nttmul_transform_batch_{w}").argtypes = [vp, u32, vp, vp, sz]
    lib.nttmul_transform_device.argtypes = [vp, u32, vp, vp, sz, i32, i32, vp]
    for name in NTT256_WRAPPERS:
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = None
    return lib


def _elf_sections(elf: bytes) -> dict:
    """{section name: bytes} of an ELF64 image (NOBITS sections map to b"")."""
    import struct
    if elf[:4] != b"\x7fELF" or elf[4] != 2:
        raise ValueError("not an ELF64 image")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)

    def sec(i):
        return struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
    stroff = sec(shstrndx)[4]
    out = {}
    for i in range(shnum):
        name, typ, _, _, off, size = sec(i)
        key = elf[stroff + name:elf.index(b"\0", stroff + name)].decode(errors="replace")
        out[key] = b"" if typ == 8 else elf[off:off + size]
    return out


_BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _device_code(fatbin: bytes):
    """The machine-code sections (.text, .rodata kernel descriptors, .note kernel metadata) of
    every amdgcn code object in a .hip_fatbin section, concatenated in bundle order; or None
    when the section holds no parsable offload bundle."""
    import struct
    parts, pos = [], fatbin.find(_BUNDLE_MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fatbin, pos + 24)
        cur = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, cur)
            triple = fatbin[cur + 24:cur + 24 + tlen]
            cur += 24 + tlen
            if b"amdgcn" in triple and size:
                secs = _elf_sections(fatbin[pos + off:pos + off + size])
                parts += [triple] + [secs.get(k, b"") for k in (".text", ".rodata", ".note")]
        pos = fatbin.find(_BUNDLE_MAGIC, cur)
    return b"".join(parts) if parts else None


def code_object_id(path: str = LIB_PATH) -> str:
    """Identity of the device code in libnttmul.so: sha256 (16 hex digits) of the machine code of
    its gfx950 code objects -- each one's .text, .rodata (kernel descriptors) and .note (kernel
    metadata: names, register and LDS counts) -- read from the .hip_fatbin section's offload
    bundles (the whole section when it holds none).  Symbol tables are left out: they carry
    the compiler's per-source `__hip_cuid_*` marker, which changes with any edit of the .hip
    file even when no kernel does.  Host-only changes keep the id; any kernel change alters it.
    bench.py keys the committed PMC/ISA profiles (profiles/) by it, so a profile of another
    build is never reported as this build's."""
    import hashlib
    with open(path, "rb") as f:
        elf = f.read()
    if elf[:4] != b"\x7fELF" or elf[4] != 2:
        raise ValueError(f"{path}: not an ELF64 file")
    fat = _elf_sections(elf).get(".hip_fatbin")
    if fat is None:
        raise ValueError(f"{path}: no .hip_fatbin section")
    code = _device_code(fat)
    return hashlib.sha256(fat if code is None else code).hexdigest()[:16]


def _amdgcn_elfs(path: str) -> list:
    """The gfx950 code objects (ELF images) of a HIP shared library's .hip_fatbin offload bundles."""
    import struct
    with open(path, "rb") as f:
        elf = f.read()
    fat = _elf_sections(elf).get(".hip_fatbin")
    if fat is None:
        raise ValueError(f"{path}: no .hip_fatbin section")
    out, pos = [], fat.find(_BUNDLE_MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fat, pos + 24)
        cur = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fat, cur)
            triple = fat[cur + 24:cur + 24 + tlen]
            cur += 24 + tlen
            if b"amdgcn" in triple and size:
                out.append(fat[pos + off:pos + off + size])
        pos = fat.find(_BUNDLE_MAGIC, cur)
    return out


def _elf_symbols(elf: bytes):
    """(name, value, size, type, section index) of every .symtab entry of an ELF64 image, and the
    (address, file offset) of each section."""
    import struct
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    syms = []
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[s[6]][4]
        for k in range(s[5] // 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, s[4] + 24 * k)
            nm = elf[stroff + name:elf.index(b"\0", stroff + name)].decode(errors="replace")
            syms.append((nm, value, size, info & 15, shndx))
    return syms, [(s[3], s[4]) for s in secs]


_BUILTIN = {"j": "u32", "m": "u64", "y": "u64", "i": "i32", "l": "i64", "b": "bool", "h": "u8"}


def _demangle_args(s: str, i: int):
    """Template arguments I...E of an Itanium-mangled nttmul kernel name from position i (at the
    'I'), as short strings ("Arith32P3", "u32", "12", "false"); returns (args, next position) or
    None for a form the kernels do not use."""
    assert s[i] == "I"
    i += 1
    args = []
    while s[i] != "E":
        c = s[i]
        if c in _BUILTIN:
            args.append(_BUILTIN[c])
            i += 1
        elif c == "L":  # literal: L<type><value>E, n = negative
            j = s.index("E", i)
            t, v = s[i + 1], s[i + 2:j]
            v = "-" + v[1:] if v.startswith("n") else v
            args.append({"0": "false", "1": "true"}[v] if t == "b" else v)
            i = j + 1
        elif s.startswith("NS_", i):  # nttmul::<id>[<args>]
            i += 3
            j = i
            while s[j].isdigit():
                j += 1
            ln = int(s[i:j])
            name = s[j:j + ln]
            i = j + ln
            if s[i] == "I":
                sub = _demangle_args(s, i)
                if sub is None:
                    return None
                name += "<" + ",".join(sub[0]) + ">"
                i = sub[1]
            if s[i] != "E":
                return None
            i += 1
            args.append(name)
        else:
            return None
    return args, i + 1


def kernel_key(symbol: str) -> str:
    """Short name of a kernel symbol of libnttmul.so, e.g.
    _ZN6nttmul6k_rowsINS_9Arith32P3EjjLi12ELi0ELb0EEEv... -> k_rows<Arith32P3,u32,u32,12,0,false>
    (the mangled symbol itself for a form this small demangler does not cover)."""
    if not symbol.startswith("_ZN6nttmul"):
        return symbol
    i = len("_ZN6nttmul")
    j = i
    while j < len(symbol) and symbol[j].isdigit():
        j += 1
    if j == i:
        return symbol
    ln = int(symbol[i:j])
    name = symbol[j:j + ln]
    k = j + ln
    if k < len(symbol) and symbol[k] == "I":
        try:
            r = _demangle_args(symbol, k)
        except (IndexError, KeyError, ValueError):
            r = None
        if r is None:
            return symbol
        return name + "<" + ",".join(r[0]) + ">"
    return name


def dispatch_key(name: str) -> str:
    """The kernel_key of one kernel named the way the library's dispatch describes it
    (nttmul_kernel_name: "k_rows<Arith32P3,u32,u32,12,0>", "...,prio>", "k_cols8<Arith64,u64,fwd>",
    "k_cols_fwd<Arith64,u64,4>"): the template arguments the short names leave out are filled in
    as kernels.hip instantiates them."""
    import re
    m = re.fullmatch(r"(\w+)<(.*)>", name.strip())
    if not m:
        return name.strip()
    kern, args = m.group(1), m.group(2).split(",")
    if kern == "k_rows":
        prio = args[-1] == "prio"
        args = (args[:-1] if prio else args) + ["true" if prio else "false"]
    elif kern == "k_cols_fwd":
        args = args + ["2"]
    elif kern == "k_cols8":
        w = "u64" if args[0] == "Arith64" else "u32"
        args = ([args[0], args[1], w, "0", "2"] if args[2] == "fwd" else [args[0], w, args[1], "1", "1"])
    return f"{kern}<{','.join(args)}>"


def kernel_hashes(path: str = LIB_PATH) -> dict:
    """Identity of every kernel in libnttmul.so's gfx950 code object, one by one: {kernel_key:
    sha256 (16 hex digits) of the kernel's machine code (its .text range) and its 64-byte kernel
    descriptor (<symbol>.kd: register, LDS, scratch and kernarg sizes), with the descriptor's
    kernel_code_entry_byte_offset (bytes 16-23, the distance from descriptor to code, which moves
    with every other kernel's size) zeroed}.  The kernels take everything through their arguments
    (no PC-relative data: no s_getpc_b64 in the listing), so a kernel's bytes change only when
    its own code does: a profile keyed by these hashes stays valid across edits of other kernels
    and of host code, and a claim "kernel X unchanged" is checkable (code_object_id is the
    whole-object digest)."""
    import hashlib
    out = {}
    for co in _amdgcn_elfs(path):
        syms, secs = _elf_symbols(co)
        by_name = {s[0]: s for s in syms}
        for nm, value, size, typ, shndx in syms:
            if typ != 2 or not size or nm + ".kd" not in by_name:  # STT_FUNC with a descriptor
                continue
            addr, off = secs[shndx]
            code = co[off + value - addr:off + value - addr + size]
            kd = by_name[nm + ".kd"]
            kaddr, koff = secs[kd[4]]
            desc = bytearray(co[koff + kd[1] - kaddr:koff + kd[1] - kaddr + 64])
            desc[16:24] = bytes(8)
            out[kernel_key(nm)] = hashlib.sha256(code + bytes(desc)).hexdigest()[:16]
    return out


def dispatched_kernel_hashes(names: str, path: str = LIB_PATH) -> dict:
    """{kernel_key: kernel hash}, in dispatch order, for a nttmul_kernel_name string
    ("a + b + c"); raises KeyError naming a kernel the code object does not hold."""
    table = kernel_hashes(path)
    out = {}
    for nm in (x.strip() for x in names.split("+")):
        key = dispatch_key(nm)
        if key not in table:
            raise KeyError(f"{nm} ({key}) is not a kernel of {path}")
        out[key] = table[key]
    return out


def exported_symbols() -> list:
    """Function names declared in include/nttmul.h (for the ABI completeness test)."""
    import re
    text = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|void|char\s*\*|const char \*)\s*\*?\s*"
                                 r"(nttmul_\w+|i?ntt256_\w+|ntt_red256_\w+|mulntt256_\w+|"
                                 r"inttmul256_\w+)\s*\(", text, re.M)))


def strerror(status: int) -> str:
    return load_library().nttmul_strerror(status).decode()


def _ptr(x) -> int:
    """Raw address of a numpy array or a torch tensor (device pointer for CUDA/HIP tensors)."""
    if isinstance(x, np.ndarray):
        assert x.flags.c_contiguous
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        assert x.is_contiguous()
        return x.data_ptr()
    return int(x)


def _dev_arg(x, batch: int, n: int, word_bits: int, dev: int) -> int:
    """Device pointer of an operand of a *_device call, after checking what the C ABI cannot:
    a torch tensor must hold at least batch * n words of word_bits on HIP device `dev`
    (a raw integer address is passed through unchecked, as in C)."""
    if word_bits not in (32, 64):
        raise ValueError("word_bits must be 32 or 64")
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("device operands must be contiguous")
        if x.element_size() * 8 != word_bits:
            raise ValueError(f"tensor of {x.element_size() * 8}-bit elements for word_bits={word_bits}")
        if x.numel() < batch * n:
            raise ValueError(f"tensor of {x.numel()} words < batch * n = {batch * n}")
        if x.device.type != "cuda" or x.device.index != dev:
            raise ValueError(f"tensor on {x.device}, context call on device {dev}")
        return x.data_ptr()
    return _ptr(x)


class Context:
    """An (n, q) multiplier bound to one or more HIP devices (≙ an opened FPGA handle).

    Caller memory (include/nttmul.h; host arrays and device tensors alike).  Alignment: operands
    need the alignment of their word only.  Aliasing: out may be the input itself for every
    transform (forward, inverse, transform in every mode), and c may be a or b for pointwise; for
    products c must not overlap a or b; partial overlap is never allowed.  Footprint: a call
    writes exactly batch * n words of its output and nothing else in caller memory; inputs are
    never written.

    Lifetime: one context serves any sequence of calls, from one host thread at a time.  close()
    (nttmul_destroy) does not wait for the streams passed to the *_device calls: synchronise them
    first, a kernel still queued there would read freed tables."""

    def __init__(self, n: int, q: int, psi: int = 0, ndev: int = 1, first_dev: int = 0,
                 validate: bool = False, cyclic: bool = False, share_devices: bool = False,
                 issue_prio: int = 0, zero_copy_kb: int = 0, copy_threads: int = 0,
                 scratch_mb: int = 0, small_server: int = 0,
                 _lib: Optional[ctypes.CDLL] = None):
        """cyclic=True: FPGA-compat product mod (x^n - 1, q) (Hardware_Multiplier/PolyMult.v);
        `psi` then carries the primitive n-th root omega (0 = the smallest one).
        share_devices=True: `ndev` slices may map several onto one device (round-robin).
        issue_prio, zero_copy_kb, copy_threads, scratch_mb, small_server: the nttmul_params
        dispatch knobs (include/nttmul.h; 0 = the library default)."""
        self._lib = load_library() if _lib is None else _lib
        self._h = ctypes.c_void_p()
        flags = ((NTTMUL_FLAG_VALIDATE if validate else 0) | (NTTMUL_FLAG_CYCLIC if cyclic else 0)
                 | (NTTMUL_FLAG_SHARE_DEVICES if share_devices else 0))
        prm = _Params(n, q, psi, ndev, first_dev, flags, issue_prio, zero_copy_kb, copy_threads,
                      scratch_mb, small_server)
        st = self._lib.nttmul_create_sized(ctypes.byref(self._h), ctypes.byref(prm),
                                           ctypes.sizeof(prm))
        if st != NTTMUL_OK:
            raise NttmulError(st, strerror(st))
        info = Info()
        self._lib.nttmul_get_info(self._h, ctypes.byref(info))
        self.info = info
        self.n, self.q, self.psi = info.n, info.q, info.psi
        self.word_bits = info.word_bits
        self.first_dev = first_dev

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.nttmul_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int):
        if st != NTTMUL_OK:
            raise NttmulError(st, f"{strerror(st)}: {self._lib.nttmul_last_error(self._h).decode()}")

    def last_host_path(self) -> int:
        """nttmul_last_host_path: 0 staged, 1 direct DMA, 2 zero-copy, 3 device server, -1 no
        call yet."""
        return int(self._lib.nttmul_last_host_path(self._h))

    def server_status(self):
        """nttmul_server_status: (setup / launch failures of the device server so far, the last
        one's message)."""
        buf = ctypes.create_string_buffer(256)
        n = self._lib.nttmul_server_status(self._h, buf, len(buf))
        if n < 0:
            self._check(n)
        return int(n), buf.value.decode()

    def diag_server_failpoint(self, site: str, hip_error: int = HIP_ERROR_OUT_OF_MEMORY,
                              skip: int = 0) -> None:
        """nttmul_diag_server_failpoint (a context of load_diag_library() only): arm `site`, one
        of DIAG_SITES, to fail once with hip_error after `skip` further passes."""
        self._check(self._lib.nttmul_diag_server_failpoint(self._h, DIAG_SITES.index(site),
                                                           hip_error, skip))

    def diag_server_state(self) -> dict:
        """nttmul_diag_server_state (a context of load_diag_library() only), as a dict."""
        st = DiagServerState()
        self._check(self._lib.nttmul_diag_server_state(self._h, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in DiagServerState._fields_}

    def kernel_name(self, word_bits: int = 0, batch: int = 0) -> str:
        """The device kernel(s) a product call of `batch` polynomials dispatches to
        (nttmul_kernel_name_batch; batch 0 = a large batch), e.g. "k_rows<Arith32P3,u32,u32,12,0>",
        or "k_rows<Arith32P,u32,u32,10,0,prio>" for a batch of at most 4 waves per SIMD."""
        word_bits = word_bits or (32 if self.q < (1 << 32) else 64)
        buf = ctypes.create_string_buffer(256)
        st = self._lib.nttmul_kernel_name_batch(self._h, word_bits, batch, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def last_kernel_name(self) -> str:
        """The kernel(s) the last product call launched (nttmul_last_kernel_name; "" before)."""
        buf = ctypes.create_string_buffer(256)
        st = self._lib.nttmul_last_kernel_name(self._h, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    @property
    def io_dtype(self):
        return np.uint32 if self.q < (1 << 32) else np.uint64

    def multiply(self, a, b, dtype=None, out=None) -> np.ndarray:
        """c = a * b mod (x^n + 1, q) for host arrays of shape [n] or [batch, n].  `out`: the
        result array (same shape and dtype); with a, b and out in page-locked memory
        (host_empty) the library DMAs straight from and to them instead of staging."""
        dtype = dtype or self.io_dtype
        a = np.ascontiguousarray(a, dtype=dtype)
        b = np.ascontiguousarray(b, dtype=dtype)
        if a.shape != b.shape or a.shape[-1] != self.n:
            raise ValueError("a and b must both have shape [..., n]")
        if out is not None and (out.shape != a.shape or out.dtype != a.dtype
                                or not out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous array of a's shape and dtype")
        c = np.empty_like(a) if out is None else out
        batch = a.size // self.n
        fn = self._lib.nttmul_multiply_batch_u32 if dtype == np.uint32 else self._lib.nttmul_multiply_batch_u64
        self._check(fn(self._h, c.ctypes.data, a.ctypes.data, b.ctypes.data, batch))
        return c

    def _unary(self, op: str, x, dtype=None) -> np.ndarray:
        dtype = dtype or self.io_dtype
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.shape[-1] != self.n:
            raise ValueError("input must have shape [..., n]")
        out = np.empty_like(x)
        w = "u32" if dtype == np.uint32 else "u64"
        fn = getattr(self._lib, f"nttmul_{op}_batch_{w}")
        self._check(fn(self._h, out.ctypes.data, x.ctypes.data, x.size // self.n))
        return out

    def forward(self, a, dtype=None) -> np.ndarray:
        """Negacyclic forward NTT, bit-reversed output (NTT/ntt.C:342 mulntt_ct_std2rev)."""
        return self._unary("forward", a, dtype)

    def inverse(self, a_hat, dtype=None) -> np.ndarray:
        """Inverse of forward(): nttmul_gs_rev2std (NTT/ntt.C:428) then n^-1."""
        return self._unary("inverse", a_hat, dtype)

    def transform(self, x, mode: int, dtype=None) -> np.ndarray:
        """nttmul_transform_batch: mode = XF_FORWARD/XF_INVERSE | XF_STD2REV/XF_REV2STD
        [| XF_UNSCALED] — the reference's wrapper set (NTT/ntt256.h:20-69) for this context."""
        dtype = dtype or self.io_dtype
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.shape[-1] != self.n:
            raise ValueError("input must have shape [..., n]")
        out = np.empty_like(x)
        w = "u32" if dtype == np.uint32 else "u64"
        fn = getattr(self._lib, f"nttmul_transform_batch_{w}")
        self._check(fn(self._h, mode, out.ctypes.data, x.ctypes.data, x.size // self.n))
        return out

    def transform_device(self, out, x, mode: int, batch: int, word_bits: int,
                         dev: Optional[int] = None, stream: int = 0):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch, self.n, word_bits, dev) for t in (out, x)]
        self._check(self._lib.nttmul_transform_device(self._h, mode, *args, batch,
                                                      word_bits, dev, stream or None))

    def pointwise(self, a, b, dtype=None) -> np.ndarray:
        """c[i] = a[i] * b[i] mod q (NTT/ntt.C:131 mul_array)."""
        dtype = dtype or self.io_dtype
        a = np.ascontiguousarray(a, dtype=dtype)
        b = np.ascontiguousarray(b, dtype=dtype)
        if a.shape != b.shape or a.shape[-1] != self.n:
            raise ValueError("a and b must both have shape [..., n]")
        c = np.empty_like(a)
        w = "u32" if dtype == np.uint32 else "u64"
        fn = getattr(self._lib, f"nttmul_pointwise_batch_{w}")
        self._check(fn(self._h, c.ctypes.data, a.ctypes.data, b.ctypes.data, a.size // self.n))
        return c

    def forward_device(self, out, a, batch: int, word_bits: int, dev: Optional[int] = None,
                       stream: int = 0):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch, self.n, word_bits, dev) for t in (out, a)]
        self._check(self._lib.nttmul_forward_batch_device(self._h, *args, batch,
                                                          word_bits, dev, stream or None))

    def inverse_device(self, out, a, batch: int, word_bits: int, dev: Optional[int] = None,
                       stream: int = 0):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch, self.n, word_bits, dev) for t in (out, a)]
        self._check(self._lib.nttmul_inverse_batch_device(self._h, *args, batch,
                                                          word_bits, dev, stream or None))

    def pointwise_device(self, c, a, b, batch: int, word_bits: int, dev: Optional[int] = None,
                         stream: int = 0):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch, self.n, word_bits, dev) for t in (c, a, b)]
        self._check(self._lib.nttmul_pointwise_batch_device(self._h, *args,
                                                            batch, word_bits, dev, stream or None))

    def multiply_device(self, c, a, b, batch: int, word_bits: int, dev: Optional[int] = None,
                        stream: int = 0):
        """Device-resident batch (pointers or torch tensors on `dev`), enqueued on `stream`."""
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch, self.n, word_bits, dev) for t in (c, a, b)]
        self._check(self._lib.nttmul_multiply_batch_device(self._h, *args, batch,
                                                           word_bits, dev, stream or None))

    def fill_random_device(self, a, b, p0: int, count: int, word_bits: int, seed: int = SEED,
                           dev: Optional[int] = None, stream: int = 0):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, count, self.n, word_bits, dev) for t in (a, b)]
        self._check(self._lib.nttmul_fill_random_device(self._h, *args, p0, count, seed,
                                                        word_bits, dev, stream or None))


# ---- products against NTT-domain operands (include/nttmul_mac.h) ---------------------------------

_MAC_LIB: Optional[ctypes.CDLL] = None


def load_mac_library() -> ctypes.CDLL:
    """Load lib/libnttmul_mac.so (include/nttmul_mac.h): the ABI and kernels of libnttmul.so plus
    the fused multiply-accumulate against NTT-domain operands.  load_library() is unaffected."""
    global _MAC_LIB
    if _MAC_LIB is not None:
        return _MAC_LIB
    if not os.path.exists(MAC_LIB_PATH):
        raise ImportError(f"{MAC_LIB_PATH} not built: run __graft_entry__.build() or make -C {PKG_DIR}")
    _MAC_LIB = _bind_mac(_bind(ctypes.CDLL(MAC_LIB_PATH)))
    return _MAC_LIB


def _bind_mac(lib: ctypes.CDLL) -> ctypes.CDLL:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    lib.nttmul_mac_ntt_device.argtypes = [vp, vp, vp, vp, sz, u32, i32, i32, i32, vp]
    for w in ("u32", "u64"):
        getattr(lib, f"nttmul_mac_ntt_{w}").argtypes = [vp, vp, vp, vp, sz, u32, i32]
    lib.nttmul_mac_kernel_name.argtypes = [vp, i32, ctypes.c_char_p, sz]
    return lib


def mac_exported_symbols() -> list:
    """Function names declared in include/nttmul_mac.h."""
    import re
    return sorted(set(re.findall(r"^\s*int\s+(nttmul_mac_\w+)\s*\(", open(MAC_HEADER_PATH).read(), re.M)))


class MacContext(Context):
    """A Context created through lib/libnttmul_mac.so: every Context method, plus
    c[p] = INTT(sum_t NTT(a[p][t]) o b_hat[p or 0][t]) for n <= 4096 (include/nttmul_mac.h).

    Caller memory, as for Context: operands need the alignment of their word only; c must not
    overlap a or b_hat (no aliasing form is allowed); a call writes exactly batch * n words of c
    and nothing else in caller memory, and never writes a or b_hat."""

    def __init__(self, n: int, q: int, **kw):
        super().__init__(n, q, _lib=load_mac_library(), **kw)

    def mac_kernel_name(self, word_bits: int = 0) -> str:
        """nttmul_mac_kernel_name, e.g. "k_mac<Arith32P,u32,u32,12>"."""
        word_bits = word_bits or (32 if self.q < (1 << 32) else 64)
        buf = ctypes.create_string_buffer(256)
        st = self._lib.nttmul_mac_kernel_name(self._h, word_bits, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def mac_ntt_device(self, c, a, b_hat, batch: int, terms: int, word_bits: int,
                       shared: bool = False, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        a [batch][terms][n], b_hat [batch][terms][n] ([terms][n] when shared), c [batch][n]."""
        dev = self.first_dev if dev is None else dev
        counts = (batch, batch * terms, terms if shared else batch * terms)
        args = [_dev_arg(t, k, self.n, word_bits, dev) for t, k in zip((c, a, b_hat), counts)]
        self._check(self._lib.nttmul_mac_ntt_device(self._h, *args, batch, terms, int(shared),
                                                    word_bits, dev, stream or None))

    def mac_ntt(self, a, b_hat, shared: bool = False, dtype=None) -> np.ndarray:
        """Host arrays: a of shape [batch, terms, n]; b_hat of a's shape, or [terms, n] when
        shared.  Returns c of shape [batch, n]."""
        dtype = dtype or self.io_dtype
        a = np.ascontiguousarray(a, dtype=dtype)
        b_hat = np.ascontiguousarray(b_hat, dtype=dtype)
        if a.ndim != 3 or a.shape[-1] != self.n or a.shape[1] == 0:
            raise ValueError("a must have shape [batch, terms, n] with terms > 0")
        if b_hat.shape != (a.shape[1:] if shared else a.shape):
            raise ValueError("b_hat must have a's shape, or [terms, n] when shared")
        c = np.empty((a.shape[0], self.n), dtype=dtype)
        fn = self._lib.nttmul_mac_ntt_u32 if dtype == np.uint32 else self._lib.nttmul_mac_ntt_u64
        self._check(fn(self._h, c.ctypes.data, a.ctypes.data, b_hat.ctypes.data, a.shape[0],
                       a.shape[1], int(shared)))
        return c


# ---- what the limb-aware libraries' bindings share ------------------------------------------------

_LIMB_LIBS: dict = {}


def _load_limb_library(path: str, *binders) -> ctypes.CDLL:
    """The library at `path`, loaded once: the plain and the mac ABI bound, then each of
    `binders` applied."""
    lib = _LIMB_LIBS.get(path)
    if lib is None:
        if not os.path.exists(path):
            raise ImportError(f"{path} not built: run __graft_entry__.build() or make -C {PKG_DIR}")
        lib = _bind_mac(_bind(ctypes.CDLL(path)))
        for bind in binders:
            bind(lib)
        _LIMB_LIBS[path] = lib
    return lib


def _header_symbols(header: str, prefix: str) -> list:
    """Function names starting with `prefix` declared in the header at `header`."""
    import re
    return sorted(set(re.findall(r"^\s*(?:int|void|const char \*)\s*(%s\w+)\s*\(" % prefix,
                                 open(header).read(), re.M)))


def _flags(validate: bool, cyclic: bool, share_devices: bool) -> int:
    return ((NTTMUL_FLAG_VALIDATE if validate else 0) | (NTTMUL_FLAG_CYCLIC if cyclic else 0)
            | (NTTMUL_FLAG_SHARE_DEVICES if share_devices else 0))


def _bind_handle(lib: ctypes.CDLL, prefix: str, info, create_args: list) -> None:
    """The entry points every handle has: create (after out, params and size: create_args),
    destroy, last_error, get_info."""
    vp = ctypes.c_void_p
    getattr(lib, f"{prefix}_create").argtypes = [ctypes.POINTER(vp), ctypes.POINTER(_Params),
                                                 ctypes.c_size_t] + create_args
    getattr(lib, f"{prefix}_destroy").argtypes = [vp]
    getattr(lib, f"{prefix}_destroy").restype = None
    getattr(lib, f"{prefix}_last_error").argtypes = [vp]
    getattr(lib, f"{prefix}_last_error").restype = ctypes.c_char_p
    getattr(lib, f"{prefix}_get_info").argtypes = [vp, ctypes.POINTER(info)]


class _Entries:
    """lib.<prefix>_<name> as the attribute <name>: looked up on first use, a plain attribute from
    then on, so a call costs what `lib.<prefix>_<name>` written out costs."""

    def __init__(self, lib: ctypes.CDLL, prefix: str):
        self._lib, self._prefix = lib, prefix

    def __getattr__(self, name: str):
        fn = getattr(self._lib, f"{self._prefix}_{name}")
        setattr(self, name, fn)
        return fn


class _Handle:
    """What the handle classes of the limb-aware libraries share.  Class attributes: _PREFIX, the
    C prefix of the library's entry points (self._c.<name> is <prefix>_<name>); _OPS, the op names
    in <prefix>_kernel_name's numbering; _NAME_CAP, the bytes kernel_name asks for."""
    _PREFIX = ""
    _OPS: tuple = ()
    _NAME_CAP = 256

    def _open(self, lib: ctypes.CDLL, info, prm: _Params, *args):
        """<prefix>_create(&h, &prm, sizeof prm, *args), then <prefix>_get_info into self.info."""
        self._lib, self._c = lib, _Entries(lib, self._PREFIX)
        self._h = ctypes.c_void_p()
        st = self._c.create(ctypes.byref(self._h), ctypes.byref(prm), ctypes.sizeof(prm), *args)
        if st != NTTMUL_OK:
            raise NttmulError(st, lib.nttmul_strerror(st).decode())
        self._c.get_info(self._h, ctypes.byref(info))
        self.info = info

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._c.destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int):
        if st != NTTMUL_OK:
            raise NttmulError(st, f"{self._lib.nttmul_strerror(st).decode()}: "
                                  f"{self._c.last_error(self._h).decode()}")

    @property
    def io_dtype(self):
        return np.uint32 if self.word_bits == 32 else np.uint64

    def _kernel_name(self, op, *extra) -> str:
        op = self._OPS.index(op) if isinstance(op, str) else int(op)
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.kernel_name(self._h, op, *extra, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()


class _LimbContext(_Handle):
    """A handle over one basis `moduli` and [batch, limbs, n] operands (RnsContext, RnsMpContext,
    GaloisContext): n, limbs, word_bits, moduli, first_dev, and <prefix>_limb_info."""

    def _open_limbs(self, lib, info, n, moduli, ndev, first_dev, flags, scratch_mb=0):
        moduli = [int(q) for q in moduli]
        prm = _Params(n, 0, 0, ndev, first_dev, flags, 0, 0, 0, scratch_mb, 0)
        qs = (ctypes.c_uint64 * max(1, len(moduli)))(*moduli)
        self._open(lib, info, prm, qs, len(moduli))
        self.n, self.limbs, self.word_bits = info.n, info.limbs, info.word_bits
        self.moduli = tuple(moduli)
        self.first_dev = first_dev

    def limb_info(self, limb: int) -> Info:
        """<prefix>_limb_info: q, psi, omega, ... of one limb."""
        info = Info()
        self._check(self._c.limb_info(self._h, limb, ctypes.byref(info)))
        return info

    def _dev_args(self, operands, polys, dev):
        return [_dev_arg(t, k * self.limbs, self.n, self.word_bits, dev)
                for t, k in zip(operands, polys)]


# ---- one launch over all limbs of an RNS basis (include/nttmul_rns.h) ----------------------------

RNS_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_rns.so")
RNS_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_rns.h")
RNS_MAX_LIMBS = 64
RNS_OPS = ("multiply", "forward", "inverse", "mac")   # nttmul_rns_kernel_name's op numbers


class RnsInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("limbs", ctypes.c_uint32),
                ("word_bits", ctypes.c_uint32), ("ndev", ctypes.c_int)]


def load_rns_library() -> ctypes.CDLL:
    """Load lib/libnttmul_rns.so (include/nttmul_rns.h): the ABI and kernels of libnttmul_mac.so
    plus the limb-aware kernels.  load_library() and load_mac_library() are unaffected."""
    return _load_limb_library(RNS_LIB_PATH, _bind_rns)


def _bind_rns(lib: ctypes.CDLL, prefix: str = "nttmul_rns", info=RnsInfo) -> ctypes.CDLL:
    """nttmul_rns_*, and with the other prefix and info type nttmul_rnsmp_*."""
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    _bind_handle(lib, prefix, info, [ctypes.POINTER(ctypes.c_uint64), u32])
    getattr(lib, f"{prefix}_limb_info").argtypes = [vp, u32, ctypes.POINTER(Info)]
    getattr(lib, f"{prefix}_multiply_device").argtypes = [vp, vp, vp, vp, sz, i32, vp]
    getattr(lib, f"{prefix}_forward_device").argtypes = [vp, vp, vp, sz, i32, vp]
    getattr(lib, f"{prefix}_inverse_device").argtypes = [vp, vp, vp, sz, i32, vp]
    getattr(lib, f"{prefix}_mac_ntt_device").argtypes = [vp, vp, vp, vp, sz, u32, i32, i32, vp]
    getattr(lib, f"{prefix}_multiply").argtypes = [vp, vp, vp, vp, sz]
    getattr(lib, f"{prefix}_forward").argtypes = [vp, vp, vp, sz]
    getattr(lib, f"{prefix}_inverse").argtypes = [vp, vp, vp, sz]
    getattr(lib, f"{prefix}_mac_ntt").argtypes = [vp, vp, vp, vp, sz, u32, i32]
    getattr(lib, f"{prefix}_kernel_name").argtypes = [vp, i32, ctypes.c_char_p, sz]
    return lib


def rns_exported_symbols() -> list:
    """Function names declared in include/nttmul_rns.h."""
    return _header_symbols(RNS_HEADER_PATH, "nttmul_rns_")


class _RnsOps(_LimbContext):
    """What RnsContext and RnsMpContext share: the four operations over [batch, limbs, n]
    operands, as <prefix>_<op> on host arrays and <prefix>_<op>_device on device memory."""
    _OPS = RNS_OPS

    # device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`

    def multiply_device(self, c, a, b, batch: int, dev: Optional[int] = None, stream: int = 0):
        """c, a, b: [batch][limbs][n]."""
        dev = self.first_dev if dev is None else dev
        args = self._dev_args((c, a, b), (batch,) * 3, dev)
        self._check(self._c.multiply_device(self._h, *args, batch, dev, stream or None))

    def forward_device(self, out, a, batch: int, dev: Optional[int] = None, stream: int = 0):
        dev = self.first_dev if dev is None else dev
        args = self._dev_args((out, a), (batch,) * 2, dev)
        self._check(self._c.forward_device(self._h, *args, batch, dev, stream or None))

    def inverse_device(self, out, a, batch: int, dev: Optional[int] = None, stream: int = 0):
        dev = self.first_dev if dev is None else dev
        args = self._dev_args((out, a), (batch,) * 2, dev)
        self._check(self._c.inverse_device(self._h, *args, batch, dev, stream or None))

    def mac_ntt_device(self, c, a, b_hat, batch: int, terms: int, shared: bool = False,
                       dev: Optional[int] = None, stream: int = 0):
        """a [batch][terms][limbs][n], b_hat likewise ([terms][limbs][n] when shared),
        c [batch][limbs][n]."""
        dev = self.first_dev if dev is None else dev
        args = self._dev_args((c, a, b_hat),
                              (batch, batch * terms, terms if shared else batch * terms), dev)
        self._check(self._c.mac_ntt_device(self._h, *args, batch, terms, int(shared), dev,
                                               stream or None))

    # host arrays

    def _host(self, x, ndim, what):
        x = np.ascontiguousarray(x, dtype=self.io_dtype)
        if x.ndim != ndim or x.shape[-2:] != (self.limbs, self.n):
            raise ValueError(f"{what} must have shape "
                             f"[batch, {'terms, ' if ndim == 4 else ''}limbs, n]")
        return x

    def multiply(self, a, b) -> np.ndarray:
        """c[p][l] = a[p][l] * b[p][l] mod (x^n + 1, q_l) for arrays of shape [batch, limbs, n]."""
        a, b = self._host(a, 3, "a"), self._host(b, 3, "b")
        if a.shape != b.shape:
            raise ValueError("a and b must have the same shape")
        c = np.empty_like(a)
        self._check(self._c.multiply(self._h, c.ctypes.data, a.ctypes.data, b.ctypes.data,
                                         a.shape[0]))
        return c

    def forward(self, a) -> np.ndarray:
        a = self._host(a, 3, "a")
        out = np.empty_like(a)
        self._check(self._c.forward(self._h, out.ctypes.data, a.ctypes.data, a.shape[0]))
        return out

    def inverse(self, a_hat) -> np.ndarray:
        a_hat = self._host(a_hat, 3, "a_hat")
        out = np.empty_like(a_hat)
        self._check(self._c.inverse(self._h, out.ctypes.data, a_hat.ctypes.data,
                                        a_hat.shape[0]))
        return out

    def mac_ntt(self, a, b_hat, shared: bool = False) -> np.ndarray:
        """a of shape [batch, terms, limbs, n]; b_hat of a's shape, or [terms, limbs, n] when
        shared.  Returns c of shape [batch, limbs, n]."""
        a = self._host(a, 4, "a")
        b_hat = np.ascontiguousarray(b_hat, dtype=self.io_dtype)
        if a.shape[1] == 0:
            raise ValueError("terms must be > 0")
        if b_hat.shape != (a.shape[1:] if shared else a.shape):
            raise ValueError("b_hat must have a's shape, or [terms, limbs, n] when shared")
        c = np.empty((a.shape[0], self.limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.mac_ntt(self._h, c.ctypes.data, a.ctypes.data, b_hat.ctypes.data,
                                        a.shape[0], a.shape[1], int(shared)))
        return c


class RnsContext(_RnsOps):
    """nttmul_rns: the moduli q_0 .. q_{L-1} of one degree n <= 4096, every operation one launch
    over [batch, limbs, n] operands (include/nttmul_rns.h).  Words are info.word_bits wide: 32
    when every q_l < 2^31, 64 when every q_l >= 2^32.

    Caller memory, as for Context: operands need the alignment of their word only; out may be the
    input itself for forward and inverse, c must not overlap a, b or b_hat, and partial overlap is
    never allowed; a call writes exactly batch * limbs * n words of its output and nothing else
    in caller memory, and never writes an input."""
    _PREFIX = "nttmul_rns"

    def __init__(self, n: int, moduli, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False):
        self._open_limbs(load_rns_library(), RnsInfo(), n, moduli, ndev, first_dev,
                         _flags(validate, cyclic, share_devices))

    def kernel_name(self, op) -> str:
        """nttmul_rns_kernel_name for op 0..3 or "multiply" / "forward" / "inverse" / "mac", e.g.
        "k_rns_rows<Arith32P3,u32,12>"."""
        return self._kernel_name(op)


# ---- RNS base conversion and ModDown (include/nttmul_bconv.h) ------------------------------------

BCONV_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_bconv.so")
BCONV_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_bconv.h")
BCONV_OPS = ("convert", "moddown")                    # nttmul_bconv_kernel_name's op numbers


class BconvInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("from_limbs", ctypes.c_uint32),
                ("to_limbs", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int)]


def load_bconv_library() -> ctypes.CDLL:
    """Load lib/libnttmul_bconv.so (include/nttmul_bconv.h): the ABI and kernels of
    libnttmul_rns.so plus the base-conversion kernels.  The other loaders are unaffected."""
    return _load_limb_library(BCONV_LIB_PATH, _bind_rns, _bind_bconv)


def _bind_bconv(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64p, prm = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_Params)
    _bind_handle(lib, "nttmul_bconv", BconvInfo, [u64p, u32, u64p, u32])
    lib.nttmul_bconv_plan.argtypes = [prm, sz, u64p, u32, u64p, u32, u64p, u64p, u64p]
    for op in BCONV_OPS:
        getattr(lib, f"nttmul_bconv_{op}_device").argtypes = [vp, vp, vp, sz, i32, vp]
        getattr(lib, f"nttmul_bconv_{op}").argtypes = [vp, vp, vp, sz]
    lib.nttmul_bconv_kernel_name.argtypes = [vp, i32, ctypes.c_char_p, sz]


def bconv_exported_symbols() -> list:
    """Function names declared in include/nttmul_bconv.h."""
    return _header_symbols(BCONV_HEADER_PATH, "nttmul_bconv_")


def _bconv_bases(n, from_q, to_q, flags):
    from_q, to_q = [int(q) for q in from_q], [int(q) for q in to_q]
    prm = _Params(n, 0, 0, 1, 0, flags, 0, 0, 0, 0, 0)
    fq = (ctypes.c_uint64 * max(1, len(from_q)))(*from_q)
    tq = (ctypes.c_uint64 * max(1, len(to_q)))(*to_q)
    return from_q, to_q, prm, fq, tq


def bconv_plan(n: int, from_q, to_q, flags: int = 0):
    """nttmul_bconv_plan, without a device: (inv, w, binv) as lists of Python integers with
    inv[i] = Bh_i^-1 mod b_i, w[i][j] = Bh_i mod c_j, binv[j] = B^-1 mod c_j.  Raises NttmulError
    with the status nttmul_bconv_create would return for these bases."""
    lib = load_bconv_library()
    from_q, to_q, prm, fq, tq = _bconv_bases(n, from_q, to_q, flags)
    L, K = len(from_q), len(to_q)
    inv, w, binv = ((ctypes.c_uint64 * max(1, k))() for k in (L, L * K, K))
    st = lib.nttmul_bconv_plan(ctypes.byref(prm), ctypes.sizeof(prm), fq, L, tq, K, inv, w, binv)
    if st != NTTMUL_OK:
        raise NttmulError(st, lib.nttmul_strerror(st).decode())
    return list(inv[:L]), [list(w[i * K:(i + 1) * K]) for i in range(L)], list(binv[:K])


class BaseConverter(_Handle):
    """nttmul_bconv: conversion from the basis from_q (L primes) to the disjoint basis to_q
    (K primes) of one word class for one degree n <= 4096 (include/nttmul_bconv.h).  convert maps
    [batch, L, n] to [batch, K, n]; moddown maps [batch, K + L, n] (limbs of to_q, then of from_q)
    to [batch, K, n].  Words are word_bits wide."""
    _PREFIX = "nttmul_bconv"
    _OPS = BCONV_OPS

    def __init__(self, n: int, from_q, to_q, ndev: int = 1, first_dev: int = 0,
                 validate: bool = False, cyclic: bool = False, share_devices: bool = False):
        from_q, to_q, prm, fq, tq = _bconv_bases(n, from_q, to_q,
                                                 _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev = ndev, first_dev
        info = BconvInfo()
        self._open(load_bconv_library(), info, prm, fq, len(from_q), tq, len(to_q))
        self.n, self.word_bits = info.n, info.word_bits
        self.from_limbs, self.to_limbs = info.from_limbs, info.to_limbs
        self.from_q, self.to_q = tuple(from_q), tuple(to_q)
        self.first_dev = first_dev

    def kernel_name(self, op) -> str:
        """nttmul_bconv_kernel_name for op 0..1 or "convert" / "moddown", e.g. "k_bconv<u32,0>"."""
        return self._kernel_name(op)

    def _in_limbs(self, op: str) -> int:
        return self.from_limbs + (self.to_limbs if op == "moddown" else 0)

    # device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`

    def _device(self, op, out, x, batch, dev, stream):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch * k, self.n, self.word_bits, dev)
                for t, k in ((out, self.to_limbs), (x, self._in_limbs(op)))]
        self._check(getattr(self._c, f"{op}_device")(self._h, *args, batch, dev, stream or None))

    def convert_device(self, out, x, batch: int, dev: Optional[int] = None, stream: int = 0):
        """x [batch][from_limbs][n] -> out [batch][to_limbs][n]."""
        self._device("convert", out, x, batch, dev, stream)

    def moddown_device(self, out, x, batch: int, dev: Optional[int] = None, stream: int = 0):
        """x [batch][to_limbs + from_limbs][n] -> out [batch][to_limbs][n]."""
        self._device("moddown", out, x, batch, dev, stream)

    # host arrays

    def _host(self, op, x):
        x = np.ascontiguousarray(x, dtype=self.io_dtype)
        if x.ndim != 3 or x.shape[1:] != (self._in_limbs(op), self.n):
            raise ValueError(f"{op}: x must have shape [batch, {self._in_limbs(op)}, {self.n}]")
        out = np.empty((x.shape[0], self.to_limbs, self.n), dtype=self.io_dtype)
        self._check(getattr(self._c, op)(self._h, out.ctypes.data, x.ctypes.data, x.shape[0]))
        return out

    def convert(self, x) -> np.ndarray:
        """out[p][j] = (sum_i (x[p][i] Bh_i^-1 mod b_i) Bh_i) mod c_j for x of shape
        [batch, from_limbs, n]; returns [batch, to_limbs, n]."""
        return self._host("convert", x)

    def moddown(self, x) -> np.ndarray:
        """out[p][j] = (x[p][j] - convert(x[p][to_limbs:])[j]) B^-1 mod c_j for x of shape
        [batch, to_limbs + from_limbs, n]; returns [batch, to_limbs, n]."""
        return self._host("moddown", x)


# ---- limb-aware multi-pass RNS, 4096 < n <= 65536 (include/nttmul_rnsmp.h) ----------------------

RNSMP_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_rnsmp.so")
RNSMP_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_rnsmp.h")
RNSMP_N = (8192, 16384, 32768, 65536)


class RnsMpInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("limbs", ctypes.c_uint32),
                ("word_bits", ctypes.c_uint32), ("ndev", ctypes.c_int),
                ("scratch_mb", ctypes.c_uint32)]


def load_rnsmp_library() -> ctypes.CDLL:
    """Load lib/libnttmul_rnsmp.so (include/nttmul_rnsmp.h): the ABI and kernels of
    libnttmul_bconv.so plus the limb-aware multi-pass kernels.  The other loaders are
    unaffected."""
    return _load_limb_library(RNSMP_LIB_PATH, _bind_rns, _bind_rnsmp)


def _bind_rnsmp(lib: ctypes.CDLL) -> None:
    _bind_rns(lib, "nttmul_rnsmp", RnsMpInfo)


def rnsmp_exported_symbols() -> list:
    """Function names declared in include/nttmul_rnsmp.h."""
    return _header_symbols(RNSMP_HEADER_PATH, "nttmul_rnsmp_")


class RnsMpContext(_RnsOps):
    """nttmul_rnsmp: the moduli q_0 .. q_{L-1} of one degree n in 8192 .. 65536, every pass of
    every operation one launch over [batch, limbs, n] operands (include/nttmul_rnsmp.h; n <= 4096
    is RnsContext's).  Words are info.word_bits wide: 32 when every q_l < 2^31, 64 when every
    q_l >= 2^32.  scratch_mb: MiB per scratch buffer (0 = the library default, 512); larger
    batches run in sub-batches of whole polynomials.

    Caller memory, as for RnsContext: operands need the alignment of their word only; out may be
    the input itself for forward and inverse, c must not overlap a, b or b_hat, and partial
    overlap is never allowed; a call writes exactly batch * limbs * n words of its output and
    nothing else in caller memory, and never writes an input.

    Lifetime: one context serves any sequence of calls on any streams, from one host thread at a
    time (the scratch is handed between streams by an event).  close() does not wait for the
    streams passed to the *_device calls: synchronise them first."""
    _PREFIX = "nttmul_rnsmp"
    _NAME_CAP = 512

    def __init__(self, n: int, moduli, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False, scratch_mb: int = 0):
        self._open_limbs(load_rnsmp_library(), RnsMpInfo(), n, moduli, ndev, first_dev,
                         _flags(validate, cyclic, share_devices), scratch_mb)

    def kernel_name(self, op) -> str:
        """nttmul_rnsmp_kernel_name for op 0..3 or "multiply" / "forward" / "inverse" / "mac": the
        launch sequence, e.g. "k_rnsmp_cols_fwd<Arith64,u64,4,1> + k_rnsmp_xform<Arith64,u64,4,0>"."""
        return self._kernel_name(op)


# ---- Galois automorphisms over all RNS limbs (include/nttmul_galois.h) ---------------------------

GALOIS_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_galois.so")
GALOIS_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_galois.h")
GALOIS_OPS = ("coeff", "ntt", "ntt_many")             # nttmul_galois_kernel_name's op numbers
GALOIS_MAX_COUNT = 16


class GaloisInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("limbs", ctypes.c_uint32),
                ("word_bits", ctypes.c_uint32), ("ndev", ctypes.c_int)]


def load_galois_library() -> ctypes.CDLL:
    """Load lib/libnttmul_galois.so (include/nttmul_galois.h): the ABI and kernels of
    libnttmul_rnsmp.so plus the automorphism kernels.  The other loaders are unaffected."""
    return _load_limb_library(GALOIS_LIB_PATH, _bind_rns, _bind_galois)


def _bind_galois(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u32p = ctypes.POINTER(u32)
    _bind_handle(lib, "nttmul_galois", GaloisInfo, [ctypes.POINTER(ctypes.c_uint64), u32])
    lib.nttmul_galois_limb_info.argtypes = [vp, u32, ctypes.POINTER(Info)]
    lib.nttmul_galois_element.argtypes = [u32, ctypes.c_int64, i32, u32p]
    lib.nttmul_galois_plan.argtypes = [u32, u32, vp, vp, vp]
    lib.nttmul_galois_coeff_device.argtypes = [vp, vp, vp, u32, sz, i32, vp]
    lib.nttmul_galois_ntt_device.argtypes = [vp, vp, vp, u32, sz, i32, vp]
    lib.nttmul_galois_ntt_many_device.argtypes = [vp, vp, vp, u32p, u32, sz, i32, vp]
    lib.nttmul_galois_coeff.argtypes = [vp, vp, vp, u32, sz]
    lib.nttmul_galois_ntt.argtypes = [vp, vp, vp, u32, sz]
    lib.nttmul_galois_kernel_name.argtypes = [vp, i32, u32, ctypes.c_char_p, sz]


def galois_exported_symbols() -> list:
    """Function names declared in include/nttmul_galois.h."""
    return _header_symbols(GALOIS_HEADER_PATH, "nttmul_galois_")


def galois_element(n: int, step: int, conjugate: bool = False) -> int:
    """nttmul_galois_element: k = 5^step mod 2n (a negative step: powers of 5^-1), times 2n - 1
    when conjugate.  Host only."""
    lib = load_galois_library()
    k = ctypes.c_uint32()
    st = lib.nttmul_galois_element(n, step, int(conjugate), ctypes.byref(k))
    if st != NTTMUL_OK:
        raise NttmulError(st, lib.nttmul_strerror(st).decode())
    return k.value


def galois_plan(n: int, k: int):
    """nttmul_galois_plan: (coeff_src, coeff_neg, ntt_src), the index tables the kernels compute
    per lane: out[j] = (-in if coeff_neg[j] else in)[coeff_src[j]] in coefficient order,
    out_hat[j] = in_hat[ntt_src[j]] in NTT order.  Host only."""
    lib = load_galois_library()
    if not 0 <= n < 1 << 32 or not 0 <= k < 1 << 32:
        raise NttmulError(NTTMUL_EINVAL, lib.nttmul_strerror(NTTMUL_EINVAL).decode())
    size = n if 256 <= n <= 65536 else 1
    src, neg, hat = (np.zeros(size, dtype=np.uint32), np.zeros(size, dtype=np.uint8),
                     np.zeros(size, dtype=np.uint32))
    st = lib.nttmul_galois_plan(n, k, src.ctypes.data, neg.ctypes.data, hat.ctypes.data)
    if st != NTTMUL_OK:
        raise NttmulError(st, lib.nttmul_strerror(st).decode())
    return src, neg, hat


class GaloisContext(_LimbContext):
    """nttmul_galois: the automorphisms sigma_k : a(x) -> a(x^k) mod (x^n + 1), k odd, over the
    moduli q_0 .. q_{L-1} of one degree n in 256 .. 65536, each call one launch over
    [batch, limbs, n] operands (include/nttmul_galois.h).  coeff_*: coefficient order, canonical
    outputs; ntt_*: the bit-reversed canonical transforms RnsContext / RnsMpContext.forward write
    and mac_ntt reads as b_hat.  Words are info.word_bits wide: 32 when every q_l < 2^31, 64 when
    every q_l >= 2^32.

    Caller memory: operands need the alignment of their word only; out must not overlap the input
    (no in-place form); a call writes exactly count * batch * limbs * n words of its output and
    nothing else in caller memory, and never writes an input.

    close() does not wait for the streams passed to the *_device calls: synchronise them first."""

    _PREFIX = "nttmul_galois"
    _OPS = GALOIS_OPS
    _NAME_CAP = 128

    def __init__(self, n: int, moduli, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False):
        self._open_limbs(load_galois_library(), GaloisInfo(), n, moduli, ndev, first_dev,
                         _flags(validate, cyclic, share_devices))

    def kernel_name(self, op, count: int = 1) -> str:
        """nttmul_galois_kernel_name for op 0..2 or "coeff" / "ntt" / "ntt_many", e.g.
        "k_galois_coeff<u32,0>"."""
        return self._kernel_name(op, count)

    # device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`

    def coeff_device(self, out, x, k: int, batch: int, dev: Optional[int] = None, stream: int = 0):
        """out = sigma_k(x) in coefficient order; out, x: [batch][limbs][n]."""
        dev = self.first_dev if dev is None else dev
        args = self._dev_args((out, x), (batch,) * 2, dev)
        self._check(self._lib.nttmul_galois_coeff_device(self._h, *args, k, batch, dev,
                                                         stream or None))

    def ntt_device(self, out, x_hat, k: int, batch: int, dev: Optional[int] = None,
                   stream: int = 0):
        """out = sigma_k on bit-reversed transforms; out, x_hat: [batch][limbs][n]."""
        dev = self.first_dev if dev is None else dev
        args = self._dev_args((out, x_hat), (batch,) * 2, dev)
        self._check(self._lib.nttmul_galois_ntt_device(self._h, *args, k, batch, dev,
                                                       stream or None))

    def ntt_many_device(self, out, x_hat, ks, batch: int, dev: Optional[int] = None,
                        stream: int = 0):
        """out[c] = sigma_{ks[c]}(x_hat) for every c in one launch; out
        [len(ks)][batch][limbs][n], x_hat [batch][limbs][n]."""
        dev = self.first_dev if dev is None else dev
        ks = [int(k) for k in ks]
        args = self._dev_args((out, x_hat), (batch * len(ks), batch), dev)
        karr = (ctypes.c_uint32 * max(1, len(ks)))(*ks)
        self._check(self._lib.nttmul_galois_ntt_many_device(self._h, *args, karr, len(ks), batch,
                                                            dev, stream or None))

    # host arrays

    def _host(self, x, what):
        x = np.ascontiguousarray(x, dtype=self.io_dtype)
        if x.ndim != 3 or x.shape[-2:] != (self.limbs, self.n):
            raise ValueError(f"{what} must have shape [batch, limbs, n]")
        return x

    def coeff(self, a, k: int) -> np.ndarray:
        a = self._host(a, "a")
        out = np.empty_like(a)
        self._check(self._lib.nttmul_galois_coeff(self._h, out.ctypes.data, a.ctypes.data, k,
                                                  a.shape[0]))
        return out

    def ntt(self, a_hat, k: int) -> np.ndarray:
        a_hat = self._host(a_hat, "a_hat")
        out = np.empty_like(a_hat)
        self._check(self._lib.nttmul_galois_ntt(self._h, out.ctypes.data, a_hat.ctypes.data, k,
                                                a_hat.shape[0]))
        return out


# ---- digit ModUp and ModDown for hybrid key switching (include/nttmul_ks.h) ----------------------

KS_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_ks.so")
KS_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_ks.h")
KS_OPS = ("modup", "moddown")                         # nttmul_ks_kernel_name's op numbers


class KsInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q_limbs", ctypes.c_uint32),
                ("p_limbs", ctypes.c_uint32), ("digit_limbs", ctypes.c_uint32),
                ("digits", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int)]


def load_ks_library() -> ctypes.CDLL:
    """Load lib/libnttmul_ks.so (include/nttmul_ks.h): the ABI and kernels of libnttmul_galois.so
    plus the digit ModUp kernel.  The other loaders are unaffected."""
    return _load_limb_library(KS_LIB_PATH, _bind_rns, _bind_ks)


def _bind_ks(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64p, prm = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_Params)
    _bind_handle(lib, "nttmul_ks", KsInfo, [u64p, u32, u64p, u32, u32])
    lib.nttmul_ks_plan.argtypes = [prm, sz, u64p, u32, u64p, u32, u32] + [vp] * 6
    for op in KS_OPS:
        getattr(lib, f"nttmul_ks_{op}_device").argtypes = [vp, vp, vp, sz, i32, vp]
        getattr(lib, f"nttmul_ks_{op}").argtypes = [vp, vp, vp, sz]
    lib.nttmul_ks_kernel_name.argtypes = [vp, i32, ctypes.c_char_p, sz]


def ks_exported_symbols() -> list:
    """Function names declared in include/nttmul_ks.h."""
    return _header_symbols(KS_HEADER_PATH, "nttmul_ks_")


def _ks_bases(n, q, p, flags):
    q, p = [int(v) for v in q], [int(v) for v in p]
    prm = _Params(n, 0, 0, 1, 0, flags, 0, 0, 0, 0, 0)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    return q, p, prm, qa, pa


def ks_plan(n: int, q, p, digit_limbs: int, flags: int = 0):
    """nttmul_ks_plan, without a device: (inv, w, gadget, pinv, pw, Pinv) as lists of Python
    integers, with M = len(q) + len(p) and m over the extended basis q_0 .., p_0 ..:
    inv[i] = Dh_i^-1 mod q_i, w[i][m] = Dh_i mod m-th modulus, gadget[d][m] = the key generator's
    factor of digit d mod m-th modulus, and (pinv, pw, Pinv) = bconv_plan(n, p, q).  Raises
    NttmulError with the status nttmul_ks_create would return for these arguments."""
    lib = load_ks_library()
    q, p, prm, qa, pa = _ks_bases(n, q, p, flags)
    L, K = len(q), len(p)
    if not 0 <= digit_limbs < 1 << 32:
        raise NttmulError(NTTMUL_EINVAL, lib.nttmul_strerror(NTTMUL_EINVAL).decode())
    M = L + K
    dnum = -(-L // digit_limbs) if 0 < digit_limbs <= L else 1
    sizes = (L, L * M, dnum * M, K, K * L, L)
    t = [(ctypes.c_uint64 * max(1, k))() for k in sizes]
    st = lib.nttmul_ks_plan(ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K, digit_limbs,
                            *(ctypes.addressof(x) for x in t))
    if st != NTTMUL_OK:
        raise NttmulError(st, lib.nttmul_strerror(st).decode())
    inv, w, gadget, pinv, pw, Pinv = (list(x[:k]) for x, k in zip(t, sizes))
    rows = lambda flat, width: [flat[i:i + width] for i in range(0, len(flat), width)]
    return inv, rows(w, M), rows(gadget, M), pinv, rows(pw, L), Pinv


class KeySwitchBasis(_Handle):
    """nttmul_ks: the bases Q = q (L primes) and P = p (K primes), disjoint and of one word class,
    with digits of digit_limbs limbs of Q, for one degree n in 256 .. 65536
    (include/nttmul_ks.h).  modup maps [batch, L, n] to [batch, digits, L + K, n], the operand `a`
    of RnsContext / RnsMpContext.mac_ntt with terms = digits over the extended basis q + p;
    moddown maps [batch, L + K, n] to [batch, L, n].  Coefficient order, canonical words of
    info.word_bits.

    Caller memory: operands need the alignment of their word only; out must not overlap the
    input; modup writes exactly batch * digits * (L + K) * n words and moddown batch * L * n.

    close() does not wait for the streams passed to the *_device calls: synchronise them first."""

    _PREFIX = "nttmul_ks"
    _OPS = KS_OPS
    _NAME_CAP = 128

    def __init__(self, n: int, q, p, digit_limbs: int, ndev: int = 1, first_dev: int = 0,
                 validate: bool = False, cyclic: bool = False, share_devices: bool = False):
        q, p, prm, qa, pa = _ks_bases(n, q, p, _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev = ndev, first_dev
        info = KsInfo()
        self._open(load_ks_library(), info, prm, qa, len(q), pa, len(p), digit_limbs)
        self.n, self.word_bits = info.n, info.word_bits
        self.q_limbs, self.p_limbs = info.q_limbs, info.p_limbs
        self.digit_limbs, self.digits = info.digit_limbs, info.digits
        self.q, self.p = tuple(q), tuple(p)
        self.first_dev = first_dev

    def kernel_name(self, op) -> str:
        """nttmul_ks_kernel_name for op 0..1 or "modup" / "moddown", e.g. "k_ks_modup<u32>"."""
        return self._kernel_name(op)

    def _limbs(self, op: str):
        """(output, input) limb polynomials per batch entry."""
        ext = self.q_limbs + self.p_limbs
        return (self.digits * ext, self.q_limbs) if op == "modup" else (self.q_limbs, ext)

    # device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`

    def _device(self, op, out, x, batch, dev, stream):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch * k, self.n, self.word_bits, dev)
                for t, k in zip((out, x), self._limbs(op))]
        fn = getattr(self._lib, f"nttmul_ks_{op}_device")
        self._check(fn(self._h, *args, batch, dev, stream or None))

    def modup_device(self, out, x, batch: int, dev: Optional[int] = None, stream: int = 0):
        """x [batch][L][n] -> out [batch][digits][L + K][n]."""
        self._device("modup", out, x, batch, dev, stream)

    def moddown_device(self, out, x, batch: int, dev: Optional[int] = None, stream: int = 0):
        """x [batch][L + K][n] -> out [batch][L][n]."""
        self._device("moddown", out, x, batch, dev, stream)

    # host arrays

    def _host(self, op, x):
        out_limbs, in_limbs = self._limbs(op)
        x = np.ascontiguousarray(x, dtype=self.io_dtype)
        if x.ndim != 3 or x.shape[1:] != (in_limbs, self.n):
            raise ValueError(f"{op}: x must have shape [batch, {in_limbs}, {self.n}]")
        out = np.empty((x.shape[0], out_limbs, self.n), dtype=self.io_dtype)
        fn = getattr(self._lib, f"nttmul_ks_{op}")
        self._check(fn(self._h, out.ctypes.data, x.ctypes.data, x.shape[0]))
        return out

    def modup(self, x) -> np.ndarray:
        """out[p][d][m] = (sum over i in D_d of (x[p][i] Dh_i^-1 mod q_i) Dh_i) mod the m-th
        modulus of q + p, for x of shape [batch, L, n]; returns [batch, digits, L + K, n]."""
        out = self._host("modup", x)
        return out.reshape(out.shape[0], self.digits, self.q_limbs + self.p_limbs, self.n)

    def moddown(self, x) -> np.ndarray:
        """out[p][i] = (x[p][i] - convert(x[p][L:])[i]) P^-1 mod q_i for x of shape
        [batch, L + K, n]; returns [batch, L, n]."""
        return self._host("moddown", x)


# ---- the mac against several NTT-domain operands (include/nttmul_macn.h) -------------------------

MACN_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_macn.so")
MACN_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_macn.h")
MACN_MAX_COMPS = 2


def load_macn_library() -> ctypes.CDLL:
    """Load lib/libnttmul_macn.so (include/nttmul_macn.h): the ABI and kernels of libnttmul_ks.so
    plus the mac against several NTT-domain operands.  The other loaders are unaffected."""
    return _load_limb_library(MACN_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn)


def _bind_macn(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    for prefix in ("nttmul_rns", "nttmul_rnsmp"):
        getattr(lib, f"{prefix}_macn_ntt_device").argtypes = [vp, vp, vp, vp, sz, u32, u32, i32,
                                                              i32, vp]
        getattr(lib, f"{prefix}_macn_ntt").argtypes = [vp, vp, vp, vp, sz, u32, u32, i32]
        getattr(lib, f"{prefix}_macn_kernel_name").argtypes = [vp, u32, ctypes.c_char_p, sz]


def macn_exported_symbols() -> list:
    """Function names declared in include/nttmul_macn.h."""
    return _header_symbols(MACN_HEADER_PATH, "nttmul_rns")


class _MacnOps:
    """What RnsMacnContext and RnsMpMacnContext add to their context:
    c[p][i] = INTT(sum_t NTT(a[p][t]) o b_hat[p or shared][i][t]) for i < comps, the forward
    transforms of a shared by the components.  Component i equals mac_ntt against b_hat[..][i] bit
    for bit.

    Caller memory: operands need the alignment of their word only; c must overlap neither a nor
    b_hat; a call writes exactly batch * comps * limbs * n words of c and never writes an input."""

    def macn_kernel_name(self, comps: int) -> str:
        """<prefix>_macn_kernel_name, e.g. "k_rns_macn<Arith32P,u32,12,2>"; comps = 1 names the
        context's mac."""
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.macn_kernel_name(self._h, comps, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def macn_ntt_device(self, c, a, b_hat, batch: int, terms: int, comps: int,
                        shared: bool = True, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        a [batch][terms][limbs][n], b_hat [comps][terms][limbs][n] when shared, or
        [batch][comps][terms][limbs][n]; c [batch][comps][limbs][n]."""
        dev = self.first_dev if dev is None else dev
        args = self._dev_args((c, a, b_hat), (batch * comps, batch * terms,
                                              (1 if shared else batch) * comps * terms), dev)
        self._check(self._c.macn_ntt_device(self._h, *args, batch, terms, comps, int(shared), dev,
                                            stream or None))

    def macn_ntt(self, a, b_hat, shared: bool = True) -> np.ndarray:
        """a of shape [batch, terms, limbs, n]; b_hat of shape [comps, terms, limbs, n] when
        shared, or [batch, comps, terms, limbs, n].  Returns c of shape [batch, comps, limbs, n]."""
        a = self._host(a, 4, "a")
        b_hat = np.ascontiguousarray(b_hat, dtype=self.io_dtype)
        if a.shape[1] == 0:
            raise ValueError("terms must be > 0")
        if b_hat.ndim != (4 if shared else 5) or b_hat.shape[-3:] != a.shape[1:] \
                or (not shared and b_hat.shape[0] != a.shape[0]):
            raise ValueError("b_hat must have shape [comps, terms, limbs, n] when shared, or "
                             "[batch, comps, terms, limbs, n]")
        comps = b_hat.shape[-4]
        c = np.empty((a.shape[0], comps, self.limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.macn_ntt(self._h, c.ctypes.data, a.ctypes.data, b_hat.ctypes.data,
                                     a.shape[0], a.shape[1], comps, int(shared)))
        return c


class RnsMacnContext(_MacnOps, RnsContext):
    """An RnsContext created through lib/libnttmul_macn.so: every RnsContext method, plus
    macn_ntt (include/nttmul_macn.h), for n <= 4096."""

    def __init__(self, n: int, moduli, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False):
        self._open_limbs(load_macn_library(), RnsInfo(), n, moduli, ndev, first_dev,
                         _flags(validate, cyclic, share_devices))


class RnsMpMacnContext(_MacnOps, RnsMpContext):
    """An RnsMpContext created through lib/libnttmul_macn.so: every RnsMpContext method, plus
    macn_ntt (include/nttmul_macn.h), for n in 8192 .. 65536.  A sub-batch keeps both
    batch * terms and batch * comps polynomials within scratch_mb."""

    def __init__(self, n: int, moduli, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False, scratch_mb: int = 0):
        self._open_limbs(load_macn_library(), RnsMpInfo(), n, moduli, ndev, first_dev,
                         _flags(validate, cyclic, share_devices), scratch_mb)


# ---- hoisted rotations (include/nttmul_hoist.h) --------------------------------------------------

HOIST_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_hoist.so")
HOIST_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_hoist.h")
HOIST_MAX_ROTS = GALOIS_MAX_COUNT


def load_hoist_library() -> ctypes.CDLL:
    """Load lib/libnttmul_hoist.so (include/nttmul_hoist.h): the ABI and kernels of
    libnttmul_macn.so plus the hoisted rotations.  The other loaders are unaffected."""
    return _load_limb_library(HOIST_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn,
                              _bind_hoist)


def _bind_hoist(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u32p = ctypes.POINTER(u32)
    for prefix in ("nttmul_rns", "nttmul_rnsmp"):
        getattr(lib, f"{prefix}_hoist_ntt_device").argtypes = [vp, vp, vp, vp, u32p, u32, sz, u32,
                                                               u32, i32, vp]
        getattr(lib, f"{prefix}_hoist_ntt").argtypes = [vp, vp, vp, vp, u32p, u32, sz, u32, u32]
        getattr(lib, f"{prefix}_hoist_kernel_name").argtypes = [vp, u32, ctypes.c_char_p, sz]


def hoist_exported_symbols() -> list:
    """Function names declared in include/nttmul_hoist.h."""
    return _header_symbols(HOIST_HEADER_PATH, "nttmul_rns")


class _HoistOps:
    """What RnsHoistContext and RnsMpHoistContext add to their context:
    c[p][r][i] = INTT(sum_t sigma_{k_r}(a_hat[p][t]) o b_hat[r][i][t]) for r < rots, i < comps,
    with sigma_k the NTT-order permutation of GaloisContext.ntt, applied while a_hat is loaded.
    Result (r, i) equals mac_ntt of GaloisContext.coeff(a, k_r) against b_hat[r][i] bit for bit
    when a_hat = forward(a).

    Caller memory: operands need the alignment of their word only; c must overlap neither a_hat
    nor b_hat; a call writes exactly batch * rots * comps * limbs * n words of c and never writes
    an input."""

    def hoist_kernel_name(self, comps: int) -> str:
        """<prefix>_hoist_kernel_name, e.g. "k_rns_hoist<Arith32P,u32,12,2>"."""
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.hoist_kernel_name(self._h, comps, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def hoist_ntt_device(self, c, a_hat, b_hat, ks, batch: int, terms: int, comps: int,
                         dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        a_hat [batch][terms][limbs][n], b_hat [len(ks)][comps][terms][limbs][n],
        c [batch][len(ks)][comps][limbs][n]; ks: the rotations, host integers."""
        dev = self.first_dev if dev is None else dev
        ks = [int(k) for k in ks]
        rots = len(ks)
        args = self._dev_args((c, a_hat, b_hat), (batch * rots * comps, batch * terms,
                                                  rots * comps * terms), dev)
        karr = (ctypes.c_uint32 * max(1, rots))(*ks)
        self._check(self._c.hoist_ntt_device(self._h, *args, karr, rots, batch, terms, comps, dev,
                                             stream or None))

    def hoist_ntt(self, a_hat, b_hat, ks) -> np.ndarray:
        """a_hat of shape [batch, terms, limbs, n]; b_hat of shape [rots, comps, terms, limbs, n]
        with rots = len(ks).  Returns c of shape [batch, rots, comps, limbs, n]."""
        a_hat = self._host(a_hat, 4, "a_hat")
        b_hat = np.ascontiguousarray(b_hat, dtype=self.io_dtype)
        ks = [int(k) for k in ks]
        if a_hat.shape[1] == 0:
            raise ValueError("terms must be > 0")
        if b_hat.ndim != 5 or b_hat.shape[-3:] != a_hat.shape[1:] or b_hat.shape[0] != len(ks):
            raise ValueError("b_hat must have shape [len(ks), comps, terms, limbs, n]")
        rots, comps = b_hat.shape[:2]
        c = np.empty((a_hat.shape[0], rots, comps, self.limbs, self.n), dtype=self.io_dtype)
        karr = (ctypes.c_uint32 * max(1, rots))(*ks)
        self._check(self._c.hoist_ntt(self._h, c.ctypes.data, a_hat.ctypes.data,
                                      b_hat.ctypes.data, karr, rots, a_hat.shape[0],
                                      a_hat.shape[1], comps))
        return c


class RnsHoistContext(_HoistOps, RnsMacnContext):
    """An RnsContext created through lib/libnttmul_hoist.so: every RnsMacnContext method, plus
    hoist_ntt (include/nttmul_hoist.h), for n <= 4096."""

    def __init__(self, n: int, moduli, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False):
        self._open_limbs(load_hoist_library(), RnsInfo(), n, moduli, ndev, first_dev,
                         _flags(validate, cyclic, share_devices))


class RnsMpHoistContext(_HoistOps, RnsMpMacnContext):
    """An RnsMpContext created through lib/libnttmul_hoist.so: every RnsMpMacnContext method, plus
    hoist_ntt (include/nttmul_hoist.h), for n in 8192 .. 65536.  A sub-batch is a run of output
    units (p, r) whose units * comps polynomials stay within scratch_mb."""

    def __init__(self, n: int, moduli, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False, scratch_mb: int = 0):
        self._open_limbs(load_hoist_library(), RnsMpInfo(), n, moduli, ndev, first_dev,
                         _flags(validate, cyclic, share_devices), scratch_mb)


# ---- ModDown and rescale on NTT-domain limbs (include/nttmul_mdntt.h) ----------------------------

MDNTT_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_mdntt.so")
MDNTT_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_mdntt.h")


class MdNttInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q_limbs", ctypes.c_uint32),
                ("p_limbs", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int), ("scratch_mb", ctypes.c_uint32)]


def load_mdntt_library() -> ctypes.CDLL:
    """Load lib/libnttmul_mdntt.so (include/nttmul_mdntt.h): the ABI and kernels of
    libnttmul_hoist.so plus the NTT-domain ModDown.  The other loaders are unaffected."""
    return _load_limb_library(MDNTT_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn,
                              _bind_hoist, _bind_mdntt)


def _bind_mdntt(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64p = ctypes.POINTER(ctypes.c_uint64)
    _bind_handle(lib, "nttmul_mdntt", MdNttInfo, [u64p, u32, u64p, u32])
    lib.nttmul_mdntt_moddown_device.argtypes = [vp, vp, vp, sz, i32, vp]
    lib.nttmul_mdntt_moddown.argtypes = [vp, vp, vp, sz]
    lib.nttmul_mdntt_kernel_name.argtypes = [vp, ctypes.c_char_p, sz]


def mdntt_exported_symbols() -> list:
    """Function names declared in include/nttmul_mdntt.h."""
    return _header_symbols(MDNTT_HEADER_PATH, "nttmul_mdntt_")


class NttModDown(_Handle):
    """nttmul_mdntt: the bases Q = q (L primes) and P = p (K primes), disjoint and of one word
    class, for one degree n in 256 .. 65536 (include/nttmul_mdntt.h).  moddown maps x_hat
    [batch, L + K, n], every limb in NTT order as RnsContext / RnsMpContext.forward writes it, to
    [batch, L, n] in NTT order: forward over q of KeySwitchBasis.moddown of inverse over q + p of
    x_hat, bit for bit, with only the K limbs of p transformed back.  p = (the last prime,) is the
    CKKS rescale in its floor form (BGV's is NttPlainModDown).

    Caller memory: operands need the alignment of their word only; out must not overlap x_hat;
    a call writes exactly batch * L * n words of out and never writes x_hat.

    close() waits for the last use of the context's scratch, not for the streams passed to
    moddown_device: synchronise them first."""

    _PREFIX = "nttmul_mdntt"
    _NAME_CAP = 256

    def __init__(self, n: int, q, p, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False, scratch_mb: int = 0):
        q, p, prm, qa, pa = _ks_bases(n, q, p, _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev, prm.scratch_mb = ndev, first_dev, scratch_mb
        info = MdNttInfo()
        self._open(load_mdntt_library(), info, prm, qa, len(q), pa, len(p))
        self.n, self.word_bits = info.n, info.word_bits
        self.q_limbs, self.p_limbs = info.q_limbs, info.p_limbs
        self.q, self.p = tuple(q), tuple(p)
        self.first_dev = first_dev

    def kernel_name(self) -> str:
        """nttmul_mdntt_kernel_name: a sub-batch's kernels joined by " + ", e.g.
        "k_mdntt_inv<Arith32P,u32,12> + k_mdntt_fwd<Arith32P,u32,12>"."""
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.kernel_name(self._h, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def moddown_device(self, out, x_hat, batch: int, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        x_hat [batch][L + K][n] -> out [batch][L][n]."""
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch * k, self.n, self.word_bits, dev)
                for t, k in zip((out, x_hat), (self.q_limbs, self.q_limbs + self.p_limbs))]
        self._check(self._c.moddown_device(self._h, *args, batch, dev, stream or None))

    def moddown(self, x_hat) -> np.ndarray:
        """x_hat of shape [batch, L + K, n]; returns [batch, L, n]."""
        ext = self.q_limbs + self.p_limbs
        x_hat = np.ascontiguousarray(x_hat, dtype=self.io_dtype)
        if x_hat.ndim != 3 or x_hat.shape[1:] != (ext, self.n):
            raise ValueError(f"moddown: x_hat must have shape [batch, {ext}, {self.n}]")
        out = np.empty((x_hat.shape[0], self.q_limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.moddown(self._h, out.ctypes.data, x_hat.ctypes.data, x_hat.shape[0]))
        return out


# ---- ModUp and the key mac on NTT-domain limbs (include/nttmul_ksntt.h) --------------------------

KSNTT_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_ksntt.so")
KSNTT_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_ksntt.h")
KSNTT_OPS = ("modup", "mac")


class KsNttInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q_limbs", ctypes.c_uint32),
                ("p_limbs", ctypes.c_uint32), ("digit_limbs", ctypes.c_uint32),
                ("digits", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int), ("scratch_mb", ctypes.c_uint32)]


def load_ksntt_library() -> ctypes.CDLL:
    """Load lib/libnttmul_ksntt.so (include/nttmul_ksntt.h): the ABI and kernels of
    libnttmul_mdntt.so plus the NTT-domain ModUp and key mac.  The other loaders are unaffected."""
    return _load_limb_library(KSNTT_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn,
                              _bind_hoist, _bind_mdntt, _bind_ksntt)


def _bind_ksntt(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    _bind_handle(lib, "nttmul_ksntt", KsNttInfo, [u64p, u32, u64p, u32, u32])
    lib.nttmul_ksntt_modup_device.argtypes = [vp, vp, vp, sz, i32, vp]
    lib.nttmul_ksntt_modup.argtypes = [vp, vp, vp, sz]
    lib.nttmul_ksntt_mac_device.argtypes = [vp, vp, vp, vp, u32p, u32, sz, u32, u32, i32, vp]
    lib.nttmul_ksntt_mac.argtypes = [vp, vp, vp, vp, u32p, u32, sz, u32, u32]
    lib.nttmul_ksntt_kernel_name.argtypes = [vp, i32, u32, ctypes.c_char_p, sz]


def ksntt_exported_symbols() -> list:
    """Function names declared in include/nttmul_ksntt.h."""
    return _header_symbols(KSNTT_HEADER_PATH, "nttmul_ksntt_")


class NttKeySwitch(_Handle):
    """nttmul_ksntt: the bases Q = q (L primes) and P = p (K primes), disjoint and of one word
    class, with digits of alpha limbs of Q, for one degree n in 256 .. 65536
    (include/nttmul_ksntt.h).  Every limb of every operand is in NTT order, as RnsContext /
    RnsMpContext.forward writes it.

    modup maps x_hat [batch, L, n] to [batch, digits, L + K, n]: forward over q + p of
    KeySwitchBasis.modup of inverse over q of x_hat, bit for bit, with a digit's own limbs copied.
    mac is the hoisted mac with NTT-domain output,
    c_hat[p][r][i] = sum_t sigma_{k_r}(a_hat[p][t]) o b_hat[r][i][t], forward of hoist_ntt bit for
    bit; its c_hat is what NttModDown.moddown reads.

    Caller memory: operands need the alignment of their word only; the output must overlap no
    input; modup writes exactly batch * digits * (L + K) * n words and mac
    batch * rots * comps * (L + K) * n, and neither writes an input.

    close() waits for the last use of the context's scratch, not for the streams passed to the
    *_device calls: synchronise them first."""

    _PREFIX = "nttmul_ksntt"
    _NAME_CAP = 256

    def __init__(self, n: int, q, p, alpha: int, ndev: int = 1, first_dev: int = 0,
                 validate: bool = False, cyclic: bool = False, share_devices: bool = False,
                 scratch_mb: int = 0):
        q, p, prm, qa, pa = _ks_bases(n, q, p, _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev, prm.scratch_mb = ndev, first_dev, scratch_mb
        info = KsNttInfo()
        self._open(self._library(), info, prm, qa, len(q), pa, len(p), alpha)  # self.info
        self.n, self.word_bits = info.n, info.word_bits
        self.q_limbs, self.p_limbs = info.q_limbs, info.p_limbs
        self.limbs = info.q_limbs + info.p_limbs
        self.digit_limbs, self.digits = info.digit_limbs, info.digits
        self.scratch_mb = info.scratch_mb
        self.q, self.p = tuple(q), tuple(p)
        self.first_dev = first_dev

    @staticmethod
    def _library() -> ctypes.CDLL:
        """The library the context is created through (a subclass: a library built on it)."""
        return load_ksntt_library()

    def kernel_name(self, op, comps: int = 1) -> str:
        """nttmul_ksntt_kernel_name for op 0..1 or "modup" / "mac": a sub-batch's kernels joined
        by " + ", e.g. "k_mdntt_inv<Arith32P,u32,12> + k_ksntt_fwd<Arith32P,u32,12>" or
        "k_ksntt_mac<Arith64,u64,2>"."""
        op = KSNTT_OPS.index(op) if isinstance(op, str) else int(op)
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.kernel_name(self._h, op, comps, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def modup_device(self, up_hat, x_hat, batch: int, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        x_hat [batch][L][n] -> up_hat [batch][digits][L + K][n]."""
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch * k, self.n, self.word_bits, dev)
                for t, k in zip((up_hat, x_hat), (self.digits * self.limbs, self.q_limbs))]
        self._check(self._c.modup_device(self._h, *args, batch, dev, stream or None))

    def modup(self, x_hat) -> np.ndarray:
        """x_hat of shape [batch, L, n]; returns [batch, digits, L + K, n]."""
        x_hat = np.ascontiguousarray(x_hat, dtype=self.io_dtype)
        if x_hat.ndim != 3 or x_hat.shape[1:] != (self.q_limbs, self.n):
            raise ValueError(f"modup: x_hat must have shape [batch, {self.q_limbs}, {self.n}]")
        out = np.empty((x_hat.shape[0], self.digits, self.limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.modup(self._h, out.ctypes.data, x_hat.ctypes.data, x_hat.shape[0]))
        return out

    def mac_device(self, c_hat, a_hat, b_hat, ks, batch: int, terms: int, comps: int,
                   dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        a_hat [batch][terms][L + K][n], b_hat [len(ks)][comps][terms][L + K][n],
        c_hat [batch][len(ks)][comps][L + K][n]; ks: the rotations, host integers."""
        dev = self.first_dev if dev is None else dev
        ks = [int(k) for k in ks]
        rots = len(ks)
        polys = (batch * rots * comps, batch * terms, rots * comps * terms)
        args = [_dev_arg(t, k * self.limbs, self.n, self.word_bits, dev)
                for t, k in zip((c_hat, a_hat, b_hat), polys)]
        karr = (ctypes.c_uint32 * max(1, rots))(*ks)
        self._check(self._c.mac_device(self._h, *args, karr, rots, batch, terms, comps, dev,
                                       stream or None))

    def mac(self, a_hat, b_hat, ks) -> np.ndarray:
        """a_hat of shape [batch, terms, L + K, n]; b_hat of shape [rots, comps, terms, L + K, n]
        with rots = len(ks).  Returns c_hat of shape [batch, rots, comps, L + K, n]."""
        a_hat = np.ascontiguousarray(a_hat, dtype=self.io_dtype)
        b_hat = np.ascontiguousarray(b_hat, dtype=self.io_dtype)
        ks = [int(k) for k in ks]
        if a_hat.ndim != 4 or a_hat.shape[2:] != (self.limbs, self.n) or a_hat.shape[1] == 0:
            raise ValueError(f"mac: a_hat must have shape [batch, terms > 0, {self.limbs}, {self.n}]")
        if b_hat.ndim != 5 or b_hat.shape[-3:] != a_hat.shape[1:] or b_hat.shape[0] != len(ks):
            raise ValueError("mac: b_hat must have shape [len(ks), comps, terms, L + K, n]")
        rots, comps = b_hat.shape[:2]
        c = np.empty((a_hat.shape[0], rots, comps, self.limbs, self.n), dtype=self.io_dtype)
        karr = (ctypes.c_uint32 * max(1, rots))(*ks)
        self._check(self._c.mac(self._h, c.ctypes.data, a_hat.ctypes.data, b_hat.ctypes.data, karr,
                                rots, a_hat.shape[0], a_hat.shape[1], comps))
        return c


# ---- the weighted sum of rotations before ModDown (include/nttmul_lintrans.h) --------------------

LINTRANS_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_lintrans.so")
LINTRANS_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_lintrans.h")


class LinTransInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q_limbs", ctypes.c_uint32),
                ("p_limbs", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int)]


def load_lintrans_library(path: str = LINTRANS_LIB_PATH) -> ctypes.CDLL:
    """Load lib/libnttmul_lintrans.so (include/nttmul_lintrans.h): the ABI and kernels of
    libnttmul_ksntt.so plus the weighted sum of rotations.  The other loaders are unaffected."""
    return _load_limb_library(path, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn, _bind_hoist,
                              _bind_mdntt, _bind_ksntt, _bind_lintrans)


def _bind_lintrans(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    _bind_handle(lib, "nttmul_lintrans", LinTransInfo, [u64p, u32, u64p, u32])
    lib.nttmul_lintrans_apply_device.argtypes = [vp, vp, vp, vp, vp, vp, u32p, u32, sz, u32, u32,
                                                 i32, vp]
    lib.nttmul_lintrans_apply.argtypes = [vp, vp, vp, vp, vp, vp, u32p, u32, sz, u32, u32]
    lib.nttmul_lintrans_kernel_name.argtypes = [vp, u32, i32, ctypes.c_char_p, sz]


def lintrans_exported_symbols() -> list:
    """Function names declared in include/nttmul_lintrans.h."""
    return _header_symbols(LINTRANS_HEADER_PATH, "nttmul_lintrans_")


class NttLinTrans(_Handle):
    """nttmul_lintrans: the bases Q = q (L primes) and P = p (K primes), disjoint and of one word
    class, for one degree n in 256 .. 65536 (include/nttmul_lintrans.h).  Every limb of every
    operand is in NTT order, as RnsContext / RnsMpContext.forward writes it.

    apply is the weighted sum of rotations in Q u P,
    c_hat[p][i] = sum_r w_hat[r] o (sum_t sigma_{k_r}(a_hat[p][t]) o b_hat[r][i][t]
                                    + [i = 0] P sigma_{k_r}(c0_hat[p])),
    one launch for any number of rotations.  w_hat = None: every weight is 1.  c0_hat = None: that
    term is dropped.  Its c_hat is what NttModDown.moddown reads with batch * comps polynomials.

    Caller memory: operands need the alignment of their word only; the output must overlap no
    input; apply writes exactly batch * comps * (L + K) * n words and never writes an input."""

    _PREFIX = "nttmul_lintrans"
    _NAME_CAP = 256

    def __init__(self, n: int, q, p, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False, lib_path: Optional[str] = None):
        q, p, prm, qa, pa = _ks_bases(n, q, p, _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev = ndev, first_dev
        info = LinTransInfo()
        lib = load_lintrans_library(lib_path) if lib_path else self._library()
        self._open(lib, info, prm, qa, len(q), pa, len(p))  # self.info
        self.n, self.word_bits = info.n, info.word_bits
        self.q_limbs, self.p_limbs = info.q_limbs, info.p_limbs
        self.limbs = info.q_limbs + info.p_limbs
        self.q, self.p = tuple(q), tuple(p)
        self.first_dev = first_dev

    @staticmethod
    def _library() -> ctypes.CDLL:
        """The library the context is created through (a subclass: a library built on it)."""
        return load_lintrans_library()

    def kernel_name(self, comps: int = 1, weighted: bool = False) -> str:
        """nttmul_lintrans_kernel_name, e.g. "k_lintrans<Arith64,u64,2,1>"."""
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.kernel_name(self._h, comps, int(bool(weighted)), buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def apply_device(self, c_hat, a_hat, b_hat, k, batch: int, terms: int, comps: int,
                     w_hat=None, c0_hat=None, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        a_hat [batch][terms][L + K][n], b_hat [len(k)][comps][terms][L + K][n],
        w_hat [len(k)][L + K][n] or None, c0_hat [batch][L][n] or None,
        c_hat [batch][comps][L + K][n]; k: the rotations, host integers."""
        dev = self.first_dev if dev is None else dev
        k = [int(x) for x in k]
        rots = len(k)
        polys = (batch * comps, batch * terms, rots * comps * terms)
        args = [_dev_arg(t, m * self.limbs, self.n, self.word_bits, dev)
                for t, m in zip((c_hat, a_hat, b_hat), polys)]
        wp = None if w_hat is None else _dev_arg(w_hat, rots * self.limbs, self.n,
                                                 self.word_bits, dev)
        zp = None if c0_hat is None else _dev_arg(c0_hat, batch * self.q_limbs, self.n,
                                                  self.word_bits, dev)
        karr = (ctypes.c_uint32 * max(1, rots))(*k)
        self._check(self._c.apply_device(self._h, *args, wp, zp, karr, rots, batch, terms, comps,
                                         dev, stream or None))

    def apply(self, a_hat, b_hat, k, w_hat=None, c0_hat=None) -> np.ndarray:
        """a_hat of shape [batch, terms, L + K, n]; b_hat of shape [rots, comps, terms, L + K, n]
        with rots = len(k); w_hat of shape [rots, L + K, n] or None; c0_hat of shape [batch, L, n]
        or None.  Returns c_hat of shape [batch, comps, L + K, n]."""
        a_hat = np.ascontiguousarray(a_hat, dtype=self.io_dtype)
        b_hat = np.ascontiguousarray(b_hat, dtype=self.io_dtype)
        k = [int(x) for x in k]
        if a_hat.ndim != 4 or a_hat.shape[2:] != (self.limbs, self.n) or a_hat.shape[1] == 0:
            raise ValueError(f"apply: a_hat must have shape [batch, terms > 0, {self.limbs}, {self.n}]")
        if b_hat.ndim != 5 or b_hat.shape[-3:] != a_hat.shape[1:] or b_hat.shape[0] != len(k):
            raise ValueError("apply: b_hat must have shape [len(k), comps, terms, L + K, n]")
        rots, comps = b_hat.shape[:2]
        batch = a_hat.shape[0]
        wp = zp = None
        if w_hat is not None:
            w_hat = np.ascontiguousarray(w_hat, dtype=self.io_dtype)
            if w_hat.shape != (rots, self.limbs, self.n):
                raise ValueError("apply: w_hat must have shape [len(k), L + K, n]")
            wp = w_hat.ctypes.data
        if c0_hat is not None:
            c0_hat = np.ascontiguousarray(c0_hat, dtype=self.io_dtype)
            if c0_hat.shape != (batch, self.q_limbs, self.n):
                raise ValueError("apply: c0_hat must have shape [batch, L, n]")
            zp = c0_hat.ctypes.data
        c = np.empty((batch, comps, self.limbs, self.n), dtype=self.io_dtype)
        karr = (ctypes.c_uint32 * max(1, rots))(*k)
        self._check(self._c.apply(self._h, c.ctypes.data, a_hat.ctypes.data, b_hat.ctypes.data,
                                  wp, zp, karr, rots, batch, a_hat.shape[1], comps))
        return c


# ---- the product of two ciphertexts on NTT-domain limbs (include/nttmul_ctmul.h) -----------------

CTMUL_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_ctmul.so")
CTMUL_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_ctmul.h")
CTMUL_OPS = ("high", "relin")


class CtMulInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q_limbs", ctypes.c_uint32),
                ("p_limbs", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int)]


def load_ctmul_library(path: str = CTMUL_LIB_PATH) -> ctypes.CDLL:
    """Load lib/libnttmul_ctmul.so (include/nttmul_ctmul.h): the ABI and kernels of
    libnttmul_lintrans.so plus the ciphertext product.  The other loaders are unaffected."""
    return _load_limb_library(path, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn, _bind_hoist,
                              _bind_mdntt, _bind_ksntt, _bind_lintrans, _bind_ctmul)


def _bind_ctmul(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64p = ctypes.POINTER(ctypes.c_uint64)
    _bind_handle(lib, "nttmul_ctmul", CtMulInfo, [u64p, u32, u64p, u32])
    lib.nttmul_ctmul_high_device.argtypes = [vp, vp, vp, vp, sz, u32, i32, vp]
    lib.nttmul_ctmul_high.argtypes = [vp, vp, vp, vp, sz, u32]
    lib.nttmul_ctmul_relin_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, u32, u32, i32, vp]
    lib.nttmul_ctmul_relin.argtypes = [vp, vp, vp, vp, vp, vp, sz, u32, u32]
    lib.nttmul_ctmul_kernel_name.argtypes = [vp, i32, ctypes.c_char_p, sz]


def ctmul_exported_symbols() -> list:
    """Function names declared in include/nttmul_ctmul.h."""
    return _header_symbols(CTMUL_HEADER_PATH, "nttmul_ctmul_")


class NttCtMul(_Handle):
    """nttmul_ctmul: the bases Q = q (L primes) and P = p (K primes), disjoint and of one word
    class, for one degree n in 256 .. 65536 (include/nttmul_ctmul.h).  Every limb of every
    operand is in NTT order, as RnsContext / RnsMpContext.forward writes it.  x_hat and y_hat hold
    `pairs` ciphertexts (c_0, c_1) over Q per batch entry, [batch, pairs, 2, L, n]; the same array
    for both is the square.

    high is the s^2 term, d2_hat[p] = sum_s x_hat[p][s][1] o y_hat[p][s][1], what
    NttKeySwitch.modup reads.  relin is its key switch plus P (d0, d1) in Q u P,
    c_hat[p][i] = sum_t up_hat[p][t] o key_hat[i][t] + P e_i[p], with e_0 = sum_s x[s][0] o y[s][0]
    and e_1 = sum_s (x[s][0] o y[s][1] + x[s][1] o y[s][0]); its c_hat is what NttModDown.moddown
    reads with batch * 2 polynomials.

    Caller memory: operands need the alignment of their word only; the output must overlap no
    input (inputs may alias each other); high writes exactly batch * L * n words and relin
    batch * 2 * (L + K) * n, and neither writes an input."""

    _PREFIX = "nttmul_ctmul"
    _NAME_CAP = 256

    def __init__(self, n: int, q, p, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False, lib_path: Optional[str] = None):
        q, p, prm, qa, pa = _ks_bases(n, q, p, _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev = ndev, first_dev
        info = CtMulInfo()
        lib = load_ctmul_library(lib_path) if lib_path else self._library()
        self._open(lib, info, prm, qa, len(q), pa, len(p))  # self.info
        self.n, self.word_bits = info.n, info.word_bits
        self.q_limbs, self.p_limbs = info.q_limbs, info.p_limbs
        self.limbs = info.q_limbs + info.p_limbs
        self.q, self.p = tuple(q), tuple(p)
        self.first_dev = first_dev

    @staticmethod
    def _library() -> ctypes.CDLL:
        """The library the context is created through (a subclass: a library built on it)."""
        return load_ctmul_library()

    def kernel_name(self, op) -> str:
        """nttmul_ctmul_kernel_name for op 0..1 or "high" / "relin", e.g.
        "k_ctmul_relin<Arith64,u64>"."""
        op = CTMUL_OPS.index(op) if isinstance(op, str) else int(op)
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.kernel_name(self._h, op, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def _pair_args(self, x_hat, y_hat, batch, pairs, dev):
        polys = batch * pairs * 2 * self.q_limbs
        xp = _dev_arg(x_hat, polys, self.n, self.word_bits, dev)
        yp = xp if y_hat is x_hat else _dev_arg(y_hat, polys, self.n, self.word_bits, dev)
        return xp, yp

    def high_device(self, d2_hat, x_hat, y_hat, batch: int, pairs: int,
                    dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        x_hat, y_hat [batch][pairs][2][L][n] -> d2_hat [batch][L][n]."""
        dev = self.first_dev if dev is None else dev
        out = _dev_arg(d2_hat, batch * self.q_limbs, self.n, self.word_bits, dev)
        xp, yp = self._pair_args(x_hat, y_hat, batch, pairs, dev)
        self._check(self._c.high_device(self._h, out, xp, yp, batch, pairs, dev, stream or None))

    def relin_device(self, c_hat, up_hat, key_hat, x_hat, y_hat, batch: int, pairs: int,
                     terms: int, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        up_hat [batch][terms][L + K][n], key_hat [2][terms][L + K][n], x_hat and y_hat
        [batch][pairs][2][L][n] -> c_hat [batch][2][L + K][n]."""
        dev = self.first_dev if dev is None else dev
        polys = (batch * 2, batch * terms, 2 * terms)
        args = [_dev_arg(t, m * self.limbs, self.n, self.word_bits, dev)
                for t, m in zip((c_hat, up_hat, key_hat), polys)]
        xp, yp = self._pair_args(x_hat, y_hat, batch, pairs, dev)
        self._check(self._c.relin_device(self._h, *args, xp, yp, batch, pairs, terms, dev,
                                         stream or None))

    def _host_pairs(self, what, x_hat, y_hat):
        same = y_hat is x_hat
        x_hat = np.ascontiguousarray(x_hat, dtype=self.io_dtype)
        y_hat = x_hat if same else np.ascontiguousarray(y_hat, dtype=self.io_dtype)
        if x_hat.ndim != 5 or x_hat.shape[2:] != (2, self.q_limbs, self.n) or x_hat.shape[1] == 0:
            raise ValueError(f"{what}: x_hat must have shape [batch, pairs > 0, 2, "
                             f"{self.q_limbs}, {self.n}]")
        if y_hat.shape != x_hat.shape:
            raise ValueError(f"{what}: y_hat must have x_hat's shape")
        return x_hat, y_hat

    def high(self, x_hat, y_hat) -> np.ndarray:
        """x_hat, y_hat of shape [batch, pairs, 2, L, n] (the same array: the square).  Returns
        d2_hat of shape [batch, L, n]."""
        x_hat, y_hat = self._host_pairs("high", x_hat, y_hat)
        batch, pairs = x_hat.shape[:2]
        d2 = np.empty((batch, self.q_limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.high(self._h, d2.ctypes.data, x_hat.ctypes.data, y_hat.ctypes.data,
                                 batch, pairs))
        return d2

    def relin(self, up_hat, key_hat, x_hat, y_hat) -> np.ndarray:
        """up_hat of shape [batch, terms, L + K, n]; key_hat of shape [2, terms, L + K, n]; x_hat,
        y_hat of shape [batch, pairs, 2, L, n].  Returns c_hat of shape [batch, 2, L + K, n]."""
        up_hat = np.ascontiguousarray(up_hat, dtype=self.io_dtype)
        key_hat = np.ascontiguousarray(key_hat, dtype=self.io_dtype)
        x_hat, y_hat = self._host_pairs("relin", x_hat, y_hat)
        if up_hat.ndim != 4 or up_hat.shape[2:] != (self.limbs, self.n) or up_hat.shape[1] == 0:
            raise ValueError(f"relin: up_hat must have shape [batch, terms > 0, {self.limbs}, "
                             f"{self.n}]")
        if key_hat.shape != (2,) + up_hat.shape[1:]:
            raise ValueError("relin: key_hat must have shape [2, terms, L + K, n]")
        if x_hat.shape[0] != up_hat.shape[0]:
            raise ValueError("relin: x_hat and up_hat must have the same batch")
        batch, pairs = x_hat.shape[:2]
        c = np.empty((batch, 2, self.limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.relin(self._h, c.ctypes.data, up_hat.ctypes.data, key_hat.ctypes.data,
                                  x_hat.ctypes.data, y_hat.ctypes.data, batch, pairs,
                                  up_hat.shape[1]))
        return c


# ---- exact base extension and rounded ModDown (include/nttmul_xconv.h) ---------------------------

XCONV_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_xconv.so")
XCONV_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_xconv.h")
XCONV_OPS = ("extend", "moddown")


class XConvInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q_limbs", ctypes.c_uint32),
                ("p_limbs", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int), ("scratch_mb", ctypes.c_uint32),
                ("band_log2", ctypes.c_uint32), ("scale", ctypes.c_uint64)]


def load_xconv_library() -> ctypes.CDLL:
    """Load lib/libnttmul_xconv.so (include/nttmul_xconv.h): the ABI and kernels of
    libnttmul_ctmul.so plus the exact base extension and the rounded ModDown.  The other loaders
    are unaffected."""
    return _load_limb_library(XCONV_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn,
                              _bind_hoist, _bind_mdntt, _bind_ksntt, _bind_lintrans, _bind_ctmul,
                              _bind_xconv)


def _bind_xconv(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64, u64p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    _bind_handle(lib, "nttmul_xconv", XConvInfo, [u64p, u32, u64p, u32, u64])
    for op in XCONV_OPS:
        getattr(lib, f"nttmul_xconv_{op}_device").argtypes = [vp, vp, vp, sz, i32, vp]
        getattr(lib, f"nttmul_xconv_{op}").argtypes = [vp, vp, vp, sz]
    lib.nttmul_xconv_plan.argtypes = [ctypes.POINTER(_Params), sz, u64p, u32, u64p, u32, u64,
                                      vp, vp, vp, vp]
    lib.nttmul_xconv_kernel_name.argtypes = [vp, i32, ctypes.c_char_p, sz]


def xconv_exported_symbols() -> list:
    """Function names declared in include/nttmul_xconv.h."""
    return _header_symbols(XCONV_HEADER_PATH, "nttmul_xconv_")


def xconv_plan(n: int, q, p, scale: int = 1, flags: int = 0):
    """nttmul_xconv_plan, without a device: (yscale, w_ext, w_md, v) as lists of Python integers.
    yscale[j] = t Ph_j^-1 mod p_j; w_ext[j][l] = Ph_j mod q_l for j < K and w_ext[K][l] = -P mod
    q_l; w_md[j][l] = Ph_j t^-1 mod q_l and w_md[K][l] = -P t^-1 mod q_l; v[l] = t P^-1 mod q_l.
    Raises NttmulError with the status nttmul_xconv_create would return for these arguments before
    any device access."""
    lib = load_xconv_library()
    q, p, prm, qa, pa = _ks_bases(n, q, p, flags)
    L, K = len(q), len(p)
    if not 0 <= scale < 1 << 64:
        raise NttmulError(NTTMUL_EINVAL, lib.nttmul_strerror(NTTMUL_EINVAL).decode())
    sizes = (K, (K + 1) * L, (K + 1) * L, L)
    t = [(ctypes.c_uint64 * max(1, k))() for k in sizes]
    st = lib.nttmul_xconv_plan(ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K, scale,
                               *(ctypes.addressof(x) for x in t))
    if st != NTTMUL_OK:
        raise NttmulError(st, lib.nttmul_strerror(st).decode())
    yscale, w_ext, w_md, v = (list(x[:k]) for x, k in zip(t, sizes))
    rows = lambda flat, width: [flat[i:i + width] for i in range(0, len(flat), width)]
    return yscale, rows(w_ext, L), rows(w_md, L), v


class NttExactConv(_Handle):
    """nttmul_xconv: the bases Q = q (L primes) and P = p (K primes), disjoint and of one word
    class, and a scale t, for one degree n in 256 .. 65536 (include/nttmul_xconv.h).  Every limb
    of every operand is in NTT order, as RnsContext / RnsMpContext.forward writes it.

    extend maps p_hat [batch, K, n] over P to [batch, L, n] over Q: the centred representative in
    [-(P-1)/2, (P-1)/2] of t * (the input's CRT value) mod P, reduced modulo each q_l.  scale = 1
    is the exact basis extension, K = 1 is ModRaise.  moddown maps x_hat [batch, L + K, n] to
    [batch, L, n]: round(t X / P) mod q_l for the CRT value X over Q u P; scale = 1 is the rounded
    ModDown (NttModDown.moddown floors).

    Both are exact for every coefficient with |frac(phi) - 1/2| > eps, phi = sum_j y_j / p_j and
    eps = K * 2**-info.band_log2 (self.eps as a Fraction); inside that band the result is the exact
    value or its neighbour by one P, the same in every limb.

    Caller memory: operands need the alignment of their word only; out must not overlap the
    input; a call writes exactly batch * L * n words of out and never writes the input.

    close() waits for the last use of the context's scratch, not for the streams passed to the
    *_device calls: synchronise them first."""

    _PREFIX = "nttmul_xconv"
    _OPS = XCONV_OPS
    _NAME_CAP = 256

    def __init__(self, n: int, q, p, scale: int = 1, ndev: int = 1, first_dev: int = 0,
                 validate: bool = False, cyclic: bool = False, share_devices: bool = False,
                 scratch_mb: int = 0):
        q, p, prm, qa, pa = _ks_bases(n, q, p, _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev, prm.scratch_mb = ndev, first_dev, scratch_mb
        info = XConvInfo()
        lib = load_xconv_library()
        if not 0 <= scale < 1 << 64:
            raise NttmulError(NTTMUL_EINVAL, lib.nttmul_strerror(NTTMUL_EINVAL).decode())
        self._open(lib, info, prm, qa, len(q), pa, len(p), scale)
        self.n, self.word_bits = info.n, info.word_bits
        self.q_limbs, self.p_limbs = info.q_limbs, info.p_limbs
        self.q, self.p, self.scale = tuple(q), tuple(p), info.scale
        self.band_log2 = info.band_log2
        self.first_dev = first_dev

    @property
    def eps(self):
        """The guard band of a, K 2^-band_log2, as a fractions.Fraction."""
        from fractions import Fraction
        return Fraction(self.p_limbs, 1 << self.band_log2)

    def kernel_name(self, op) -> str:
        """nttmul_xconv_kernel_name for op 0..1 or "extend" / "moddown", e.g.
        "k_mdntt_inv<Arith32P,u32,12> + k_xconv_fwd<Arith32P,u32,12,1>"."""
        return self._kernel_name(op)

    def _in_limbs(self, op: str) -> int:
        return self.p_limbs if op == "extend" else self.q_limbs + self.p_limbs

    def _device(self, op, out, src, batch, dev, stream):
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(t, batch * k, self.n, self.word_bits, dev)
                for t, k in zip((out, src), (self.q_limbs, self._in_limbs(op)))]
        self._check(getattr(self._c, f"{op}_device")(self._h, *args, batch, dev, stream or None))

    def _host(self, op, src) -> np.ndarray:
        limbs = self._in_limbs(op)
        src = np.ascontiguousarray(src, dtype=self.io_dtype)
        if src.ndim != 3 or src.shape[1:] != (limbs, self.n):
            raise ValueError(f"{op}: the input must have shape [batch, {limbs}, {self.n}]")
        out = np.empty((src.shape[0], self.q_limbs, self.n), dtype=self.io_dtype)
        self._check(getattr(self._c, op)(self._h, out.ctypes.data, src.ctypes.data, src.shape[0]))
        return out

    def extend_device(self, out, p_hat, batch: int, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        p_hat [batch][K][n] -> out [batch][L][n]."""
        self._device("extend", out, p_hat, batch, dev, stream)

    def moddown_device(self, out, x_hat, batch: int, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        x_hat [batch][L + K][n] -> out [batch][L][n]."""
        self._device("moddown", out, x_hat, batch, dev, stream)

    def extend(self, p_hat) -> np.ndarray:
        """p_hat of shape [batch, K, n]; returns [batch, L, n]."""
        return self._host("extend", p_hat)

    def moddown(self, x_hat) -> np.ndarray:
        """x_hat of shape [batch, L + K, n]; returns [batch, L, n]."""
        return self._host("moddown", x_hat)


# ---- level views of the key operands (include/nttmul_level.h) ------------------------------------

LEVEL_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_level.so")
LEVEL_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_level.h")
LEVEL_OPS = ("mac", "lintrans", "relin")


class LevelView(ctypes.Structure):
    """nttmul_level_view: the limbs of Q and the terms the viewed operand was made with."""
    _fields_ = [("top_q_limbs", ctypes.c_uint32), ("top_terms", ctypes.c_uint32)]


def load_level_library() -> ctypes.CDLL:
    """Load lib/libnttmul_level.so (include/nttmul_level.h): the ABI and kernels of
    libnttmul_xconv.so plus the view forms of mac, apply and relin.  The other loaders are
    unaffected."""
    return _load_limb_library(LEVEL_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn,
                              _bind_hoist, _bind_mdntt, _bind_ksntt, _bind_lintrans, _bind_ctmul,
                              _bind_xconv, _bind_level)


def _bind_level(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u32p, view = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(LevelView)
    lib.nttmul_ksntt_mac_view_device.argtypes = [vp, vp, vp, vp, u32p, u32, sz, u32, u32, view,
                                                 i32, vp]
    lib.nttmul_ksntt_mac_view.argtypes = [vp, vp, vp, vp, u32p, u32, sz, u32, u32, view]
    lib.nttmul_lintrans_apply_view_device.argtypes = [vp, vp, vp, vp, vp, vp, u32p, u32, sz, u32,
                                                      u32, view, i32, vp]
    lib.nttmul_lintrans_apply_view.argtypes = [vp, vp, vp, vp, vp, vp, u32p, u32, sz, u32, u32,
                                               view]
    lib.nttmul_ctmul_relin_view_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, u32, u32, view,
                                                   i32, vp]
    lib.nttmul_ctmul_relin_view.argtypes = [vp, vp, vp, vp, vp, vp, sz, u32, u32, view]
    lib.nttmul_level_kernel_name.argtypes = [i32, u32, u32, u32, i32, ctypes.c_char_p, sz]


def level_exported_symbols() -> list:
    """Function names declared in include/nttmul_level.h."""
    return _header_symbols(LEVEL_HEADER_PATH, "nttmul_")


def level_kernel_name(op, logn: int, word_bits: int, comps: int = 1,
                      weighted: bool = False) -> str:
    """nttmul_level_kernel_name for op 0..2 or "mac" / "lintrans" / "relin", e.g.
    "k_level_lintrans<Arith64,u64,2,1>".  Needs no context and no device."""
    lib = load_level_library()
    op = LEVEL_OPS.index(op) if isinstance(op, str) else int(op)
    buf = ctypes.create_string_buffer(256)
    st = lib.nttmul_level_kernel_name(op, logn, word_bits, comps, int(bool(weighted)), buf,
                                      len(buf))
    if st < 0:
        raise NttmulError(st, lib.nttmul_strerror(st).decode())
    return buf.value.decode()


def _level_view(view) -> LevelView:
    top_q_limbs, top_terms = view
    return LevelView(int(top_q_limbs), int(top_terms))


def _viewed_host(x, dtype, ndim: int, tail: tuple, what: str) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=dtype)
    if x.ndim != ndim or x.shape[-len(tail):] != tail:
        raise ValueError(f"{what} must have shape [..., {', '.join(map(str, tail))}]")
    return x


class NttLevelKeySwitch(NttKeySwitch):
    """An NttKeySwitch created through lib/libnttmul_level.so: every NttKeySwitch method, and
    mac / mac_device take view=(top_q_limbs, top_terms) (include/nttmul_level.h): b_hat is then
    the key made for the chain's top level, [rots][comps][top_terms][top_q_limbs + K][n], and the
    context, whose q must be the first L primes of that chain, reads its own limbs and terms of
    it.  view=None is the dense call."""

    @staticmethod
    def _library() -> ctypes.CDLL:
        return load_level_library()

    def mac_device(self, c_hat, a_hat, b_hat, ks, batch: int, terms: int, comps: int,
                   dev: Optional[int] = None, stream: int = 0, view=None):
        if view is None:
            return super().mac_device(c_hat, a_hat, b_hat, ks, batch, terms, comps, dev, stream)
        dev = self.first_dev if dev is None else dev
        v = _level_view(view)
        ks = [int(k) for k in ks]
        rots = len(ks)
        args = [_dev_arg(t, k, self.n, self.word_bits, dev)
                for t, k in zip((c_hat, a_hat, b_hat),
                                (batch * rots * comps * self.limbs, batch * terms * self.limbs,
                                 rots * comps * v.top_terms * (v.top_q_limbs + self.p_limbs)))]
        karr = (ctypes.c_uint32 * max(1, rots))(*ks)
        self._check(self._c.mac_view_device(self._h, *args, karr, rots, batch, terms, comps,
                                            ctypes.byref(v), dev, stream or None))

    def mac(self, a_hat, b_hat, ks, view=None) -> np.ndarray:
        """view given: b_hat of shape [rots, comps, top_terms, top_q_limbs + K, n]; the call's
        terms are a_hat's."""
        if view is None:
            return super().mac(a_hat, b_hat, ks)
        v = _level_view(view)
        a_hat = np.ascontiguousarray(a_hat, dtype=self.io_dtype)
        ks = [int(k) for k in ks]
        if a_hat.ndim != 4 or a_hat.shape[2:] != (self.limbs, self.n) or a_hat.shape[1] == 0:
            raise ValueError(f"mac: a_hat must have shape [batch, terms > 0, {self.limbs}, {self.n}]")
        b_hat = _viewed_host(b_hat, self.io_dtype, 5,
                             (v.top_terms, v.top_q_limbs + self.p_limbs, self.n), "mac: b_hat")
        if b_hat.shape[0] != len(ks):
            raise ValueError("mac: b_hat must have len(ks) rotations")
        rots, comps = b_hat.shape[:2]
        c = np.empty((a_hat.shape[0], rots, comps, self.limbs, self.n), dtype=self.io_dtype)
        karr = (ctypes.c_uint32 * max(1, rots))(*ks)
        self._check(self._c.mac_view(self._h, c.ctypes.data, a_hat.ctypes.data, b_hat.ctypes.data,
                                     karr, rots, a_hat.shape[0], a_hat.shape[1], comps,
                                     ctypes.byref(v)))
        return c


class NttLevelLinTrans(NttLinTrans):
    """An NttLinTrans created through lib/libnttmul_level.so: every NttLinTrans method, and
    apply / apply_device take view=(top_q_limbs, top_terms): b_hat is then
    [rots][comps][top_terms][top_q_limbs + K][n] and w_hat, when given,
    [rots][top_q_limbs + K][n], both made for the chain's top level.  view=None is the dense
    call."""

    @staticmethod
    def _library() -> ctypes.CDLL:
        return load_level_library()

    def apply_device(self, c_hat, a_hat, b_hat, k, batch: int, terms: int, comps: int,
                     w_hat=None, c0_hat=None, dev: Optional[int] = None, stream: int = 0,
                     view=None):
        if view is None:
            return super().apply_device(c_hat, a_hat, b_hat, k, batch, terms, comps, w_hat,
                                        c0_hat, dev, stream)
        dev = self.first_dev if dev is None else dev
        v = _level_view(view)
        k = [int(x) for x in k]
        rots = len(k)
        top = v.top_q_limbs + self.p_limbs
        args = [_dev_arg(t, m, self.n, self.word_bits, dev)
                for t, m in zip((c_hat, a_hat, b_hat),
                                (batch * comps * self.limbs, batch * terms * self.limbs,
                                 rots * comps * v.top_terms * top))]
        wp = None if w_hat is None else _dev_arg(w_hat, rots * top, self.n, self.word_bits, dev)
        zp = None if c0_hat is None else _dev_arg(c0_hat, batch * self.q_limbs, self.n,
                                                  self.word_bits, dev)
        karr = (ctypes.c_uint32 * max(1, rots))(*k)
        self._check(self._c.apply_view_device(self._h, *args, wp, zp, karr, rots, batch, terms,
                                              comps, ctypes.byref(v), dev, stream or None))

    def apply(self, a_hat, b_hat, k, w_hat=None, c0_hat=None, view=None) -> np.ndarray:
        """view given: b_hat of shape [rots, comps, top_terms, top_q_limbs + K, n] and w_hat of
        shape [rots, top_q_limbs + K, n] or None; the call's terms are a_hat's."""
        if view is None:
            return super().apply(a_hat, b_hat, k, w_hat, c0_hat)
        v = _level_view(view)
        top = v.top_q_limbs + self.p_limbs
        a_hat = np.ascontiguousarray(a_hat, dtype=self.io_dtype)
        k = [int(x) for x in k]
        if a_hat.ndim != 4 or a_hat.shape[2:] != (self.limbs, self.n) or a_hat.shape[1] == 0:
            raise ValueError(f"apply: a_hat must have shape [batch, terms > 0, {self.limbs}, {self.n}]")
        b_hat = _viewed_host(b_hat, self.io_dtype, 5, (v.top_terms, top, self.n), "apply: b_hat")
        if b_hat.shape[0] != len(k):
            raise ValueError("apply: b_hat must have len(k) rotations")
        rots, comps = b_hat.shape[:2]
        batch = a_hat.shape[0]
        wp = zp = None
        if w_hat is not None:
            w_hat = _viewed_host(w_hat, self.io_dtype, 3, (rots, top, self.n), "apply: w_hat")
            wp = w_hat.ctypes.data
        if c0_hat is not None:
            c0_hat = np.ascontiguousarray(c0_hat, dtype=self.io_dtype)
            if c0_hat.shape != (batch, self.q_limbs, self.n):
                raise ValueError("apply: c0_hat must have shape [batch, L, n]")
            zp = c0_hat.ctypes.data
        c = np.empty((batch, comps, self.limbs, self.n), dtype=self.io_dtype)
        karr = (ctypes.c_uint32 * max(1, rots))(*k)
        self._check(self._c.apply_view(self._h, c.ctypes.data, a_hat.ctypes.data,
                                       b_hat.ctypes.data, wp, zp, karr, rots, batch,
                                       a_hat.shape[1], comps, ctypes.byref(v)))
        return c


class NttLevelCtMul(NttCtMul):
    """An NttCtMul created through lib/libnttmul_level.so: every NttCtMul method, and
    relin / relin_device take view=(top_q_limbs, top_terms): key_hat is then
    [2][top_terms][top_q_limbs + K][n], the relinearisation key made for the chain's top level.
    view=None is the dense call."""

    @staticmethod
    def _library() -> ctypes.CDLL:
        return load_level_library()

    def relin_device(self, c_hat, up_hat, key_hat, x_hat, y_hat, batch: int, pairs: int,
                     terms: int, dev: Optional[int] = None, stream: int = 0, view=None):
        if view is None:
            return super().relin_device(c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms,
                                        dev, stream)
        dev = self.first_dev if dev is None else dev
        v = _level_view(view)
        args = [_dev_arg(t, m, self.n, self.word_bits, dev)
                for t, m in zip((c_hat, up_hat, key_hat),
                                (batch * 2 * self.limbs, batch * terms * self.limbs,
                                 2 * v.top_terms * (v.top_q_limbs + self.p_limbs)))]
        xp, yp = self._pair_args(x_hat, y_hat, batch, pairs, dev)
        self._check(self._c.relin_view_device(self._h, *args, xp, yp, batch, pairs, terms,
                                              ctypes.byref(v), dev, stream or None))

    def relin(self, up_hat, key_hat, x_hat, y_hat, view=None) -> np.ndarray:
        """view given: key_hat of shape [2, top_terms, top_q_limbs + K, n]; the call's terms are
        up_hat's."""
        if view is None:
            return super().relin(up_hat, key_hat, x_hat, y_hat)
        v = _level_view(view)
        up_hat = np.ascontiguousarray(up_hat, dtype=self.io_dtype)
        x_hat, y_hat = self._host_pairs("relin", x_hat, y_hat)
        if up_hat.ndim != 4 or up_hat.shape[2:] != (self.limbs, self.n) or up_hat.shape[1] == 0:
            raise ValueError(f"relin: up_hat must have shape [batch, terms > 0, {self.limbs}, "
                             f"{self.n}]")
        key_hat = _viewed_host(key_hat, self.io_dtype, 4,
                               (2, v.top_terms, v.top_q_limbs + self.p_limbs, self.n),
                               "relin: key_hat")
        if x_hat.shape[0] != up_hat.shape[0]:
            raise ValueError("relin: x_hat and up_hat must have the same batch")
        batch, pairs = x_hat.shape[:2]
        c = np.empty((batch, 2, self.limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.relin_view(self._h, c.ctypes.data, up_hat.ctypes.data,
                                       key_hat.ctypes.data, x_hat.ctypes.data, y_hat.ctypes.data,
                                       batch, pairs, up_hat.shape[1], ctypes.byref(v)))
        return c


# ---- ciphertext sums, plaintext products, the full tensor (include/nttmul_ctlin.h) ---------------

CTLIN_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_ctlin.so")
CTLIN_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_ctlin.h")
CTLIN_OPS = ("combine", "tensor")
CTLIN_MAX_TERMS, CTLIN_MAX_COMPS = 16, 3
CTLIN_ONE, CTLIN_SCALAR, CTLIN_PLAIN = 0, 1, 2


class CtLinInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("limbs", ctypes.c_uint32),
                ("word_bits", ctypes.c_uint32), ("ndev", ctypes.c_int)]


class CtLinTerm(ctypes.Structure):
    """nttmul_ctlin_term."""
    _fields_ = [("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("kind", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def load_ctlin_library() -> ctypes.CDLL:
    """Load lib/libnttmul_ctlin.so (include/nttmul_ctlin.h): the ABI and kernels of
    libnttmul_level.so plus combine and tensor.  The other loaders are unaffected."""
    return _load_limb_library(CTLIN_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn,
                              _bind_hoist, _bind_mdntt, _bind_ksntt, _bind_lintrans, _bind_ctmul,
                              _bind_xconv, _bind_level, _bind_ctlin)


def _bind_ctlin(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    terms = ctypes.POINTER(CtLinTerm)
    _bind_handle(lib, "nttmul_ctlin", CtLinInfo, [ctypes.POINTER(ctypes.c_uint64), u32])
    lib.nttmul_ctlin_combine_device.argtypes = [vp, vp, terms, u32, sz, u32, i32, vp]
    lib.nttmul_ctlin_combine.argtypes = [vp, vp, terms, u32, sz, u32]
    lib.nttmul_ctlin_tensor_device.argtypes = [vp, vp, vp, vp, sz, u32, i32, vp]
    lib.nttmul_ctlin_tensor.argtypes = [vp, vp, vp, vp, sz, u32]
    lib.nttmul_ctlin_kernel_name.argtypes = [vp, i32, u32, ctypes.c_char_p, sz]


def ctlin_exported_symbols() -> list:
    """Function names declared in include/nttmul_ctlin.h."""
    return _header_symbols(CTLIN_HEADER_PATH, "nttmul_ctlin_")


def ctlin_one(x) -> tuple:
    """The term x (weight 1) of NttCtLin.combine: (x, w, kind)."""
    return (x, None, CTLIN_ONE)


def ctlin_scalar(x, w) -> tuple:
    """The term w[l] x: w holds one constant per limb, [L]."""
    return (x, w, CTLIN_SCALAR)


def ctlin_plain(x, w) -> tuple:
    """The term w o x: w is an NTT-domain plaintext [L, n], shared by batch and components."""
    return (x, w, CTLIN_PLAIN)


def ctlin_const_scalar(w) -> tuple:
    """The constant w[l] added to component 0 (every slot)."""
    return (None, w, CTLIN_SCALAR)


def ctlin_const_plain(w) -> tuple:
    """The NTT-domain plaintext w [L, n] added to component 0."""
    return (None, w, CTLIN_PLAIN)


class NttCtLin(_Handle):
    """nttmul_ctlin: one basis q of L primes of one word class for one degree n in 256 .. 65536
    (include/nttmul_ctlin.h).  Every limb of every operand is in NTT order, as RnsContext /
    RnsMpContext.forward writes it.

    combine is out[p][c] = sum_i W_i o X_i[p][c] over terms made by ctlin_one, ctlin_scalar,
    ctlin_plain, ctlin_const_scalar and ctlin_const_plain, every x and out [batch, comps, L, n]
    with comps in 1 .. 3.  tensor is (d_0, d_1, d_2) [batch, 3, L, n] of x_hat, y_hat
    [batch, pairs, 2, L, n]; the same array for both is the square.

    Caller memory: operands need the alignment of their word only; combine's out may be exactly
    one or more of its x (the same array) and must overlap nothing else, tensor's output must
    overlap no input; combine writes exactly batch * comps * L * n words, tensor batch * 3 * L * n,
    and neither writes an input."""

    _PREFIX = "nttmul_ctlin"
    _OPS = CTLIN_OPS

    def __init__(self, n: int, q, ndev: int = 1, first_dev: int = 0, validate: bool = False,
                 cyclic: bool = False, share_devices: bool = False):
        q = [int(m) for m in q]
        prm = _Params(n, 0, 0, ndev, first_dev, _flags(validate, cyclic, share_devices), 0, 0, 0,
                      0, 0)
        qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
        info = CtLinInfo()
        self._open(load_ctlin_library(), info, prm, qa, len(q))   # self.info
        self.n, self.limbs, self.word_bits = info.n, info.limbs, info.word_bits
        self.q = tuple(q)
        self.first_dev = first_dev

    def kernel_name(self, op, comps: int = 1) -> str:
        """nttmul_ctlin_kernel_name for op 0..1 or "combine" / "tensor", e.g.
        "k_ctlin_combine<Arith64,u64,2>" (comps is ignored by tensor)."""
        return self._kernel_name(op, comps)

    def _terms(self, terms, ptr_of):
        """The nttmul_ctlin_term array of [(x, w, kind), ..]; ptr_of(operand, polys, words)."""
        terms = list(terms)
        arr = (CtLinTerm * max(1, len(terms)))()
        for t, (x, w, kind) in zip(arr, terms):
            t.kind, t.reserved = int(kind), 0
            t.x = None if x is None else ptr_of(x, None)
            t.w = None if w is None else ptr_of(w, kind)
        return arr, len(terms)

    def combine_device(self, out, terms, batch: int, comps: int, dev: Optional[int] = None,
                       stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        every x [batch][comps][L][n], a scalar's w [L], a plaintext's w [L][n] ->
        out [batch][comps][L][n].  out may be one or more of the x."""
        dev = self.first_dev if dev is None else dev
        polys = batch * comps * self.limbs

        def ptr_of(v, kind):
            if kind is None:
                return _dev_arg(v, polys, self.n, self.word_bits, dev)
            if kind == CTLIN_SCALAR:
                return _dev_arg(v, self.limbs, 1, self.word_bits, dev)
            return _dev_arg(v, self.limbs, self.n, self.word_bits, dev)

        op = _dev_arg(out, polys, self.n, self.word_bits, dev)
        arr, count = self._terms(terms, ptr_of)
        self._check(self._c.combine_device(self._h, op, arr, count, batch, comps, dev,
                                           stream or None))

    def combine(self, terms, out: Optional[np.ndarray] = None) -> np.ndarray:
        """terms of numpy arrays: every x of one shape [batch, comps, L, n], a scalar's w [L], a
        plaintext's w [L, n]; a call of constant terms alone needs `out` for its shape.  out: the
        array written and returned (it may be one or more of the x); a new one by default."""
        terms = list(terms)
        dt = self.io_dtype
        keep, shape = [], None if out is None else out.shape

        def host(v, kind):
            if v is out:
                return out.ctypes.data
            a = np.ascontiguousarray(v, dtype=dt)
            keep.append(a)
            return a.ctypes.data

        for x, w, kind in terms:
            if x is not None:
                if shape is None:
                    shape = np.shape(x)
                if np.shape(x) != shape:
                    raise ValueError("combine: every x must have out's shape")
            if w is not None and np.shape(w) != ((self.limbs,) if kind == CTLIN_SCALAR
                                                 else (self.limbs, self.n)):
                raise ValueError("combine: w must have shape [L] (scalar) or [L, n] (plaintext)")
        if shape is None or len(shape) != 4 or shape[2:] != (self.limbs, self.n):
            raise ValueError(f"combine: x must have shape [batch, comps, {self.limbs}, {self.n}]")
        if out is None:
            out = np.empty(shape, dtype=dt)
        elif not (isinstance(out, np.ndarray) and out.dtype == dt and out.flags.c_contiguous):
            raise ValueError("combine: out must be a contiguous array of the context's words")
        arr, count = self._terms(terms, host)
        self._check(self._c.combine(self._h, out.ctypes.data, arr, count, shape[0], shape[1]))
        return out

    def tensor_device(self, d_hat, x_hat, y_hat, batch: int, pairs: int,
                      dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        x_hat, y_hat [batch][pairs][2][L][n] -> d_hat [batch][3][L][n]."""
        dev = self.first_dev if dev is None else dev
        out = _dev_arg(d_hat, batch * 3 * self.limbs, self.n, self.word_bits, dev)
        polys = batch * pairs * 2 * self.limbs
        xp = _dev_arg(x_hat, polys, self.n, self.word_bits, dev)
        yp = xp if y_hat is x_hat else _dev_arg(y_hat, polys, self.n, self.word_bits, dev)
        self._check(self._c.tensor_device(self._h, out, xp, yp, batch, pairs, dev, stream or None))

    def tensor(self, x_hat, y_hat) -> np.ndarray:
        """x_hat, y_hat of shape [batch, pairs, 2, L, n] (the same array: the square).  Returns
        d_hat of shape [batch, 3, L, n]."""
        same = y_hat is x_hat
        x_hat = np.ascontiguousarray(x_hat, dtype=self.io_dtype)
        y_hat = x_hat if same else np.ascontiguousarray(y_hat, dtype=self.io_dtype)
        if x_hat.ndim != 5 or x_hat.shape[2:] != (2, self.limbs, self.n) or x_hat.shape[1] == 0:
            raise ValueError(f"tensor: x_hat must have shape [batch, pairs > 0, 2, {self.limbs}, "
                             f"{self.n}]")
        if y_hat.shape != x_hat.shape:
            raise ValueError("tensor: y_hat must have x_hat's shape")
        batch, pairs = x_hat.shape[:2]
        d = np.empty((batch, 3, self.limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.tensor(self._h, d.ctypes.data, x_hat.ctypes.data, y_hat.ctypes.data,
                                   batch, pairs))
        return d


# ---- BGV's plaintext-preserving ModDown and rescale (include/nttmul_tmd.h) ------------------------

TMD_LIB_PATH = os.path.join(PKG_DIR, "lib", "libnttmul_tmd.so")
TMD_HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "nttmul_tmd.h")


class TmdInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logn", ctypes.c_uint32), ("q_limbs", ctypes.c_uint32),
                ("p_limbs", ctypes.c_uint32), ("word_bits", ctypes.c_uint32),
                ("ndev", ctypes.c_int), ("scratch_mb", ctypes.c_uint32),
                ("t", ctypes.c_uint64), ("msg_factor", ctypes.c_uint64)]


def load_tmd_library() -> ctypes.CDLL:
    """Load lib/libnttmul_tmd.so (include/nttmul_tmd.h): the ABI and kernels of
    libnttmul_ctlin.so plus the plaintext-preserving ModDown.  The other loaders are
    unaffected."""
    return _load_limb_library(TMD_LIB_PATH, _bind_rns, _bind_rnsmp, _bind_ks, _bind_macn,
                              _bind_hoist, _bind_mdntt, _bind_ksntt, _bind_lintrans, _bind_ctmul,
                              _bind_xconv, _bind_level, _bind_ctlin, _bind_tmd)


def _bind_tmd(lib: ctypes.CDLL) -> None:
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u64, u64p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    _bind_handle(lib, "nttmul_tmd", TmdInfo, [u64p, u32, u64p, u32, u64])
    lib.nttmul_tmd_moddown_device.argtypes = [vp, vp, vp, sz, i32, vp]
    lib.nttmul_tmd_moddown.argtypes = [vp, vp, vp, sz]
    lib.nttmul_tmd_plan.argtypes = [ctypes.POINTER(_Params), sz, u64p, u32, u64p, u32, u64,
                                    vp, vp, vp, vp, vp]
    lib.nttmul_tmd_kernel_name.argtypes = [vp, ctypes.c_char_p, sz]


def tmd_exported_symbols() -> list:
    """Function names declared in include/nttmul_tmd.h."""
    return _header_symbols(TMD_HEADER_PATH, "nttmul_tmd_")


def tmd_plan(q, p, t: int, n: int = 256, flags: int = 0):
    """nttmul_tmd_plan, without a device: (yscale, g, w, v, msg_factor) in Python integers.
    yscale[j] = Ph_j^-1 mod p_j; g[j] = -p_j^-1 mod t; w[j][l] = Ph_j mod q_l for j < K,
    w[K][l] = P mod q_l and w[K + 1][l] = -P mod q_l; v[l] = P^-1 mod q_l; msg_factor = P^-1 mod
    t.  The constants do not depend on n, which only has to suit the primes.  Raises NttmulError
    with the status nttmul_tmd_create would return for these arguments before any device
    access."""
    lib = load_tmd_library()
    q, p, prm, qa, pa = _ks_bases(n, q, p, flags)
    L, K = len(q), len(p)
    if not 0 <= t < 1 << 64:
        raise NttmulError(NTTMUL_EINVAL, lib.nttmul_strerror(NTTMUL_EINVAL).decode())
    sizes = (K, K, (K + 2) * L, L, 1)
    tab = [(ctypes.c_uint64 * max(1, k))() for k in sizes]
    st = lib.nttmul_tmd_plan(ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K, t,
                             *(ctypes.addressof(x) for x in tab))
    if st != NTTMUL_OK:
        raise NttmulError(st, lib.nttmul_strerror(st).decode())
    yscale, g, w, v, mf = (list(x[:k]) for x, k in zip(tab, sizes))
    return yscale, g, [w[i:i + L] for i in range(0, len(w), L)], v, mf[0]


class NttPlainModDown(_Handle):
    """nttmul_tmd: the bases Q = q (L primes) and P = p (K primes), disjoint and of one word
    class, and an odd plaintext modulus t >= 3, for one degree n in 256 .. 65536
    (include/nttmul_tmd.h).  moddown maps x_hat [batch, L + K, n], every limb in NTT order as
    RnsContext / RnsMpContext.forward writes it, to [batch, L, n] in NTT order: (X - d) / P mod q_l
    for the CRT value X over Q u P, with d = X (mod P) and d = 0 (mod t), so that
    P * out = X (mod t).  The message of a BGV ciphertext comes out multiplied by
    self.msg_factor = P^-1 mod t.  p = (the last prime,) is the BGV rescale.  The result equals
    NttModDown.moddown(x_hat) - forward(u), |u| <= (t - 1) / 2, bit for bit.

    Caller memory: operands need the alignment of their word only; out must not overlap x_hat;
    a call writes exactly batch * L * n words of out and never writes x_hat.

    close() waits for the last use of the context's scratch, not for the streams passed to
    moddown_device: synchronise them first."""

    _PREFIX = "nttmul_tmd"
    _NAME_CAP = 256

    def __init__(self, n: int, q, p, t: int, ndev: int = 1, first_dev: int = 0,
                 validate: bool = False, cyclic: bool = False, share_devices: bool = False,
                 scratch_mb: int = 0):
        q, p, prm, qa, pa = _ks_bases(n, q, p, _flags(validate, cyclic, share_devices))
        prm.ndev, prm.first_dev, prm.scratch_mb = ndev, first_dev, scratch_mb
        info = TmdInfo()
        lib = load_tmd_library()
        if not 0 <= t < 1 << 64:
            raise NttmulError(NTTMUL_EINVAL, lib.nttmul_strerror(NTTMUL_EINVAL).decode())
        self._open(lib, info, prm, qa, len(q), pa, len(p), t)
        self.n, self.word_bits = info.n, info.word_bits
        self.q_limbs, self.p_limbs = info.q_limbs, info.p_limbs
        self.q, self.p, self.t = tuple(q), tuple(p), info.t
        self.msg_factor = info.msg_factor
        self.first_dev = first_dev

    def kernel_name(self) -> str:
        """nttmul_tmd_kernel_name: a sub-batch's kernels joined by " + ", e.g.
        "k_mdntt_inv<Arith32P,u32,12> + k_tmd_fwd<Arith32P,u32,12>"."""
        buf = ctypes.create_string_buffer(self._NAME_CAP)
        st = self._c.kernel_name(self._h, buf, len(buf))
        if st < 0:
            self._check(st)
        return buf.value.decode()

    def moddown_device(self, out, x_hat, batch: int, dev: Optional[int] = None, stream: int = 0):
        """Device-resident operands (pointers or torch tensors on `dev`), enqueued on `stream`:
        x_hat [batch][L + K][n] -> out [batch][L][n]."""
        dev = self.first_dev if dev is None else dev
        args = [_dev_arg(x, batch * k, self.n, self.word_bits, dev)
                for x, k in zip((out, x_hat), (self.q_limbs, self.q_limbs + self.p_limbs))]
        self._check(self._c.moddown_device(self._h, *args, batch, dev, stream or None))

    def moddown(self, x_hat) -> np.ndarray:
        """x_hat of shape [batch, L + K, n]; returns [batch, L, n]."""
        ext = self.q_limbs + self.p_limbs
        x_hat = np.ascontiguousarray(x_hat, dtype=self.io_dtype)
        if x_hat.ndim != 3 or x_hat.shape[1:] != (ext, self.n):
            raise ValueError(f"moddown: x_hat must have shape [batch, {ext}, {self.n}]")
        out = np.empty((x_hat.shape[0], self.q_limbs, self.n), dtype=self.io_dtype)
        self._check(self._c.moddown(self._h, out.ctypes.data, x_hat.ctypes.data, x_hat.shape[0]))
        return out


# ---- planner API ------------------------------------------------------------

class _HostBlock:
    """Owner of one nttmul_host_alloc block (freed with the last numpy view of it)."""

    def __init__(self, nbytes: int):
        lib = load_library()
        lib.nttmul_host_alloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        lib.nttmul_host_free.argtypes = [ctypes.c_void_p]
        lib.nttmul_host_free.restype = None
        p = ctypes.c_void_p()
        st = lib.nttmul_host_alloc(ctypes.byref(p), nbytes)
        if st != NTTMUL_OK:
            raise NttmulError(st, strerror(st))
        self._lib, self.ptr, self.nbytes = lib, p.value, nbytes

    def __del__(self):
        if getattr(self, "ptr", None):
            self._lib.nttmul_host_free(self.ptr)
            self.ptr = None


def host_empty(shape, dtype) -> np.ndarray:
    """Uninitialised numpy array in page-locked host memory (nttmul_host_alloc): host-buffer
    calls whose operands all live in such arrays DMA directly, without the staging copy."""
    dtype = np.dtype(dtype)
    count = int(np.prod(shape))
    blk = _HostBlock(max(1, count * dtype.itemsize))
    buf = (ctypes.c_char * blk.nbytes).from_address(blk.ptr)
    buf._nttmul_block = blk                      # the ctypes buffer keeps the block alive
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


def is_prime(q: int) -> bool:
    return bool(load_library().nttmul_is_prime(q))


def smallest_psi(n: int, q: int) -> int:
    """generate_params.C:25-44: smallest element of order exactly 2n (0 if none)."""
    return int(load_library().nttmul_smallest_psi(n, q))


def smallest_omega(n: int, q: int) -> int:
    return int(load_library().nttmul_smallest_omega(n, q))


def find_prime(n: int, bits: int, cyclic: bool = False) -> int:
    """Largest prime q < 2^bits with q == 1 (mod 2n) (mod n if cyclic)."""
    q = ctypes.c_uint64()
    st = load_library().nttmul_find_prime(n, bits, int(cyclic), ctypes.byref(q))
    if st != NTTMUL_OK:
        raise NttmulError(st, strerror(st))
    return q.value


def table(n: int, q: int, name: str, psi: int = 0) -> np.ndarray:
    """One of the NTT/ntt.h:63-183 tables for (n, q, psi)."""
    out = np.zeros(n, dtype=np.uint64)
    st = load_library().nttmul_table(n, q, psi, TABLES.index(name), out.ctypes.data)
    if st != NTTMUL_OK:
        raise NttmulError(st, strerror(st))
    return out


def fpga_R(n: int, K: int) -> int:
    return int(load_library().nttmul_fpga_R(n, K))


def fpga_twiddles(n: int, q: int, w: int, R: int, P: int = 8) -> np.ndarray:
    """generate_twiddles (generate_params.C:54-73): the PolyMult.v W / W_INV stream."""
    lib = load_library()
    cnt = lib.nttmul_fpga_twiddles(n, q, w, R, P, None, 0)
    out = np.zeros(cnt, dtype=np.uint64)
    lib.nttmul_fpga_twiddles(n, q, w, R, P, out.ctypes.data, cnt)
    return out


# ---- text formats ------------------------------------------------------------

def read_coefficients(path: str, max_count: int) -> np.ndarray:
    """time_testing256.c:17-44 ler_coeficientes."""
    out = np.zeros(max_count, dtype=np.int32)
    cnt = load_library().nttmul_read_coefficients(path.encode(), out.ctypes.data, max_count)
    if cnt < 0:
        raise OSError(f"cannot open {path}")
    return out[:cnt]


def read_hex(path: str, max_count: int) -> np.ndarray:
    out = np.zeros(max_count, dtype=np.uint64)
    cnt = load_library().nttmul_read_hex(path.encode(), out.ctypes.data, max_count)
    if cnt < 0:
        raise OSError(f"cannot open {path}")
    return out[:cnt]


def write_hex(path: str, a) -> None:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if load_library().nttmul_write_hex(path.encode(), a.ctypes.data, a.size) < 0:
        raise OSError(f"cannot write {path}")


def multiply(a, b, n: int, q: int) -> np.ndarray:
    """multiply(a, b, n, q) -> c: the north-star entry point, one-shot."""
    with Context(n, q) as ctx:
        return ctx.multiply(a, b)


def _product256(name: str, c: np.ndarray, a: np.ndarray, b: np.ndarray) -> None:
    for x in (a, b, c):
        if not (isinstance(x, np.ndarray) and x.dtype == np.int32 and x.size == 256
                and x.flags.c_contiguous):
            raise TypeError("ntt256 products take contiguous int32 arrays of 256 coefficients")
    getattr(load_library(), name)(c.ctypes.data, a.ctypes.data, b.ctypes.data)


def ntt256_product1(c: np.ndarray, a: np.ndarray, b: np.ndarray) -> None:
    """NTT/ntt256.C:5 — c = a * b at n = 256, q = 12289 (result written into c)."""
    _product256("ntt256_product1", c, a, b)


def ntt256_product4(c: np.ndarray, a: np.ndarray, b: np.ndarray) -> None:
    """NTT/ntt256.C:16."""
    _product256("ntt256_product4", c, a, b)


def ntt_red256_product1(c: np.ndarray, a: np.ndarray, b: np.ndarray) -> None:
    """NTT-RED/ntt_red256.C:5."""
    _product256("ntt_red256_product1", c, a, b)


def ntt_red256_product4(c: np.ndarray, a: np.ndarray, b: np.ndarray) -> None:
    """NTT-RED/ntt_red256.C:30."""
    _product256("ntt_red256_product4", c, a, b)


def ntt256_transform(name: str, a: np.ndarray) -> None:
    """One of the reference's n = 256 wrappers (NTT/ntt256.h:20-69, e.g. "ntt256_ct_std2rev",
    "inttmul256_gs_rev2std") in place on a contiguous int32 array of 256 coefficients."""
    if name not in NTT256_WRAPPERS:
        raise ValueError(f"unknown ntt256 wrapper {name}")
    if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.size == 256
            and a.flags.c_contiguous):
        raise TypeError("ntt256 wrappers take a contiguous int32 array of 256 coefficients")
    getattr(load_library(), name)(a.ctypes.data)
