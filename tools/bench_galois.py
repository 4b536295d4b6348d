"""Galois automorphisms over all RNS limbs (lib/libnttmul_galois.so, nttmul_galois_*_device)
against a device-to-device copy of the same bytes in the same run, against the algorithmic HBM
bound, and against what a caller does today: torch index_select with a precomputed int64 index
(plus where for the signs).  One MI355X, device-resident, interleaved in one run:

    python tools/bench_galois.py [--rows 32:4096x16384:4,...] [--rounds 9] [--reps 0] [--warmup 3]
                                 [--no-torch] [--out profiles/galois/bench.json]

A row is bits:n x batch:L.  The default rows are the fat shapes n = 4096 x 16,384 and
n = 65536 x 1,024 with L = 4 in both word classes, the thin shape n = 4096 x 64, and the sizes
below n = 65536 at the same bytes (n = 16384 and 32768 in both classes, n = 8192 on 64-bit words):
the coefficient kernel stages a limb polynomial whole up to n = 32768 on 32-bit and n = 16384 on
64-bit words and in two or four residue classes above.  The moduli are the
first L primes = 1 mod 2^17 below the top of the class.  Per row the timed sequences are (device
events around `reps` back-to-back calls, one synchronise per window):
  coeff / ntt            one nttmul_galois_*_device call, k = 5^3 mod 2n
  ntt_many4              one nttmul_galois_ntt_many_device call with 4 automorphisms
  ntt_x4                 the same 4 automorphisms as four nttmul_galois_ntt_device calls
  copy / copy_x4         hipMemcpyAsync device to device of the input's bytes (once, four times)
  torch_coeff / torch_ntt  index_select along n with a precomputed int64 index; torch_coeff adds
                         where(neg, (q - x) % q, x) with q broadcast per limb
They run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per call).  Before timing, each library call is
compared bit for bit with the torch composition, which is built from nttmul_galois_plan's tables.
--reps 0 picks 20 for rows of at least 2^26 words and 200 below; the torch composition runs a tenth
as many per window.

Beside each time the line records the algorithmic bytes, 2 n w per limb polynomial for the single
calls and (1 + count) n w for ntt_many (w bytes per word), the achieved rate, and the ratio of the
median to the interleaved copy's median (copy_x4's for ntt_x4; for ntt_many4 the ratio is to
copy's median scaled by the bytes, (1 + 4) / 2).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = ("32:4096x16384:4,64:4096x16384:4,32:65536x1024:4,64:65536x1024:4,32:4096x64:4,"
                "32:16384x4096:4,32:32768x2048:4,64:8192x8192:4,64:16384x4096:4,64:32768x2048:4")
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 1 << 17
MANY = 4


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def bench_row(torch, nttmul, bits, n, batch, L, args):
    moduli = primes_below(nttmul, TOP[bits], L)
    ctx = nttmul.GaloisContext(n, moduli)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(n + L)
    x = torch.empty((batch, L, n), dtype=dtype, device="cuda")
    for l, q in enumerate(moduli):
        x[:, l, :] = torch.randint(0, q, (batch, n), generator=gen, device="cuda",
                                   dtype=torch.int64).to(dtype)
    out = torch.empty_like(x)
    out4 = torch.empty((MANY,) + tuple(x.shape), dtype=dtype, device="cuda")
    k = nttmul.galois_element(n, 3)
    ks = [nttmul.galois_element(n, s) for s in (1, 2, 3, 4)]
    src, neg, hat = nttmul.galois_plan(n, k)
    src_t = torch.from_numpy(src.astype("int64")).cuda()
    neg_t = torch.from_numpy(neg.astype(bool)).cuda()
    hat_t = torch.from_numpy(hat.astype("int64")).cuda()
    q_t = torch.tensor(moduli, dtype=torch.int64, device="cuda").to(dtype).reshape(1, L, 1)
    nbytes = x.numel() * x.element_size()

    def copy():
        out.copy_(x, non_blocking=True)        # hipMemcpyAsync, device to device

    def copy_x4():
        for c in range(MANY):
            out4[c].copy_(x, non_blocking=True)

    def ntt_x4():
        for c in range(MANY):
            ctx.ntt_device(out4[c], x, ks[c], batch, stream=stream)

    def torch_coeff():
        g = torch.index_select(x, 2, src_t)
        return torch.where(neg_t, (q_t - g) % q_t, g)

    def torch_ntt():
        return torch.index_select(x, 2, hat_t)

    variants = {"coeff": lambda: ctx.coeff_device(out, x, k, batch, stream=stream),
                "ntt": lambda: ctx.ntt_device(out, x, k, batch, stream=stream),
                "ntt_many4": lambda: ctx.ntt_many_device(out4, x, ks, batch, stream=stream),
                "ntt_x4": ntt_x4, "copy": copy, "copy_x4": copy_x4}
    # the library computes the composition's result, bit for bit (and many = four singles)
    variants["coeff"]()
    assert torch.equal(out, torch_coeff()), "coeff differs from the torch composition"
    variants["ntt"]()
    assert torch.equal(out, torch_ntt()), "ntt differs from the torch composition"
    variants["ntt_many4"]()
    many = out4.clone()
    out4.fill_(-1)
    ntt_x4()
    assert torch.equal(out4, many), "ntt_many differs from four single calls"
    assert torch.equal(out4[2], out), "ntt_many differs from the torch composition"
    del many
    if not args.no_torch:
        variants["torch_coeff"] = torch_coeff
        variants["torch_ntt"] = torch_ntt

    reps = args.reps or (20 if x.numel() >= 1 << 26 else 200)
    calls = {v: max(1, reps // 10) if v.startswith("torch") else reps for v in variants}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    names = list(variants)
    ms = {v: [] for v in names}
    for r in range(args.rounds):
        for v in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[v]):
                variants[v]()
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1) / calls[v])

    hashes = nttmul.kernel_hashes(nttmul.GALOIS_LIB_PATH)
    kernels = {op: ctx.kernel_name(op, MANY) for op in nttmul.GALOIS_OPS}
    stat = {v: {"median": round(statistics.median(t), 5), "min": round(min(t), 5),
                "max": round(max(t), 5)} for v, t in ms.items()}
    row = {"word_bits": bits, "n": n, "batch": batch, "limbs": L, "k": k, "ks": ks, "reps": calls,
           "ms_per_call": stat, "kernels": kernels,
           "kernel_hashes": {name: hashes[name] for name in kernels.values()}}
    copy_med = stat["copy"]["median"]
    row["copy_spread"] = [round(stat["copy"]["min"] / copy_med, 3),
                          round(stat["copy"]["max"] / copy_med, 3)]
    traffic = {"coeff": 2 * nbytes, "ntt": 2 * nbytes, "ntt_many4": (1 + MANY) * nbytes,
               "ntt_x4": 2 * MANY * nbytes, "copy": 2 * nbytes, "copy_x4": 2 * MANY * nbytes}
    yard = {"coeff": copy_med, "ntt": copy_med, "ntt_many4": copy_med * (1 + MANY) / 2,
            "ntt_x4": stat["copy_x4"]["median"]}
    row["bounds"] = {}
    for v, b in traffic.items():
        med = stat[v]["median"]
        row["bounds"][v] = {"algorithmic_bytes": b,
                            "achieved_tbps": round(b / (med * 1e-3) / 1e12, 3)}
        if v in yard:
            row["bounds"][v]["median_over_copy"] = round(med / yard[v], 3)
    row["many_over_four_singles"] = round(stat["ntt_many4"]["median"] / stat["ntt_x4"]["median"], 3)
    if not args.no_torch:
        row["torch_over_library"] = {
            "coeff": round(stat["torch_coeff"]["median"] / stat["coeff"]["median"], 2),
            "ntt": round(stat["torch_ntt"]["median"] / stat["ntt"]["median"], 2)}
    ctx.close()
    return row


def parse_rows(text):
    rows = []
    for item in text.split(","):
        bits, shape, limbs = item.split(":")
        n, batch = (int(v) for v in shape.split("x"))
        if int(bits) not in TOP:
            raise ValueError(f"word bits {bits}: 32 or 64")
        rows.append((int(bits), n, batch, int(limbs)))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--rows", default=DEFAULT_ROWS,
                    help="comma-separated bits:n x batch:L, e.g. 32:4096x16384:4")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch composition out")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
    except ValueError as e:
        ap.error(f"--rows: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_galois.py measures on a GPU; none is visible")
    line = {"bench": "galois", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "many": MANY, "rows": []}
    for row in rows:
        line["rows"].append(bench_row(torch, nttmul, *row, args))
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
