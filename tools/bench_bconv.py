"""RNS base conversion and ModDown in one launch (lib/libnttmul_bconv.so, nttmul_bconv_*_device)
against its two bounds, and against what a caller does today: a torch int64 composition of convert
on the same device.  Device-resident, interleaved in one run:

    python tools/bench_bconv.py [--rows 32:4096x16384:4x4,...] [--rounds 9] [--reps 0] [--warmup 3]
                                [--no-torch] [--out profiles/bconv/bench.json]

A row is bits:n x batch:L x K.  The default rows are the 32-bit class at n = 4096 x 16,384 for
(L, K) = (4, 4), (4, 12) and (1, 4), the 64-bit class at (4, 4), and a thin shape n = 4096 x 64.
The bases are the first L primes = 1 mod 8192 below the top of the class, then the next K.  Per row
the timed sequences are (device events around `reps` back-to-back calls, one synchronise per
window):
  convert / moddown      one nttmul_bconv_*_device call
  torch_convert          32-bit class only: y_i = x_i inv_i mod b_i and sum_i (y_i w_ij mod c_j) mod c_j
                         in int64 tensors (each product reduced: two of them overflow int64)
They run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per call).  Before timing, each call is compared bit
for bit with the torch composition (32-bit class) or with Python integers on a sample of
coefficients (64-bit class).  --reps 0 picks 20 for rows of at least 16384 polynomials and 200
below; the torch composition runs a tenth as many per window.

Beside each time the line records the algorithmic bytes, (L + K) n w per polynomial for convert
and (L + 2 K) n w for moddown (w bytes per word), their time at 5.7 and 6.1 TB/s (the rates
DESIGN.md records for the streaming column passes), and the VALU issue bound of the `make
asm-bconv` listing: the instruction counts below per thread, 4.2 cycles per wave64 instruction and
SIMD, 1,024 SIMDs at 2.4 GHz.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = "32:4096x16384:4x4,32:4096x16384:4x12,32:4096x16384:1x4,64:4096x16384:4x4,32:4096x64:4x4"
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 4096
HBM_TBPS = (5.7, 6.1)
CYCLES_PER_VALU, SIMDS, CLOCK_HZ = 4.2, 1024, 2.4e9
TILE = 4
# VALU instructions per thread in the `make asm-bconv` listing (a thread holds `coefs`
# coefficients): per tile of 4 target limbs `tile`, per group of `cadence` source limbs with its
# fold `group`, per source limb of the shorter last group `tail` and that group's fold `tail_fold`,
# per stored word `store` (convert, moddown)
LISTING = {
    32: dict(coefs=4, cadence=2, tile=16, group=106, tail=33, tail_fold=34, store=(5, 12)),
    64: dict(coefs=1, cadence=4, tile=8, group=292, tail=40, tail_fold=134, store=(24, 48)),
}


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def valu_per_thread(bits, L, K, op):
    m = LISTING[bits]
    groups, rest = divmod(L, m["cadence"])
    tiles = (K + TILE - 1) // TILE
    per_tile = m["tile"] + groups * m["group"] + (rest * m["tail"] + m["tail_fold"] if rest else 0)
    return tiles * per_tile + K * m["coefs"] * m["store"][op == "moddown"]


def bounds(bits, n, batch, L, K, op):
    wbytes = bits // 8
    limbs = L + K + (K if op == "moddown" else 0)
    nbytes = batch * n * limbs * wbytes
    valu = valu_per_thread(bits, L, K, op)
    waves = batch * n / (64 * LISTING[bits]["coefs"])
    valu_ms = waves / SIMDS * valu * CYCLES_PER_VALU / CLOCK_HZ * 1e3
    return {"algorithmic_bytes": nbytes,
            "hbm_ms": [round(nbytes / (r * 1e12) * 1e3, 5) for r in HBM_TBPS],
            "valu_per_thread": valu, "valu_issue_ms": round(valu_ms, 5)}


def bench_row(torch, nttmul, bits, n, batch, L, K, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    from_q, to_q = primes[:L], primes[L:]
    conv = nttmul.BaseConverter(n, from_q, to_q)
    inv, w, binv = nttmul.bconv_plan(n, from_q, to_q)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)

    def words(moduli):                       # [batch][len(moduli)][n], limb l below moduli[l]
        x = torch.empty((batch, len(moduli), n), dtype=dtype, device="cuda")
        for l, q in enumerate(moduli):
            x[:, l, :] = torch.randint(0, q, (batch, n), generator=gen, device="cuda",
                                       dtype=torch.int64).to(dtype)
        return x

    x = words(to_q + from_q)                 # moddown's input; its last L limbs are convert's
    xf = x[:, K:, :].contiguous()
    out = torch.empty((batch, K, n), dtype=dtype, device="cuda")

    def torch_convert():
        res = []
        ys = [(xf[:, i, :].to(torch.int64) * inv[i]) % from_q[i] for i in range(L)]
        for j in range(K):
            acc = (ys[0] * w[0][j]) % to_q[j]
            for i in range(1, L):
                acc += (ys[i] * w[i][j]) % to_q[j]
            res.append(acc % to_q[j])
        return torch.stack(res, dim=1)

    variants = {"convert": lambda: conv.convert_device(out, xf, batch, stream=stream),
                "moddown": lambda: conv.moddown_device(out, x, batch, stream=stream)}
    # both operations compute the reference, bit for bit
    if bits == 32 and not args.no_torch:
        variants["torch_convert"] = torch_convert
        want = torch_convert()
        variants["convert"]()
        assert torch.equal(out.to(torch.int64), want), "convert differs from the torch composition"
        variants["moddown"]()
        for j in range(K):
            d = (x[:, j, :].to(torch.int64) - want[:, j, :]) % to_q[j]
            ref = (d * binv[j]) % to_q[j]                  # d, binv < 2^31
            assert torch.equal(out[:, j, :].to(torch.int64), ref), "moddown differs from the composition"
        del want
    else:
        import random
        from math import prod
        Bp, rng = prod(from_q), random.Random(7)
        spots = [(rng.randrange(batch), rng.randrange(n)) for _ in range(64)]
        for op in ("convert", "moddown"):
            variants[op]()
            torch.cuda.synchronize()
            for p, k in spots:
                col = [int(v) for v in x[p, :, k].tolist()]
                s = sum(col[K + i] * inv[i] % b * (Bp // b) for i, b in enumerate(from_q))
                ref = [s % c if op == "convert" else (col[j] - s) * binv[j] % c
                       for j, c in enumerate(to_q)]
                assert [int(v) for v in out[p, :, k].tolist()] == ref, f"{op} differs at {(p, k)}"

    reps = args.reps or (20 if batch >= 16384 else 200)
    calls = {k: max(1, reps // 10) if k.startswith("torch") else reps for k in variants}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    names = list(variants)
    ms = {k: [] for k in names}
    for r in range(args.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[k]):
                variants[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls[k])

    hashes = nttmul.kernel_hashes(nttmul.BCONV_LIB_PATH)
    row = {"word_bits": bits, "n": n, "batch": batch, "from_limbs": L, "to_limbs": K, "reps": calls,
           "ms_per_call": {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                               "max": round(max(v), 5)} for k, v in ms.items()},
           "bounds": {op: bounds(bits, n, batch, L, K, op) for op in ("convert", "moddown")},
           "kernel_hashes": {conv.kernel_name(op): hashes[conv.kernel_name(op)]
                             for op in ("convert", "moddown")}}
    for op in ("convert", "moddown"):
        med = row["ms_per_call"][op]["median"]
        b = row["bounds"][op]
        b["achieved_tbps"] = round(b["algorithmic_bytes"] / (med * 1e-3) / 1e12, 3)
        b["median_over_bound"] = round(med / max(b["hbm_ms"][1], b["valu_issue_ms"]), 3)
    conv.close()
    return row


def parse_rows(text):
    rows = []
    for item in text.split(","):
        bits, shape, limbs = item.split(":")
        n, batch = (int(v) for v in shape.split("x"))
        L, K = (int(v) for v in limbs.split("x"))
        if int(bits) not in TOP:
            raise ValueError(f"word bits {bits}: 32 or 64")
        rows.append((int(bits), n, batch, L, K))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--rows", default=DEFAULT_ROWS,
                    help="comma-separated bits:n x batch:L x K, e.g. 32:4096x16384:4x4")
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
        raise SystemExit("bench_bconv.py measures on a GPU; none is visible")
    line = {"bench": "bconv", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "hbm_tbps": list(HBM_TBPS),
            "valu_model": {"cycles_per_instruction": CYCLES_PER_VALU, "simds": SIMDS,
                           "clock_hz": CLOCK_HZ, "listing": LISTING},
            "rows": [bench_row(torch, nttmul, *row, args) for row in rows]}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
