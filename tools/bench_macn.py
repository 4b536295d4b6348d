"""The mac against two NTT-domain operands (lib/libnttmul_macn.so, nttmul_*_macn_ntt_device with
comps = 2) against the two mac_ntt calls it replaces, and the whole hybrid key switch with either,
device-resident, shared b_hat, interleaved in one run:

    python tools/bench_macn.py [--rows 32:4096x16384:4x2x2,...] [--rounds 9] [--reps 0]
                               [--warmup 3] [--out profiles/macn/bench.json]

A row is bits:n x batch:L x K x alpha, as tools/bench_ks.py's, with the same default rows:
n = 4096 x 16,384 and n = 65536 x 1,024 in both word classes for (L, K, alpha) = (4, 2, 2)
(limbs 6, terms 2) and (12, 4, 4) (limbs 16, terms 3), and the thin shape n = 4096 x 64.  The mac
context holds the extended basis Q u P.  Per row the timed sequences are (device events around
`reps` back-to-back sequences, one synchronise per window):
  macn      one macn_ntt_device, comps = 2, into [batch][2][L + K][n]
  mac2      two mac_ntt_device calls of the same context (the kernels libnttmul_ks.so holds, bit
            for bit), one per component, into two [batch][L + K][n] buffers
  ks_macn   modup, macn, one moddown over batch * 2:   3 launches at n <= 4096, 5 above
  ks_mac2   modup, then mac_ntt and moddown per component: 5 launches, 9 above
They run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per sequence).  Before timing, macn's components
are compared bit for bit with mac2's outputs, and the two key switches with each other.
--reps 0 picks 10 for rows of at least 2^26 coefficients and 100 below.

Beside each ratio macn / mac2 the line records mac2's own spread, (max - min) / median, and
whether macn is ahead by more than that spread; the transform counts alone predict
(terms + 2) / (2 terms + 2).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = ",".join(f"{bits}:{shape}:{lk}" for shape in ("4096x16384", "65536x1024")
                        for bits in (32, 64) for lk in ("4x2x2", "12x4x4")) + \
    ",32:4096x64:4x2x2,64:4096x64:4x2x2"
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 65536


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def bench_row(torch, nttmul, bits, n, batch, L, K, alpha, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    ext, M, dnum = q + p, L + K, -(-L // alpha)
    ks = nttmul.KeySwitchBasis(n, q, p, alpha)
    Mac = nttmul.RnsMacnContext if n <= 4096 else nttmul.RnsMpMacnContext
    mac = Mac(n, ext)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)

    def words(polys, moduli):                # [polys][len(moduli)][n], limb l below moduli[l]
        x = torch.empty((polys, len(moduli), n), dtype=dtype, device="cuda")
        for l, m in enumerate(moduli):
            x[:, l, :] = torch.randint(0, m, (polys, n), generator=gen, device="cuda",
                                       dtype=torch.int64).to(dtype)
        return x

    x = words(batch, q)                      # the key switch's input
    key_hat = words(2 * dnum, ext).view(2, dnum, M, n)      # any canonical vector is a b_hat
    up = torch.empty((batch, dnum, M, n), dtype=dtype, device="cuda")
    ks.modup_device(up, x, batch, stream=stream)
    mid = torch.empty((batch, 2, M, n), dtype=dtype, device="cuda")
    out = torch.empty((batch, 2, L, n), dtype=dtype, device="cuda")
    mid1 = [torch.empty((batch, M, n), dtype=dtype, device="cuda") for _ in range(2)]
    out1 = [torch.empty((batch, L, n), dtype=dtype, device="cuda") for _ in range(2)]

    def macn():
        mac.macn_ntt_device(mid, up, key_hat, batch, dnum, 2, shared=True, stream=stream)

    def mac2():
        for i in range(2):
            mac.mac_ntt_device(mid1[i], up, key_hat[i], batch, dnum, shared=True, stream=stream)

    def ks_macn():
        ks.modup_device(up, x, batch, stream=stream)
        macn()
        ks.moddown_device(out, mid, batch * 2, stream=stream)

    def ks_mac2():
        ks.modup_device(up, x, batch, stream=stream)
        for i in range(2):
            mac.mac_ntt_device(mid1[i], up, key_hat[i], batch, dnum, shared=True, stream=stream)
            ks.moddown_device(out1[i], mid1[i], batch, stream=stream)

    variants = {"macn": macn, "mac2": mac2, "ks_macn": ks_macn, "ks_mac2": ks_mac2}
    ks_macn()
    ks_mac2()
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(mid[:, i], mid1[i]), f"component {i} differs from mac_ntt"
        assert torch.equal(out[:, i], out1[i]), f"key-switch component {i} differs"
    assert not torch.equal(mid[:, 0], mid[:, 1])

    reps = args.reps or (10 if batch * n >= 1 << 26 else 100)
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
            for _ in range(reps):
                variants[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)

    stat = {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                "max": round(max(v), 5)} for k, v in ms.items()}

    def versus(new, old):
        spread = (stat[old]["max"] - stat[old]["min"]) / stat[old]["median"]
        ratio = stat[new]["median"] / stat[old]["median"]
        return {"ratio": round(ratio, 3), f"{old}_spread": round(spread, 3),
                "ahead_by_more_than_the_spread": bool(ratio < 1 - spread)}

    hashes = nttmul.kernel_hashes(nttmul.MACN_LIB_PATH)
    kernels = mac.macn_kernel_name(2).split(" + ") + mac.macn_kernel_name(1).split(" + ")
    row = {"word_bits": bits, "n": n, "batch": batch, "q_limbs": L, "p_limbs": K,
           "digit_limbs": alpha, "limbs": M, "terms": dnum, "reps": reps, "ms_per_call": stat,
           "macn_over_mac2": versus("macn", "mac2"),
           "transform_count_ratio": round((dnum + 2) / (2 * dnum + 2), 3),
           "ks_macn_over_ks_mac2": versus("ks_macn", "ks_mac2"),
           "launches": {"ks_macn": 3 if n <= 4096 else 5, "ks_mac2": 5 if n <= 4096 else 9},
           "kernel_hashes": {k: hashes[nttmul.dispatch_key(k)] for k in sorted(set(kernels))}}
    ks.close()
    mac.close()
    return row


def parse_rows(text):
    rows = []
    for item in text.split(","):
        bits, shape, limbs = item.split(":")
        n, batch = (int(v) for v in shape.split("x"))
        L, K, alpha = (int(v) for v in limbs.split("x"))
        if int(bits) not in TOP:
            raise ValueError(f"word bits {bits}: 32 or 64")
        rows.append((int(bits), n, batch, L, K, alpha))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--rows", default=DEFAULT_ROWS,
                    help="comma-separated bits:n x batch:L x K x alpha, e.g. 32:4096x16384:4x2x2")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=0, help="sequences per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
    except ValueError as e:
        ap.error(f"--rows: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_macn.py measures on a GPU; none is visible")
    line = {"bench": "macn", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "rows": []}
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
