"""BGV's plaintext-preserving ModDown (lib/libnttmul_tmd.so, nttmul_tmd_moddown_device) against the
floor form of the same commit (lib/libnttmul_mdntt.so, nttmul_mdntt_moddown_device) and against a
device-to-device copy of x_hat, interleaved in one run, device-resident:

    python tools/bench_tmd.py [--rows 32:4096x16384:4x1,...] [--t 65537] [--rounds 7] [--reps 0]
                              [--warmup 3] [--lib PATH] [--out profiles/tmd/bench.json]

A row is bits:n x batch:L x K; the default rows are tools/bench_mdntt.py's.  The bases are the
first L primes = 1 mod 2^17 below the top of the class, then the next K.  Per row the timed
sequences are (device events around `reps` back-to-back calls, one synchronise per window):
  tmd       one nttmul_tmd_moddown_device call (2 launches up to n = 4096, 4 above)
  floor     one nttmul_mdntt_moddown_device call: the same transforms, without the mod-t sum and
            the (K + 1)-th product, so strictly less work
  copy      hipMemcpyAsync device to device of x_hat's bytes
They run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per call), tmd / floor, and floor's own spread
((max - min) / median), the yardstick the extra cost has to exceed to count.  No threshold is set:
the ratio is the price of keeping the plaintext.

Before timing, the two results are related through the identity out = floor - forward(u mod q_l)
on the first 33 entries (or the whole batch where it is smaller), u from the library's inverse of
the P limbs in integers on the host.  --reps 0 picks 20 for rows of at least 2^26 coefficients and
200 below.  --lib PATH measures another build of libnttmul_tmd.so (the floor form stays
lib/libnttmul_mdntt.so's).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
from math import prod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = ",".join(f"{bits}:{shape}:{lk}" for shape in ("4096x16384", "65536x1024")
                        for bits in (32, 64) for lk in ("4x1", "4x2", "12x4")) + \
    ",32:4096x64:4x1,64:4096x64:4x1"
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 65536
RELATED = 33


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def u_residues(np, coef_p, q, p, t, bits):
    """[cnt, L, n]: the centred u of the P limbs' coefficients coef_p [cnt, K, n], modulo each q_l."""
    P = prod(p)
    v = 0
    for j, m in enumerate(p):
        ys, g = pow(P // m, -1, m), -pow(m, -1, t) % t
        if bits == 32 and t < 1 << 32:         # every product below 2^64
            y = coef_p[:, j].astype(np.uint64) * np.uint64(ys) % np.uint64(m)
            v = (v + y % np.uint64(t) * np.uint64(g)) % np.uint64(t)
        else:
            y = coef_p[:, j].astype(object) * ys % m
            v = (v + y * g) % t
    v = v.astype(object)
    neg = np.asarray(v > (t - 1) // 2).astype(bool)
    dt = np.uint32 if bits == 32 else np.uint64
    return np.stack([np.where(neg, m - (t - v), v) for m in q], axis=1).astype(dt)


def relate(np, nttmul, Ctx, n, q, p, t, bits, x, out, floor):
    """The identity on x's first entries; raises where it does not hold."""
    cnt, L = min(RELATED, x.shape[0]), len(q)
    view = np.uint32 if bits == 32 else np.uint64
    host = lambda a: a[:cnt].cpu().numpy().view(view)                     # noqa: E731
    with Ctx(n, p) as cp, Ctx(n, q) as cq:
        coef_p = cp.inverse(np.ascontiguousarray(host(x)[:, L:]))
        u_hat = cq.forward(u_residues(np, coef_p, q, p, t, bits))
    mods = np.array(q, dtype=view)[None, :, None]
    want = (host(floor) + (mods - u_hat)) % mods
    if not np.array_equal(host(out), want):
        raise SystemExit("tmd differs from the floor form minus forward(u)")
    return cnt


def bench_row(torch, nttmul, np, bits, n, batch, L, K, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    M = L + K
    Ctx = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
    tm, md = nttmul.NttPlainModDown(n, q, p, args.t), nttmul.NttModDown(n, q, p)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)
    x = torch.empty((batch, M, n), dtype=dtype, device="cuda")
    for l, m in enumerate(q + p):
        x[:, l, :] = torch.randint(0, m, (batch, n), generator=gen, device="cuda",
                                   dtype=torch.int64).to(dtype)
    out = torch.empty((batch, L, n), dtype=dtype, device="cuda")
    floor, xcopy = torch.empty_like(out), torch.empty_like(x)

    variants = {"tmd": lambda: tm.moddown_device(out, x, batch, stream=stream),
                "floor": lambda: md.moddown_device(floor, x, batch, stream=stream),
                "copy": lambda: xcopy.copy_(x, non_blocking=True)}
    variants["tmd"]()
    variants["floor"]()
    torch.cuda.synchronize()
    related = relate(np, nttmul, Ctx, n, q, p, args.t, bits, x, out, floor)

    reps = args.reps or (20 if batch * n >= 1 << 26 else 200)
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
    spread = (stat["floor"]["max"] - stat["floor"]["min"]) / stat["floor"]["median"]
    ratio = stat["tmd"]["median"] / stat["floor"]["median"]
    poly = batch * n * (bits // 8)
    hashes = nttmul.kernel_hashes(nttmul.TMD_LIB_PATH)
    kernels = tm.kernel_name().split(" + ")
    row = {"word_bits": bits, "n": n, "batch": batch, "q_limbs": L, "p_limbs": K, "t": args.t,
           "reps": reps, "related_entries": related, "ms_per_call": stat,
           "copy_tbps": round(2 * M * poly / (stat["copy"]["median"] * 1e-3) / 1e12, 3),
           "tmd_over_floor": round(ratio, 3), "floor_spread": round(spread, 3),
           "costs_more_than_the_spread": bool(ratio - 1 > spread),
           "kernel_hashes": {k: hashes[nttmul.dispatch_key(k)] for k in kernels}}
    tm.close()
    md.close()
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
                    help="comma-separated bits:n x batch:L x K, e.g. 32:4096x16384:4x1")
    ap.add_argument("--t", type=int, default=65537, help="the plaintext modulus")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libnttmul_tmd.so to measure")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
    except ValueError as e:
        ap.error(f"--rows: {e}")

    import numpy as np
    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_tmd.py measures on a GPU; none is visible")
    if args.lib:
        nttmul.TMD_LIB_PATH = os.path.abspath(args.lib)
    line = {"bench": "tmd", "device": torch.cuda.get_device_name(0),
            "library": os.path.relpath(nttmul.TMD_LIB_PATH, ROOT),
            "floor_library": os.path.relpath(nttmul.MDNTT_LIB_PATH, ROOT), "t": args.t,
            "rounds": args.rounds, "warmup": args.warmup, "rows": []}
    for row in rows:
        line["rows"].append(bench_row(torch, nttmul, np, *row, args))
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
