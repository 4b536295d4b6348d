"""ModDown on NTT-domain limbs (lib/libnttmul_mdntt.so, nttmul_mdntt_moddown_device) against the
three-call composition it replaces and against a device-to-device copy of x_hat, interleaved in
one run, device-resident:

    python tools/bench_mdntt.py [--rows 32:4096x16384:4x1,...] [--rounds 9] [--reps 0]
                                [--warmup 3] [--lib PATH] [--out profiles/mdntt/bench.json]

A row is bits:n x batch:L x K.  The default rows are n = 4096 x 16,384 and n = 65536 x 1,024 in
both word classes for (L, K) = (4, 1) (the rescale), (4, 2) and (12, 4), and the thin shape
n = 4096 x 64.  The bases are the first L primes = 1 mod 2^17 below the top of the class, then the
next K.  Per row the timed sequences are (device events around `reps` back-to-back calls, one
synchronise per window):
  mdntt     one nttmul_mdntt_moddown_device call (2 launches up to n = 4096, 4 above)
  today     nttmul_rns(mp)_inverse_device over the L + K limbs, nttmul_ks_moddown_device,
            nttmul_rns(mp)_forward_device over the L limbs (3 launches, 5 above n = 4096)
  copy      hipMemcpyAsync device to device of x_hat's bytes
They run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per call) and `today`'s own spread
((max - min) / median), the yardstick a lead has to exceed.  Before timing, mdntt is compared bit
for bit with `today`'s result.  --reps 0 picks 20 for rows of at least 2^26 coefficients and 200
below.

Beside each time the line records the algorithmic bytes per call, (2 L + 3 K) n w per polynomial
for mdntt (x_hat read once, y written and read once, out written once; whatever re-reads of y miss
the caches come on top) and (6 L + 3 K) n w for the composition (w bytes per word), and their time
at the rate the interleaved copy reached (2 bytes moved per byte copied).

--lib PATH measures another build of the library, e.g. the other grid order of the forward kernels
(make ab-mdntt: lib/ab/libnttmul_mdntt_limbslow.so).  Prints one JSON line (and writes it to
--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = ",".join(f"{bits}:{shape}:{lk}" for shape in ("4096x16384", "65536x1024")
                        for bits in (32, 64) for lk in ("4x1", "4x2", "12x4")) + \
    ",32:4096x64:4x1,64:4096x64:4x1"
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 65536


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def bench_row(torch, nttmul, bits, n, batch, L, K, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    ext, M = q + p, L + K
    Ctx = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
    md = nttmul.NttModDown(n, q, p)
    big, low, ks = Ctx(n, ext), Ctx(n, q), nttmul.KeySwitchBasis(n, q, p, 1)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    wbytes = bits // 8
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)
    x = torch.empty((batch, M, n), dtype=dtype, device="cuda")
    for l, m in enumerate(ext):
        x[:, l, :] = torch.randint(0, m, (batch, n), generator=gen, device="cuda",
                                   dtype=torch.int64).to(dtype)
    out = torch.empty((batch, L, n), dtype=dtype, device="cuda")
    coef, xcopy = torch.empty_like(x), torch.empty_like(x)
    down, want = torch.empty_like(out), torch.empty_like(out)

    def today():
        big.inverse_device(coef, x, batch, stream=stream)
        ks.moddown_device(down, coef, batch, stream=stream)
        low.forward_device(want, down, batch, stream=stream)

    variants = {"mdntt": lambda: md.moddown_device(out, x, batch, stream=stream),
                "today": today,
                "copy": lambda: xcopy.copy_(x, non_blocking=True)}
    variants["mdntt"]()
    today()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "mdntt differs from the composition"

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
    poly = batch * n * wbytes
    copy_tbps = 2 * M * poly / (stat["copy"]["median"] * 1e-3) / 1e12
    nbytes = {"mdntt": (2 * L + 3 * K) * poly, "today": (6 * L + 3 * K) * poly}
    spread = (stat["today"]["max"] - stat["today"]["min"]) / stat["today"]["median"]
    lead = stat["today"]["median"] / stat["mdntt"]["median"]
    hashes = nttmul.kernel_hashes(nttmul.MDNTT_LIB_PATH)
    names = md.kernel_name().split(" + ")
    row = {"word_bits": bits, "n": n, "batch": batch, "q_limbs": L, "p_limbs": K, "reps": reps,
           "ms_per_call": stat, "copy_tbps": round(copy_tbps, 3),
           "today_over_mdntt": round(lead, 3), "today_spread": round(spread, 3),
           "ahead_by_more_than_the_spread": bool(lead - 1 > spread),
           "launches": {"mdntt": len(names), "today": 3 if n <= 4096 else 5},
           "transforms": {"mdntt": L + K, "today": 2 * L + K}, "bounds": {},
           "kernel_hashes": {k: hashes[nttmul.dispatch_key(k)] for k in names}}
    for op in ("mdntt", "today"):
        med = stat[op]["median"]
        bound = nbytes[op] / (copy_tbps * 1e12) * 1e3
        row["bounds"][op] = {"algorithmic_bytes": nbytes[op], "hbm_ms_at_copy_rate": round(bound, 5),
                             "achieved_tbps": round(nbytes[op] / (med * 1e-3) / 1e12, 3),
                             "median_over_bound": round(med / bound, 3)}
    for h in (md, big, low, ks):
        h.close()
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None,
                    help="another build of libnttmul_mdntt.so to measure (make ab-mdntt)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
    except ValueError as e:
        ap.error(f"--rows: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_mdntt.py measures on a GPU; none is visible")
    if args.lib:
        nttmul.MDNTT_LIB_PATH = os.path.abspath(args.lib)
    line = {"bench": "mdntt", "device": torch.cuda.get_device_name(0),
            "library": os.path.relpath(nttmul.MDNTT_LIB_PATH, ROOT), "rounds": args.rounds,
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
