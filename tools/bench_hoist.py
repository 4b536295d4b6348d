"""Hoisted rotations (lib/libnttmul_hoist.so, nttmul_*_hoist_ntt_device) against one macn_ntt per
rotation, device-resident, interleaved in one run:

    python tools/bench_hoist.py [--rows 32:4096x16384:4x2x2,...] [--rots 1,2,4,8] [--rounds 7]
                                [--reps 0] [--warmup 2] [--mem-gib 48]
                                [--out profiles/hoist/bench.json]

A row is bits:n x batch:L x K x alpha, as tools/bench_macn.py's, with the same default rows:
n = 4096 x 16,384 and n = 65536 x 1,024 in both word classes for (L, K, alpha) = (4, 2, 2)
(limbs 6, dnum 2) and (12, 4, 4) (limbs 16, dnum 3), and the thin shape n = 4096 x 64.  The batch
of a row is halved until the row's buffers for the largest R (the digits, their transform, one
rotated copy for the check, c of batch * R * 2 polynomials, the baseline's output) fit --mem-gib;
the row records the batch it ran.  The context holds the extended basis Q u P.  Per row and per
R in --rots the timed sequences are (device events around `reps` back-to-back sequences, one
synchronise per window):
  hoist     one forward over batch * dnum and one hoist_ntt_device with R rotations (the real
            list: 5^1 .. 5^(R-1) and the conjugation 2n - 1), comps = 2
  macn_R    R macn_ntt_device calls (comps = 2, shared) on digits that are rotated already.  That
            is the unhoisted path with its galois_coeff and modup left out, so it favours the old
            side; all R calls read one digits buffer and write one output (the words do not change
            the time), which favours it again where that buffer stays in cache
  hoist_k1  the same forward and hoist_ntt_device with every k = 1: contiguous sources.  hoist
            against hoist_k1 is the cost of the gather
They run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per sequence).  Before timing, every rotation's pair
of results is compared bit for bit with macn_ntt on galois_coeff of the digits.
--reps 0 picks 5 for rows of at least 2^26 words per polynomial set (batch * limbs * n) and 50
below.

Beside each ratio hoist / macn_R the line records macn_R's own spread, (max - min) / median,
whether hoist is ahead by more than that spread, the transform-count ratio
(dnum + 2 R) / (R (dnum + 2)), and hoist_ntt's algorithmic bytes per second: a_hat once, b_hat
once, c once, over the median of a window of hoist_ntt alone (timed as a fourth variant,
hoist_only).  Prints one JSON line (and writes it to --out)."""
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


def rotations(n, R):
    """The real list: the conjugation and the first R - 1 powers of 5 (pairwise distinct)."""
    ks = [2 * n - 1] + [pow(5, e, 2 * n) for e in range(1, R)]
    assert len(set(ks)) == R
    return ks


def row_bytes(batch, M, n, dnum, R, wb):
    """digits, their transform, one rotated copy, c of the hoisted call, the baseline's output."""
    return batch * M * n * wb * (3 * dnum + 2 * R + 2)


def fit_batch(batch, M, n, dnum, R, wb, limit):
    while batch > 1 and row_bytes(batch, M, n, dnum, R, wb) > limit:
        batch //= 2
    return batch


def hoist_bytes(batch, M, n, dnum, R, wb):
    """What hoist_ntt must move: a_hat and b_hat read once, c written once."""
    return M * n * wb * (batch * dnum + R * 2 * dnum + batch * R * 2)


def bench_row(torch, nttmul, bits, n, batch, L, K, alpha, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    ext, M, dnum, wb = q + p, L + K, -(-L // alpha), bits // 8
    rots = sorted(args.rot_list)
    asked, batch = batch, fit_batch(batch, M, n, dnum, rots[-1], wb, args.mem_gib << 30)
    Ctx = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
    ctx = Ctx(n, ext)
    gal = nttmul.GaloisContext(n, ext)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)

    def words(polys, moduli):                # [polys][len(moduli)][n], limb l below moduli[l]
        x = torch.empty((polys, len(moduli), n), dtype=dtype, device="cuda")
        for l, m in enumerate(moduli):
            x[:, l, :] = torch.randint(0, m, (polys, n), generator=gen, device="cuda",
                                       dtype=torch.int64).to(dtype)
        return x

    Rmax = rots[-1]
    up = words(batch * dnum, ext)            # the raised digits: any canonical words
    key_hat = words(Rmax * 2 * dnum, ext).view(Rmax, 2, dnum, M, n)
    up_hat = torch.empty_like(up)
    rot = torch.empty_like(up)
    c = torch.empty((batch * Rmax * 2, M, n), dtype=dtype, device="cuda")
    c1 = torch.empty((batch, 2, M, n), dtype=dtype, device="cuda")

    # every rotation's results against macn_ntt on the rotated digits, bit for bit
    ks = rotations(n, Rmax)
    ctx.forward_device(up_hat, up, batch * dnum, stream=stream)
    ctx.hoist_ntt_device(c, up_hat, key_hat, ks, batch, dnum, 2, stream=stream)
    cv = c.view(batch, Rmax, 2, M, n)
    for r, k in enumerate(ks):
        gal.coeff_device(rot, up, k, batch * dnum, stream=stream)
        ctx.macn_ntt_device(c1, rot, key_hat[r], batch, dnum, 2, shared=True, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(cv[:, r], c1), f"rotation {r} (k = {k}) differs from macn_ntt"
    assert not torch.equal(cv[:, 0], cv[:, Rmax - 1]) or Rmax == 1

    reps = args.reps or (5 if batch * M * n >= 1 << 26 else 50)
    hashes = nttmul.kernel_hashes(nttmul.HOIST_LIB_PATH)
    kernels = ctx.hoist_kernel_name(2).split(" + ") + ctx.macn_kernel_name(2).split(" + ") + \
        ctx.kernel_name("forward").split(" + ")
    row = {"word_bits": bits, "n": n, "batch": batch, "batch_asked": asked, "q_limbs": L,
           "p_limbs": K, "digit_limbs": alpha, "limbs": M, "terms": dnum, "reps": reps,
           "rotations": {},
           "kernel_hashes": {k: hashes[nttmul.dispatch_key(k)] for k in sorted(set(kernels))}}
    for R in rots:
        ks, ones = rotations(n, R), [1] * R
        kh = key_hat[:R].contiguous()

        def hoist_only(ks=ks, R=R, kh=kh):
            ctx.hoist_ntt_device(c, up_hat, kh, ks, batch, dnum, 2, stream=stream)

        def hoist(ks=ks, R=R, kh=kh):
            ctx.forward_device(up_hat, up, batch * dnum, stream=stream)
            ctx.hoist_ntt_device(c, up_hat, kh, ks, batch, dnum, 2, stream=stream)

        def hoist_k1(ones=ones, R=R, kh=kh):
            ctx.forward_device(up_hat, up, batch * dnum, stream=stream)
            ctx.hoist_ntt_device(c, up_hat, kh, ones, batch, dnum, 2, stream=stream)

        def macn_R(R=R, kh=kh):
            for r in range(R):
                ctx.macn_ntt_device(c1, rot, kh[r], batch, dnum, 2, shared=True, stream=stream)

        variants = {"hoist": hoist, "macn_R": macn_R, "hoist_k1": hoist_k1,
                    "hoist_only": hoist_only}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        names = list(variants)
        ms = {k: [] for k in names}
        for rnd in range(args.rounds):
            for k in names[rnd % len(names):] + names[:rnd % len(names)]:
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
            return ratio, spread

        def ahead(new, old):                 # is `new` faster by more than `old`'s own spread
            ratio, spread = versus(new, old)
            return {"ratio": round(ratio, 3), f"{old}_spread": round(spread, 3),
                    "ahead_by_more_than_the_spread": bool(ratio < 1 - spread)}

        def gather_cost(new, old):           # does the gather cost more than `old`'s own spread
            ratio, spread = versus(new, old)
            return {"ratio": round(ratio, 3), f"{old}_spread": round(spread, 3),
                    "gather_costs_more_than_the_spread": bool(ratio > 1 + spread)}

        row["rotations"][str(R)] = {
            "k": ks, "ms_per_call": stat,
            "hoist_over_macn_R": ahead("hoist", "macn_R"),
            "transform_count_ratio": round((dnum + 2 * R) / (R * (dnum + 2)), 3),
            "gather_over_contiguous": gather_cost("hoist", "hoist_k1"),
            "hoist_ntt_GBps": round(hoist_bytes(batch, M, n, dnum, R, wb) /
                                    (stat["hoist_only"]["median"] * 1e-3) / 1e9, 1),
            "launches": {"hoist": (1 if n <= 4096 else 2) * 2,
                         "macn_R": (1 if n <= 4096 else 3) * R}}
    ctx.close()
    gal.close()
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
    ap.add_argument("--rots", default="1,2,4,8", help="comma-separated rotation counts, 1 .. 16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=0, help="sequences per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mem-gib", type=int, default=48,
                    help="the batch of a row is halved until its buffers fit this many GiB")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
        args.rot_list = [int(v) for v in args.rots.split(",")]
        if not args.rot_list or min(args.rot_list) < 1 or max(args.rot_list) > 16:
            raise ValueError("--rots: 1 .. 16")
    except ValueError as e:
        ap.error(f"--rows / --rots: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_hoist.py measures on a GPU; none is visible")
    line = {"bench": "hoist", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "mem_gib": args.mem_gib, "rows": []}
    for row in rows:
        line["rows"].append(bench_row(torch, nttmul, *row, args))
        torch.cuda.empty_cache()
        print(f"row {len(line['rows'])} of {len(rows)} done", file=sys.stderr, flush=True)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
