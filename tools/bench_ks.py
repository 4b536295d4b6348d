"""Digit ModUp and ModDown for hybrid key switching (lib/libnttmul_ks.so, nttmul_ks_*_device)
against a device-to-device copy in the same run, against the algorithmic HBM bound at that copy's
rate, and, for n <= 4096, against what a caller does without the library: dnum nttmul_bconv
converters plus the torch copies that assemble the mac operand.  Device-resident, interleaved in
one run:

    python tools/bench_ks.py [--rows 32:4096x16384:4x2x2,...] [--rounds 9] [--reps 0] [--warmup 3]
                             [--out profiles/ks/bench.json]

A row is bits:n x batch:L x K x alpha.  The default rows are n = 4096 x 16,384 and
n = 65536 x 1,024 in both word classes for (L, K, alpha) = (4, 2, 2) and (12, 4, 4), and the thin
shape n = 4096 x 64.  The bases are the first L primes = 1 mod 2^17 below the top of the class,
then the next K.  Per row the timed sequences are (device events around `reps` back-to-back calls,
one synchronise per window):
  modup / moddown   one nttmul_ks_*_device call
  today             n <= 4096 only: per digit d one nttmul_bconv_convert_device from D_d to
                    (Q u P) \\ D_d into a dense buffer, one strided torch copy of it into the mac
                    layout (two where the digit splits the targets) and one of the digit's own limbs
  copy              hipMemcpyAsync device to device of modup's input bytes
They run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per call).  Before timing, modup is compared bit
for bit with `today`'s result (n <= 4096), and modup and moddown with Python integers on a sample
of coefficients.  --reps 0 picks 20 for rows of at least 2^26 coefficients and 200 below; `today`
runs a tenth as many per window.

Beside each time the line records the algorithmic bytes per call, (L + dnum (L + K)) n w per
polynomial for modup (every digit limb read once, every output word written once) and
(2 L + K) n w for moddown (w bytes per word), and their time at the rate the interleaved copy
reached (2 bytes moved per byte copied).  Prints one JSON line (and writes it to --out)."""
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
    digits = [range(lo, min(lo + alpha, L)) for lo in range(0, L, alpha)]
    ks = nttmul.KeySwitchBasis(n, q, p, alpha)
    inv, w, _, pinv, pw, Pinv = nttmul.ks_plan(n, q, p, alpha)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    wbytes = bits // 8
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)

    def words(moduli):                       # [batch][len(moduli)][n], limb l below moduli[l]
        x = torch.empty((batch, len(moduli), n), dtype=dtype, device="cuda")
        for l, m in enumerate(moduli):
            x[:, l, :] = torch.randint(0, m, (batch, n), generator=gen, device="cuda",
                                       dtype=torch.int64).to(dtype)
        return x

    x = words(q)                             # modup's input
    xd = words(ext)                          # moddown's input
    up = torch.empty((batch, dnum, M, n), dtype=dtype, device="cuda")
    down = torch.empty((batch, L, n), dtype=dtype, device="cuda")
    xcopy = torch.empty_like(x)

    variants = {"modup": lambda: ks.modup_device(up, x, batch, stream=stream),
                "moddown": lambda: ks.moddown_device(down, xd, batch, stream=stream),
                "copy": lambda: xcopy.copy_(x, non_blocking=True)}

    convs = []
    if n <= 4096:
        # what a caller does today: a converter per digit (it refuses overlapping bases), a dense
        # output, and strided copies into [batch][dnum][L + K][n]
        others = [[m for m in range(M) if m not in D] for D in digits]
        convs = [nttmul.BaseConverter(n, [q[i] for i in D], [ext[m] for m in o])
                 for D, o in zip(digits, others)]
        dense = torch.empty((batch, max(len(o) for o in others), n), dtype=dtype, device="cuda")
        today_out = torch.empty_like(up)

        def today():
            for d, (D, o, conv) in enumerate(zip(digits, others, convs)):
                xin = x[:, D.start:D.stop, :].contiguous()
                buf = dense[:, :len(o), :] if len(o) == dense.shape[1] else \
                    dense.view(-1)[:batch * len(o) * n].view(batch, len(o), n)
                conv.convert_device(buf, xin, batch, stream=stream)
                today_out[:, d, :D.start, :] = buf[:, :D.start, :]
                today_out[:, d, D.stop:, :] = buf[:, D.start:, :]
                today_out[:, d, D.start:D.stop, :] = xin

        variants["today"] = today
        today()
        variants["modup"]()
        torch.cuda.synchronize()
        assert torch.equal(up, today_out), "modup differs from the converters' composition"

    # both calls against Python integers on a sample of coefficients
    import random
    from math import prod
    rng = random.Random(7)
    spots = [(rng.randrange(batch), rng.randrange(n)) for _ in range(32)]
    variants["modup"]()
    variants["moddown"]()
    torch.cuda.synchronize()
    Pp = prod(p)
    for b, k in spots:
        col = [int(v) for v in x[b, :, k].tolist()]
        for d, D in enumerate(digits):
            Dd = prod(q[i] for i in D)
            s = sum(col[i] * inv[i] % q[i] * (Dd // q[i]) for i in D)
            assert [int(v) for v in up[b, d, :, k].tolist()] == [s % m for m in ext], \
                f"modup differs at {(b, d, k)}"
        col = [int(v) for v in xd[b, :, k].tolist()]
        s = sum(col[L + j] * pinv[j] % pj * (Pp // pj) for j, pj in enumerate(p))
        assert [int(v) for v in down[b, :, k].tolist()] == \
            [(col[i] - s) * Pinv[i] % qi for i, qi in enumerate(q)], f"moddown differs at {(b, k)}"

    reps = args.reps or (20 if batch * n >= 1 << 26 else 200)
    calls = {k: max(1, reps // 10) if k == "today" else reps for k in variants}
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

    stat = {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                "max": round(max(v), 5)} for k, v in ms.items()}
    poly = batch * n * wbytes
    copy_tbps = 2 * L * poly / (stat["copy"]["median"] * 1e-3) / 1e12
    nbytes = {"modup": (L + dnum * M) * poly, "moddown": (2 * L + K) * poly}
    hashes = nttmul.kernel_hashes(nttmul.KS_LIB_PATH)
    row = {"word_bits": bits, "n": n, "batch": batch, "q_limbs": L, "p_limbs": K,
           "digit_limbs": alpha, "digits": dnum, "reps": calls, "ms_per_call": stat,
           "copy_tbps": round(copy_tbps, 3), "bounds": {},
           "kernel_hashes": {ks.kernel_name(op): hashes[nttmul.dispatch_key(ks.kernel_name(op))]
                             for op in ("modup", "moddown")}}
    for op in ("modup", "moddown"):
        med = stat[op]["median"]
        bound = nbytes[op] / (copy_tbps * 1e12) * 1e3
        row["bounds"][op] = {"algorithmic_bytes": nbytes[op], "hbm_ms_at_copy_rate": round(bound, 5),
                             "achieved_tbps": round(nbytes[op] / (med * 1e-3) / 1e12, 3),
                             "median_over_bound": round(med / bound, 3)}
    if "today" in stat:
        row["launches_today"] = sum(3 if 0 < D.start and D.stop < M else 2 for D in digits) + \
            2 * dnum
        row["today_over_modup"] = round(stat["today"]["median"] / stat["modup"]["median"], 3)
    ks.close()
    for conv in convs:
        conv.close()
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
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
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
        raise SystemExit("bench_ks.py measures on a GPU; none is visible")
    line = {"bench": "ks", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
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
